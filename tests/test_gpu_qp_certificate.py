"""GPU: wbc_qp_certificate (csrc/wbc_k_cert.hip) against its host restatement wbc_workload.qp_certificate on every output, the golden QP cases in one
batch, tick_certificate, in place on guarded device memory, the refusals, the QP mirror's getDualSolution / getObjVal and wbc_torch.qp_solve.

Tolerance of a device-against-restatement comparison: TEN TIMES the restatement's own error against the exact rationals on the same inputs
(cert_common.restatement_error over the first EXACT_N certified instances: multipliers, and u, w where v is given), never below ten times one
ulp (no double is resolved below that). The figure multiplies the size of what an output is formed from: the vector's own largest entry for
y; max(1, .) for u and w (exactly 0 where the active normals span the space) and the objective; for the stationarity residual the terms
it is summed from, |H| |x| + |g| (or |A|'(|A| |x| + |b|)) plus |y_bounds| + |C|'|y_rows| — at an unconstrained minimiser grad f itself is 0 to
rounding, the terms are not; max(1, |(x; C x)|_inf) for the primal violation; |y|_inf (times that) for the wrong-signed multiplier (the
complementarity product)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cert_common as cc
import common
import devguard
import wbc_capi as capi
import wbc_workload
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu
EXACT_N = 6
ULP = 2.220446049250313e-16


@pytest.fixture(scope="module")
def bt():
    b = WbcBatch([], 128)
    yield b
    b.close()


def _kw(P, x, st=None, ws=None, v=None):
    kw = dict(C_=P["C"], lb=P["lb"], ub=P["ub"], Clb=P["Clb"], Cub=P["Cub"], status=st, working_set=ws, v=v)
    kw.update(dict(A=P["A"], b=P["b"]) if P.get("A") is not None else dict(H=P["H"], g=P["g"]))
    return kw


def _grad_terms(P, x, yb, yr):
    """[B]: the largest entry of what grad f - N'y is summed from"""
    if P.get("A") is not None:
        A = np.abs(P["A"])
        t = np.einsum("bmi,bm->bi", A, np.einsum("bmi,bi->bm", A, np.abs(x)) + np.abs(P["b"]))
    else:
        t = np.einsum("bij,bj->bi", np.abs(P["H"]), np.abs(x)) + np.abs(P["g"])
    t = t + np.abs(yb)
    if P["C"] is not None:
        t = t + np.einsum("bpi,bp->bi", np.abs(P["C"]), np.abs(yr))
    return t.max(axis=1)


def _tolerance(P, host, v):
    idx = [i for i in range(len(host["cert_status"])) if host["cert_status"][i] == capi.CERT_OK][:EXACT_N]
    sub = {k: a[idx] for k, a in host.items()}
    err = cc.restatement_error(P, sub, idx, v)
    return 10.0 * max(err, ULP), err


def _compare(dev, host, P, x, tol, what, only_kkt=False):
    """every output of the device against the restatement (only_kkt: the four residuals alone); returns the largest ratio error / tolerance seen"""
    assert np.array_equal(dev["n_active"], host["n_active"]), (what, np.nonzero(dev["n_active"] != host["n_active"]))
    assert np.array_equal(dev["cert_status"], host["cert_status"]), (what, dev["cert_status"], host["cert_status"])
    B = len(x)
    cat = lambda d, a, b: np.concatenate([d[a], d[b]], axis=1)
    yd, yh = cat(dev, "y_bounds", "y_rows"), cat(host, "y_bounds", "y_rows")
    ymax = np.abs(yh).max(axis=1, initial=0.0)
    terms = _grad_terms(P, x, host["y_bounds"], host["y_rows"])
    vals = np.abs(x).max(axis=1)
    if P["C"] is not None:
        vals = np.maximum(vals, np.abs(np.einsum("bpi,bi->bp", P["C"], x)).max(axis=1))
    vals = np.maximum(1.0, vals)
    checks = [("y", np.abs(yd - yh).max(axis=1, initial=0.0), ymax),
              ("objective", np.abs(dev["objective"] - host["objective"]), np.maximum(1.0, np.abs(host["objective"]))),
              ("kkt[0] stationarity", np.abs(dev["kkt"][:, 0] - host["kkt"][:, 0]), terms),
              ("kkt[1] violation", np.abs(dev["kkt"][:, 1] - host["kkt"][:, 1]), vals),
              ("kkt[2] wrong sign", np.abs(dev["kkt"][:, 2] - host["kkt"][:, 2]), ymax),
              ("kkt[3] complementarity", np.abs(dev["kkt"][:, 3] - host["kkt"][:, 3]), ymax * vals)]
    if only_kkt:
        checks = checks[2:]
    elif "sens_x" in dev:
        wd, wh = cat(dev, "sens_bounds", "sens_rows"), cat(host, "sens_bounds", "sens_rows")
        checks += [("u", np.abs(dev["sens_x"] - host["sens_x"]).max(axis=1), np.maximum(1.0, np.abs(host["sens_x"]).max(axis=1))),
                   ("w", np.abs(wd - wh).max(axis=1, initial=0.0), np.maximum(1.0, np.abs(wh).max(axis=1, initial=0.0)))]
    worst = 0.0
    for name, diff, scale in checks:
        assert diff.shape == (B,) and scale.shape == (B,)
        bad = diff > tol * scale
        assert not bad.any(), "%s: %s: instance %d off by %.3e, allowed %.3e" % (what, name, np.argmax(bad), diff[np.argmax(bad)], tol * scale[np.argmax(bad)])
        worst = max(worst, float((diff / np.where(scale > 0, scale, 1.0)).max()) / tol)
    assert (yd[host["side"] == 0] == 0).all(), what                   # inactive entries are exactly zero
    return worst


DEFAULTS = {"packed_kernel": 1}          # include/wbc.h: the value a handle has before its first wbc_batch_set_option of that name
CASES = [("n26_p16", lambda: cc.random_problem(26, 16, 12), {}), ("n25_p10", lambda: cc.random_problem(25, 10, 4), {}),
         ("n12_p6", lambda: cc.random_problem(12, 6, 2), {}), ("n26_p0", lambda: cc.random_problem(26, 0, 0), {}),
         ("n3_p2", lambda: cc.random_problem(3, 2, 0), {}), ("n26_p16_B67", lambda: cc.random_problem(26, 16, 12, 67), {}),
         ("n26_p16_B1", lambda: cc.random_problem(26, 16, 12, 1), {}), ("ls_m32", cc.ls_problem, {}),
         ("n26_p16_one_per_wave", lambda: cc.random_problem(26, 16, 12), {"packed_kernel": 0})]


@pytest.mark.parametrize("name,make,options", CASES, ids=[c[0] for c in CASES])
def test_device_against_host_restatement(bt, name, make, options):
    P = make()
    v = P["v"]
    before = {k: getattr(bt, "_options", {}).get(k, DEFAULTS[k]) for k in options}
    for k, val in options.items():
        bt.set_option(k, val)
    try:
        if P.get("A") is not None:
            x, st, _, ws = bt.qp_solve_ls(P["A"], P["b"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
        else:
            x, st, _, ws = bt.qp_solve(P["H"], P["g"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
        if options:
            assert bt.stat("last_qp_path") == 1
    finally:
        for k, val in before.items():
            bt.set_option(k, val)
    assert np.array_equal(st, P["status"])
    tol = None
    for w in (ws, None):
        dev = bt.qp_certificate(x, **_kw(P, x, st, w, v))
        host = cc.host_certificates(P, x=x, status=st, working_set=w, v=v)
        if tol is None:
            tol, err = _tolerance(P, host, v)
        worst = _compare(dev, host, P, x, tol, "%s, working set %s" % (name, "given" if w is not None else "read off x"))
        print("%s (working set %s): restatement against exact rationals %.2e, device against restatement at most %.2f of the allowed %.2e" % (
            name, "given" if w is not None else "read off x", err, worst, tol))
        assert (dev["cert_status"][st == 0] == capi.CERT_OK).all() and (dev["kkt"][st == 0, 2] == 0).all()
    dev0 = bt.qp_certificate(x, **_kw(P, x, st, ws, None))                                   # without v: the same numbers, no sens_* outputs
    assert set(dev0) == set(dev) - {"sens_x", "sens_bounds", "sens_rows"}
    devw = bt.qp_certificate(x, **_kw(P, x, st, ws, v))
    assert all(devguard.same_bytes(dev0[k], devw[k]) for k in dev0)


def test_golden_cases_in_one_batch(bt):
    """the seven qp_cases: statuses; the DEPENDENT and UNSOLVED rows — and a row with a NaN — leave the other instances' bits as a batch without them has them"""
    P = cc.qp_cases()
    x, st, _, ws = bt.qp_solve(P["H"], P["g"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
    assert np.array_equal(st, P["status"])
    full = bt.qp_certificate(x, **_kw(P, x, st, ws, P["v"]))
    got = dict(zip(P["names"], full["cert_status"].tolist()))
    assert got == {"all_bounds_active": 0, "bounds_only": 0, "contradictory_equalities": 1, "duplicate_equalities": 2, "infeasible_box": 1,
                   "locked_and_mixed": 0, "unconstrained": 0}, got
    by = {nm: i for i, nm in enumerate(P["names"])}
    assert full["n_active"][by["all_bounds_active"]] == 26 and full["n_active"][by["unconstrained"]] == 0
    i = by["unconstrained"]
    assert np.abs(full["sens_x"][i] - np.linalg.solve(P["H"][i], P["v"][i])).max() <= 1e-9 * np.abs(full["sens_x"][i]).max()
    i = by["duplicate_equalities"]
    assert full["objective"][i] != 0 and full["n_active"][i] > 0 and (full["kkt"][i, [0, 2, 3]] == 0).all()
    assert all((full[k][i] == 0).all() for k in ("y_bounds", "y_rows", "sens_x", "sens_bounds", "sens_rows"))
    for nm in ("contradictory_equalities", "infeasible_box"):
        assert all((np.asarray(full[k][by[nm]]) == 0).all() for k in full if k != "cert_status"), nm
    host = cc.host_certificates(P, x=x, status=st, working_set=ws, v=P["v"])
    tol, _ = _tolerance(P, host, P["v"])
    _compare(full, host, P, x, tol, "qp_cases")
    keep = np.nonzero(full["cert_status"] == 0)[0]
    sub = {k: (None if P[k] is None else np.ascontiguousarray(P[k][keep])) for k in ("H", "g", "C", "lb", "ub", "Clb", "Cub")}
    alone = bt.qp_certificate(x[keep], **_kw(sub, x[keep], st[keep], ws[keep], P["v"][keep]))
    assert all(devguard.same_bytes(alone[k], np.ascontiguousarray(full[k][keep])) for k in full)
    Hn = P["H"].copy()
    Hn[by["bounds_only"], 4, 7] = np.nan
    xn = x.copy()
    xn[by["locked_and_mixed"], 2] = np.inf
    bad = bt.qp_certificate(xn, **_kw(dict(P, H=Hn), xn, st, ws, P["v"]))
    for nm in ("bounds_only", "locked_and_mixed"):
        assert bad["cert_status"][by[nm]] == capi.CERT_NUMERICAL and all((np.asarray(bad[k][by[nm]]) == 0).all() for k in bad if k != "cert_status")
    rest = [i for i in range(len(x)) if P["names"][i] not in ("bounds_only", "locked_and_mixed")]
    assert all(devguard.same_bytes(np.ascontiguousarray(bad[k][rest]), np.ascontiguousarray(full[k][rest])) for k in full)
    assert all(np.isfinite(np.asarray(bad[k], dtype=np.float64)).all() for k in bad)


def test_non_finite_rows_of_the_least_squares_form(bt):
    """(A, b) form, where the kernel forms A x - b, grad f and the objective from the staged image before the data check ends the instance:
    a NaN in A, an inf in x, a NaN in b, C and v each give NUMERICAL with every output zero and finite, and the other instances keep the
    bits they have in the clean batch"""
    P = cc.ls_problem()
    B = 12
    sub = {k: np.array(P[k][:B]) for k in ("A", "b", "C", "lb", "ub", "Clb", "Cub", "v")}
    x, st, _, ws = bt.qp_solve_ls(sub["A"], sub["b"], sub["C"], sub["lb"], sub["ub"], sub["Clb"], sub["Cub"], want_working_set=True)
    clean = bt.qp_certificate(x, **_kw(sub, x, st, ws, sub["v"]))
    assert (clean["cert_status"] == capi.CERT_OK).all() and (clean["objective"] != 0).all()
    bad = {k: a.copy() for k, a in sub.items()}
    xb = x.copy()
    bad["A"][1, 30, 3] = np.nan
    xb[4, 7] = np.inf
    bad["b"][6, 0] = np.nan
    bad["C"][8, 15, 25] = -np.inf
    bad["v"][10, 0] = np.nan
    hit = [1, 4, 6, 8, 10]
    rest = [i for i in range(B) if i not in hit]
    got = bt.qp_certificate(xb, **_kw(bad, xb, st, ws, bad["v"]))
    assert (got["cert_status"][hit] == capi.CERT_NUMERICAL).all() and (got["cert_status"][rest] == capi.CERT_OK).all()
    for k in got:
        a = np.asarray(got[k], dtype=np.float64)
        assert np.isfinite(a).all(), k
        if k != "cert_status":
            assert (a[hit] == 0).all(), (k, a[hit])
        assert devguard.same_bytes(np.ascontiguousarray(got[k][rest]), np.ascontiguousarray(clean[k][rest])), k
    host = cc.host_certificates(dict(bad, x=xb), x=xb, status=st, working_set=ws, v=bad["v"])
    assert np.array_equal(host["cert_status"], got["cert_status"]) and (host["objective"][hit] == 0).all()


@pytest.mark.parametrize("name", ["c3", "everything"])
def test_tick_certificate(name):
    """assemble + tick + certificate on the device, B = 48, seed 7: qdot, status and working set have the bits of wbc_tick with the working set
    out; every output against the restatement on the arrays wbc_assemble returns (the certificate's own inputs); the four residuals against the
    restatement on the ORACLE'S assembled data at the same qdot (two roundings of one problem: the residuals agree to the size of their terms,
    the multipliers only to that times the problem's conditioning); no wrong-signed multiplier; the stationarity residual relative to
    max(1, |g|_inf) no more than ten times what the restatement shows at the oracle's own answer."""
    P = cc.tick_problem(name)
    model = common.models()[0]
    B = len(P["x"])
    b2 = WbcBatch(model, B)
    try:
        b2.configure(common.config(name, model))
        dev_in = {k: torch.from_numpy(np.array(a)).cuda() for k, a in P["inputs"].items()}
        r = devguard.to_host(b2.tick_certificate(dev_in, cc.DT))
        t = devguard.to_host(b2.tick(dev_in, cc.DT, want_working_set=True))
        a = devguard.to_host(b2.assemble(dev_in, cc.DT, want=("A", "b", "C", "Clb", "Cub", "lb", "ub")))
    finally:
        b2.close()
    assert all(devguard.same_bytes(r[k], t[k]) for k in ("qdot", "status", "iters", "working_set")) and np.array_equal(r["status"], P["status"])
    solved = r["status"] == 0
    assert (r["cert_status"][solved] == capi.CERT_OK).all() and (r["cert_status"][~solved] == capi.CERT_UNSOLVED).all()
    assert (r["kkt"][solved, 2] == 0).all(), r["kkt"][solved, 2].max()
    Pd = dict(a, x=r["qdot"], status=r["status"])
    host = cc.host_certificates(Pd, status=r["status"], working_set=r["working_set"])
    tol, err = _tolerance(Pd, host, None)
    worst = _compare(r, host, Pd, r["qdot"], tol, name)
    host_o = cc.host_certificates(P, x=r["qdot"], status=r["status"], working_set=r["working_set"])
    worst_o = _compare(r, host_o, P, r["qdot"], tol, name + ", the oracle's data", only_kkt=True)
    gmax = np.maximum(1.0, np.abs(P["g"][solved]).max(axis=1))
    stat = float((r["kkt"][solved, 0] / gmax).max())
    ref = float((cc.host_certificates(P, status=P["status"])["kkt"][solved, 0] / gmax).max())
    print("%s: restatement against exact rationals %.2e; device against restatement at most %.2f (the oracle's data, residuals: %.2f) of the allowed "
          "%.2e; largest kkt[0] / max(1, |g|_inf) = %.3e (restatement at the oracle's answer: %.3e)" % (name, err, worst, worst_o, tol, stat, ref))
    assert stat <= 10.0 * max(ref, ULP), "largest kkt[0] / max(1, |g|_inf) on %s: %.3e (restatement at the oracle's answer: %.3e)" % (name, stat, ref)


def test_in_place_on_guarded_device_memory(bt):
    """device pointers, a non-default stream, guard rows around every array: inputs come back byte for byte, nothing outside the outputs' live
    rows is written, and the result has the bits of the call on plain host arrays"""
    P = cc.random_problem(26, 16, 12)
    O = cc.random_problem(26, 16, 12, 67)                           # rows of another valid batch for the input guards
    x, st, _, ws = bt.qp_solve(P["H"], P["g"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
    ref = bt.qp_certificate(x, **_kw(P, x, st, ws, P["v"]))
    ref0 = bt.qp_certificate(x, **_kw(P, x, st, None, None))
    stream = torch.cuda.Stream()
    other = dict(H=O["H"], g=O["g"], C=O["C"], lb=O["lb"], ub=O["ub"], Clb=O["Clb"], Cub=O["Cub"], x=O["x"], v=O["v"], status=O["status"],
                 working_set=np.zeros((67, 2), dtype=np.int64))
    for mode in ("other", "nan"):
        s = devguard.Session(mode, stream)
        live = dict(H=P["H"], g=P["g"], C=P["C"], lb=P["lb"], ub=P["ub"], Clb=P["Clb"], Cub=P["Cub"], x=x, v=P["v"], status=st, working_set=ws)
        d = s.put_all(live, other)
        bt.allocator = s.alloc
        try:
            got = s.run(lambda: bt.qp_certificate(d["x"], H=d["H"], g=d["g"], C_=d["C"], lb=d["lb"], ub=d["ub"], Clb=d["Clb"], Cub=d["Cub"],
                                                  status=d["status"], working_set=d["working_set"], v=d["v"]))
            got0 = s.run(lambda: bt.qp_certificate(d["x"], H=d["H"], g=d["g"], C_=d["C"], lb=d["lb"], ub=d["ub"], Clb=d["Clb"], Cub=d["Cub"]))
        finally:
            bt.allocator = None
        s.check("qp_certificate, guards: %s" % mode)
        assert len(s.outputs) == 9 + 6
        assert devguard.same_bytes(devguard.to_host(got), ref), mode
        assert devguard.same_bytes(devguard.to_host(got0), ref0), mode   # status, working_set, v and the sens_* outputs left NULL


def test_refusals(bt):
    """every WBC_E_ARG of wbc_qp_certificate, each naming its field"""
    n, p, m, B = 4, 2, 5, 2
    arr = {k: np.zeros(s) for k, s in dict(H=(B, n, n), g=(B, n), A=(B, m, n), b=(B, m), C=(B, p, n), lb=(B, n), ub=(B, n), Clb=(B, p), Cub=(B, p),
                                            x=(B, n), v=(B, n), y=(B, n), yr=(B, p)).items()}
    ptr = lambda k: arr[k].ctypes.data

    def call(fields, outs=("y_bounds",), **sizes):
        q = capi.WbcQpProblem()
        q.n, q.p, q.m = sizes.get("n", n), sizes.get("p", p), sizes.get("m", m if "A" in fields else 0)
        for k in fields:
            setattr(q, k, ptr(k))
        o = capi.WbcQpCert()
        for k in outs:
            setattr(o, k, ptr("yr" if k in ("y_rows", "sens_rows") else "y"))
        rc = bt.lib.wbc_qp_certificate(bt._h, B, C.byref(q), C.byref(o), capi.MEM_HOST, None)
        return rc, (bt.lib.wbc_last_error() or b"").decode()
    base = ("C", "lb", "ub", "Clb", "Cub", "x")
    for fields, outs, sizes, words in (
            (("H", "g", "A", "b") + base, ("y_bounds",), {}, ("both", "H, g", "A, b")),
            (base, ("y_bounds",), {}, ("neither", "H, g", "A, b")),
            (("H",) + base, ("y_bounds",), {}, ("H and g",)),
            (("H", "g", "C", "lb", "ub", "Clb", "Cub"), ("y_bounds",), {}, ("x is required",)),
            (("H", "g") + base, ("y_bounds",), dict(n=27), ("n = 27",)),
            (("H", "g") + base, ("y_bounds",), dict(n=0), ("n = 0",)),
            (("H", "g") + base, ("y_bounds",), dict(p=25), ("p = 25",)),
            (("A", "b") + base, ("y_bounds",), dict(m=97), ("m = 97",)),
            (("A", "b") + base, ("y_bounds",), dict(m=0), ("m = 0",)),
            (("H", "g", "lb", "ub", "Clb", "Cub", "x"), ("y_bounds",), {}, ("C, Clb, Cub",)),
            (("H", "g", "C", "lb", "Clb", "Cub", "x"), ("y_bounds",), {}, ("lb and ub",)),
            (("H", "g") + base, ("sens_x",), {}, ("sens_x", "without v")),
            (("H", "g") + base, ("sens_bounds",), {}, ("sens_bounds", "without v")),
            (("H", "g") + base, ("sens_rows",), {}, ("sens_rows", "without v"))):
        rc, msg = call(fields, outs, **sizes)
        assert rc == capi.E_ARG and all(w in msg for w in words), (fields, outs, sizes, rc, msg)
    rc, msg = call(("H", "g", "v") + base, ("sens_x", "sens_bounds", "sens_rows"))
    assert rc == 0, msg                                            # (with v they are accepted; H = 0 ends in cert_status, not in a refusal)
    assert bt.lib.wbc_qp_certificate(bt._h, B, None, None, capi.MEM_HOST, None) == capi.E_ARG
    assert bt.lib.wbc_qp_certificate(bt._h, 0, None, None, capi.MEM_HOST, None) == capi.E_ARG


def test_qp_mirror_dual_solution_and_objective():
    """QP.getDualSolution / getObjVal / kkt on one (m, n, p) = (32, 26, 16) problem against the restatement"""
    from QP_Wrapper import QP
    P = cc.ls_problem()
    i = 0
    qp = QP(P["A"][i], P["b"][i], P["lb"][i], P["ub"][i], P["C"][i].T, P["Clb"][i], P["Cub"][i])
    y0 = qp.getDualSolution()                                                                      # before a solve: n + p zeros
    assert y0.shape == (26 + 16,) and (y0 == 0).all() and qp.getObjVal() == 0.0 and (qp.kkt == 0).all()
    buf0 = np.full(26 + 16, 7.0)
    assert qp.getDualSolution(buf0) is buf0 and (buf0 == 0).all()
    assert QP(P["A"][i], P["b"][i], P["lb"][i], P["ub"][i]).getDualSolution().shape == (26,)       # a bounds-only QP: n
    x = qp.solveQP()
    assert qp.status == 0
    ws = np.asarray(qp._ws).reshape(1, 2)
    one = {k: (P[k][i:i + 1] if isinstance(P[k], np.ndarray) else P[k]) for k in P}
    host = cc.host_certificates(one, x=x[None], working_set=ws)
    tol, _ = _tolerance(one, host, None)
    y = qp.getDualSolution()
    yh = np.concatenate([host["y_bounds"][0], host["y_rows"][0]])
    assert y.shape == (26 + 16,) and np.abs(y - yh).max() <= tol * np.abs(yh).max()
    buf = np.full(26 + 16, 7.0)
    assert qp.getDualSolution(buf) is buf and np.array_equal(buf, y)
    assert abs(qp.getObjVal() - host["objective"][0]) <= tol * max(1.0, abs(host["objective"][0]))
    assert qp.kkt.shape == (4,) and qp.kkt[2] == 0 and qp.kkt[1] <= 1e-9
    bad = QP(P["A"][i], P["b"][i], np.ones(26), -np.ones(26), P["C"][i].T, P["Clb"][i], P["Cub"][i])   # an infeasible box: unsolved, zeros
    bad.solveQP()
    assert bad.status != 0 and (bad.getDualSolution() == 0).all() and bad.getObjVal() == 0.0


def test_torch_qp_solve_gradients(bt):
    """wbc_torch.qp_solve: gradients of sum(x . v) with respect to g, lb, ub, Clb, Cub, H and C against the host formulas, B = 8, (12, 6, 2)"""
    import wbc_torch
    P = cc.random_problem(12, 6, 2)
    B = 8
    names = ("H", "g", "C", "lb", "ub", "Clb", "Cub")
    t = {k: torch.from_numpy(np.ascontiguousarray(P[k][:B])).cuda().requires_grad_(True) for k in names}
    v = torch.from_numpy(np.ascontiguousarray(P["v"][:B])).cuda()
    x, st = wbc_torch.qp_solve(t["H"], t["g"], t["C"], t["lb"], t["ub"], t["Clb"], t["Cub"], bt)
    assert not st.requires_grad and (st.cpu().numpy() == P["status"][:B]).all()
    (x * v).sum().backward()
    xh = x.detach().cpu().numpy()
    sub = {k: (P[k][:B] if isinstance(P[k], np.ndarray) else P[k]) for k in P}
    host = cc.host_certificates(sub, x=xh, status=P["status"][:B], v=P["v"][:B])
    tol, err = _tolerance(sub, host, P["v"][:B])
    y = np.concatenate([host["y_bounds"], host["y_rows"]], axis=1)
    w = np.concatenate([host["sens_bounds"], host["sens_rows"]], axis=1)
    worst = 0.0
    for i in range(B):
        G = wbc_workload.qp_gradients(xh[i], y[i], host["sens_x"][i], w[i], host["side"][i])
        if host["cert_status"][i] != capi.CERT_OK:
            G = {k: np.zeros_like(a) for k, a in G.items()}
        for k in names:
            got = t[k].grad[i].cpu().numpy()
            d = np.abs(got - G[k]).max() / max(1.0, np.abs(G[k]).max())
            worst = max(worst, d / tol)
            assert d <= tol, (k, i, d, tol)
    print("wbc_torch.qp_solve: gradients against the host formulas at most %.2f of the allowed %.2e (restatement against exact rationals %.2e)" % (worst, tol, err))
    assert t["lb"].grad[:, -2:].abs().max() > 0 and torch.equal(t["lb"].grad[:, -2:], t["ub"].grad[:, -2:])   # the fixed variables: half and half
