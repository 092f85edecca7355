"""GPU: wbc_qp_certificate (csrc/wbc_k_cert.hip) against its host restatement wbc_workload.qp_certificate on every output — in the middle and at the
ends of its documented range (EDGE_SHAPES), and where the active set is special (k == n, k > n, an x off the optimum, the working-set and read-off
rules) —, the golden QP cases in one batch, tick_certificate, in place on guarded device memory, the refusals, the QP mirror's getDualSolution / getObjVal and wbc_torch.qp_solve.

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


_kw, _grad_terms, _compare = cc.kw, cc.grad_terms, cc.compare          # (shared with tests/test_gpu_instance_sequences.py)


def _tolerance(P, host, v, exact_n=None):
    return cc.tolerance(P, host, v, EXACT_N if exact_n is None else exact_n)


DEFAULTS = {"packed_kernel": 1}          # include/wbc.h: the value a handle has before its first wbc_batch_set_option of that name
CASES = [("n26_p16", lambda: cc.random_problem(26, 16, 12), {}), ("n25_p10", lambda: cc.random_problem(25, 10, 4), {}),
         ("n12_p6", lambda: cc.random_problem(12, 6, 2), {}), ("n26_p0", lambda: cc.random_problem(26, 0, 0), {}),
         ("n3_p2", lambda: cc.random_problem(3, 2, 0), {}), ("n26_p16_B67", lambda: cc.random_problem(26, 16, 12, 67), {}),
         ("n26_p16_B1", lambda: cc.random_problem(26, 16, 12, 1), {}), ("ls_m32", cc.ls_problem, {}),
         ("n26_p16_one_per_wave", lambda: cc.random_problem(26, 16, 12), {"packed_kernel": 0})]
# the ends of the documented range, B = 16 each, (A, b) form (m, n, p, equalities): two full 48-row chunks with rows on lanes 16..23; a second chunk of
# one row (odd-row padding); odd m in one chunk with odd n; exactly one chunk with p just past 16; no box (lb = ub = None) without and with rows;
# the smallest shape with random_qps' fixed pair; n = m = 1; and p = 24 in the (H, g) form. The exact rationals behind their tolerance cost a second per
# instance at n = 26: the first four certified instances there, and ALL sixteen at n <= 13, where they cost nothing — and where a prefix is no sample:
# at (3, 3, 0, 0) A is square, cond(A'A) runs from 4.5 to 3.5e4 over the batch and the restatement's own error from 1.1e-16 to 4.6e-12 (instance 8,
# a vertex: the exact u is 0, the device's is, numpy's z - Q1 Q1'z leaves 4.6e-12 after L^-T)
EDGE_SHAPES = [(96, 26, 24, 12, True), (49, 26, 16, 12, True), (47, 13, 5, 2, True), (48, 26, 17, 8, True), (95, 26, 0, 0, False), (33, 26, 24, 4, False),
               (3, 3, 0, 0, True)]
EDGE_EXACT_N = 4


def _exact_n(name, n):
    return (16 if n <= 13 else EDGE_EXACT_N) if name in EDGE_NAMES else EXACT_N


def _edge(m, n, p, n_eq, box, B=16):
    return cc.ls_problem(B, m, n, p, n_eq, 200 + m, box)


EDGE_CASES = [("ls_m%d_n%d_p%d%s" % (s[0], s[1], s[2], "" if s[4] else "_no_box"), (lambda s=s: _edge(*s)), {}) for s in EDGE_SHAPES]
EDGE_CASES += [("ls_m1_n1_p0", cc.ls_problem_free_bounds, {}), ("n26_p24", lambda: cc.random_problem(26, 24, 12, 16), {})]
EDGE_NAMES = {c[0] for c in EDGE_CASES}
CASES += EDGE_CASES


@pytest.mark.parametrize("name,make,options", CASES, ids=[c[0] for c in CASES])
def test_device_against_host_restatement(bt, name, make, options):
    P = make()
    v = P["v"]
    assert name not in EDGE_NAMES or ((P["status"] == 0).all() and len(P["status"]) == 16)
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
            tol, err = _tolerance(P, host, v, _exact_n(name, x.shape[1]))
        worst = _compare(dev, host, P, x, tol, "%s, working set %s" % (name, "given" if w is not None else "read off x"))
        print("%s (working set %s): restatement against exact rationals %.2e, device against restatement at most %.2f of the allowed %.2e" % (
            name, "given" if w is not None else "read off x", err, worst, tol))
        assert (dev["cert_status"][st == 0] == capi.CERT_OK).all() and (dev["kkt"][st == 0, 2] == 0).all()
    dev0 = bt.qp_certificate(x, **_kw(P, x, st, ws, None))                                   # without v: the same numbers, no sens_* outputs
    assert set(dev0) == set(dev) - {"sens_x", "sens_bounds", "sens_rows"}
    devw = bt.qp_certificate(x, **_kw(P, x, st, ws, v))
    assert all(devguard.same_bytes(dev0[k], devw[k]) for k in dev0)


def _solve(bt, P):
    """the device's answer with its working set, held to the oracle's status"""
    if P.get("A") is not None:
        x, st, _, ws = bt.qp_solve_ls(P["A"], P["b"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
    else:
        x, st, _, ws = bt.qp_solve(P["H"], P["g"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], want_working_set=True)
    assert np.array_equal(st, P["status"])
    return x, st, ws


def _both(bt, P, x, st, ws, v):
    return bt.qp_certificate(x, **_kw(P, x, st, ws, v)), cc.host_certificates(P, x=x, status=st, working_set=ws, v=v)


@pytest.mark.parametrize("case", ["vertex", "more_normals_than_variables", "non_optimal_x", "working_set_rules", "read_off_rule"])
def test_certificate_of_special_active_sets(bt, case):
    """Device against restatement (the rule and _compare of test_device_against_host_restatement) where the active set is special:
    vertex — k == n, the normals span the space, u = 0; more_normals_than_variables — k > n, DEPENDENT before the Cholesky; non_optimal_x — an
    x off the optimum three ways, so that kkt[1], kkt[2] and kkt[3] are NOT zero (the tolerance is the one of the same data at the optimum: the
    conditioning is the data's); working_set_rules — bits on infinite sides, bits beyond n and p, both bits at once, equalities whatever their
    bits; read_off_rule — without a working set, a variable 0.5e-7 from its bound counts as active and one 2e-7 from it does not."""
    if case == "vertex":
        P = cc.vertex_problem()
        x, st, ws = _solve(bt, P)
        for w in (ws, None):
            dev, host = _both(bt, P, x, st, w, P["v"])
            assert (st == 0).all() and (host["n_active"] == 6).all() and np.abs(host["sens_x"]).max() <= 5e-17
            tol, err = _tolerance(P, host, P["v"], EDGE_EXACT_N)
            worst = _compare(dev, host, P, x, tol, case)                                          # (sens_bounds among the rest)
            assert (dev["cert_status"] == capi.CERT_OK).all() and np.abs(dev["sens_x"]).max() <= tol * 1.0
            print("vertex: restatement against exact rationals %.2e, device at most %.2f of the allowed %.2e" % (err, worst, tol))
    elif case == "more_normals_than_variables":
        P = cc.overdetermined_problem()
        x, st, ws = _solve(bt, P)
        for w in (ws, None):
            dev, host = _both(bt, P, x, st, w, P["v"])
            assert (st == 0).all() and (host["cert_status"] == capi.CERT_DEPENDENT).all() and (host["n_active"] == 8).all()
            tol, _ = _tolerance(P, host, P["v"])                                                   # nothing certified: ten ulp
            assert tol == 10.0 * ULP
            _compare(dev, host, P, x, tol, case)                                                   # objective and kkt[1] among the rest
            assert (dev["cert_status"] == capi.CERT_DEPENDENT).all() and (dev["n_active"] == 8).all()
            assert (dev["kkt"][:, [0, 2, 3]] == 0).all()
            assert all((dev[k] == 0).all() for k in ("y_bounds", "y_rows", "sens_x", "sens_bounds", "sens_rows"))
    elif case == "non_optimal_x":
        P = cc.random_problem(26, 16, 12)
        x, st, ws = _solve(bt, P)
        assert (st == 0).all()
        tol, err = _tolerance(P, cc.host_certificates(P, x=x, status=st, working_set=ws, v=P["v"]), P["v"])
        for way in ("flip", "outside", "shift"):
            x2, ws2, moved = cc.off_optimum(P, x, ws, way)
            dev, host = _both(bt, P, x2, st, ws2, P["v"])
            k = host["kkt"][moved]
            assert moved.sum() >= len(x) // 2 and (host["cert_status"] == capi.CERT_OK).all()
            assert (k[:, 1] > 0).all() and (k[:, 3] > 0).all()
            # a multiplier of the wrong sign: at every flipped bound, at some of the variables pushed outside; a shift of 1e-4 changes no sign
            assert (k[:, 2] > 0).all() if way == "flip" else (k[:, 2] > 0).any() if way == "outside" else True
            assert way != "outside" or (k[:, 1] >= 1e-3 * (1 - 1e-9)).all()
            worst = _compare(dev, host, P, x2, tol, "%s, %s" % (case, way))
            print("non-optimal x (%s): %d moved, kkt[2] > 0 on %d; device at most %.2f of the allowed %.2e" % (way, moved.sum(), (k[:, 2] > 0).sum(), worst, tol))
    elif case == "working_set_rules":
        full = np.uint64(0xFFFFFFFFFFFFFFFF)
        # bits on infinite sides: no box at all, every bit of word 0 set
        P = _edge(33, 26, 24, 4, False)
        x, st, ws = _solve(bt, P)
        plain, host = _both(bt, P, x, st, ws, P["v"])
        tol, _ = _tolerance(P, host, P["v"], EDGE_EXACT_N)
        worst = [_compare(plain, host, P, x, tol, case + ", no box")]
        for word0 in (full, np.uint64(0x00000000FFFFFFFF), np.uint64(0xFFFFFFFF00000000)):
            w2 = ws.copy().view(np.uint64)
            w2[:, 0] = word0
            w2 = w2.view(np.int64)
            dev, host2 = _both(bt, P, x, st, w2, P["v"])
            assert devguard.same_bytes(dev, plain) and np.array_equal(host2["n_active"], host["n_active"]), hex(int(word0))
        # bits at variable positions >= n and row positions >= p
        P = _edge(47, 13, 5, 2, True)
        n, p = 13, 5
        x, st, ws = _solve(bt, P)
        plain, host = _both(bt, P, x, st, ws, P["v"])
        tol, _ = _tolerance(P, host, P["v"], 16)
        worst.append(_compare(plain, host, P, x, tol, case + ", (47, 13, 5)"))
        w2 = ws.copy().view(np.uint64)
        low = lambda k: np.uint64(((1 << 32) - (1 << k)) * ((1 << 32) + 1))                          # bits k..31 of both halves
        for rows, extra in ((slice(0, 16, 2), (low(n), low(p))), (slice(1, 16, 2), (np.uint64(1 << n), np.uint64(1 << (32 + p))))):
            w2[rows, 0] |= extra[0]
            w2[rows, 1] |= extra[1]
        assert (w2 != ws.view(np.uint64)).all()
        dev, host2 = _both(bt, P, x, st, w2.view(np.int64), P["v"])
        assert devguard.same_bytes(dev, plain) and np.array_equal(host2["n_active"], host["n_active"])
        # both bits at once: inactive; an equality: active whatever its bits
        P = cc.random_problem(26, 16, 12)
        x, st, ws = _solve(bt, P)
        plain, host = _both(bt, P, x, st, ws, P["v"])
        tol, _ = _tolerance(P, host, P["v"])
        both, none, eq = ws.copy(), ws.copy(), ws.copy()
        hit = np.zeros(len(x), dtype=bool)
        for i in range(len(x)):
            for word, j in [(0, j) for j in range(24)] + [(1, j) for j in range(12, 16)]:        # the inequalities: variables 0..23, rows 12..15
                if cc.ws_bits(ws, i, word, j) in (1, 2):
                    cc.ws_set(both, i, word, j, 3)
                    cc.ws_set(none, i, word, j, 0)
                    hit[i] = True
                    break
            for j in (24, 25):                                                                     # the fixed pair and the twelve equality rows
                cc.ws_set(eq, i, 0, j, (0, 3)[j - 24])
            for j in range(12):
                cc.ws_set(eq, i, 1, j, (0, 2, 3, 1)[(i + j) % 4])
        assert hit.sum() >= len(x) // 2 and (eq != ws).any(axis=1).all()
        dev_b, host_b = _both(bt, P, x, st, both, P["v"])
        dev_n, host_n = _both(bt, P, x, st, none, P["v"])
        assert devguard.same_bytes(dev_b, dev_n) and np.array_equal(host_b["n_active"], host["n_active"] - hit)
        worst.append(_compare(dev_b, host_b, P, x, tol, case + ", both bits"))
        dev_e, host_e = _both(bt, P, x, st, eq, P["v"])
        assert devguard.same_bytes(dev_e, plain) and np.array_equal(host_e["n_active"], host["n_active"])
        worst.append(_compare(dev_e, host_e, P, x, tol, case + ", equalities"))
        print("working-set rules: device at most %.2f of the allowed tolerance" % max(worst))
    else:
        P = cc.random_problem(26, 16, 12)
        x, st, ws = _solve(bt, P)
        tol, _ = _tolerance(P, cc.host_certificates(P, x=x, status=st, working_set=ws, v=P["v"]), P["v"])
        x2, near, far = cc.near_bounds(P, x, ws)
        dev, host = _both(bt, P, x2, st, None, P["v"])
        rows = np.arange(len(x))
        assert (host["side"][rows, near] == 1).all() and (host["side"][rows, far] == 0).all()
        assert np.array_equal(dev["n_active"], host["n_active"]) and np.array_equal(dev["cert_status"], host["cert_status"])
        yd, yh = np.concatenate([dev["y_bounds"], dev["y_rows"]], axis=1), np.concatenate([host["y_bounds"], host["y_rows"]], axis=1)
        certified = host["cert_status"] == capi.CERT_OK
        assert certified.sum() >= len(x) // 2 and np.array_equal(yd[certified] != 0, yh[certified] != 0)
        assert (yd[rows, far] == 0).all() and (yh[rows, near][certified] != 0).all()
        print("read-off rule: device at most %.2f of the allowed %.2e" % (_compare(dev, host, P, x2, tol, case), tol))


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
