"""CPU: wbc_qp_certificate at the boundary (header, export, struct sizes) and its host restatement wbc_workload.qp_certificate / qp_gradients —
against exact rationals (common.exact_kkt), against central differences of the oracle's solve, and on tests/golden/qp_cases.npz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cert_common as cc
import common
import oracle
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_certificate():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    assert re.search(r"int\s+wbc_qp_certificate\s*\(\s*WbcBatch\s*\*", header)
    for word in ("WbcQpProblem", "WbcQpCert", "WBC_CERT_DEPENDENT", "1e-12", "getDualSolution", "sens_bounds", "Householder"):
        assert word in header, word
    lib = capi.load_library()
    assert hasattr(lib, "wbc_qp_certificate") and "wbc_qp_certificate" in capi.SIGNATURES
    sp, sc = C.c_int32(), C.c_int32()
    assert lib.wbc_qp_certificate_sizes(C.byref(sp), C.byref(sc)) == 0
    assert (sp.value, sc.value) == (C.sizeof(capi.WbcQpProblem), C.sizeof(capi.WbcQpCert))
    assert "cert" not in capi.VARIANT_FAMILIES and lib.wbc_variant_count(b"cert") < 0          # a kernel without variant-table rows


def _first_solved(P, k):
    return [i for i in range(len(P["status"])) if P["status"][i] == 0][:k]


# largest relative error of the multipliers against the exact rationals, 4 instances each, as measured with the QR route: c3 3.2e-15,
# "everything" 7.6e-15, random (26, 16, 12) 5.2e-15 (the Schur route gave 7e-8 on c3); the bounds are 10 x those
@pytest.mark.parametrize("family,bound", [("c3", 3.2e-14), ("everything", 7.6e-14), ("random", 5.2e-14)])
def test_restatement_against_exact_rationals(family, bound):
    P = cc.random_problem(26, 16, 12) if family == "random" else cc.tick_problem(family)
    idx = _first_solved(P, 4)
    assert len(idx) == 4
    cert = cc.host_certificates(P, idx=idx)
    assert (cert["cert_status"] == capi.CERT_OK).all()
    err = cc.restatement_error(P, cert, idx, solver=common.exact_kkt)
    print("%s: multipliers against the exact rationals, largest relative error %.3e (bound %.1e)" % (family, err, bound))
    assert err <= bound, err
    assert cc.restatement_error(P, cert, idx[:1]) == cc.restatement_error(P, cert, idx[:1], solver=common.exact_kkt)   # exact_kkt_int: the same bits


@pytest.mark.parametrize("family", ["c3", "everything", "random"])
def test_no_wrong_signed_multiplier_on_any_solved_instance(family):
    P = cc.random_problem(26, 16, 12) if family == "random" else cc.tick_problem(family)
    cert = cc.host_certificates(P, status=P["status"])
    solved = P["status"] == 0
    assert solved.sum() >= len(solved) - 1                         # the oracle solves 48 / 47 / 64 of them
    assert (cert["cert_status"][solved] == capi.CERT_OK).all() and (cert["cert_status"][~solved] == capi.CERT_UNSOLVED).all()
    assert (cert["kkt"][solved, 2] == 0.0).all(), cert["kkt"][solved, 2].max()
    y = np.concatenate([cert["y_bounds"], cert["y_rows"]], axis=1)
    assert (y[cert["side"] == 1] >= 0).all() and (y[cert["side"] == 2] <= 0).all() and (y[cert["side"] == 0] == 0).all()
    assert (y[~solved] == 0).all() and (cert["objective"][~solved] == 0).all()


def _solve(P, **over):
    Q = dict(P, **over)
    return oracle.qp_solve(Q["H"], Q["g"], Q["C"], Q["lb"], Q["ub"], Q["Clb"], Q["Cub"], nthreads=8)[0:2]


def _sides(Q, x):
    """the active sides read off x, every instance of the batch"""
    p = Q["C"] is not None
    return np.array([wbc_workload.qp_active_sides(x[i], Q["C"][i] if p else None, Q["lb"][i], Q["ub"][i], Q["Clb"][i] if p else None,
                                                  Q["Cub"][i] if p else None)[0] for i in range(len(x))])


EPS = 1e-6


@pytest.mark.parametrize("n,p,n_eq", cc.SHAPES)
def test_sensitivities_against_central_differences_of_the_oracle(n, p, n_eq):
    """-u = (dx/dg) v (the Jacobian is symmetric) and w_j = dL/de_j for L = v'x, by central differences of the oracle's solve with eps = 1e-6.
    An instance is skipped if one of its inequality multipliers is below 1e-4 (the active set is about to change) or if the active set does
    change under +-eps; at most 10 % may be. Error |delta| / max(1, |u|_inf) <= 1e-6: the differences' own noise at cond(H) ~ 1e5."""
    P = cc.random_problem(n, p, n_eq)
    B = len(P["x"])
    v = P["v"]
    cert = cc.host_certificates(P, status=P["status"], v=v)
    side = cert["side"]
    y = np.concatenate([cert["y_bounds"], cert["y_rows"]], axis=1)
    w = np.concatenate([cert["sens_bounds"], cert["sens_rows"]], axis=1)
    ineq = (side == 1) | (side == 2)
    skip = (P["status"] != 0) | (cert["cert_status"] != capi.CERT_OK) | np.array([(np.abs(y[i][ineq[i]]) < 1e-4).any() for i in range(B)])
    # dx/dg . v
    xp, sp = _solve(P, g=P["g"] + EPS * v)
    xm, sm = _solve(P, g=P["g"] - EPS * v)
    skip |= (sp != 0) | (sm != 0) | (_sides(P, xp) != side).any(axis=1) | (_sides(P, xm) != side).any(axis=1)
    scale = np.maximum(1.0, np.abs(cert["sens_x"]).max(axis=1))
    err_u = np.abs((xp - xm) / (2 * EPS) + cert["sens_x"]).max(axis=1) / scale
    # w_j: every active constraint of every instance shifted by +-eps (both sides of an equality), one batch per position in the active list
    lo = np.concatenate([P["lb"]] + ([P["Clb"]] if p else []), axis=1)
    hi = np.concatenate([P["ub"]] + ([P["Cub"]] if p else []), axis=1)
    err_w = np.zeros(B)
    for pos in range(int(cert["n_active"].max())):
        j = np.array([np.nonzero(side[i])[0][pos] if cert["n_active"][i] > pos else -1 for i in range(B)])
        has = j >= 0
        L = []
        for sgn in (+1.0, -1.0):
            l2, h2 = lo.copy(), hi.copy()
            for i in np.nonzero(has)[0]:
                if side[i, j[i]] in (1, 3):
                    l2[i, j[i]] += sgn * EPS
                if side[i, j[i]] in (2, 3):
                    h2[i, j[i]] += sgn * EPS
            x2, s2 = _solve(P, lb=l2[:, :n], ub=h2[:, :n], Clb=l2[:, n:] if p else None, Cub=h2[:, n:] if p else None)
            Q = dict(P, lb=l2[:, :n], ub=h2[:, :n], Clb=l2[:, n:] if p else None, Cub=h2[:, n:] if p else None)
            skip |= has & ((s2 != 0) | (_sides(Q, x2) != side).any(axis=1))
            L.append((x2 * v).sum(axis=1))
        fd = (L[0] - L[1]) / (2 * EPS)
        wj = np.array([w[i, j[i]] if has[i] else 0.0 for i in range(B)])
        err_w = np.maximum(err_w, np.where(has, np.abs(fd - wj) / scale, 0.0))
    print("(%d, %d, %d): skipped %d of %d; worst error of -u %.2e, of w %.2e" % (n, p, n_eq, skip.sum(), B, err_u[~skip].max(), err_w[~skip].max()))
    assert skip.sum() <= B // 10, skip.sum()
    assert err_u[~skip].max() <= 1e-6 and err_w[~skip].max() <= 1e-6, (err_u[~skip].max(), err_w[~skip].max())


def test_gradients_of_H_and_C_along_random_directions():
    """dL/dH and dL/dC of wbc_workload.qp_gradients against central differences along one random direction each, (12, 6, 2)"""
    P = cc.random_problem(12, 6, 2)
    B, n = P["x"].shape
    v = P["v"]
    cert = cc.host_certificates(P, status=P["status"], v=v)
    rng = np.random.default_rng(9)
    dH = rng.normal(size=P["H"].shape)
    dH = dH + dH.transpose(0, 2, 1)
    dC = rng.normal(size=P["C"].shape)
    y = np.concatenate([cert["y_bounds"], cert["y_rows"]], axis=1)
    w = np.concatenate([cert["sens_bounds"], cert["sens_rows"]], axis=1)
    ineq = (cert["side"] == 1) | (cert["side"] == 2)
    skip = (P["status"] != 0) | (cert["cert_status"] != 0) | np.array([(np.abs(y[i][ineq[i]]) < 1e-4).any() for i in range(B)])
    fd = {}
    for name, d in (("H", dH), ("C", dC)):
        L = []
        for sgn in (+1.0, -1.0):
            Q = dict(P, **{name: P[name] + sgn * EPS * d})
            x2, s2 = _solve(Q)
            skip |= (s2 != 0) | (_sides(Q, x2) != cert["side"]).any(axis=1)
            L.append((x2 * v).sum(axis=1))
        fd[name] = (L[0] - L[1]) / (2 * EPS)
    assert skip.sum() <= B // 10
    worst = 0.0
    for i in np.nonzero(~skip)[0]:
        G = wbc_workload.qp_gradients(P["x"][i], y[i], cert["sens_x"][i], w[i], cert["side"][i])
        scale = max(1.0, np.abs(cert["sens_x"][i]).max())
        worst = max(worst, abs((G["H"] * dH[i]).sum() - fd["H"][i]) / scale, abs((G["C"] * dC[i]).sum() - fd["C"][i]) / scale)
        assert np.array_equal(G["g"], -cert["sens_x"][i])
        eq = cert["side"][i] == 3
        glo, ghi = np.concatenate([G["lb"], G["Clb"]]), np.concatenate([G["ub"], G["Cub"]])
        assert np.array_equal(glo[eq], 0.5 * w[i][eq]) and np.array_equal(ghi[eq], 0.5 * w[i][eq]) and np.allclose(glo + ghi, w[i], rtol=0, atol=0)
    print("dL/dH, dL/dC along a random direction: worst error %.2e over %d instances" % (worst, (~skip).sum()))
    assert worst <= 1e-6, worst


def test_golden_qp_cases():
    P = cc.qp_cases()
    cert = cc.host_certificates(P, status=P["status"], v=P["v"])
    by = {nm: i for i, nm in enumerate(P["names"])}
    st = dict(zip(P["names"], cert["cert_status"].tolist()))
    assert st["duplicate_equalities"] == capi.CERT_DEPENDENT
    assert st["contradictory_equalities"] == capi.CERT_UNSOLVED and st["infeasible_box"] == capi.CERT_UNSOLVED
    assert all(st[nm] == capi.CERT_OK for nm in ("unconstrained", "all_bounds_active", "bounds_only", "locked_and_mixed"))
    i = by["unconstrained"]
    assert cert["n_active"][i] == 0 and (cert["y_bounds"][i] == 0).all() and (cert["y_rows"][i] == 0).all()
    assert np.abs(cert["sens_x"][i] - np.linalg.solve(P["H"][i], P["v"][i])).max() <= 1e-9 * np.abs(cert["sens_x"][i]).max()
    i = by["all_bounds_active"]
    assert cert["n_active"][i] == 26 and np.abs(cert["sens_x"][i]).max() <= 1e-12        # the normals span the space: u = 0
    i = by["duplicate_equalities"]                                 # DEPENDENT: violation, objective and k are given, the rest is zero
    assert cert["n_active"][i] > 0 and cert["objective"][i] != 0 and (cert["y_rows"][i] == 0).all() and (cert["sens_x"][i] == 0).all()
    for nm in ("contradictory_equalities", "infeasible_box"):
        assert all((np.asarray(cert[k][by[nm]]) == 0).all() for k in cc.CERT_KEYS if k != "cert_status")
    # a non-finite entry or an indefinite H: NUMERICAL, everything zero
    i = by["bounds_only"]
    kw = cc.instance(P, i)
    Hn = kw["H"].copy()
    Hn[3, 3] = np.nan
    assert wbc_workload.qp_certificate(P["x"][i], **dict(kw, H=Hn))["cert_status"] == capi.CERT_NUMERICAL
    c = wbc_workload.qp_certificate(P["x"][i], **dict(kw, H=-kw["H"]))
    assert c["cert_status"] == capi.CERT_NUMERICAL and c["objective"] == 0 and c["n_active"] == 0 and (c["kkt"] == 0).all()


# ---- the ends of the documented range (the shapes tests/test_gpu_qp_certificate.py sends through the device)
ULP = 2.220446049250313e-16
# (m, n, p, equalities, box) of cert_common.ls_problem, B = 16, seed 200 + m; then n = m = 1 and p = 24 in the (H, g) form. Largest relative error of
# y, u and w against the exact rationals over the first four instances, as measured: 1.68e-15, 1.11e-15, 7.03e-16, 1.76e-15, 1.73e-17, 1.44e-15,
# 3.93e-14 (n = 3: one free variable next to the fixed pair), 1.43e-16, 3.84e-15; the bounds are 10 x those, and 10 ulp where that is less
EDGE = [("ls_96_26_24", lambda: cc.ls_problem(16, 96, 26, 24, 12, 296, True), 1.68e-14), ("ls_49_26_16", lambda: cc.ls_problem(16, 49, 26, 16, 12, 249, True), 1.11e-14),
        ("ls_47_13_5", lambda: cc.ls_problem(16, 47, 13, 5, 2, 247, True), 7.03e-15), ("ls_48_26_17", lambda: cc.ls_problem(16, 48, 26, 17, 8, 248, True), 1.76e-14),
        ("ls_95_26_0_no_box", lambda: cc.ls_problem(16, 95, 26, 0, 0, 295, False), 10 * ULP), ("ls_33_26_24_no_box", lambda: cc.ls_problem(16, 33, 26, 24, 4, 233, False), 1.44e-14),
        ("ls_3_3_0", lambda: cc.ls_problem(16, 3, 3, 0, 0, 203, True), 3.93e-13), ("ls_1_1_0", cc.ls_problem_free_bounds, 10 * ULP),
        ("n26_p24", lambda: cc.random_problem(26, 24, 12, 16), 3.84e-14), ("vertex_30_6", cc.vertex_problem, 4.70e-15)]


@pytest.mark.parametrize("name,make,bound", EDGE, ids=[e[0] for e in EDGE])
def test_restatement_against_exact_rationals_at_the_ends_of_the_range(name, make, bound):
    """every instance solved by the oracle and certified OK with no wrong-signed multiplier, read off x and with the working set given alike; y, u and
    w of the first four against the exact rationals"""
    P = make()
    assert len(P["x"]) == 16 and (P["status"] == 0).all()
    full = cc.host_certificates(P, status=P["status"], v=P["v"])
    assert (full["cert_status"] == capi.CERT_OK).all() and (full["kkt"][:, 2] == 0).all()
    given = cc.host_certificates(P, status=P["status"], working_set=cc.working_sets(P, P["x"]), v=P["v"])
    assert all(np.array_equal(full[k], given[k]) for k in full)
    idx = list(range(4))
    err = cc.restatement_error(P, {k: a[idx] for k, a in full.items()}, idx, P["v"])
    print("%s: y, u, w against the exact rationals, largest relative error %.3e (bound %.1e); active %d..%d" % (
        name, err, bound, full["n_active"].min(), full["n_active"].max()))
    assert err <= bound, err
    if name == "ls_95_26_0_no_box":
        assert (full["n_active"] == 0).all() and (full["y_bounds"] == 0).all() and full["y_rows"].shape == (16, 0)
    if name == "vertex_30_6":                                        # k == n: the normals span the space
        assert (full["n_active"] == 6).all() and np.abs(full["sens_x"]).max() <= 5e-17


def test_more_active_normals_than_variables():
    """k > n: eight equality rows through the origin on five variables. DEPENDENT before any factorisation; violation, objective and k are given"""
    P = cc.overdetermined_problem()
    assert (P["status"] == 0).all()
    for ws in (None, cc.working_sets(P, P["x"])):
        cert = cc.host_certificates(P, status=P["status"], working_set=ws, v=P["v"])
        assert (cert["cert_status"] == capi.CERT_DEPENDENT).all() and (cert["n_active"] == 8).all() and (cert["side"][:, 5:] == 3).all()
        assert all((cert[k] == 0).all() for k in ("y_bounds", "y_rows", "sens_x", "sens_bounds", "sens_rows")) and (cert["kkt"][:, [0, 2, 3]] == 0).all()
        assert np.abs(cert["objective"]).max() <= 1e-25 and np.abs(cert["kkt"][:, 1]).max() <= 1e-25      # x = 0 to rounding
    x = np.full_like(P["x"], 0.1)                                    # away from the feasible point: the two that are still given, at their values
    cert = cc.host_certificates(P, x=x, v=P["v"])
    obj = np.array([0.5 * (A @ xi) @ (A @ xi) - b @ (A @ xi) for A, b, xi in zip(P["A"], P["b"], x)])
    viol = np.abs(np.einsum("bpi,bi->bp", P["C"], x)).max(axis=1)
    assert (cert["cert_status"] == capi.CERT_DEPENDENT).all() and (cert["n_active"] == 8).all() and (viol > 1e-3).all()
    assert np.allclose(cert["objective"], obj, rtol=1e-12, atol=0) and np.allclose(cert["kkt"][:, 1], viol, rtol=1e-12, atol=0)


def test_working_set_rules_of_the_restatement():
    """qp_active_sides / qp_certificate: a bit on an infinite side, bits beyond n and p, both bits at once, equalities whatever their bits, and the
    1e-7 rule that reads the set off x"""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    P = cc.ls_problem(16, 33, 26, 24, 4, 233, False)                                          # no box: every side of every variable is infinite
    ws = cc.working_sets(P, P["x"])
    plain = cc.host_certificates(P, working_set=ws, v=P["v"])
    w2 = ws.copy().view(np.uint64)
    w2[:, 0] = full
    marked = cc.host_certificates(P, working_set=w2.view(np.int64), v=P["v"])
    assert all(np.array_equal(plain[k], marked[k]) for k in plain) and (plain["side"][:, :26] == 0).all()
    i = 0
    kw = cc.instance(P, i)
    inf = dict(lb=np.full(26, -1e20), ub=np.full(26, np.inf))                                  # +-1e20 and beyond: no bound
    side = wbc_workload.qp_active_sides(P["x"][i], kw["C_"], inf["lb"], inf["ub"], kw["Clb"], kw["Cub"], w2.view(np.int64)[i])[0]
    assert np.array_equal(side, plain["side"][i])
    P = cc.ls_problem(16, 47, 13, 5, 2, 247, True)                                            # bits beyond n = 13 and p = 5
    ws = cc.working_sets(P, P["x"])
    plain = cc.host_certificates(P, working_set=ws, v=P["v"])
    w2 = ws.copy().view(np.uint64)
    w2[:, 0] |= np.uint64(((1 << 32) - (1 << 13)) * ((1 << 32) + 1))
    w2[:, 1] |= np.uint64(((1 << 32) - (1 << 5)) * ((1 << 32) + 1))
    marked = cc.host_certificates(P, working_set=w2.view(np.int64), v=P["v"])
    assert all(np.array_equal(plain[k], marked[k]) for k in plain)
    P = cc.random_problem(26, 16, 12)                                                         # both bits; equalities
    x = P["x"]
    ws = cc.working_sets(P, x)
    plain = cc.host_certificates(P, working_set=ws)
    assert all(np.array_equal(plain[k], a) for k, a in cc.host_certificates(P).items())       # (the set read off x is the set given)
    both, none, eq = ws.copy(), ws.copy(), ws.copy()
    hit = np.zeros(len(x), dtype=bool)
    for i in range(len(x)):
        for word, j in [(0, j) for j in range(24)] + [(1, j) for j in range(12, 16)]:
            if cc.ws_bits(ws, i, word, j) in (1, 2):
                cc.ws_set(both, i, word, j, 3)
                cc.ws_set(none, i, word, j, 0)
                hit[i] = True
                break
        for j in (24, 25):
            cc.ws_set(eq, i, 0, j, (0, 3)[j - 24])
        for j in range(12):
            cc.ws_set(eq, i, 1, j, (0, 2, 3, 1)[(i + j) % 4])
    cb, cn, ce = (cc.host_certificates(P, working_set=w) for w in (both, none, eq))
    assert hit.sum() >= len(x) // 2 and np.array_equal(cb["n_active"], plain["n_active"] - hit)
    assert all(np.array_equal(cb[k], cn[k]) for k in cb) and all(np.array_equal(ce[k], plain[k]) for k in ce)
    assert (plain["side"][:, 24:26] == 3).all() and (plain["side"][:, 26:38] == 3).all()
    x2, near, far = cc.near_bounds(P, x, ws)                                                   # the read-off rule
    rows = np.arange(len(x))
    c2 = cc.host_certificates(P, x=x2)
    assert (c2["side"][rows, near] == 1).all() and (c2["side"][rows, far] == 0).all() and (c2["y_bounds"][rows, far] == 0).all()
    ok = c2["cert_status"] == capi.CERT_OK
    assert ok.sum() >= len(x) // 2 and (c2["y_bounds"][rows, near][ok] != 0).all() and np.array_equal(c2["n_active"], (c2["side"] != 0).sum(axis=1))


def test_residuals_of_a_non_optimal_x():
    """x off the optimum three ways (cert_common.off_optimum): the violation and the complementarity product are nonzero on every moved instance, a
    wrong-signed multiplier at every flipped bound and at some of the variables pushed outside"""
    P = cc.random_problem(26, 16, 12)
    ws = cc.working_sets(P, P["x"])
    for way in ("flip", "outside", "shift"):
        x2, ws2, moved = cc.off_optimum(P, P["x"], ws, way)
        k = cc.host_certificates(P, x=x2, working_set=ws2)["kkt"][moved]
        assert moved.sum() >= len(x2) // 2 and (k[:, 1] > 0).all() and (k[:, 3] > 0).all(), way
        assert (k[:, 2] > 0).all() if way == "flip" else (k[:, 2] > 0).any() if way == "outside" else (k[:, 2] == 0).all(), way
