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
