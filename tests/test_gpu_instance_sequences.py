"""GPU: the three grid-stride kernels past a workgroup's first instance. wbc_qp_kernel<NM, WARM> and wbc_integrate_kernel (csrc/wbc_k_misc.hip) and
wbc_qp_cert_kernel (csrc/wbc_k_cert.hip) loop `for (b = blockIdx.x; b < B; b += gridDim.x)` over one __shared__ block, and their grid is
min(B, handle grid) with a handle grid of some thousands: at the batch sizes of the other tests every workgroup serves ONE instance. The option
"grid" (include/wbc.h) makes a workgroup serve many: at 1 one workgroup walks the whole batch in order, 3 and 7 give other predecessor /
successor pairs, and at the default every instance has a workgroup of its own.

Every test asserts two things. (1) The grid = 1 answers against the reference of the operation — the oracle for the QP and for integrate, the
host restatement wbc_workload.qp_certificate for the certificate — at the tolerances of that kernel's existing test (test_gpu_parity.py:
test_qp_packed_edge_cases..., test_integrate_parity; test_gpu_qp_certificate.py: cert_common.compare / tolerance). (2) Every output at every grid
has the bytes of the default-grid output: an instance's answer may not depend on which instances its workgroup served before it. Every test makes
its own handle ("grid" is per handle)."""
import functools

import numpy as np
import pytest

import cert_common as cc
import devguard
import oracle
import wbc_capi as capi
import wbc_model
import wbc_workload
from wbc_batch import WbcBatch

pytestmark = pytest.mark.gpu
GRIDS = (1, 3, 7)
B = 67
DT = 0.002


def _same_at_every_grid(bt, run, what):
    """run() at the default grid, then at 1, 3 and 7: all four have the same bytes. -> the grid = 1 result"""
    default = run()
    first = None
    for grid in GRIDS:
        bt.set_option("grid", grid)
        got = run()
        first = got if first is None else first
        for k in default:
            assert devguard.same_bytes(got[k], default[k]), "%s: %s at grid %d differs from the default grid's, first at instance %d" % (
                what, k, grid, _first_difference(got[k], default[k]))
    return first


def _first_difference(a, b):
    a, b = (np.ascontiguousarray(t).reshape(len(t), -1).view(np.uint8) for t in (a, b))
    return int(np.argmax((a != b).any(axis=1)))


# ------------------------------------------------------------------------------------------------ the one-per-wavefront QP kernel
@functools.lru_cache(maxsize=None)
def _mixed_fates(n, p, m):
    """the recipe of test_gpu_parity.test_qp_packed_edge_cases_agree_with_the_oracle_and_the_one_per_wavefront_kernel, restated (seed by shape): instances
    of eight kinds side by side — plain, infeasible against the box, contradictory equalities, a redundant equality, (p > n: more equality rows than
    unknowns, through the origin), H = 0, a NaN bound, nothing active but rows — with the oracle's answers in both forms"""
    rng = np.random.default_rng(1000 * n + m)
    A = rng.normal(size=(B, m, n))
    b = rng.normal(size=(B, m))
    C = rng.normal(size=(B, p, n))
    lb, ub = -rng.uniform(0.3, 1.0, (B, n)), rng.uniform(0.3, 1.0, (B, n))
    cl, cu = -rng.uniform(0.3, 1.0, (B, p)), rng.uniform(0.3, 1.0, (B, p))
    kinds = np.arange(B) % 8
    cl[kinds == 1, 0], cu[kinds == 1, 0] = 50.0, 60.0
    C[kinds == 2, 1] = C[kinds == 2, 0]
    cl[kinds == 2, 0] = cu[kinds == 2, 0] = 0.1
    cl[kinds == 2, 1] = cu[kinds == 2, 1] = -0.1
    C[kinds == 3, 1] = 2.0 * C[kinds == 3, 0]
    cl[kinds == 3, 0] = cu[kinds == 3, 0] = 0.05
    cl[kinds == 3, 1] = cu[kinds == 3, 1] = 0.1
    if p > n:
        cl[kinds == 4] = cu[kinds == 4] = 0.0
    A[kinds == 5] = 0.0
    lb[kinds == 6, 0] = np.nan
    lb[kinds == 7], ub[kinds == 7] = -1e3, 1e3
    d = dict(A=A, b=b, C=C, lb=lb, ub=ub, Clb=cl, Cub=cu, H=np.einsum("bmi,bmj->bij", A, A), g=-np.einsum("bmi,bm->bi", A, b))
    d["ls"] = oracle.qp_solve_ls(A, b, C, lb, ub, cl, cu, nthreads=8)
    d["hg"] = oracle.qp_solve(d["H"], d["g"], C, lb, ub, cl, cu, nthreads=8)
    for a in list(d.values()) + list(d["ls"]) + list(d["hg"]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


# name, (n, p, m), form, use_mfma, hot start, the kernel's (NM, WARM). One shape per compiled core size (launch_qp: the smallest of 12 / 16 / 24 / 26 that
# holds n; 16 or 26 with working sets); the (A, b) form on the matrix cores and on the vector path, there with m = 96 (two full 48-row chunks) and m = 49
# (a second chunk of one odd row)
QP_CASES = [("hg_n8", (8, 10, 20), "hg", None, False, (12, 0)), ("hg_n14", (14, 9, 20), "hg", None, False, (16, 0)),
            ("hg_n20", (20, 12, 40), "hg", None, False, (24, 0)), ("hg_n26", (26, 24, 49), "hg", None, False, (26, 0)),
            ("ls_n8_m20_vector", (8, 10, 20), "ls", 0, False, (12, 0)), ("ls_n14_m20_vector", (14, 9, 20), "ls", 0, False, (16, 0)),
            ("ls_n14_m20_mfma", (14, 9, 20), "ls", 1, False, (16, 0)), ("ls_n20_m40_mfma", (20, 12, 40), "ls", 1, False, (24, 0)),
            ("ls_n20_m49_vector", (20, 12, 49), "ls", 0, False, (24, 0)), ("ls_n26_m96_vector", (26, 24, 96), "ls", 0, False, (26, 0)),
            ("ls_n26_m49_vector", (26, 24, 49), "ls", 0, False, (26, 0)), ("ls_n26_m96_mfma", (26, 24, 96), "ls", 1, False, (26, 0)),
            ("hg_n14_hot", (14, 9, 20), "hg", None, True, (16, 1)), ("ls_n26_m49_vector_hot", (26, 24, 49), "ls", 0, True, (26, 1)),
            ("ls_n14_m20_mfma_hot", (14, 9, 20), "ls", 1, True, (16, 1))]


@pytest.mark.parametrize("name,shape,form,mfma,hot,variant", QP_CASES, ids=[c[0] for c in QP_CASES])
def test_one_per_wavefront_qp_kernel(name, shape, form, mfma, hot, variant):
    """x, status, iters (and H_out, g_out in the (A, b) form; the working sets when hot-started, seeded with the cold run's own sets)"""
    n, p, m = shape
    d = _mixed_fates(n, p, m)
    xr, sr, ir = d[form]
    ok = sr == 0
    assert len(set(sr.tolist())) >= 2 and ok.sum() >= B // 4 and (xr[~ok] == 0).all()
    con = (d["C"], d["lb"], d["ub"], d["Clb"], d["Cub"])
    bt = WbcBatch([], B)
    try:
        bt.set_option("packed_kernel", 0)

        def run(seeds=None, want=False):
            if form == "hg":
                r = bt.qp_solve(d["H"], d["g"], *con, working_set=seeds, want_working_set=want)
                out = dict(zip(("x", "status", "iters", "working_set"), r))
            else:
                r = bt.qp_solve_ls(d["A"], d["b"], *con, use_mfma=bool(mfma), want_Hg=True, working_set=seeds, want_working_set=want)
                out = dict(zip(("x", "status", "iters", "H_out", "g_out", "working_set"), r))
            assert bt.stat("last_qp_path") == 1 and capi.variant_args(bt.stat("last_qp_variant"), 2) == variant
            return out
        seeds = run(want=True)["working_set"] if hot else None
        got = _same_at_every_grid(bt, (lambda: run(seeds, True)) if hot else run, name)
    finally:
        bt.close()
    assert np.array_equal(got["status"], sr), (np.nonzero(got["status"] != sr), got["status"][got["status"] != sr], sr[got["status"] != sr])
    assert (got["x"][~ok] == 0).all()
    err = np.abs(got["x"] - xr)[ok].max()
    print("%s: |x - x_oracle| at most %.2e on %d solved of %d, statuses %s" % (name, err, ok.sum(), B, sorted(set(sr.tolist()))))
    assert err < 1e-8, err
    if hot:
        assert (got["working_set"][~ok] == 0).all() and (got["working_set"][ok] != 0).any()
    else:
        assert (got["iters"][ok] == ir[ok]).all(), np.nonzero(ok & (got["iters"] != ir))
    if form == "ls":                                               # test_qp_ls_forms_H_and_g's figure
        rel = lambda a, r: np.abs(a - r).max() / max(1.0, np.abs(r).max())
        assert rel(got["H_out"], d["H"]) < 1e-13 and rel(got["g_out"], d["g"]) < 1e-13


# ------------------------------------------------------------------------------------------------ the certificate kernel
OK, UNSOLVED, DEP_QR, DEP_K, NUM_NAN, NUM_CHOL = range(6)
# 37 instances: every ordered pair of the six fates (a fate after itself included) is adjacent once — an Euler circuit of the complete directed graph
FATES = [0, 5, 5, 4, 5, 3, 5, 2, 5, 1, 5, 0, 4, 4, 3, 4, 2, 4, 1, 4, 0, 3, 3, 2, 3, 1, 3, 0, 2, 2, 1, 2, 0, 1, 1, 0, 0]
EXPECT = {OK: capi.CERT_OK, UNSOLVED: capi.CERT_UNSOLVED, DEP_QR: capi.CERT_DEPENDENT, DEP_K: capi.CERT_DEPENDENT, NUM_NAN: capi.CERT_NUMERICAL,
          NUM_CHOL: capi.CERT_NUMERICAL}
ZERO_ALWAYS = ("y_bounds", "y_rows", "sens_x", "sens_bounds", "sens_rows")        # include/wbc.h, WBC_CERT_*: zero unless OK
EXACT_N = 4


@pytest.mark.parametrize("form", ["hg", "ls"])
def test_certificate_kernel(form):
    """(H, g) at (n, p) = (26, 16) and (A, b) at (m, n, p) = (49, 26, 16), 12 equality rows, solved by the device; then instances are edited into the
    six ways the kernel leaves an instance: OK; UNSOLVED (a status passed in) before any LDS write; DEPENDENT at the QR tolerance (an equality
    row duplicated onto another); DEPENDENT at k > n (a working set that marks all 26 variables next to the 12 equalities); NUMERICAL after
    staging (a NaN in H or A); NUMERICAL inside the Cholesky (H negated, A = 0). With v given."""
    assert len(FATES) == 37 and {(a, b) for a, b in zip(FATES, FATES[1:])} == {(a, b) for a in range(6) for b in range(6)}
    fate = np.array(FATES)
    n = 26
    P0 = cc.random_problem(26, 16, 12, len(FATES)) if form == "hg" else cc.ls_problem(len(FATES), 49, 26, 16, 12, 249)
    M = "H" if form == "hg" else "A"
    bt = WbcBatch([], len(FATES))
    try:
        if form == "hg":
            x, st, _, ws = bt.qp_solve(P0["H"], P0["g"], P0["C"], P0["lb"], P0["ub"], P0["Clb"], P0["Cub"], want_working_set=True)
        else:
            x, st, _, ws = bt.qp_solve_ls(P0["A"], P0["b"], P0["C"], P0["lb"], P0["ub"], P0["Clb"], P0["Cub"], want_working_set=True)
        assert np.array_equal(st, P0["status"]) and (st == 0).all()
        P = {k: (np.array(a) if isinstance(a, np.ndarray) else a) for k, a in P0.items()}
        st, ws = st.copy(), ws.copy()
        st[fate == UNSOLVED] = capi.QP_INFEASIBLE
        P["C"][fate == DEP_QR, 1] = P["C"][fate == DEP_QR, 0]        # (the row keeps its own bounds: still an equality, now violated)
        ws.view(np.uint64)[fate == DEP_K, 0] = np.uint64((1 << n) - 1)
        P[M][fate == NUM_CHOL] = -P[M][fate == NUM_CHOL] if form == "hg" else 0.0
        finite = dict(P)                                           # (for the scales of the comparison: the data before the NaN goes in)
        finite[M] = P[M].copy()
        P[M][fate == NUM_NAN, 7, 4] = np.nan
        v = P["v"]
        host = cc.host_certificates(P, x=x, status=st, working_set=ws, v=v)
        assert np.array_equal(host["cert_status"], [EXPECT[f] for f in FATES])
        assert (host["n_active"][fate == DEP_K] >= 38).all() and (host["n_active"][fate == DEP_QR] <= n).all() and (host["n_active"][fate == OK] > 12).all()
        got = _same_at_every_grid(bt, lambda: bt.qp_certificate(x, **cc.kw(P, x, st, ws, v)), "certificate, " + form)
    finally:
        bt.close()
    tol, err = cc.tolerance(P, host, v, EXACT_N)
    worst = cc.compare(got, host, finite, x, tol, "certificate, %s, grid 1" % form)
    print("certificate (%s): restatement against exact rationals %.2e, device at grid 1 against restatement at most %.2f of the allowed %.2e" % (
        form, err, worst, tol))
    assert np.array_equal(got["cert_status"], [EXPECT[f] for f in FATES])
    for k, a in got.items():
        a = np.asarray(a, dtype=np.float64)
        assert np.isfinite(a).all(), k
        if k in ZERO_ALWAYS:
            assert (a[fate != OK] == 0).all(), k
        elif k != "cert_status":                                   # kkt, objective, n_active: all zero but for DEPENDENT's kkt[1], objective and k
            assert (a[np.isin(fate, (UNSOLVED, NUM_NAN, NUM_CHOL))] == 0).all(), k
    dep = np.isin(fate, (DEP_QR, DEP_K))
    assert (got["kkt"][dep][:, [0, 2, 3]] == 0).all() and (got["objective"][dep] != 0).all() and (got["n_active"][dep] > 12).all()
    assert (got["kkt"][fate == DEP_QR, 1] > 0).all()               # (the duplicated row keeps its own C x: violated)
    assert (got["y_rows"][fate == OK] != 0).any(axis=1).all() and (got["sens_x"][fate == OK] != 0).any(axis=1).all()


# ------------------------------------------------------------------------------------------------ the integrate kernel
def test_integrate_kernel():
    """a1_wx200, a1_px100 and laikago_vx300 interleaved by model_id (their nq and nv differ: what one instance writes, the next one's padding must not
    show), the first eight instances small-angle; then the x 300 velocities of test_integrate_parity (every quaternion branch). 1e-13 / 1e-12 as there."""
    models = [wbc_model.load_model(nm) for nm in ("a1_wx200", "a1_px100_pin_ver", "laikago_vx300")]
    rng = np.random.default_rng(9)
    mid = (np.arange(B) % 3).astype(np.int32)
    qs = [wbc_workload.sample_q(mdl, B, rng) for mdl in models]
    q = np.ascontiguousarray(np.where(mid[:, None] == 0, qs[0], np.where(mid[:, None] == 1, qs[1], qs[2])))
    v = rng.normal(size=(B, 26)) * 2
    v[:8, 3:6] = 0
    big = rng.normal(size=(B, 26)) * 300
    assert len({(mdl.nq, mdl.nv) for mdl in models}) >= 2
    # on device memory, outputs pre-filled with NaN: a padding entry that a later instance of a workgroup left unwritten would show
    import torch
    nan_filled = lambda like, shape, dtype: torch.full(shape, float("nan"), dtype=torch.float64, device=like.device)
    qd, midd = torch.from_numpy(q).cuda(), torch.from_numpy(mid).cuda()
    for what, vel, bound in (("v", v, 1e-13), ("300 v", big, 1e-12)):
        ref = oracle.integrate(models, q, vel, DT, mid)
        veld = torch.from_numpy(vel).cuda()
        bt = WbcBatch(models, B, allocator=nan_filled)             # (a handle per call: each starts from the default grid)
        try:
            got = _same_at_every_grid(bt, lambda: dict(q_next=bt.integrate(qd, veld, DT, midd).cpu().numpy()), "integrate, " + what)["q_next"]
        finally:
            bt.close()
        assert np.isfinite(got).all()
        err = np.abs(got - ref).max()
        print("integrate (%s): |q_next - oracle| at most %.2e" % (what, err))
        assert err < bound, err
