"""Shared by tests/test_qp_certificate_host.py and tests/test_gpu_qp_certificate.py: the problems (random QPs by the recipe of
test_gpu_parity._random_qps, restated; the oracle's tick problems; tests/golden/qp_cases.npz), the host restatement over a batch, and the exact
rational duals and sensitivities the restatement is measured against. Everything computed here is computed once and read-only."""
import functools
import os

import numpy as np

import common
import oracle
import wbc_capi as capi
import wbc_workload

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(26, 16, 12), (25, 10, 4), (12, 6, 2), (26, 0, 0), (3, 2, 0)]          # n, p, equalities among the rows
CERT_KEYS = ("y_bounds", "y_rows", "kkt", "objective", "n_active", "cert_status", "sens_x", "sens_bounds", "sens_rows")
PROBLEM_KEYS = ("H", "g", "A", "b", "C", "lb", "ub", "Clb", "Cub")
DT = 0.002


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def random_qps(rng, B, n, p, n_eq, fixed_value=0.0):
    """test_gpu_parity._random_qps, restated"""
    A = rng.normal(size=(B, n + 6, n))
    H = np.einsum("bmi,bmj->bij", A, A) + 1e-3 * np.eye(n)
    g = rng.normal(size=(B, n)) * 4
    C = rng.normal(size=(B, p, n))
    lb, ub = -rng.uniform(0.02, 0.8, (B, n)), rng.uniform(0.02, 0.8, (B, n))
    lb[:, -2:] = fixed_value
    ub[:, -2:] = fixed_value
    cl, cu = -rng.uniform(0.02, 0.8, (B, p)), rng.uniform(0.02, 0.8, (B, p))
    cl[:, :n_eq] = cu[:, :n_eq] = rng.normal(size=(B, n_eq)) * 0.1
    return H, g, C, lb, ub, cl, cu


def oracle_solve(P):
    """the oracle's answer to a problem dict: (x, status)"""
    if P.get("A") is not None:
        x, st, _ = oracle.qp_solve_ls(P["A"], P["b"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], nthreads=8)
    else:
        x, st, _ = oracle.qp_solve(P["H"], P["g"], P["C"], P["lb"], P["ub"], P["Clb"], P["Cub"], nthreads=8)
    return x, st


@functools.lru_cache(maxsize=None)
def random_problem(n, p, n_eq, B=64):
    """the (H, g) problems of shape (n, p, n_eq), seed 100 + n, with the oracle's answers and a direction v per instance"""
    rng = np.random.default_rng(100 + n)
    H, g, C, lb, ub, cl, cu = random_qps(rng, B, n, p, n_eq)
    P = dict(H=H, g=g, C=C if p else None, lb=lb, ub=ub, Clb=cl if p else None, Cub=cu if p else None)
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def ls_problem(B=64, m=32, n=26, p=16, n_eq=12):
    """the (A, b) form: random_qps' constraints around a least-squares objective of m rows (seed 132)"""
    rng = np.random.default_rng(132)
    _, _, C, lb, ub, cl, cu = random_qps(rng, B, n, p, n_eq)
    P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)) * 2, C=C, lb=lb, ub=ub, Clb=cl, Cub=cu)
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def tick_problem(name, B=48, seed=7):
    """the oracle's tick problems of configuration `name` (common.tick_inputs, seed 7): assemble's A, b, C, bounds and tick's qdot, status"""
    model = common.models()[0]
    cfg = common.config(name, model)
    d = common.tick_inputs(model, cfg, B, seed)
    a = oracle.assemble([model], [cfg], d, DT, B)
    t = oracle.tick([model], [cfg], d, DT, B, want_q_next=False)
    P = dict(A=a["A"], b=a["b"], C=a["C"], lb=a["lb"], ub=a["ub"], Clb=a["Clb"], Cub=a["Cub"], x=t["qdot"], status=t["status"],
             g=a["g"], inputs=d)
    _freeze(P["inputs"])
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def qp_cases():
    z = np.load(os.path.join(HERE, "golden", "qp_cases.npz"))
    P = {k: z[k] for k in ("H", "g", "C", "lb", "ub", "Clb", "Cub", "x", "status")}
    P["names"] = [str(s) for s in z["names"]]
    P["v"] = np.random.default_rng(5).normal(size=P["g"].shape)
    return _freeze(P)


def instance(P, i):
    """problem i of a batch as the keyword arguments of wbc_workload.qp_certificate"""
    kw = {("C_" if k == "C" else k): P[k][i] for k in PROBLEM_KEYS if P.get(k) is not None}
    if "A" in kw:
        kw.pop("H", None), kw.pop("g", None)
    return kw


def host_certificates(P, x=None, status=None, working_set=None, v=None, idx=None):
    """wbc_workload.qp_certificate over the batch (or the instances idx) -> dict of stacked arrays, `side` included"""
    x = P["x"] if x is None else x
    idx = range(len(x)) if idx is None else idx
    rows = [wbc_workload.qp_certificate(x[i], status=None if status is None else status[i], working_set=None if working_set is None else working_set[i],
                                        v=None if v is None else v[i], **instance(P, i)) for i in idx]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def exact_kkt_int(H, g, rows, rhs):
    """common.exact_kkt's system  H x + N'lam = -g,  N x = rhs  solved as exactly, an order of magnitude faster: every row is scaled to
    integers (the data are doubles, or rationals with power-of-two denominators), fraction-free Bareiss elimination, and rationals only in
    the back substitution. The same unique solution, rounded to doubles once at the end; test_qp_certificate_host.py holds the two to
    identical bits. Returns (x, lam) as floats."""
    import math
    from fractions import Fraction
    n, p = len(g), len(rhs)
    N = n + p
    M = [[Fraction(0)] * (N + 1) for _ in range(N)]
    for i in range(n):
        for j in range(n):
            M[i][j] = Fraction(H[i][j])
        for j in range(p):
            M[i][n + j] = M[n + j][i] = Fraction(float(rows[j][i]))
        M[i][N] = -Fraction(g[i])
    for j in range(p):
        M[n + j][N] = Fraction(float(rhs[j]))
    Z = []
    for r in M:
        d = 1
        for a in r:
            d = d * a.denominator // math.gcd(d, a.denominator)
        Z.append([int(a * d) for a in r])
    prev = 1
    for c in range(N):
        piv = next((r for r in range(c, N) if Z[r][c] != 0), None)
        assert piv is not None, "active rows are dependent"
        Z[c], Z[piv] = Z[piv], Z[c]
        pc = Z[c]
        pcc = pc[c]
        for r in range(c + 1, N):
            rr = Z[r]
            f = rr[c]
            Z[r] = [0] * (c + 1) + [(pcc * rr[j] - f * pc[j]) // prev for j in range(c + 1, N + 1)]
        prev = pcc
    sol = [Fraction(0)] * N
    for i in reversed(range(N)):
        sol[i] = Fraction(Z[i][N] - sum(Z[i][j] * sol[j] for j in range(i + 1, N))) / Z[i][i]
    sol = [float(v) for v in sol]
    return np.array(sol[:n]), np.array(sol[n:])


def exact_solution(P, i, side, v=None, solver=None):
    """For instance i with the active sides `side`: the exact rational KKT solution on the double-precision data (H, g in rationals from A, b in
    the least-squares form), by `solver` (common.exact_kkt or, the default, exact_kkt_int). -> (x, y [n + p] in qpOASES' sign, u, w [n + p]);
    u, w None without v."""
    solver = solver or exact_kkt_int
    kw = instance(P, i)
    n = len(P["x"][i])
    if "A" in kw:
        H, g = common.exact_normal_equations(kw["A"], kw["b"])
    else:
        H, g = kw["H"], kw["g"]
    C = kw.get("C_")
    Nall = np.vstack([np.eye(n)] + ([C] if C is not None else []))
    lo = np.concatenate([kw["lb"]] + ([kw["Clb"]] if C is not None else []))
    hi = np.concatenate([kw["ub"]] + ([kw["Cub"]] if C is not None else []))
    act = np.nonzero(side)[0]
    e = np.where(side == 2, hi, lo)[act]
    x, lam = solver(H, g, Nall[act], e)                        # H x + g + N'lam = 0: y = -lam
    y = np.zeros(len(side))
    y[act] = -lam
    u = w = None
    if v is not None:                                          # H u + N'w = v, N u = 0
        u, wl = solver(H, [-float(t) for t in v], Nall[act], np.zeros(len(act)))
        w = np.zeros(len(side))
        w[act] = wl
    return x, y, u, w


def rel_err(a, ref, floor=0.0):
    """largest entry of |a - ref| relative to the largest entry of |ref| (to `floor` where ref is smaller: 1.0 for the sensitivities, whose exact
    value is 0 when the active normals span the space)"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = float(np.abs(a - ref).max(initial=0.0))
    s = max(floor, float(np.abs(ref).max(initial=0.0)))
    return d / s if s > 0 else d


def restatement_error(P, cert, idx, v=None, solver=None):
    """the host restatement's own error against the exact rationals over the instances idx (positions in `cert`), the certified ones: the largest
    relative error of y (and, with v, of u and w relative to max(1, |.|)) -> float"""
    worst = 0.0
    for j, i in enumerate(idx):
        if cert["cert_status"][j] != capi.CERT_OK:
            continue
        _, y, u, w = exact_solution(P, i, cert["side"][j], None if v is None else v[i], solver)
        worst = max(worst, rel_err(np.concatenate([cert["y_bounds"][j], cert["y_rows"][j]]), y))
        if v is not None:
            worst = max(worst, rel_err(cert["sens_x"][j], u, 1.0), rel_err(np.concatenate([cert["sens_bounds"][j], cert["sens_rows"][j]]), w, 1.0))
    return worst
