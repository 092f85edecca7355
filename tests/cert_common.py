"""Shared by tests/test_qp_certificate_host.py, tests/test_gpu_qp_certificate.py and tests/test_gpu_instance_sequences.py: the problems (random QPs by the recipe of
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
def ls_problem(B=64, m=32, n=26, p=16, n_eq=12, seed=132, box=True):
    """the (A, b) form: random_qps' constraints around a least-squares objective of m rows. box=False: lb = ub = None (no bounds, so no fixed
    pair either); p = 0: no rows"""
    rng = np.random.default_rng(seed)
    _, _, C, lb, ub, cl, cu = random_qps(rng, B, n, p, n_eq)
    P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)) * 2, C=C if p else None, lb=lb if box else None, ub=ub if box else None,
             Clb=cl if p else None, Cub=cu if p else None)
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def ls_problem_free_bounds(B=16, m=1, n=1, seed=211):
    """the (A, b) form with a box none of whose variables is fixed and no rows: the recipe for n = 1, where random_qps' fixed pair would leave
    nothing to solve"""
    rng = np.random.default_rng(seed)
    P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)) * 2, C=None, lb=-rng.uniform(0.02, 0.8, (B, n)), ub=rng.uniform(0.02, 0.8, (B, n)),
             Clb=None, Cub=None)
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def vertex_problem(B=16, m=30, n=6, seed=307):
    """k == n: a tight box (half-widths 0.02 .. 0.05) around a least-squares objective whose b is scaled by 20 — every variable ends at a bound,
    the active normals span the space and u = 0"""
    rng = np.random.default_rng(seed)
    P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)) * 20, C=None, lb=-rng.uniform(0.02, 0.05, (B, n)), ub=rng.uniform(0.02, 0.05, (B, n)),
             Clb=None, Cub=None)
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


@functools.lru_cache(maxsize=None)
def overdetermined_problem(B=16, m=12, n=5, p=8, seed=1258):
    """k > n: p = 8 equality rows through the origin on n = 5 variables inside the box +-1 — x = 0 is the one feasible point, the oracle solves
    it, and the eight always-active rows are more normals than variables"""
    rng = np.random.default_rng(seed)
    P = dict(A=rng.normal(size=(B, m, n)), b=rng.normal(size=(B, m)) * 2, C=rng.normal(size=(B, p, n)), lb=-np.ones((B, n)), ub=np.ones((B, n)),
             Clb=np.zeros((B, p)), Cub=np.zeros((B, p)))
    P["x"], P["status"] = oracle_solve(P)
    P["v"] = rng.normal(size=(B, n))
    return _freeze(P)


def working_sets(P, x):
    """[B, 2] int64 in the layout of include/wbc.h (word 0 the variables, word 1 the rows; bit i a lower side, bit 32 + i an upper side) from the
    sides read off x; an equality is marked at its lower side"""
    B, n = x.shape
    ws = np.zeros((B, 2), dtype=np.uint64)
    for i in range(B):
        kw_ = instance(P, i)
        side = wbc_workload.qp_active_sides(x[i], kw_.get("C_"), kw_.get("lb"), kw_.get("ub"), kw_.get("Clb"), kw_.get("Cub"))[0]
        for j, s in enumerate(side):
            word, bit = (0, j) if j < n else (1, j - n)
            if s:
                ws[i, word] |= np.uint64(1 << (bit + (32 if s == 2 else 0)))
    return ws.view(np.int64)


def ws_bits(ws, i, word, j):
    """(lower | upper << 1) of constraint j in word `word` of instance i"""
    w = int(ws.view(np.uint64)[i, word])
    return ((w >> j) & 1) | (((w >> (32 + j)) & 1) << 1)


def ws_set(ws, i, word, j, bits):
    """set the two bits of constraint j (ws: a writable [B, 2] int64)"""
    u = ws.view(np.uint64)
    w = int(u[i, word]) & ~((1 << j) | (1 << (32 + j)))
    u[i, word] = np.uint64(w | ((bits & 1) << j) | (((bits >> 1) & 1) << (32 + j)))


def off_optimum(P, x, ws, way):
    """x and working set moved off the optimum, one variable per instance among those with lb < ub: "flip" — the first variable the working set
    has at a bound goes to its other bound, and the working set says so; "outside" — the first variable the working set leaves free goes 1e-3
    past its upper bound; "shift" — that variable moves by 1e-4 and stays inside. -> (x, ws, moved [B] bool)"""
    x2, ws2 = np.array(x), np.array(ws)
    B, n = x.shape
    moved = np.zeros(B, dtype=bool)
    for i in range(B):
        for j in range(n):
            if P["lb"][i, j] == P["ub"][i, j]:
                continue
            bits = ws_bits(ws, i, 0, j)
            if way == "flip" and bits in (1, 2):
                x2[i, j] = P["ub"][i, j] if bits == 1 else P["lb"][i, j]
                ws_set(ws2, i, 0, j, 3 - bits)
            elif way == "outside" and bits == 0:
                x2[i, j] = P["ub"][i, j] + 1e-3
            elif way == "shift" and bits == 0 and P["ub"][i, j] - x[i, j] > 2e-4:
                x2[i, j] = x[i, j] + 1e-4
            else:
                continue
            moved[i] = True
            break
    return x2, ws2, moved


def near_bounds(P, x, ws):
    """for the rule that reads the active set off x (|x - lo| < 1e-7 max(1, |lo|)): per instance two variables with lb < ub — those the working
    set has at their lower bound first, then the free ones — are placed at lo + 0.5e-7 max(1, |lo|) (active) and lo + 2e-7 max(1, |lo|) (not).
    -> (x, near [B], far [B])"""
    x2 = np.array(x)
    B, n = x.shape
    near, far = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for i in range(B):
        free = [j for j in range(n) if P["lb"][i, j] < P["ub"][i, j]]
        order = sorted(free, key=lambda j: {1: 0, 0: 1}.get(ws_bits(ws, i, 0, j), 2))
        near[i], far[i] = order[0], order[1]
        for j, f in ((near[i], 0.5e-7), (far[i], 2e-7)):
            x2[i, j] = P["lb"][i, j] + f * max(1.0, abs(P["lb"][i, j]))
    return x2, near, far


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
    lo = np.concatenate([kw.get("lb", np.full(n, -1e30))] + ([kw["Clb"]] if C is not None else []))     # (no box: no bounds, never active)
    hi = np.concatenate([kw.get("ub", np.full(n, 1e30))] + ([kw["Cub"]] if C is not None else []))
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


# ---- device against restatement (tests/test_gpu_qp_certificate.py, whose docstring states the tolerance rule; tests/test_gpu_instance_sequences.py)
EXACT_N = 6
ULP = 2.220446049250313e-16


def kw(P, x, st=None, ws=None, v=None):
    """the keyword arguments of WbcBatch.qp_certificate for the problems P"""
    d = dict(C_=P["C"], lb=P["lb"], ub=P["ub"], Clb=P["Clb"], Cub=P["Cub"], status=st, working_set=ws, v=v)
    d.update(dict(A=P["A"], b=P["b"]) if P.get("A") is not None else dict(H=P["H"], g=P["g"]))
    return d


def grad_terms(P, x, yb, yr):
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


def tolerance(P, host, v, exact_n=EXACT_N):
    """(ten times the restatement's error against the exact rationals over the first exact_n certified instances, never below ten ulp; that error)"""
    idx = [i for i in range(len(host["cert_status"])) if host["cert_status"][i] == capi.CERT_OK][:exact_n]
    sub = {k: a[idx] for k, a in host.items()}
    err = restatement_error(P, sub, idx, v)
    return 10.0 * max(err, ULP), err


def compare(dev, host, P, x, tol, what, only_kkt=False):
    """every output of the device against the restatement (only_kkt: the four residuals alone); returns the largest ratio error / tolerance seen"""
    assert np.array_equal(dev["n_active"], host["n_active"]), (what, np.nonzero(dev["n_active"] != host["n_active"]))
    assert np.array_equal(dev["cert_status"], host["cert_status"]), (what, dev["cert_status"], host["cert_status"])
    B = len(x)
    cat = lambda d, a, b: np.concatenate([d[a], d[b]], axis=1)
    yd, yh = cat(dev, "y_bounds", "y_rows"), cat(host, "y_bounds", "y_rows")
    ymax = np.abs(yh).max(axis=1, initial=0.0)
    terms = grad_terms(P, x, host["y_bounds"], host["y_rows"])
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
