"""Shared by test_track_grad_host.py and test_gpu_track_grad.py: deliberately built tracks that reach every branch of the track evaluation,
the three tracks of the sweep tests (a gripper track, HERMITE with default tangents; a foot track, LINEAR; a trunk track, HERMITE with the
caller's tangents), the oracle's chain of K ticks with the followed rows overwritten per tick by wbc_workload.track_targets, and central
differences of that chain under test_step_grad_host.chain_directional's own tolerance rule and cap."""
import numpy as np

import oracle
import step_common as sc
import test_tick_grad_q_host as tq
import wbc_capi as capi
import wbc_workload

EPS = np.finfo(np.float64).eps
S = 4
TRUNK = capi.TARGET_TRUNK


# ---- deliberately built milestones: every branch of the evaluation and of the default-tangent rule, far from every branch boundary
# per component (a, x, b) = milestones 0, 1, 2: the case the rule takes at milestone 1 (include/wbc.h), every inequality by at least 0.2
CASE = {1: (0.0, 2.0, 1.0), 2: (0.0, 0.3, 3.0), 3: (0.0, 2.8, 3.0), 4: (0.0, 1.5, 3.0), -2: (3.0, 2.7, 0.0), -3: (3.0, 0.2, 0.0), -4: (3.0, 1.4, 0.0)}


def built_tracks():
    """-> dict(points [B, S, 3], n_points [B], du [B], cases [B, 3] (the case at milestone 1, 0 where n = 2), knot [B] (every tick on a knot),
    clamped [B] (every tick clamped)). B = 8, S = 4"""
    rows = [  # (n, du, cases of the three components at milestone 1, milestone 3)
        (2, 0.3, None, None),
        (3, 0.37, (1, 2, 3), None),
        (4, 0.41, (4, -2, -3), (5.0, -2.0, 1.0)),
        (4, 0.5, (2, 3, 4), (4.0, 4.5, 2.0)),          # du = 0.5: every second tick lands exactly on a knot
        (3, 5.0, (4, 1, -4), None),                    # every tick clamped: tick 0 at the first milestone, the others at the last
        (4, 0.29, (-4, 4, 2), (-1.0, 6.0, 3.5)),
        (3, 0.5, (3, -3, -2), None),
        (2, 0.5, None, None),
    ]
    B = len(rows)
    pts, n, du, cases = np.zeros((B, S, 3)), np.zeros(B, np.int32), np.zeros(B), np.zeros((B, 3), np.int64)
    for b, (nb, dub, cs, last) in enumerate(rows):
        n[b], du[b] = nb, dub
        if cs is None:
            pts[b, 0], pts[b, 1] = (0.5, -1.0, 2.0), (1.5, 0.7, -0.4)
        else:
            cases[b] = cs
            for c, case in enumerate(cs):
                pts[b, 0:3, c] = CASE[case]
            if last is not None:
                pts[b, 3] = last
        pts[b, nb:] = 77.0 + b                          # beyond n_points: never read
    return dict(points=pts, n_points=n, du=du, cases=cases, knot=np.array([r[1] == 0.5 for r in rows]), clamped=np.array([r[1] >= 3.0 for r in rows]))


def loss_of_tracks(points, n_points, du, K, kind, tangents, e):
    """sum_k e[k] . track_targets(k) per instance [B], and sum_k |e[k]| . |track_targets(k)| (the scale of its rounding)"""
    val, scale = np.zeros(len(points)), np.zeros(len(points))
    for k in range(K):
        t = wbc_workload.track_targets(points, n_points, du, k, kind, tangents)
        val += (e[k] * t).sum(axis=1)
        scale += (np.abs(e[k]) * np.abs(t)).sum(axis=1)
    return val, scale


# ---- the three tracks of the sweep tests, built around the targets of the inputs
def three_tracks(d, K, seed, generic=False):
    """A gripper track (HERMITE, default tangents), a track of foot 0 (LINEAR) and a trunk track (HERMITE, the caller's tangents), S = 4,
    n_points 2..4 across the instances, milestones within a centimetre of the inputs' targets. du per instance: generic = False mixes
    interior ticks, exact knots (0.5), tracks that clamp within the K ticks and one whose every tick is clamped (du = 8: instance 1 of the
    gripper track, where B allows); generic = True keeps every tick interior and off the knots (for central differences)."""
    rng = np.random.default_rng(seed)
    B = len(d["q"])
    tracks = []
    for j, (target, kind) in enumerate(((4, "hermite"), (0, "linear"), ("trunk", "hermite"))):
        base = d["trunk_target"] if target == "trunk" else d["ee_target"][:, target]
        pts = base[:, None, :] + rng.uniform(-0.01, 0.01, (B, S, 3))
        n = (2 + (np.arange(B) + j) % 3).astype(np.int32)
        if j == 0:                                                         # the default-tangent cases at milestone 1, deliberately (random milestones
            for b, cs in ((2, (2, 3, 4)), (4, (-2, -3, 1))):              # take cases 2 and 3 in one component of twenty each): CASE's, a centimetre wide
                if b < B:
                    for c, case in enumerate(cs):
                        pts[b, 0:3, c] = base[b, c] + (0.01 / 3.0) * np.array(CASE[case])
        if generic:
            du = (0.9 / max(K - 1, 1)) * rng.uniform(0.6, 0.95, B)           # (K - 1) du < 0.9 <= n - 1: no knot, no clamp after tick 0
        else:
            du = np.array([0.5, 0.37, 0.9, 0.23, 1.1, 0.5, 0.61])[(np.arange(B) + 2 * j) % 7]
            if j == 0 and B > 1:
                du[1] = 8.0
        t = dict(target=target, kind=kind, points=np.ascontiguousarray(pts), n_points=n, du=np.ascontiguousarray(du))
        if target == "trunk":
            t["tangents"] = rng.uniform(-0.01, 0.01, (B, S, 3))
        tracks.append(t)
    return tracks


def target_index(t):
    return TRUNK if t["target"] == "trunk" else int(t["target"])


def follow(d, tracks, k):
    """the inputs with the followed rows of tick k"""
    n = dict(d, ee_target=d["ee_target"].copy())
    for t in tracks:
        x = wbc_workload.track_targets(t["points"], t.get("n_points"), t["du"], k, t.get("kind", "linear"), t.get("tangents"))
        if target_index(t) == TRUNK:
            n["trunk_target"] = x
        else:
            n["ee_target"][:, target_index(t)] = x
    return n


def track_chain(m, cfg, d0, K, dt, tracks):
    """step_common.chain with the followed rows overwritten per tick by track_targets -> (states [K + 1], ticks, sides, status); states[k] holds
    the inputs tick k saw"""
    B = len(d0["q"])
    states, ticks, sides, status = [follow(d0, tracks, 0)], [], [], []
    for k in range(K):
        d = states[-1]
        t = oracle.tick([m], [cfg], d, dt, B, nthreads=8)
        a = oracle.assemble([m], [cfg], d, dt, B)
        ticks.append(t)
        sides.append(tq._sides(a, t["qdot"]))
        status.append(t["status"])
        nxt = sc.advance(cfg, d, oracle.update_state([m], d["q"], t["q_next"], d["ee_target"], None, None), None)
        states.append(follow(nxt, tracks, k + 1))
    return states, ticks, sides, status


def host_sweep(m, cfg, states, ticks, rho, dt, tracks):
    """wbc_workload.rollout_gradients(tracks=...) on the oracle's chain, seeded with rho . raw q_K -> its dict"""
    import gradq_common as gq
    K = len(ticks)
    B = len(rho)
    g = sc.pull_back([m], None, states[K]["q"], rho)
    return wbc_workload.rollout_gradients(m, cfg, [{k: v for k, v in s.items()} for s in states[:K]], np.stack([t["qdot"] for t in ticks]), dt,
                                          gq.StateFK([m]), lambda dd: oracle.assemble([m], [cfg], dd, dt, B), g_q_final=g, tracks=tracks)


def margins(m, cfg, states, ticks, K):
    """(margin [B] the smallest over the ticks, kappa [B] the largest cond(H)): test_tick_grad_q_host._certified's, tick by tick"""
    B = len(states[0]["q"])
    margin, kappa = np.full(B, np.inf), np.zeros(B)
    for k in range(K):
        _, a0, _, _, _, mg = tq._certified(m, cfg, states[k], np.zeros((B, capi.V_STRIDE)))
        margin = np.minimum(margin, mg)
        kappa = np.maximum(kappa, np.linalg.cond(a0["H"][:, :m.nv, :m.nv]))
    return margin, kappa


def track_chain_directional(m, cfg, d, rho, K, dt, vary, sides0, margin, kappa, ana, scale_terms, what):
    """test_step_grad_host.chain_directional for the chain along tracks: vary(step) -> the tracks. The same rule: FD of rho . raw q_K at h and
    h / 2, tolerance 4 |FD(h) - FD(h/2)| + floor, an instance left out where the working set differs at any of the four steps or the margin
    is below 1e-6 -> (keep, ok, line)"""
    B, H = len(rho), tq.H_E2E
    vals = {}
    same = np.ones(B, dtype=bool)
    for s in (H, -H, H / 2, -H / 2):
        states, _, sides, status = track_chain(m, cfg, d, K, dt, vary(s))
        vals[s] = (rho * states[K]["q"]).sum(axis=1)
        for k in range(K):
            same &= (sides[k] == sides0[k]).all(axis=1) & (status[k] == 0)
    fd1 = (vals[H] - vals[-H]) / (2 * H)
    fd2 = (vals[H / 2] - vals[-H / 2]) / H
    keep = same & (margin >= 1e-6)
    floor = kappa * EPS * scale_terms + EPS * np.abs(rho * track_chain(m, cfg, d, K, dt, vary(0.0))[0][K]["q"]).sum(axis=1) / (H / 2)
    tol = 4.0 * np.abs(fd1 - fd2) + floor
    err = np.abs(ana - fd2)
    line = "%s: %d of %d kept; worst |analytic - FD(h/2)| / tolerance %.3f; |analytic - FD(h/2)| up to %.3e against |FD(h) - FD(h/2)| up to %.3e, floor up to %.3e, |grad| up to %.3g" % (
        what, keep.sum(), B, (err / tol)[keep].max(), err[keep].max(), np.abs(fd1 - fd2)[keep].max(), floor[keep].max(), np.abs(fd2[keep]).max())
    return keep, bool((err[keep] <= tol[keep]).all()), line


def perturbed(tracks, s, dP, dV, dU):
    """the tracks with points + s dP[j], tangents + s dV[j] (where the track has its own), du + s dU[j]"""
    out = []
    for j, t in enumerate(tracks):
        n = dict(t, points=t["points"] + s * dP[j], du=t["du"] + s * dU[j])
        if t.get("tangents") is not None:
            n["tangents"] = t["tangents"] + s * dV[j]
        out.append(n)
    return out


def directions(tracks, seed):
    """random directions in every track's points, tangents and du; zero at and beyond n_points. The points' and tangents' are of the size
    of the milestones' spread (a centimetre), du's of du's own"""
    rng = np.random.default_rng(seed)
    dP, dV, dU = [], [], []
    for t in tracks:
        B = len(t["points"])
        live = (np.arange(S)[None, :] < t["n_points"][:, None])[:, :, None]
        dP.append(np.where(live, rng.choice([-1.0, 1.0], (B, S, 3)) * rng.uniform(0.5, 1.0, (B, S, 3)), 0.0))
        dV.append(np.where(live, rng.choice([-1.0, 1.0], (B, S, 3)) * rng.uniform(0.5, 1.0, (B, S, 3)), 0.0))
        dU.append(rng.choice([-1.0, 1.0], B) * rng.uniform(0.5, 1.0, B))
    return dP, dV, dU
