"""CPU: the track scores as a loss. wbc_rollout_vjp_scored at the boundary (header, exports, struct size, variant count) and the host
restatement wbc_workload.score_seed_gradients / rollout_gradients(score_seed=...), held to the oracle alone:
  the identity            the adjoint rests on reached_f = FK_f(q_(k+1)): the forward scores FK_f(integrated configuration) shifted rigidly by
                          (estimated base - integrated base), the adjoint differentiates FK_f at the state after the tick. Oracle chains,
                          K = 3, RUNNING (oracle.update_state) and WARMUP (the integrated configuration is the state), no IMU. The shift is one
                          subtraction and one addition per component on numbers no larger than max|position| (and the state's base is that
                          estimated base): at most 2 roundings of eps / 2 max|position| each, held to IDENT_MULT = 4 eps max|position|.
                          Measured worst: RUNNING 1.04 eps max|position| (full / seed 3; everything / seed 4: 0.51), WARMUP exactly 0.
  the score cotangent     score_seed_gradients against central differences of the scores restated from the oracle's FK, in q_(k+1) (tangent
                          steps, gradq_common.step) and in the targets, all three scores, every frame scored, err_max with a strict maximum
                          (the targets' distances per tick are 2, 5 and 3 cm: the middle tick by 2 cm). The scores are smooth in q, so the
                          central difference carries a truncation term: the house rule (test_step_grad_host.chain_directional) 4 |FD(h) -
                          FD(h/2)| plus the rounding of the difference, K_ROUND eps sum|gamma| |score| / (h / 2) with track_grad_host's K_ROUND.
                          A frame with e == 0 gives an exact zero from the 1 / e terms (bitwise), and the difference in its target is 0 to
                          rounding.
  the restated sweep      rollout_gradients(score_seed=...) with a score seed alone against central differences of the oracle chain's own
                          scores THROUGH track_grad_common.track_chain_directional, rule and cap unchanged: that function differentiates rho .
                          q_K of track_chain's last state, so the test hands it a track_chain whose last "q" holds the chain's score loss
                          (loss_in_q: with the magnitudes the loss is formed from beside it, so that the function's rounding floor is this
                          loss's). `full` / seed 3 and `everything` / seed 4, K = 3, three tracks; scored: the gripper
                          (followed), foot 1 (constant target), the trunk (followed). err_max's cotangent is given where the oracle's maximum
                          is separated from the other ticks by more than MAX_GAP (1e-6 m: ten times what a step of h = 2^-20 in a milestone
                          can move an error), elsewhere it is 0 — the maximum is not differentiable where two ticks tie.
Kept counts measured here (CPU, the oracle alone): full / seed 3: 16 of 16 in points, tangents and du; everything / seed 4: 16 of 16."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gradq_common as gq
import oracle
import step_common as sc
import test_step_grad_host as th
import test_tick_grad_q_host as tq
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
K_ROUND = 16
IDENT_MULT = 4.0
MAX_GAP = 1e-6
LIN_BOUND = 1e-11      # two runs of the sweep on `full` agree to the sweep's own bound there (test_gpu_rollout_vjp.SWEEP_BOUND["full"])
NF = capi.TARGET_TRUNK + 1
ROLES = [capi.FR_EE0 + f for f in range(capi.NEE)] + [capi.FR_TRUNK]


def test_header_declares_and_library_exports_the_scored_sweep():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    for name in ("wbc_rollout_vjp_scored", "wbc_rollout_scored_sizes"):
        assert re.search(r"int\s+%s\s*\(" % name, header), name
    for word in ("WbcScoreSeed", "g_err_sq_sum", "g_err_final", "g_err_max", "err_max_tick", "q_final", "last_scorevjp_variant"):
        assert word in header, word
    offered = header[header.index("roll-out scores as a loss"):]
    offered = offered[offered.index("Not offered"):offered.index("Statistic")]
    assert "IMU" in offered and "scores as a loss" not in offered
    lib = capi.load_library()
    for name in ("wbc_rollout_vjp_scored", "wbc_rollout_scored_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    a = C.c_int32()
    assert lib.wbc_rollout_scored_sizes(C.byref(a)) == 0 and a.value == C.sizeof(capi.WbcScoreSeed) == 48
    assert lib.wbc_variant_count(b"scorevjp") == 3 and lib.wbc_variant_count(b"trackvjp") == 2 and lib.wbc_variant_count(b"rollvjp") == 3
    assert "scorevjp" not in capi.VARIANT_FAMILIES


def _positions(m, q):
    """the six scored frames' positions [B, 6, 3] from the oracle's FK"""
    return oracle.fk([m], q, None, want_com=False)["oMf"][:, ROLES, 9:12]


def _reached(m, q_next, q_new):
    """what the forward scores: FK at the integrated configuration, shifted rigidly by (estimated base - integrated base)"""
    return _positions(m, q_next) + (q_new[:, None, 0:3] - q_next[:, None, 0:3])


# ---- 1. the identity
@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("everything", 4)])
@pytest.mark.parametrize("running", [True, False])
def test_scored_position_is_the_fk_at_the_state_after_the_tick(cfg_name, seed, running):
    m, cfg, d, _, _ = th.sweep_setup(cfg_name, seed)
    B = len(d["q"])
    cur, worst = d, 0.0
    for k in range(3):
        t = oracle.tick([m], [cfg], cur, tq.DT, B, nthreads=8)
        q_new = oracle.update_state([m], cur["q"], t["q_next"], cur["ee_target"], None, None) if running else t["q_next"]
        scored, at_state = _reached(m, t["q_next"], q_new), _positions(m, q_new)
        assert np.array_equal(q_new[:, 3:], t["q_next"][:, 3:])          # the state keeps the integrated orientation and joints
        scale = np.abs(at_state).max()
        worst = max(worst, np.abs(scored - at_state).max() / (EPS * scale))
        assert np.abs(scored - at_state).max() <= IDENT_MULT * EPS * scale
        cur = sc.advance(cfg, cur, q_new, None)
    print("%s / seed %d, %s: max|scored - FK(q_(k+1))| = %.2f eps max|position| (held to %.0f)" % (
        cfg_name, seed, "RUNNING" if running else "WARMUP", worst, IDENT_MULT))


# ---- 2. the score cotangent against central differences
def _scores(m, q_after, ee_target, trunk_target):
    """err_sq_sum, err_final, err_max [6, B] restated from the oracle's FK at q_after [K, B, 27]"""
    K = len(q_after)
    e = np.zeros((K, len(q_after[0]), NF))
    for k in range(K):
        d = _positions(m, q_after[k]) - np.concatenate([ee_target[k], trunk_target[k][:, None]], axis=1)
        e[k] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return (e * e).sum(axis=0).T, e[K - 1].T, e.max(axis=0).T, e.argmax(axis=0).T.astype(np.int32)


def _cotangent_problem(seed=3):
    m, cfg, d, _, direc = th.sweep_setup("full", seed)
    B, K = len(d["q"]), 3
    rng = np.random.default_rng(seed + 100)
    q_after = []
    for k in range(K):
        delta = np.zeros((B, capi.V_STRIDE))
        delta[:, :m.nv] = rng.normal(0, 0.02, (B, m.nv))
        q_after.append(gq.step([m], d["q"], delta))
    q_after = np.stack(q_after)
    dist = (0.02, 0.05, 0.03)                                            # the strict maximum: tick 1, by 2 cm
    ee, tr = np.zeros((K, B, 5, 3)), np.zeros((K, B, 3))
    for k in range(K):
        u = rng.normal(0, 1.0, (B, NF, 3))
        tgt = _positions(m, q_after[k]) + dist[k] * u / np.linalg.norm(u, axis=2, keepdims=True)
        ee[k], tr[k] = tgt[:, :5], tgt[:, 5]
    gam = [rng.normal(0, 1.0, (NF, B)) for _ in range(3)]
    return m, q_after, ee, tr, gam, rng


def _loss(m, q_after, ee, tr, gam):
    sq, fin, mx, tick = _scores(m, q_after, ee, tr)
    val = (gam[0] * sq + gam[1] * fin + gam[2] * mx).sum(axis=0)
    return val, (np.abs(gam[0]) * sq + np.abs(gam[1]) * fin + np.abs(gam[2]) * mx).sum(axis=0), tick


def test_score_cotangent_against_central_differences():
    m, q_after, ee, tr, gam, rng = _cotangent_problem()
    K, B = q_after.shape[:2]
    _, _, tick = _loss(m, q_after, ee, tr, gam)
    assert (tick == 1).all()
    r = wbc_workload.score_seed_gradients(m, q_after, ee, tr, gq.StateFK([m]), 63, gam[0], gam[1], gam[2], tick)
    h = 2.0 ** -13
    for trial in range(3):
        dq = np.zeros((K, B, capi.V_STRIDE))
        dq[:, :, :m.nv] = rng.choice([-1.0, 1.0], (K, B, m.nv)) * rng.uniform(0.5, 1.0, (K, B, m.nv))
        de, dt_ = rng.normal(0, 1.0, (K, B, 5, 3)), rng.normal(0, 1.0, (K, B, 3))
        if trial == 1:
            de[:], dt_[:] = 0.0, 0.0                                      # the state alone
        if trial == 2:
            dq[:] = 0.0                                                   # the targets alone
        ana = (r["g_q_trace"] * dq).sum(axis=(0, 2)) - (r["c"][:, :, :5] * de).sum(axis=(0, 2, 3)) - (r["c"][:, :, 5] * dt_).sum(axis=(0, 2))

        def L(s):
            qa = np.stack([gq.step([m], q_after[k], s * dq[k]) for k in range(K)])
            return _loss(m, qa, ee + s * de, tr + s * dt_, gam)
        (lp, sp, tp), (lm, sm, tm), (lp2, _, _), (lm2, _, _) = L(h), L(-h), L(h / 2), L(-h / 2)
        assert (tp == 1).all() and (tm == 1).all()
        fd1, fd2 = (lp - lm) / (2 * h), (lp2 - lm2) / h
        tol = 4.0 * np.abs(fd1 - fd2) + K_ROUND * EPS * np.maximum(sp, sm) / (h / 2)
        err = np.abs(ana - fd2)
        print("trial %d: |analytic - FD(h/2)| up to %.3e, tolerance %.3e .. %.3e (worst ratio %.3f), |FD(h) - FD(h/2)| up to %.3e, |grad| up to %.3g" % (
            trial, err.max(), tol.min(), tol.max(), (err / tol).max(), np.abs(fd1 - fd2).max(), np.abs(fd2).max()))
        assert (err <= tol).all(), (trial, err, tol)
        assert np.abs(ana).min() > 0


def test_each_score_alone_and_a_single_frame():
    """the three scores are separate terms and a mask with one bit is that frame alone"""
    m, q_after, ee, tr, gam, _ = _cotangent_problem()
    tick = np.ones((NF, len(q_after[0])), np.int32)
    fk = gq.StateFK([m])
    full = wbc_workload.score_seed_gradients(m, q_after, ee, tr, fk, 63, gam[0], gam[1], gam[2], tick)
    parts = [wbc_workload.score_seed_gradients(m, q_after, ee, tr, fk, 63, *[g if i == j else None for j, g in enumerate(gam)], err_max_tick=tick)
             for i in range(3)]
    total = sum(p["c"] for p in parts)
    assert np.abs(full["c"] - total).max() <= 4 * EPS * np.abs(full["c"]).max()
    assert not parts[1]["c"][:2].any() and not parts[2]["c"][[0, 2]].any()      # err_final: the last tick; err_max: its tick
    one = wbc_workload.score_seed_gradients(m, q_after, ee, tr, fk, 1 << 4, gam[0][4:5], gam[1][4:5], gam[2][4:5], tick[4:5])
    assert np.array_equal(one["c"][:, :, 4], full["c"][:, :, 4]) and not np.delete(one["c"], 4, axis=2).any()
    with pytest.raises(ValueError):
        wbc_workload.score_seed_gradients(m, q_after, ee, tr, fk, 63, g_err_max=gam[2])


def test_a_frame_on_its_target_gives_an_exact_zero():
    m, q_after, ee, tr, gam, rng = _cotangent_problem()
    K, B = q_after.shape[:2]
    ee = ee.copy()
    ee[K - 1][:, 4] = _positions(m, q_after[K - 1])[:, 4]                 # the gripper on its target on the last tick: e == 0 exactly
    tick = np.full((NF, B), K - 1, np.int32)                              # (a tick given by the caller, as the call takes it)
    r = wbc_workload.score_seed_gradients(m, q_after, ee, tr, gq.StateFK([m]), 63, gam[0], gam[1], gam[2], tick)
    assert not r["e"][K - 1, :, 4].view(np.uint64).any()
    assert not r["c"][K - 1, :, 4].any() and np.isfinite(r["g_q_trace"]).all() and np.isfinite(r["c"]).all()
    only = wbc_workload.score_seed_gradients(m, q_after, ee, tr, gq.StateFK([m]), 1 << 4, None, gam[1][4:5], gam[2][4:5], tick[4:5])
    assert not only["g_q_trace"].any() and not only["c"].any()           # nothing but the 1 / e terms: every entry is a zero
    # the difference in the target of that frame: |d| is even in the step, so the central difference is 0 to rounding
    h = 2.0 ** -13
    de = np.zeros_like(ee)
    de[K - 1][:, 4] = rng.normal(0, 1.0, (B, 3))
    g1 = [np.zeros((NF, B)), gam[1], np.zeros((NF, B))]
    (lp, sp, _), (lm, _, _) = _loss(m, q_after, ee + h * de, tr, g1), _loss(m, q_after, ee - h * de, tr, g1)
    assert (np.abs(lp - lm) / (2 * h) <= K_ROUND * EPS * sp / h).all()


# ---- 3. the restated sweep with a score seed alone, against the oracle chain's own scores
SCORED = (1, 4, capi.TARGET_TRUNK)
MASK = sum(1 << f for f in SCORED)


def _chain_scores(m, states, ticks):
    """err_sq_sum, err_final, err_max, err_max_tick [3, B] of SCORED as the forward defines them, from an oracle chain; e [K, B, 3]; and
    w [K, B, 3, 3] = |position| + |target| per component (a difference d carries a rounding of eps / 2 of that)"""
    K = len(ticks)
    e, w, dd = np.zeros((K, len(states[0]["q"]), len(SCORED))), np.zeros((K, len(states[0]["q"]), len(SCORED), 3)), np.zeros((K, len(states[0]["q"]), len(SCORED), 3))
    for k in range(K):
        pos = _reached(m, ticks[k]["q_next"], states[k + 1]["q"])
        tgt = np.concatenate([states[k]["ee_target"], states[k]["trunk_target"][:, None]], axis=1)
        d = (pos - tgt)[:, SCORED]
        e[k] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        w[k], dd[k] = (np.abs(pos) + np.abs(tgt))[:, SCORED], d
    return (e * e).sum(axis=0).T, e[K - 1].T, e.max(axis=0).T, e.argmax(axis=0).T.astype(np.int32), e, w, dd


def score_problem(cfg_name, seed, only_sq=False):
    """-> the chain, its scores, the cotangents (g_err_max where the maximum is separated by MAX_GAP alone; only_sq: the loss is
    err_sq_sum.sum()) and a loss(states, ticks) -> ([B], its magnitudes [B])"""
    m, cfg, d, _, _ = th.sweep_setup(cfg_name, seed)
    K, B = th.K_TICKS, len(d["q"])
    tracks = tg.three_tracks(d, K, seed + 50, generic=True)
    states, ticks, sides0, status = tg.track_chain(m, cfg, d, K, tq.DT, tracks)
    sq, fin, mx, tick, e, _, _ = _chain_scores(m, states, ticks)
    rng = np.random.default_rng(seed + 200)
    gam = [rng.normal(0, 1.0, (len(SCORED), B)) for _ in range(3)]
    srt = np.sort(e, axis=0)
    gam[2] = np.where((srt[-1] - srt[-2]).T > MAX_GAP, gam[2], 0.0)
    if only_sq:
        gam = [np.ones_like(gam[0]), np.zeros_like(gam[0]), np.zeros_like(gam[0])]

    def loss(st, tk):
        """-> (the loss [B], S [B]: the magnitudes it is formed from, sum |gamma| |d score / d d| (|position| + |target|))"""
        a, b, c, at, e_, w, dd = _chain_scores(m, st, tk)
        u = np.abs(dd) / np.maximum(e_, 1e-300)[..., None]                # |d e / d d|
        S = np.zeros(B)
        for i in range(len(SCORED)):
            S += np.abs(gam[0][i]) * 2.0 * (np.abs(dd[:, :, i]) * w[:, :, i]).sum(axis=(0, 2)) + np.abs(gam[1][i]) * (u[K - 1, :, i] * w[K - 1, :, i]).sum(axis=1)
            S += np.abs(gam[2][i]) * (u[at[i], np.arange(B), i] * w[at[i], np.arange(B), i]).sum(axis=1)
        return (gam[0] * a + gam[1] * b + gam[2] * c).sum(axis=0), S
    return dict(m=m, cfg=cfg, d=d, K=K, B=B, tracks=tracks, states=states, ticks=ticks, sides0=sides0, status=status, gam=gam, tick=tick, e=e,
                loss=loss, seed=dict(mask=MASK, q_final=states[K]["q"], g_err_sq_sum=gam[0], g_err_final=gam[1], g_err_max=gam[2], err_max_tick=tick))


RHO = (1.0, 1.0, -1.0)


def loss_in_q(loss):
    """a track_chain for track_chain_directional: the last state's "q" holds (loss, S, S) in its first entries and rho = RHO reads loss + S - S.
    The function's floor eps sum|rho q| / (h / 2) is then the rounding of THIS loss: the scores are formed from differences of positions and
    targets of size S, a hundred times the loss's own value, and their rounding does not shrink with it."""
    inner = tg.track_chain

    def chain(m, cfg, d, K, dt, tracks):
        states, ticks, sides, status = inner(m, cfg, d, K, dt, tracks)
        q = np.zeros_like(states[K]["q"])
        q[:, 0], S = loss(states, ticks)
        q[:, 1] = q[:, 2] = S
        return states[:K] + [dict(states[K], q=q)], ticks, sides, status
    return chain


def directional_cases(p, g, seed):
    dP, dV, dU = tg.directions(p["tracks"], seed + 9)
    zero, zu = [np.zeros_like(x) for x in dP], [np.zeros(p["B"]) for _ in dU]
    return (("d_points", dP, zero, zu, sum((g[j]["d_points"] * dP[j]).sum(axis=(1, 2)) for j in range(3)),
             sum(np.abs(g[j]["d_points"] * dP[j]).sum(axis=(1, 2)) for j in range(3))),
            ("d_tangents", zero, dV, zu, (g[2]["d_tangents"] * dV[2]).sum(axis=(1, 2)), np.abs(g[2]["d_tangents"] * dV[2]).sum(axis=(1, 2))),
            ("d_du", zero, zero, dU, sum(g[j]["d_du"] * dU[j] for j in range(3)), sum(np.abs(g[j]["d_du"] * dU[j]) for j in range(3))))


@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("everything", 4)])
def test_restated_sweep_with_a_score_seed_alone_against_the_oracle_chain(cfg_name, seed, monkeypatch):
    p = score_problem(cfg_name, seed)
    m, cfg, d, K, B, tracks = p["m"], p["cfg"], p["d"], p["K"], p["B"], p["tracks"]
    assert all((s == 0).all() for s in p["status"])
    assert (p["gam"][2] != 0).sum() >= 3 * B - 3 * B // 4, "err_max: the maximum is tied on too many instances"
    sw = wbc_workload.rollout_gradients(m, cfg, [dict(s) for s in p["states"][:K]], np.stack([t["qdot"] for t in p["ticks"]]), tq.DT, gq.StateFK([m]),
                                        lambda dd: oracle.assemble([m], [cfg], dd, tq.DT, B), tracks=tracks, score_seed=p["seed"])
    assert (sw["ticks_dropped"] == 0).all()
    # the closed forms: the constant foot target takes -sum_k c_k exactly where no task or estimator adds to it; the followed rows carry nothing
    assert not sw["d_ee_target"][:, 4].view(np.uint64).any() and not sw["d_trunk_target"].view(np.uint64).any()
    assert np.abs(sw["d_ee_target"][:, 1]).max() > 0
    margin, kappa = tg.margins(m, cfg, p["states"], p["ticks"], K)
    rho = np.zeros((B, capi.Q_STRIDE))
    rho[:, :3] = RHO
    monkeypatch.setattr(tg, "track_chain", loss_in_q(p["loss"]))
    for name, p_, v_, u_, ana, terms in directional_cases(p, sw["tracks"], seed):
        keep, ok, line = tg.track_chain_directional(m, cfg, d, rho, K, tq.DT, lambda s: tg.perturbed(tracks, s, p_, v_, u_), p["sides0"], margin, kappa,
                                                    ana, terms, "%s / seed %d, K = %d, score seed, %s" % (cfg_name, seed, K, name))
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line
        assert np.abs(ana).max() > 0


def test_both_seeds_are_the_sum_of_each():
    p = score_problem("full", 3)
    m, cfg, K, B = p["m"], p["cfg"], p["K"], p["B"]
    g = np.random.default_rng(5).normal(0, 1e-3, (B, capi.V_STRIDE))
    g[:, m.nv:] = 0.0
    run = lambda **kw: wbc_workload.rollout_gradients(      # noqa: E731
        m, cfg, [dict(s) for s in p["states"][:K]], np.stack([t["qdot"] for t in p["ticks"]]), tq.DT, gq.StateFK([m]),
        lambda dd: oracle.assemble([m], [cfg], dd, tq.DT, B), tracks=p["tracks"], **kw)
    a, b, both = run(g_q_final=g), run(score_seed=p["seed"]), run(g_q_final=g, score_seed=p["seed"])
    for k in ("d_q0", "d_task_params", "d_ee_target", "d_prev_ee_target"):
        s = a[k] + b[k]
        assert np.abs(both[k] - s).max() <= LIN_BOUND * max(1.0, np.abs(s).max()), k
    for j in range(3):
        s = a["tracks"][j]["d_points"] + b["tracks"][j]["d_points"]
        assert np.abs(both["tracks"][j]["d_points"] - s).max() <= LIN_BOUND * max(1.0, np.abs(s).max())
