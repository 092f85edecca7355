"""CPU: gradients of track roll-outs. wbc_rollout_record_tracks / wbc_rollout_vjp_tracks at the boundary (header, exports, struct sizes,
variant counts) and the host restatements, held to central differences alone:
  track_target_gradients  against central differences of wbc_workload.track_targets on deliberately built tracks (track_grad_common.built_tracks:
                          n_points 2..4, every default-tangent case at an interior milestone and n = 2, ticks exactly on a knot, ticks clamped at
                          both ends, every milestone at least 0.2 from a branch boundary). The target is linear in the points and the tangents
                          within a branch, so their difference is exact up to rounding: K_ROUND eps sum_k |e_k| . |target_k| / h, K_ROUND = 16 for the
                          at most 12 roundings of one Hermite evaluation (default tangent included) and the sum. In du the target is a cubic per
                          segment: the central difference is off by h^2 / 6 sum_k k^3 |e_k . x'''| with x''' = 12 (m0 - m1) + 6 (v0 + v1), the
                          segment's constant third derivative; the test adds that to the rounding term. On a knot the derivative is one-sided:
                          the Richardson pair 2 F(h/2) - F(h) of forward differences (error h^2 / 12 of the same sum) holds d_du to the right
                          segment's derivative.
  exact zeros             rows at or beyond n_points; d_du of an instance whose every tick is clamped
  the restated sweep      rollout_gradients(tracks=...) against central differences of the oracle's chain (oracle.tick / assemble / update_state
                          with step_common.advance, the followed rows overwritten per tick by track_targets), K = 3, configurations `full`
                          and `everything` on test_step_grad_host.sweep_setup's inputs, three tracks (gripper HERMITE with default tangents, foot 0
                          LINEAR, trunk HERMITE with the caller's tangents), chain_directional's tolerance 4 |FD(h) - FD(h/2)| + floor and its
                          cap of B // 4 instances left out. `full` and `everything` switch every foot task on, so the foot track's cotangent arrives
                          through its task rows as well as through the estimator.
Kept counts measured here (CPU, the oracle alone): full / seed 3: 16 of 16 in points, tangents and du; everything / seed 4: 16 of 16."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_step_grad_host as th
import test_tick_grad_q_host as tq
import track_grad_common as tg
import wbc_capi as capi
import wbc_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
K_ROUND = 16
KINDS = ("linear", "hermite", "hermite_tangents")


def test_header_declares_and_library_exports_the_track_gradients():
    header = open(os.path.join(ROOT, "include", "wbc.h")).read()
    for name in ("wbc_rollout_record_tracks", "wbc_rollout_vjp_tracks", "wbc_rollout_tracks_grad_sizes"):
        assert re.search(r"int\s+%s\s*\(" % name, header), name
    for word in ("WbcTrackGrad", "WbcTracksGrad", "d_points", "d_tangents", "d_du", "last_trackvjp_variant", "Not offered"):
        assert word in header, word
    lib = capi.load_library()
    for name in ("wbc_rollout_record_tracks", "wbc_rollout_vjp_tracks", "wbc_rollout_tracks_grad_sizes"):
        assert hasattr(lib, name) and name in capi.SIGNATURES
    a, b = C.c_int32(), C.c_int32()
    assert lib.wbc_rollout_tracks_grad_sizes(C.byref(a), C.byref(b)) == 0
    assert (a.value, b.value) == (C.sizeof(capi.WbcTrackGrad), C.sizeof(capi.WbcTracksGrad))
    assert tuple(capi.TRACK_GRAD_FIELDS) == ("d_points", "d_tangents", "d_du")
    assert lib.wbc_variant_count(b"trackvjp") == 2 and lib.wbc_variant_count(b"rollvjp") == 3
    assert "trackvjp" not in capi.VARIANT_FAMILIES and "rollvjp" not in capi.VARIANT_FAMILIES


# ---- track_target_gradients against central differences of track_targets
K_BUILT = 9


def _built(kind):
    t = tg.built_tracks()
    B = len(t["du"])
    rng = np.random.default_rng(5)
    e = rng.normal(0, 1.0, (K_BUILT, B, 3))
    live = (np.arange(tg.S)[None, :] < t["n_points"][:, None])[:, :, None]
    tangents = np.where(live, rng.uniform(-2.0, 2.0, (B, tg.S, 3)), 55.0) if kind == "hermite_tangents" else None
    return t, e, live, tangents, "linear" if kind == "linear" else "hermite"


def test_built_tracks_reach_every_branch():
    t = tg.built_tracks()
    assert set(t["n_points"]) == {2, 3, 4}
    assert {1, 2, 3, 4} <= set(np.abs(t["cases"]).ravel())
    v = wbc_workload.spline_tangents(t["points"], t["n_points"])
    for b in range(len(t["du"])):                                         # the rule takes the case the table names
        for c in range(3):
            case = abs(t["cases"][b, c])
            if case:
                a, x, bb = t["points"][b, 0:3, c]
                assert case == wbc_workload._tangent_case(a, x, bb)
                assert v[b, 1, c] == {1: 0.0, 2: 3.0 * (x - a), 3: 3.0 * (bb - x), 4: (bb - a) * 0.5}[case]
    tt = np.arange(K_BUILT)[:, None] * t["du"][None, :]
    assert ((tt == np.floor(tt)) & (tt > 0) & (tt < t["n_points"] - 1)).any()          # interior ticks exactly on a knot
    assert (tt >= t["n_points"] - 1).any() and t["clamped"].any() and t["knot"].any()


@pytest.mark.parametrize("kind", KINDS)
def test_points_and_tangents_against_central_differences(kind):
    t, e, live, tangents, k2 = _built(kind)
    B = len(t["du"])
    d_points, d_tangents, d_du = wbc_workload.track_target_gradients(t["points"], t["n_points"], t["du"], K_BUILT, k2, tangents, e)
    assert (d_tangents is None) == (tangents is None)
    h = 2.0 ** -10
    rng = np.random.default_rng(8)
    for what, grad in (("points", d_points), ("tangents", d_tangents)):
        if grad is None:
            continue
        for trial in range(4):
            D = np.where(live, rng.choice([-1.0, 1.0], (B, tg.S, 3)) * rng.uniform(0.5, 1.0, (B, tg.S, 3)), 0.0)
            if trial == 3:                                                # one milestone and component alone
                D = np.where(np.arange(tg.S)[None, :, None] == 1, D, 0.0)

            def L(s):
                if what == "points":
                    return tg.loss_of_tracks(t["points"] + s * D, t["n_points"], t["du"], K_BUILT, k2, tangents, e)
                return tg.loss_of_tracks(t["points"], t["n_points"], t["du"], K_BUILT, k2, tangents + s * D, e)
            (lp, sp), (lm, sm) = L(h), L(-h)
            fd = (lp - lm) / (2 * h)
            ana = (grad * D).sum(axis=(1, 2))
            bound = K_ROUND * EPS * np.maximum(sp, sm) / h
            print("%s / %s, trial %d: |analytic - FD| up to %.3e, bound %.3e .. %.3e, |grad| up to %.3g" % (
                kind, what, trial, np.abs(ana - fd).max(), bound.min(), bound.max(), np.abs(fd).max()))
            assert (np.abs(ana - fd) <= bound).all(), (kind, what, trial, np.abs(ana - fd), bound)
            assert np.abs(ana).max() > 0


def _third(t, k2, tangents, e):
    """sum_k k^3 |e_k . x'''| per instance, x''' the segment's third derivative in the parameter (0: linear, clamped)"""
    B = len(t["du"])
    out = np.zeros(B)
    if k2 == "linear":
        return out
    v = wbc_workload.spline_tangents(t["points"], t["n_points"]) if tangents is None else tangents
    for b in range(B):
        n = t["n_points"][b]
        for k in range(K_BUILT):
            tt = k * t["du"][b]
            if 0 < tt < n - 1:
                i = int(np.floor(tt))
                x3 = 12.0 * (t["points"][b, i] - t["points"][b, i + 1]) + 6.0 * (v[b, i] + v[b, i + 1])
                out[b] += k ** 3 * np.abs(e[k, b] * x3).sum()
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_du_against_differences(kind):
    t, e, live, tangents, k2 = _built(kind)
    _, _, d_du = wbc_workload.track_target_gradients(t["points"], t["n_points"], t["du"], K_BUILT, k2, tangents, e)
    h = 2.0 ** -12                                                        # k h <= 2e-3: no tick crosses a knot (the nearest is 0.01 away) but from a knot itself
    L = lambda du: tg.loss_of_tracks(t["points"], t["n_points"], du, K_BUILT, k2, tangents, e)      # noqa: E731
    third = _third(t, k2, tangents, e)
    (lp, sp), (lm, _), (l0, _), (lh, _) = L(t["du"] + h), L(t["du"] - h), L(t["du"]), L(t["du"] + h / 2)
    central = (lp - lm) / (2 * h)
    bound_c = h * h / 6.0 * third + K_ROUND * EPS * sp / h
    right = 2.0 * (lh - l0) / (h / 2) - (lp - l0) / h                     # Richardson on forward differences: the right segment's derivative
    bound_r = h * h / 12.0 * third + 6 * K_ROUND * EPS * sp / h
    off = ~t["knot"]
    print("%s: central |d_du - FD| up to %.3e (bound %.3e .. %.3e); on knots, from the right, %.3e (bound up to %.3e); |d_du| up to %.3g" % (
        kind, np.abs(d_du - central)[off].max(), bound_c[off].min(), bound_c[off].max(), np.abs(d_du - right)[t["knot"]].max(),
        bound_r[t["knot"]].max(), np.abs(d_du).max()))
    assert (np.abs(d_du - central)[off] <= bound_c[off]).all(), (d_du, central, bound_c)
    assert (np.abs(d_du - right)[t["knot"]] <= bound_r[t["knot"]]).all(), (d_du, right, bound_r)
    assert np.abs(d_du[off & ~t["clamped"]]).min() > 0 and np.abs(d_du[t["knot"]]).min() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_exact_zeros(kind):
    t, e, live, tangents, k2 = _built(kind)
    d_points, d_tangents, d_du = wbc_workload.track_target_gradients(t["points"], t["n_points"], t["du"], K_BUILT, k2, tangents, e)
    dead = np.broadcast_to(~live, d_points.shape)
    assert not d_points[dead].view(np.uint64).any() and np.abs(d_points[np.broadcast_to(live, d_points.shape)]).max() > 0
    if d_tangents is not None:
        assert not d_tangents[dead].view(np.uint64).any()
    assert not d_du[t["clamped"]].view(np.uint64).any()
    # a bad row gets zeros, its neighbours keep their bits
    bad = {k: np.array(v, copy=True) for k, v in t.items()}
    bad["points"][1, 0, 2], bad["du"][2], bad["n_points"][5] = np.nan, 0.0, 1
    r = wbc_workload.track_target_gradients(bad["points"], bad["n_points"], bad["du"], K_BUILT, k2, tangents, e)
    for got, ref in zip(r, (d_points, d_tangents, d_du)):
        if ref is not None:
            assert not got[[1, 2, 5]].view(np.uint64).any()
            assert np.array_equal(got[[0, 3, 4, 6, 7]].view(np.uint64), ref[[0, 3, 4, 6, 7]].view(np.uint64))


# ---- the restated sweep against the oracle's chain along tracks
@pytest.mark.parametrize("cfg_name,seed", [("full", 3), ("everything", 4)])
def test_restated_sweep_against_central_differences_of_the_oracle_chain(cfg_name, seed):
    m, cfg, d, rho, _ = th.sweep_setup(cfg_name, seed)
    K, B = th.K_TICKS, len(rho)
    tracks = tg.three_tracks(d, K, seed + 50, generic=True)
    states, ticks, sides0, status = tg.track_chain(m, cfg, d, K, tq.DT, tracks)
    assert all((s == 0).all() for s in status)
    sw = tg.host_sweep(m, cfg, states, ticks, rho, tq.DT, tracks)
    assert (sw["ticks_dropped"] == 0).all()
    for t in tracks:                                                      # the followed rows carry nothing
        f = tg.target_index(t)
        assert not (sw["d_trunk_target"] if f == tg.TRUNK else sw["d_ee_target"][:, f]).view(np.uint64).any()
    margin, kappa = tg.margins(m, cfg, states, ticks, K)
    dP, dV, dU = tg.directions(tracks, seed + 9)
    zero = [np.zeros_like(x) for x in dP]
    zu = [np.zeros(B) for _ in dU]
    scale = 1.0                                                           # (times h = 2^-20: a micrometre against milestones a centimetre apart)
    g = sw["tracks"]
    cases = (
        ("d_points", [scale * x for x in dP], zero, zu, sum((g[j]["d_points"] * scale * dP[j]).sum(axis=(1, 2)) for j in range(3)),
         sum(np.abs(g[j]["d_points"] * scale * dP[j]).sum(axis=(1, 2)) for j in range(3))),
        ("d_tangents", zero, [scale * x for x in dV], zu, (g[2]["d_tangents"] * scale * dV[2]).sum(axis=(1, 2)),
         np.abs(g[2]["d_tangents"] * scale * dV[2]).sum(axis=(1, 2))),
        ("d_du", zero, zero, [x for x in dU], sum(g[j]["d_du"] * dU[j] for j in range(3)),
         sum(np.abs(g[j]["d_du"] * dU[j]) for j in range(3))),
    )
    assert g[0]["d_tangents"] is None and g[1]["d_tangents"] is None
    for name, p_, v_, u_, ana, terms in cases:
        keep, ok, line = tg.track_chain_directional(m, cfg, d, rho, K, tq.DT, lambda s: tg.perturbed(tracks, s, p_, v_, u_), sides0, margin, kappa,
                                                    ana, terms, "%s / seed %d, K = %d, %s" % (cfg_name, seed, K, name))
        print(line)
        assert (~keep).sum() <= B // 4 and ok, line
        assert np.abs(ana).max() > 0
