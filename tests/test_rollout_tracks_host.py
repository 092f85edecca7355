"""Roll-outs with trunk and multi-target tracks, linear or Hermite spline (wbc_rollout_tracks) on the host: the C-ABI binding, the numpy
restatements of the track evaluation and of the default tangents against the scalar restatement of klampt's HermiteTrajectory
(Robot_Wrapper4._HermiteTrajectory), the no-overshoot property of the default tangents, and the front end's checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wbc_batch
import wbc_capi as capi
import wbc_workload
from wbc_workload import spline_tangents, track_targets, traj_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "wbc.h")).read()
ULP = np.finfo(float).eps


def test_library_exports_and_ctypes_binds_the_entry_point():
    lib = capi.load_library()
    assert "wbc_rollout_tracks" in capi.SIGNATURES and hasattr(lib, "wbc_rollout_tracks")
    assert lib.wbc_rollout_tracks.argtypes == capi.SIGNATURES["wbc_rollout_tracks"][1]
    assert re.search(r"\bwbc_rollout_tracks\s*\(", HEADER)
    assert int(re.search(r"#define WBC_MAX_TRACKS (\d+)", HEADER).group(1)) == capi.MAX_TRACKS
    assert int(re.search(r"#define WBC_TARGET_TRUNK (\d+)", HEADER).group(1)) == capi.TARGET_TRUNK
    kinds = re.search(r"enum \{ WBC_TRACK_LINEAR = (\d+), WBC_TRACK_HERMITE = (\d+) \}", HEADER)
    assert (int(kinds.group(1)), int(kinds.group(2))) == (capi.TRACK_LINEAR, capi.TRACK_HERMITE)


def test_struct_layouts_follow_the_header():
    """field order of the three structs as the header declares them; LP64 sizes and offsets"""
    for name, cls in (("WbcTrack", capi.WbcTrack), ("WbcTracks", capi.WbcTracks), ("WbcTrackScores", capi.WbcTrackScores)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            names += [re.sub(r"\[.*\]", "", w).strip("* \n") for w in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if w.strip()]
        assert names == [f for f, _ in cls._fields_], name
    assert C.sizeof(capi.WbcTrack) == 56 and capi.WbcTrack.points.offset == 16 and capi.WbcTrack.du_all.offset == 48
    assert C.sizeof(capi.WbcTracks) == 8 + 6 * 56 + 8 and capi.WbcTracks.track.offset == 8 and capi.WbcTracks.trunk_target_final.offset == 344
    assert C.sizeof(capi.WbcTrackScores) == 8 + 11 * 8 and capi.WbcTrackScores.err_sq_sum.offset == 8
    assert capi.WbcTrackScores.trace.offset == 56 and capi.WbcTrackScores.group_bad_instances.offset == 88


# ------------------------------------------------------------------------------------------------ track_targets
def _ragged(seed, B=64, S=6):
    rng = np.random.default_rng(seed)
    points = rng.normal(0, 0.3, (B, S, 3))
    n = rng.integers(2, S + 1, B).astype(np.int32)
    du = rng.choice([0.002, 1 / 8, 1 / 5, 0.3, 1.0, 2.5], B)       # 0.3: knots fall between ticks; 1.0: on them; 2.5: over them
    for b in range(B):
        points[b, n[b]:] = np.nan                                   # rows beyond an instance's own milestones are never read
    return points, n, du


KS = list(range(0, 30)) + [499, 10 ** 6]


def test_linear_tracks_are_traj_targets_bit_for_bit():
    points, n, du = _ragged(11)
    for k in KS:
        assert track_targets(points, n, du, k).tobytes() == traj_targets(points, n, du, k).tobytes(), k
        assert track_targets(points, n, du, k, kind="linear").tobytes() == traj_targets(points, n, du, k).tobytes(), k
    with pytest.raises(ValueError):
        track_targets(points, n, du, 1, kind="linear", tangents=np.zeros_like(points))
    with pytest.raises(ValueError):
        track_targets(points, n, du, 1, kind="cubic")


def test_hermite_tracks_hit_their_milestones_and_clamp_their_ends():
    points, n, _ = _ragged(12)
    B = len(points)
    rows = np.arange(B)
    for k in range(0, 8):
        got = track_targets(points, n, 1.0, k, kind="hermite")      # du = 1: tick k sits on milestone k
        want = points[rows, np.minimum(k, n - 1)]
        assert (got == want).all(), k
    for du in (0.3, np.full(B, 2.5)):
        assert (track_targets(points, n, du, 0, kind="hermite") == points[:, 0]).all()
        assert (track_targets(points, n, du, 10 ** 6, kind="hermite") == points[rows, n - 1]).all()
    assert (track_targets(points, n, -0.5, 3, kind="hermite") == points[:, 0]).all()     # t <= 0: the first milestone


def test_default_tangents_are_spline_tangents_bit_for_bit():
    points, n, du = _ragged(13)
    v = spline_tangents(points, n)
    assert np.isfinite(v).all()
    for k in KS:
        a = track_targets(points, n, du, k, kind="hermite")
        b = track_targets(points, n, du, k, kind="hermite", tangents=v)
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), k
    half = track_targets(points, n, du, 3, kind="hermite", tangents=0.5 * v)
    assert (half != track_targets(points, n, du, 3, kind="hermite")).any()               # ... and the tangents given are the ones used


def test_two_milestones_hermite_is_the_straight_line():
    rng = np.random.default_rng(14)
    points = rng.normal(0, 0.3, (64, 2, 3))
    worst = 0.0
    for k in range(0, 40):
        lin = track_targets(points, None, 1 / 32, k)
        her = track_targets(points, None, 1 / 32, k, kind="hermite")
        scale = np.abs(points).max(axis=1)                           # ulps of the larger milestone: the sum's terms are of that size
        worst = max(worst, float((np.abs(her - lin) / (ULP * scale)).max()))
    print("two milestones, hermite against linear: %.2f ulp" % worst)
    assert worst <= 4.0


def _klampt(points, n, du, k):
    from Robot_Wrapper4 import _HermiteTrajectory, _LinearTrajectory
    return np.array([_HermiteTrajectory().makeSpline(_LinearTrajectory(points[b, :n[b]])).eval(k * du[b]) for b in range(len(points))])


def test_track_targets_is_the_scalar_hermite_trajectory_bit_for_bit():
    points, n, du = _ragged(11)
    B = len(points)
    seen_inner = seen_last = False
    for k in KS:
        got = track_targets(points, n, du, k, kind="hermite")
        ref = _klampt(points, n, du, k)
        assert got.shape == (B, 3) and np.isfinite(got).all()
        assert (got == ref).all(), k
        t = k * du
        seen_inner |= bool(((t > 0) & (t < n - 1) & (t != np.floor(t))).any())
        seen_last |= bool((t >= n - 1).any())
    assert seen_inner and seen_last
    full = np.random.default_rng(15).normal(0, 0.3, (5, 4, 3))      # n_points None = every row full; du a single number
    for k in (0, 1, 7, 400, 999, 1500, 1501):
        assert (track_targets(full, None, 0.002, k, kind="hermite") == _klampt(full, [4] * 5, [0.002] * 5, k)).all()


# ------------------------------------------------------------------------------------------------ spline_tangents
def test_the_worked_example_element_by_element():
    m = np.array([0, 1, 3, 2, 2.5, 2.5, 2.6, 4.0, 4.1, 5.0])
    want = [0.0, 1.5, 0.0, 0.0, 0.0, 0.0, 3.0 * (2.6 - 2.5), 3.0 * (4.1 - 4.0), 3.0 * (4.1 - 4.0), 0.0]
    points = np.stack([m, -m, 2.0 * m], axis=1)[None]               # (mirrored and scaled: the rule is symmetric and homogeneous)
    v = spline_tangents(points)
    for i in range(10):
        assert v[0, i, 0] == want[i], i
        assert v[0, i, 1] == -want[i], i
    from Robot_Wrapper4 import _HermiteTrajectory, _LinearTrajectory
    h = _HermiteTrajectory().makeSpline(_LinearTrajectory(points[0]))
    assert (np.array(h.v) == v[0]).all()


def test_end_tangents_are_zero_and_two_milestones_get_the_chord():
    points, n, _ = _ragged(16)
    v = spline_tangents(points, n)
    rows = np.arange(len(points))
    three = n >= 3
    assert three.any() and (~three).any()
    assert (v[three, 0] == 0).all() and (v[rows[three], n[three] - 1] == 0).all()
    chord = points[~three, 1] - points[~three, 0]
    assert (v[~three, 0] == chord).all() and (v[~three, 1] == chord).all()
    for b in rows:
        assert (v[b, n[b]:] == 0).all()                             # beyond the instance's own milestones: never read, zero
    assert (np.abs(v) > 0).any(axis=(1, 2)).mean() > 0.8


def _worst_excess(points, n):
    """largest distance by which a sample of a segment (201 per segment) lies outside the interval of the segment's two milestones, and the
    same in units of eps x the larger milestone"""
    S = points.shape[1]
    u = np.arange(201) / 200.0
    excess = rel = 0.0
    for seg in range(S - 1):
        rows = n > seg + 1
        lo = np.minimum(points[rows, seg], points[rows, seg + 1])
        hi = np.maximum(points[rows, seg], points[rows, seg + 1])
        scale = np.maximum(np.abs(lo), np.abs(hi))
        for ui in u:
            x = track_targets(points[rows], n[rows], seg + ui, 1, kind="hermite")
            e = np.maximum(lo - x, x - hi)
            excess = max(excess, float(e.max()))
            rel = max(rel, float(np.where(e > 0, e / (ULP * np.maximum(scale, 1e-300)), 0.0).max()))
    return excess, rel


def _random_lists(seed, B=2000, S=7):
    rng = np.random.default_rng(seed)
    points = rng.normal(0, 1.0, (B, S, 3))
    n = rng.integers(2, S + 1, B).astype(np.int32)
    return rng, points, n


def test_no_segment_leaves_the_interval_of_its_milestones():
    """2000 seeded random milestone lists, 201 samples per segment, allowed excess 0"""
    _, points, n = _random_lists(17)
    for b in range(len(points)):
        points[b, n[b]:] = np.nan
    excess, _ = _worst_excess(points, n)
    print("worst excess over the interval of a segment's milestones: %.3e" % excess)
    assert excess <= 0.0


def test_repeated_milestones_stay_within_rounding_of_their_interval():
    """Lists with exactly repeated values (one in seven rounded to a tenth, one in ten copied from its predecessor): on a segment whose two milestones are EQUAL the interval has no
    width and the spline is cx1 * m + cx2 * m with cx1 + cx2 = 1 up to rounding. u2, u3, the three operations of each coefficient, the two
    products and the sum: at most 6 roundings of values <= 3 per coefficient, 9 eps each, and 2 eps for the products and the sum —
    20 eps x |m| bounds the excess there (the arithmetic is the contract, include/wbc.h); everywhere else it is 0 as above."""
    rng, points, n = _random_lists(17)
    points = np.where(rng.random(points.shape) < 0.15, np.round(points, 1), points)
    points[:, 1:] = np.where(rng.random(points[:, 1:].shape) < 0.1, points[:, :-1], points[:, 1:])
    for b in range(len(points)):
        points[b, n[b]:] = np.nan
    flat = points[:, 1:] == points[:, :-1]
    assert flat.sum() > 20                                          # (by construction: there are such segments)
    excess, rel = _worst_excess(points, n)
    print("with repeated milestones: worst excess %.3e = %.2f eps x |milestone|" % (excess, rel))
    assert rel <= 20.0
    open_ = points.copy()                                           # the same lists without their flat segments' rows: excess 0 again
    rows = ~flat.any(axis=(1, 2))
    assert _worst_excess(open_[rows], n[rows])[0] <= 0.0


# ------------------------------------------------------------------------------------------------ the front end
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) before the host checks" % name)


def _front_end(max_batch=8):
    bt = object.__new__(wbc_batch.WbcBatch)           # no handle: the checks under test run before any library call
    bt.lib, bt.max_batch, bt.device_id, bt._h, bt._mh = _NoLibrary(), max_batch, 0, None, []
    return bt


def test_rollout_tracks_checks_before_any_library_call():
    bt = _front_end()
    B = 4
    d = dict(q=np.zeros((B, 27)), ee_target=np.zeros((B, 5, 3)), prev_ee_target=np.zeros((B, 5, 3)),
             trunk_target=np.zeros((B, 3)), prev_trunk_target=np.zeros((B, 3)))
    pts = np.zeros((B, 3, 3))
    ok = dict(target="trunk", points=pts, kind="hermite")
    bad_tracks = [
        [], [dict(target=i % 6, points=pts) for i in range(7)],
        [dict(ok, points=np.zeros((B, 3, 2)))], [dict(ok, points=np.zeros((B + 1, 3, 3)))], [dict(ok, points=np.zeros((B, 9)))],
        [dict(ok, points=np.zeros((B, 1, 3)))], [dict(ok, points=np.zeros((B, capi.MAX_TRAJ_POINTS + 1, 3)))],
        [dict(ok, n_points=np.zeros(B + 1, np.int32))], [dict(ok, du=np.full(B - 1, 0.002))], [dict(ok, du=np.full((B, 2), 0.002))],
        [dict(ok, tangents=np.zeros((B, 2, 3)))], [dict(ok, tangents=np.zeros((B, 3, 3)), kind="linear")],
        [dict(target=4, points=pts, tangents=np.zeros((B, 3, 3)))],                   # (linear is the default kind)
        [ok, dict(target="trunk", points=pts)], [dict(target=4, points=pts), dict(target=4, points=pts, kind="hermite")],   # repeated targets
        [dict(ok, target=6)], [dict(ok, target=-1)], [dict(ok, target="gripper")], [dict(ok, kind="cubic")], [dict(ok, kind=2)],
        [dict(points=pts)], [dict(target=4)], [dict(ok, speed=1.0)],
    ]
    for tracks in bad_tracks:
        with pytest.raises(capi.WbcError):
            bt.rollout_tracks(d, 0.002, 5, tracks)
    bad_calls = [dict(group_size=3), dict(group_size=-1), dict(score=(6,)), dict(score=("trunk", 5)), dict(score=("grip",)),
                 dict(trunk_target_step=np.zeros((B, 3))),                             # together with the trunk track
                 dict(imu=np.zeros((B, 3))), dict(task_params=np.zeros((B, 84)))]
    for kw in bad_calls:
        with pytest.raises(capi.WbcError):
            bt.rollout_tracks(d, 0.002, 5, [ok], **kw)
    with pytest.raises(capi.WbcError):
        bt.rollout_tracks(d, 0.002, 0, [ok])
    no_trunk = {k: v for k, v in d.items() if k != "prev_trunk_target"}
    with pytest.raises(capi.WbcError):
        bt.rollout_tracks(no_trunk, 0.002, 5, [ok])
    with pytest.raises(capi.WbcError):
        bt.rollout_tracks(no_trunk, 0.002, 5, [dict(target=4, points=pts)], score=("trunk",))
    with pytest.raises(capi.WbcError):
        bt.rollout_tracks(d, 0.002, 5, [dict(target=4, points=pts)], trunk_target_step=np.zeros((B, 4)))
    with pytest.raises(AssertionError, match="wbc_rollout_tracks"):    # a well-formed call is the first to reach the library
        bt.rollout_tracks(d, 0.002, 5, [dict(ok, tangents=np.zeros((B, 3, 3)), n_points=np.full(B, 3, np.int32), du=np.full(B, 0.002)),
                                        dict(target=4, points=pts)], score=("trunk", 4), group_size=2, want_trace=True,
                          )
