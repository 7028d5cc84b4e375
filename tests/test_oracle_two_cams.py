"""CPU checks of the oracle's two-camera (Frame.Nleft != -1, KannalaBrandt8 stereo) branches of
SearchByProjection (local map, ORBmatcher.cc:43-213; last frame, :1676-1887) and SearchByBoW(KF, F)
(:223-425): hand-built known-answer cases for each quirk of the reference (the left ratio-test
`continue` that also skips the right search, the right radius not scaled by th, the right BoW ratio
test disabled by "|| true", the empty left window skipping the right last-frame search, the stereo
partner writes through mvLeftToRightMatch / mvRightToLeftMatch), and the literal Python restatement of
the local-map branch (oracle/sbp_definition.py, py_sbp_local_two) compared with the C oracle on seeded
cases. No GPU needed."""
import numpy as np
import pytest

from oracle.sbp_definition import py_sbp_local_two
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import MAP_POINT_DTYPE, PROJ_POINT_DTYPE, FeatureVector, MatchFrame

W = H = 512


def _frame(left, right, l2r=None, r2l=None):
    """left / right: lists of (x, y, octave, angle, desc uint8[32])."""
    pts = list(left) + list(right)
    k = np.zeros(len(pts), KEYPOINT_DTYPE)
    d = np.zeros((len(pts), 32), np.uint8)
    for i, (x, y, o, a, de) in enumerate(pts):
        k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"] = x, y, o, a
        k[i]["size"], k[i]["class_id"] = 31.0, -1
        d[i] = de
    nl = len(left)
    return MatchFrame(k, d, (0.0, float(W), 0.0, float(H)), sm.scale_factors(8), None, 0.0, nleft=nl,
                      l2r=l2r if l2r is not None else np.full(nl, -1), r2l=r2l if r2l is not None else np.full(len(right), -1))


def _desc(seed, flips=0, base=None):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, 32, dtype=np.uint8) if base is None else base.copy()
    if flips:
        bits = np.unpackbits(b)
        bits[rng.choice(256, flips, replace=False)] ^= 1
        b = np.packbits(bits)
    return b


def _mp(desc, x, y, lvl, xr=0.0, yr=0.0, lvl_r=-1, flags=sm.MP_IN_VIEW, obs=5, mid=100, cos=1.0, cos_r=1.0):
    m = np.zeros(1, MAP_POINT_DTYPE)
    m["proj_x"], m["proj_y"], m["scale_level"], m["view_cos"] = x, y, lvl, cos
    m["proj_xr"], m["proj_yr"], m["scale_level_r"], m["view_cos_r"] = xr, yr, lvl_r, cos_r
    m["flags"], m["observations"], m["id"], m["desc"] = flags, obs, mid, desc
    return m


@pytest.fixture(scope="module")
def O(oracle_lib):
    return oracle_lib


def test_local_partner_writes(O):
    """Left match + its mvLeftToRightMatch partner; right-only point + its mvRightToLeftMatch partner."""
    D, E = _desc(1), _desc(2)
    F = _frame([(100, 100, 0, 0, _desc(1, 3)), (300, 300, 0, 0, _desc(2, 40))],
               [(90, 100, 0, 0, _desc(9)), (290, 300, 0, 0, _desc(2, 2))], l2r=[0, -1], r2l=[-1, 1])
    mps = np.concatenate([_mp(D, 100.5, 100.5, 0, mid=7),
                          _mp(E, 0, 0, 0, 290.5, 300.2, 0, flags=sm.MP_IN_VIEW_R, mid=8)])
    mvp, obs = np.full(4, -1, np.int32), np.zeros(4, np.int32)
    n = O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 1.0)
    # point 7: left row 0 and its partner, right row 0 -> slot 2; point 8: right row 1 -> slot 3, partner left row 1
    assert mvp.tolist() == [7, 8, 7, 8] and n == 4


def test_local_left_ratio_continue_skips_right(O):
    """bestLevel == bestLevel2 and bestDist > ratio * bestDist2 -> `continue` (ORBmatcher.cc:115-116):
    the right-camera search of the same point never runs."""
    D = _desc(3)
    F = _frame([(100, 100, 0, 0, _desc(3, 20)), (101, 100, 0, 0, _desc(3, 22))],
               [(200, 200, 0, 0, _desc(3, 1))])
    mps = _mp(D, 100.5, 100.2, 0, 200.3, 200.1, 0, flags=sm.MP_IN_VIEW | sm.MP_IN_VIEW_R)
    mvp, obs = np.full(3, -1, np.int32), np.zeros(3, np.int32)
    assert O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 1.0) == 0 and (mvp == -1).all()
    # without the ambiguous left pair the right search runs and matches
    F2 = _frame([(100, 100, 0, 0, _desc(3, 20))], [(200, 200, 0, 0, _desc(3, 1))])
    mvp, obs = np.full(2, -1, np.int32), np.zeros(2, np.int32)
    assert O.OracleMatcher(0.8).sbp_local(F2, mvp, obs, mps, 1.0) == 2 and mvp.tolist() == [100, 100]


def test_local_right_radius_not_scaled(O):
    """The right search radius is RadiusByViewingCos(mTrackViewCosR) * scale, never * th (:141)."""
    D = _desc(4)
    F = _frame([], [(200, 200, 0, 0, _desc(4, 1))])
    mps = _mp(D, 0, 0, 0, 205.0, 200.0, 0, flags=sm.MP_IN_VIEW_R, cos_r=0.9)   # 5 px away: outside r = 4
    for th in (1.0, 3.0, 15.0):
        mvp, obs = np.full(1, -1, np.int32), np.zeros(1, np.int32)
        assert O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, th) == 0
    mps["proj_xr"] = 203.5
    mvp, obs = np.full(1, -1, np.int32), np.zeros(1, np.int32)
    assert O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 1.0) == 1


def test_local_own_partner_blocks_right(O):
    """The left branch's partner write is visible to the same point's right search: its slot is
    taken (Observations() > 0), so the right best is the next candidate."""
    D = _desc(5)
    F = _frame([(100, 100, 0, 0, _desc(5, 2))], [(90, 100, 0, 0, _desc(5, 1)), (91, 101, 0, 0, _desc(5, 30))],
               l2r=[0], r2l=[0, -1])
    mps = _mp(D, 100.2, 100.1, 0, 90.5, 100.5, 0, flags=sm.MP_IN_VIEW | sm.MP_IN_VIEW_R, obs=3, mid=9)
    mvp, obs = np.full(3, -1, np.int32), np.zeros(3, np.int32)
    n = O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 1.0)
    assert mvp.tolist() == [9, 9, 9] and n == 3   # left 0, partner right 0, right best = right 1
    mps["observations"] = 0   # Observations() == 0 does not block
    mvp, obs = np.full(3, -1, np.int32), np.zeros(3, np.int32)
    n = O.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 1.0)
    assert mvp.tolist() == [9, 9, -1] and n == 4   # right best = right 0 again, its partner left 0 again


def test_lastframe_empty_left_window_skips_right(O):
    D = _desc(6)
    F = _frame([(10, 10, 0, 0, _desc(7))], [(200, 200, 0, 0, _desc(6, 1))])
    p = np.zeros(1, PROJ_POINT_DTYPE)
    p["u"], p["v"], p["invzc"], p["octave"], p["valid"], p["observations"], p["id"], p["desc"] = \
        300, 300, 0.5, 0, 1, 4, 77, D
    ruv = np.array([[200.2, 200.1]], np.float32)
    mvp, obs = np.full(2, -1, np.int32), np.zeros(2, np.int32)
    assert O.OracleMatcher(0.9, False).sbp_lastframe_stereo(F, mvp, obs, p, ruv, 5, False, False) == 0
    p["u"], p["v"] = 11, 11   # left window now holds row 0 (a poor match): the right search runs
    mvp, obs = np.full(2, -1, np.int32), np.zeros(2, np.int32)
    n = O.OracleMatcher(0.9, False).sbp_lastframe_stereo(F, mvp, obs, p, ruv, 5, False, False)
    assert n == 1 and mvp.tolist() == [-1, 77]


def test_bow_right_ratio_disabled(O):
    """The right best is taken with its ratio test "|| true" (:359), only inside the left's
    bestDist1 <= TH_LOW, even when the left ratio test fails."""
    D = _desc(8)
    left = [(10, 10, 0, 0, _desc(8, 10)), (20, 10, 0, 0, _desc(8, 12))]     # 10 vs 12: left ratio fails at 0.6
    right = [(30, 10, 0, 0, _desc(8, 20)), (40, 10, 0, 0, _desc(8, 21))]    # 20 vs 21: ratio would fail
    F = _frame(left, right)
    kk = np.zeros(1, KEYPOINT_DTYPE)
    fk = FeatureVector({5: [0]})
    ff = FeatureVector({5: [0, 1, 2, 3]})
    n, out = O.OracleMatcher(0.6, False).search_by_bow(kk, D[None], np.array([42], np.int32), fk, F, ff)
    assert n == 1 and out.tolist() == [-1, -1, 42, -1]
    # no left candidate within TH_LOW -> no right match either
    F2 = _frame([(10, 10, 0, 0, _desc(8, 90))], right)
    ff2 = FeatureVector({5: [0, 1, 2]})
    n, out = O.OracleMatcher(0.6, False).search_by_bow(kk, D[None], np.array([42], np.int32), fk, F2, ff2)
    assert n == 0 and (out == -1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_local_two_cams_vs_python(O, seed, th):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame_two(rng, 180, 170, w=160, h=120)
    mps = sm.synth_local_map_two(rng, F, 600, copy_frac=0.7)
    mvp0, obs = sm.initial_slots(rng, F.N, 0.2)
    a, b = mvp0.copy(), mvp0.copy()
    na = O.OracleMatcher(0.8).sbp_local(F, a, obs, mps, th)
    nb = py_sbp_local_two(F, b, obs, mps, th, 0.8)
    assert na == nb and na > 0
    np.testing.assert_array_equal(a, b)


def test_two_cams_workload_exercises_branches(O):
    """The seeded two-camera workloads used by the GPU parity tests reach every branch."""
    rng = np.random.default_rng(12)
    F = sm.synth_frame_two(rng, 700, 650)
    mps = sm.synth_local_map_two(rng, F, 4000)
    mvp0, obs = sm.initial_slots(rng, F.N, 0.1)
    a = mvp0.copy()
    n = O.OracleMatcher(0.8).sbp_local(F, a, obs, mps, 3.0)
    changed = np.nonzero(a != mvp0)[0]
    assert n > 500 and (changed < F.nleft).any() and (changed >= F.nleft).any()
