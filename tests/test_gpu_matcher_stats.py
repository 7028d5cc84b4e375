"""GPU: the matcher's counting mode (orbfe_matcher_set_stats / orbfe_matcher_last_stats) and device
timing (orbfe_matcher_set_timing / orbfe_matcher_last_ms), one small search per SearchByProjection
driver. Each shape is the smallest that takes its path through sbp_run's dispatch (one workgroup up to
2,048 keypoints and 2,048 points; k_sbp_multi0 + k_sbp_multi below th 4, k_sbp_band from there;
k_sbp_local_wq from th 2.5 once the frame is past 2,048 keypoints, k_sbp_local below).

Counting must not change a result (slots and return value equal the oracle's with it on and off), is
repeatable call after call on one thread, and is reported per call: a search without it leaves
orbfe_matcher_last_stats at ORBFE_E_ARG. The words are {window candidates, Hamming pairs, passes}.

What each driver reports, read from the kernels:
  * the multi-block passes k_sbp_local, k_sbp_local_wq and k_sbp_band add both counts in pass_stats,
    a pair being a window candidate that reached the Hamming test: 0 < pairs <= candidates;
  * k_sbp_proj takes the PassIO but never calls pass_stats: the call reports ORBFE_OK with
    {0, 0, passes}, the passes counted on the host. That row alone is exempt from pairs > 0, because
    the kernel has nothing to count with; it is held to exactly {0, 0, passes >= 1} instead;
  * the one-workgroup searches k_sbp_block<0..2>, k_sbp_block2 and k_sbp_block4 all do report: each adds
    its pair count to words 0 and 1 alike and stores passes in word 2, and sbp_block_run /
    sbp_block2_run read the three words back as they are;
  * k_sbp_multi0 + k_sbp_multi only ever add to word 1 (multi_pass_end); the host reports it as word 0
    too, which is what bench.py prints as that path's window candidates: word 0 == word 1;
  * the two-camera multi-launch forms (k_sbp_local2, k_sbp_proj2) never write the words: ORBFE_E_ARG.
"""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import ORBmatcher

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


def _local(seed, n_kp, n_mps, th):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame(rng, n_kp)
    mps = sm.synth_local_map(rng, F, n_mps)
    mvp0, obs = sm.initial_slots(rng, F.N)
    return (mvp0, lambda mvp: ORBmatcher(0.8).SearchByProjectionLocalMap(F, mvp, obs, mps, th),
            lambda o, mvp: o.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, th))


def _lastframe(seed, n_kp, n_pts):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame(rng, n_kp)
    pts = sm.synth_proj_points(rng, F, n_pts)
    mvp0, obs = sm.initial_slots(rng, F.N, 0.2)
    return (mvp0, lambda mvp: ORBmatcher(0.9, True).SearchByProjectionLastFrame(F, mvp, obs, pts, 7, False, False),
            lambda o, mvp: o.OracleMatcher(0.9, True).sbp_lastframe(F, mvp, obs, pts, 7, False, False))


def _keyframe(seed, n_kp, n_pts):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame(rng, n_kp, stereo=False)
    pts = sm.synth_proj_points(rng, F, n_pts)
    mvp0, _ = sm.initial_slots(rng, F.N, 0.2)
    return (mvp0, lambda mvp: ORBmatcher(0.9, True).SearchByProjectionKeyFrame(F, mvp, pts, 10, 100),
            lambda o, mvp: o.OracleMatcher(0.9, True).sbp_kf(F, mvp, pts, 10, 100))


def _local_two(seed, n_mps):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame_two(rng, 150, 150)
    mps = sm.synth_local_map_two(rng, F, n_mps)
    mvp0, obs = sm.initial_slots(rng, F.N, 0.15)
    return (mvp0, lambda mvp: ORBmatcher(0.8).SearchByProjectionLocalMap(F, mvp, obs, mps, 3),
            lambda o, mvp: o.OracleMatcher(0.8).sbp_local(F, mvp, obs, mps, 3))


def _lastframe_two(seed, n_pts):
    rng = np.random.default_rng(seed)
    F = sm.synth_frame_two(rng, 150, 150)
    pts, ruv = sm.synth_proj_points_two(rng, F, n_pts)
    mvp0, obs = sm.initial_slots(rng, F.N, 0.2)
    return (mvp0,
            lambda mvp: ORBmatcher(0.9, True).SearchByProjectionLastFrameStereo(F, mvp, obs, pts, ruv, 7, False, False),
            lambda o, mvp: o.OracleMatcher(0.9, True).sbp_lastframe_stereo(F, mvp, obs, pts, ruv, 7, False, False))


# kind: "pass" / "block" pairs <= window candidates; "multi" word 0 == word 1; "proj" passes only;
# "none" nothing reported
CASES = {
    "k_sbp_block0": (lambda: _local(101, 300, 400, 3), "block"),
    "k_sbp_block1": (lambda: _lastframe(102, 300, 400), "block"),
    "k_sbp_block2_kf": (lambda: _keyframe(103, 300, 400), "block"),
    "k_sbp_multi": (lambda: _local(104, 300, 2049, 3), "multi"),
    "k_sbp_band": (lambda: _local(105, 300, 2049, 5), "pass"),
    "k_sbp_local_wq": (lambda: _local(106, 2049, 2049, 5), "pass"),
    "k_sbp_local": (lambda: _local(107, 2049, 2049, 1), "pass"),
    "k_sbp_proj": (lambda: _lastframe(108, 300, 2049), "proj"),
    "k_sbp_block4": (lambda: _local_two(109, 400), "block"),
    "k_sbp_block2": (lambda: _lastframe_two(110, 400), "block"),
    "k_sbp_local2": (lambda: _local_two(111, 2049), "none"),
    "k_sbp_proj2": (lambda: _lastframe_two(112, 2049), "none"),
}


def _last_stats(lib):
    w = (ctypes.c_longlong * 3)()
    rc = lib.orbfe_matcher_last_stats(w)
    return rc, [int(x) for x in w]


@pytest.mark.parametrize("name", list(CASES))
def test_matcher_stats_and_timing(gpu, om, name):
    lib = _lib.load()
    build, kind = CASES[name]
    mvp0, run_gpu, run_oracle = build()
    mvp_o = mvp0.copy()
    n_o = run_oracle(om, mvp_o)

    def search():
        mvp = mvp0.copy()
        n = run_gpu(mvp)
        assert n == n_o
        np.testing.assert_array_equal(mvp, mvp_o)

    try:
        lib.orbfe_matcher_set_stats(0)
        lib.orbfe_matcher_set_timing(0)
        search()
        assert _last_stats(lib) == (_lib.ORBFE_E_ARG, [-1, -1, -1])
        assert lib.orbfe_matcher_last_ms() == -1.0

        lib.orbfe_matcher_set_stats(1)
        search()
        rc, w = _last_stats(lib)
        print(name, "stats", rc, w)
        if kind == "none":
            assert (rc, w) == (_lib.ORBFE_E_ARG, [-1, -1, -1])
        else:
            assert rc == _lib.ORBFE_OK
            cands, pairs, passes = w
            assert passes >= 1
            if kind == "proj":
                assert (cands, pairs) == (0, 0)
            elif kind == "multi":
                assert cands == pairs
            else:
                assert pairs <= cands
        # the same search again on this thread: only generation tags and sequence numbers advance
        search()
        assert _last_stats(lib) == (rc, w)

        lib.orbfe_matcher_set_stats(0)
        search()
        assert _last_stats(lib) == (_lib.ORBFE_E_ARG, [-1, -1, -1])

        lib.orbfe_matcher_set_timing(1)
        search()
        ms = lib.orbfe_matcher_last_ms()
        print(name, "device ms", ms)
        assert ms > 0
        lib.orbfe_matcher_set_timing(0)
        search()
        assert lib.orbfe_matcher_last_ms() == -1.0
        assert kind in ("none", "proj") or w[1] > 0
    finally:
        lib.orbfe_matcher_set_stats(0)
        lib.orbfe_matcher_set_timing(0)
