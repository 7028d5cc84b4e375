"""GPU: every planted case of tests/frustum_patterns.py through every device form that turns a 3-D point and a
pose into a record or a query, bit-exactly against the C++ oracle: k_frustum (single pinhole, KannalaBrandt8 and
two-camera), the fused host call with its records, the device-resident call, k_local_batch, k_last_proj with its
search (single and two-camera) and trk_query. The search forms run on keypoints planted around every projection
(frustum_patterns.amplify / LastScene), so a wrong decision, level or 1-ulp projection changes a slot. The only
relaxed comparison is NaN-ness of the projections of the named pinhole (0, 0, +-0) points, in the frustum-only
form."""
import numpy as np
import pytest

import frustum_patterns as P
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import (MP_IN_VIEW, DeviceMatchFrame, LocalMapJob, MatchFrame, ORBmatcher, TrackJob,
                                       is_in_frustum, search_local_points, search_local_points_device)
from test_gpu_local_points_batch import last_batch as last_local_batch
from test_gpu_local_points_batch import plant
from test_gpu_sbp_lastframe_batch import last_batch as last_track_batch

pytestmark = pytest.mark.gpu
FRUSTUM = P.by_kind("frustum")
SEARCHED = [c for c in FRUSTUM if not c.nan]
LAST = P.by_kind("last")
MAXQ = 2048


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def expected(om):
    """Per frustum case, computed once: the oracle's (nToMatch, records), the planted frame and the searched row."""
    out = {}
    for c in FRUSTUM:
        ntm, rec = om.is_in_frustum(c.geom, c.cam, c.flagged(), c.rig)
        e = dict(ntm=ntm, rec=rec)
        if not c.nan:
            F = P.amplify(c, rec)
            mvp, obs = np.full(F.N, -1, np.int32), np.zeros(F.N, np.int32)
            n, ntm2 = om.search_local_points(F, c.cam, c.flagged(), mvp, obs, c.th, False, 50.0, 0.8, c.rig)
            assert ntm2 == ntm
            e.update(F=F, n=n, row=mvp)
        out[c.name] = e
    return out


def test_nothing_is_vacuous(expected):
    live = [c for c in SEARCHED if expected[c.name]["ntm"] > 0]
    assert len(live) >= len(SEARCHED) - 3 and all(expected[c.name]["n"] > 0 for c in live)
    assert [c.name for c in FRUSTUM if c.nan] == ["depth-nan-pinhole"]


@pytest.mark.parametrize("c", FRUSTUM, ids=repr)
def test_k_frustum(gpu, expected, c):
    """is_in_frustum: single pinhole (rig None), single KannalaBrandt8 (rig, one camera), two cameras."""
    e = expected[c.name]
    ntm, rec = is_in_frustum(c.geom, c.cam, c.flagged(), c.rig)
    assert ntm == e["ntm"]
    nan = np.isnan(e["rec"]["proj_x"]) | np.isnan(e["rec"]["proj_y"]) | np.isnan(e["rec"]["proj_xr"])
    assert np.nonzero(nan)[0].tolist() == list(c.nan)            # exactly the named points are relaxed
    P.assert_records_equal(rec, e["rec"], c.nan)


@pytest.mark.parametrize("c", SEARCHED, ids=repr)
def test_fused_host_call(gpu, expected, c):
    """search_local_points(track=True): the records k_frustum wrote for the search, nToMatch and the slots."""
    e = expected[c.name]
    F = e["F"]
    mvp, obs = np.full(F.N, -1, np.int32), np.zeros(F.N, np.int32)
    pts = c.flagged()
    n, ntm, rec = search_local_points(F, c.cam, pts, mvp, obs, c.th, False, 50.0, 0.8, c.rig, track=True)
    assert (n, ntm) == (e["n"], e["ntm"])
    P.assert_records_equal(rec, e["rec"])
    np.testing.assert_array_equal(mvp, e["row"])


@pytest.mark.parametrize("c", SEARCHED, ids=repr)
def test_fused_device_resident(gpu, expected, c):
    import torch
    e = expected[c.name]
    F = e["F"]
    Fd = DeviceMatchFrame(F, gpu)
    mvp = torch.full((F.N,), -1, dtype=torch.int32, device=gpu)
    obs = torch.zeros(F.N, dtype=torch.int32, device=gpu)
    pts = torch.from_numpy(c.flagged().view(np.uint8).reshape(-1).copy()).to(gpu)
    n, ntm = search_local_points_device(Fd, c.cam, pts, mvp, obs, c.th, False, 50.0, 0.8, c.rig)
    assert (n, ntm) == (e["n"], e["ntm"])
    np.testing.assert_array_equal(mvp.cpu().numpy(), e["row"])


def batch_groups():
    """The single-camera cases grouped by what one batch call shares: bounds, scale factors and camera model."""
    groups = {}
    for c in SEARCHED:
        if c.two:
            continue
        model = c.rig.left if c.rig is not None else None
        key = (c.geom.bounds, c.geom.scale_factors.tobytes(), None if model is None else bytes(model))
        groups.setdefault(key, []).append(c)
    return list(groups.values())


GROUPS = batch_groups()


@pytest.mark.parametrize("g", GROUPS, ids=lambda g: f"{g[0].name}+{len(g) - 1}")
def test_k_local_batch(gpu, expected, g):
    """SearchLocalPointsBatch: the group's cases as the frames of one call, each with its own pose, points, th and
    skip list; the first case again as the last frame, a poisoned image and a job without points in between."""
    cases = [g[0], None] + g[1:] + ["empty", g[0]]
    cap = max(64, max(expected[c.name]["F"].N for c in g))
    frames, jobs, exp = [], [], []
    for c in cases:
        if c is None or c == "empty":                            # a poisoned image / a job with n_pts = 0
            frames.append(None if c is None else expected[g[0].name]["F"])
            jobs.append(LocalMapJob.make(g[0].cam, g[0].pts if c is None else None, 1.0, g[0].skip if c is None else None,
                                         want_in_view=True))
            exp.append(c)
            continue
        frames.append(expected[c.name]["F"])
        jobs.append(LocalMapJob.make(c.cam, c.pts, c.th, c.skip, want_in_view=True))
        exp.append(c)
    B = len(cases)
    kps, desc, counts, _ = plant(gpu, frames, 1, 2, False, cap)
    mvp_in, obs_in = np.full((B, cap), -1, np.int32), np.zeros((B, cap), np.int32)
    model = g[0].rig.left if g[0].rig is not None else None
    nm, ntm, nk, out = ORBmatcher(0.8).SearchLocalPointsBatch(kps, desc, counts, cap, 1, 2, None, g[0].geom, jobs, mvp_in,
                                                              obs_in, False, 50.0, model=model)
    searched = skipped = over = 0
    for f, c in enumerate(exp):
        if c is None:
            e0 = expected[g[0].name]
            assert nm[f] == _lib.ORBFE_E_CAPACITY and nk[f] == 5000 and ntm[f] == e0["ntm"] and (out[f] == -1).all()
            over += 1
            continue
        if c == "empty":
            assert (nm[f], ntm[f], nk[f]) == (0, 0, frames[f].N) and (out[f] == -1).all()
            skipped += 1
            continue
        e = expected[c.name]
        print(f"frame {f}: {c.name} N {nk[f]} nToMatch {ntm[f]} / {e['ntm']} nmatches {nm[f]} / {e['n']}")
        assert nk[f] == e["F"].N and ntm[f] == e["ntm"]
        np.testing.assert_array_equal(jobs[f].in_view_flags, (e["rec"]["flags"] & MP_IN_VIEW).astype(np.uint8), err_msg=c.name)
        if e["ntm"] > MAXQ:
            assert nm[f] == _lib.ORBFE_E_CAPACITY and (out[f] == -1).all()
            over += 1
            continue
        assert nm[f] == e["n"], c.name
        np.testing.assert_array_equal(out[f, :e["F"].N], e["row"], err_msg=c.name)
        assert (out[f, e["F"].N:] == -1).all()
        searched += e["ntm"] > 0
        skipped += e["ntm"] == 0
    np.testing.assert_array_equal(out[0], out[B - 1])            # the same case at frame 0 and at the last frame
    assert len(g) < 3 or len({j.th for j in jobs}) == 3          # every th among the frames of a larger call
    assert last_local_batch() == (searched, skipped, over)


def last_expected(om, c):
    mvp, obs = np.full(c.F.N, -1, np.int32), np.zeros(c.F.N, np.int32)
    n = om.OracleMatcher(0.9, False).sbp_lastframe_pose(c.F, mvp, obs, c.pts, c.Tcw, c.model, c.th, c.fw, c.bw, c.Trl)
    return n, mvp


@pytest.mark.parametrize("c", LAST, ids=repr)
def test_k_last_proj(gpu, om, c):
    """SearchByProjectionLastFramePose, single and two-camera: the return value and every slot."""
    n, row = last_expected(om, c)
    assert n == (row >= 0).sum() > 0
    mvp, obs = np.full(c.F.N, -1, np.int32), np.zeros(c.F.N, np.int32)
    ng = ORBmatcher(0.9, False).SearchByProjectionLastFramePose(c.F, mvp, obs, c.pts, c.Tcw, c.model, c.th, c.fw, c.bw, c.Trl)
    assert ng == n
    np.testing.assert_array_equal(mvp, row)


def track_groups():
    groups = {}
    for c in LAST:
        if c.Trl is None:
            groups.setdefault((c.F.bounds, bytes(c.model), c.stereo), []).append(c)
    return list(groups.values())


@pytest.mark.parametrize("g", track_groups(), ids=lambda g: f"{g[0].name}+{len(g) - 1}")
def test_trk_query(gpu, om, g):
    """SearchByProjectionLastFrameBatch: the group's cases as frames of one call (own pose, th, level flags), the first
    again as the last frame, a job without points in between."""
    cases = g + ["empty", g[0]]
    cap = 64
    frames = [g[0].F if c == "empty" else c.F for c in cases]
    jobs = [TrackJob.make(g[0].Tcw, None, 7.0) if c == "empty" else TrackJob.make(c.Tcw, c.pts, c.th, c.fw, c.bw) for c in cases]
    stereo = g[0].stereo
    kps, desc, counts, ur = plant(gpu, frames, 2, 3, stereo, cap)
    geom = MatchFrame(g[0].geom.keys, g[0].geom.desc, g[0].F.bounds, g[0].F.scale_factors, None, P.MBF)
    nm, nk, out = ORBmatcher(0.9, False).SearchByProjectionLastFrameBatch(kps, desc, counts, cap, 2, 3, ur, geom, g[0].model, jobs)
    for f, c in enumerate(cases):
        if c == "empty":
            assert nm[f] == 0 and nk[f] == frames[f].N and (out[f] == -1).all()
            continue
        n, row = last_expected(om, c)
        print(f"frame {f}: {c.name} oracle {n} batch {nm[f]}")
        assert nk[f] == c.F.N and nm[f] == n, c.name
        np.testing.assert_array_equal(out[f, :c.F.N], row, err_msg=c.name)
        assert (out[f, c.F.N:] == -1).all()
    np.testing.assert_array_equal(out[0], out[len(cases) - 1])
    assert len(g) < 4 or len({j.th for j in jobs}) >= 3
    assert last_track_batch() == (len(g) + 1, 1, 0)
