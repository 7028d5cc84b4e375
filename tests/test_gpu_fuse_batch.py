"""GPU parity of the batched Fuse over device-resident keyframes with their search grids (orbfe_fuse_batch:
the Fuse(pKFi, vpMapPointMatches) calls of LocalMapping::SearchInNeighbors, LocalMapping.cc:765-775, and the
Fuse(pKF, Scw, vpPoints, 4, vpReplacePoints) calls of LoopClosing::SearchAndFuse, in one launch). Every row
is checked against the CPU oracle's OracleMatcher.fuse called once per job on the arrays the handle was made
from, with the job's skip mask written into the points as ORBFE_MP_SKIP: nfused[c] equal, best_idx[c] and
best_dist[c] array-equal. The GPU is never compared with itself, except where a test says that two GPU forms
must agree, and then both are also compared with the oracle."""
import ctypes

import numpy as np
import pytest

import backend_patterns as P
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import (MAP_POINT_3D_DTYPE, CameraModel, FeatureVector, FuseJob, KeyFrameFeatures,
                                       KFCamera, MatchFrame, ORBmatcher, Pose, TriJob)

pytestmark = pytest.mark.gpu

MP_SKIP = 4
# The seed of test_random_scenes' six scenes and masks, chosen on the CPU with the oracle alone (seeds 0, 1, 2,
# ... tried in order; the first for which every row of the four parameter sets holds at least 20 fused points
# and every job's mask hides at least one point that the oracle fuses without the mask). The test asserts both.
SCENE_SEED = 0
SCENE_KP = (300, 500, 1000, 300, 500, 1000)
SCENE_PTS = 400


def sigma2_of(K):
    return (K.scale_factors * K.scale_factors).astype(np.float32)


def inv_of(sigma2):
    """mvInvLevelSigma2 as the create forms it: 1.0f / level_sigma2[l] in float."""
    return (np.float32(1.0) / np.asarray(sigma2, np.float32)).astype(np.float32)


class Res:
    """One keyframe: the host arrays the oracle reads and the resident handle with its grid made from them."""

    def __init__(self, K, sigma2=None, handle_from=None, grid=True, fv=None):
        self.K = K
        self.sigma2 = sigma2_of(K) if sigma2 is None else np.asarray(sigma2, np.float32)
        self.fv = FeatureVector({}) if fv is None else fv
        self.h = KeyFrameFeatures(K if handle_from is None else handle_from, self.fv, self.sigma2, grid=grid)

    def close(self):
        self.h.close()


class Job:
    def __init__(self, res, cam, model=None, skip=None, bRight=False):
        self.res, self.cam, self.model, self.bRight = res, cam, model, bRight
        self.skip = None if skip is None else np.asarray(skip, bool)

    def make(self):
        if self.res is None:
            return FuseJob.make(None)
        return FuseJob.make(self.res.h, self.cam, self.model, self.skip, self.bRight)


def _oracle_rows(om, jobs, pts, th, sim3):
    ns, bis, bds = [], [], []
    for j in jobs:
        if j.res is None or j.res.K.N == 0:   # the single call returns 0 before its search
            ns.append(0)
            bis.append(np.full(len(pts), -1, np.int32))
            bds.append(np.full(len(pts), -1, np.int32))
            continue
        p = pts.copy()
        if j.skip is not None:
            p["flags"][j.skip] |= MP_SKIP
        n, bi, bd = om.OracleMatcher().fuse(j.res.K, j.cam, p, th, inv_of(j.res.sigma2), sim3=sim3, model=j.model,
                                            bRight=j.bRight)
        ns.append(n)
        bis.append(bi)
        bds.append(bd)
    return np.asarray(ns, np.int32), np.stack(bis), np.stack(bds)


def _batch(jobs, pts, th, sim3):
    nf, bi, bd = ORBmatcher().FuseBatch([j.make() for j in jobs], pts, th, sim3)
    assert nf.shape == (len(jobs),) and bi.shape == bd.shape == (len(jobs), len(pts))
    return nf, bi, bd


def _check(om, jobs, pts, th, sim3, want=None):
    got = _batch(jobs, pts, th, sim3)
    want = _oracle_rows(om, jobs, pts, th, sim3) if want is None else want
    for g, w, what in zip(got, want, ("nfused", "best_idx", "best_dist")):
        np.testing.assert_array_equal(g, w, err_msg=what)
    live = sum(1 for j in jobs if j.res is not None and j.res.K.N > 0)
    nwg = live and len(jobs) * ((len(pts) + 255) // 256)
    assert ORBmatcher.last_fuse_batch() == ((live, len(jobs) - live, nwg) if len(pts) else (0, len(jobs), 0))
    return want


# ---------------------------------------------------------------- random scenes

def build_scenes(seed=SCENE_SEED):
    """Six keyframes with their own cameras and points; the shared point set is the concatenation of the six
    scenes' points with unique ids, so every keyframe sees its own points pass and the others' fail the
    projection, bounds, distance, view-angle and window gates. masks[c]: job c's skip flags, about 10 %."""
    scenes = []
    for c, n_kp in enumerate(SCENE_KP):
        scenes.append(sm.synth_fuse_scene(np.random.default_rng(1000 * seed + c), n_kp, SCENE_PTS, dup=2))
    pts = np.concatenate([s[2] for s in scenes])
    pts["id"] = 20000 + np.arange(len(pts))
    rng = np.random.default_rng(1000 * seed + 99)
    masks = [rng.random(len(pts)) < 0.1 for _ in scenes]
    return scenes, pts, masks


def scenes_not_vacuous(om, scenes, pts, masks, th, sim3):
    """-> (smallest nfused over the rows, smallest number of masked points per row that the oracle fuses
    without the mask), from the oracle alone."""
    low, hidden = 1 << 30, 1 << 30
    for (KF, cam, _), m in zip(scenes, masks):
        inv = inv_of(sigma2_of(KF))
        p = pts.copy()
        p["flags"][m] |= MP_SKIP
        n, _, _ = om.OracleMatcher().fuse(KF, cam, p, th, inv, sim3=sim3)
        _, free, _ = om.OracleMatcher().fuse(KF, cam, pts, th, inv, sim3=sim3)
        low, hidden = min(low, n), min(hidden, int((free[m] >= 0).sum()))
    return low, hidden


@pytest.fixture(scope="module")
def scene_jobs():
    scenes, pts, masks = build_scenes()
    jobs = [Job(Res(KF), cam, skip=m) for (KF, cam, _), m in zip(scenes, masks)]
    yield scenes, pts, masks, jobs
    for j in jobs:
        j.res.close()


@pytest.mark.parametrize("th", [3.0, 4.0])
@pytest.mark.parametrize("sim3", [False, True], ids=["fuse", "sim3"])
def test_random_scenes(gpu, oracle_lib, scene_jobs, sim3, th):
    scenes, pts, masks, jobs = scene_jobs
    low, hidden = scenes_not_vacuous(oracle_lib, scenes, pts, masks, th, sim3)
    assert low >= 20 and hidden >= 1, (low, hidden)
    want = _check(oracle_lib, jobs, pts, th, sim3)
    assert (want[0] >= 20).all()


def test_batch_of_one_and_repeat(gpu, oracle_lib, scene_jobs):
    """A batch of one equals the single call (GPU against GPU) and both equal the oracle; the same six-job call
    twice, with a call over other jobs and another th in between, gives identical arrays (no stale arena)."""
    scenes, pts, masks, jobs = scene_jobs
    for sim3 in (False, True):
        j = jobs[2]
        p = pts.copy()
        p["flags"][j.skip] |= MP_SKIP
        n1, bi1, bd1 = ORBmatcher().Fuse(j.res.K, j.cam, p, 3.0, inv_of(j.res.sigma2), sim3=sim3)
        want = _check(oracle_lib, [j], pts, 3.0, sim3)
        assert n1 == want[0][0] >= 20
        np.testing.assert_array_equal(bi1, want[1][0])
        np.testing.assert_array_equal(bd1, want[2][0])
    first = _batch(jobs, pts, 3.0, False)
    _check(oracle_lib, [Job(j.res, j.cam) for j in jobs[::-1][:3]], np.ascontiguousarray(pts[:700]), 4.0, True)
    again = _batch(jobs, pts, 3.0, False)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    _check(oracle_lib, jobs, pts, 3.0, False, want=_oracle_rows(oracle_lib, jobs, pts, 3.0, False))


# ---------------------------------------------------------------- the job mix

def test_job_mix(gpu, oracle_lib):
    """In one call: a NULL handle, a keyframe without features, the same handle twice with different poses, a
    job whose skip masks every point, a monocular keyframe (no mvuRight: the 5.99 gate only), a KannalaBrandt8
    model on a single-camera keyframe, and a two-camera keyframe with bRight 0 and 1."""
    rng = np.random.default_rng(31)
    KF, cam, own = sm.synth_fuse_scene(rng, 500, 600, dup=2)
    R, t = cam.Tcw.rotation(), np.array(cam.Tcw.t[:], np.float64)
    cam_b = KFCamera.make(Pose.se3(R, t + np.array([0.004, -0.003, 0.002])), cam.fx, cam.fy, cam.cx, cam.cy)
    KF2 = sm.synth_frame_two(rng, 500, 450)
    rcam = sm.synth_camera(rng, rot_deg=20.0)
    rig = sm.synth_rig(rcam, True)
    rpts = sm.synth_local_map_3d_rig(rng, KF2, rcam, 3000, two=True)
    pts = np.concatenate([own, rpts])
    pts["id"] = 20000 + np.arange(len(pts))
    mono = MatchFrame(KF.keys, KF.desc, KF.bounds, KF.scale_factors, None, KF.mbf)
    none = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), KF.bounds, KF.scale_factors)
    kb8 = CameraModel.make("kb8", cam.fx, cam.fy, cam.cx, cam.cy, (-0.01, 0.003, -0.001, 0.0002))
    a, m, e, two = Res(KF), Res(mono), Res(none), Res(KF2)
    assert two.h.has_grid() and two.h.has_geom and e.h.has_grid() and e.h.N == 0
    jobs = [Job(None, None), Job(e, cam), Job(a, cam), Job(a, cam_b), Job(a, cam, skip=np.ones(len(pts), bool)),
            Job(m, cam), Job(a, cam, model=kb8),
            Job(two, sm.left_kf_camera(rcam), model=rig.left), Job(two, sm.right_kf_camera(rcam, rig), model=rig.right,
                                                                   bRight=True)]
    for sim3 in (False, True):
        use = jobs[:-1] if sim3 else jobs   # bRight needs sim3 == 0
        n, bi, bd = _check(oracle_lib, use, pts, 3.0, sim3)
        assert n[0] == n[1] == n[4] == 0 and (bi[0] == -1).all() and (bd[0] == -1).all() and (bi[4] == -1).all()
        assert n[2] >= 20 and n[3] >= 20 and n[5] >= 20 and n[7] >= 20, n
        assert not np.array_equal(bd[2], bd[3])   # the second pose is another search
        if not sim3:
            assert n[8] >= 20 and (bi[8][bi[8] >= 0] >= KF2.nleft).all() and (bi[7] < KF2.nleft).all()
            assert not np.array_equal(bi[2], bi[5])   # without mvuRight the stereo gate does not apply
    for r in (a, m, e, two):
        r.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts_at_the_chunk_edges(gpu, oracle_lib, n):
    rng = np.random.default_rng(7)
    KF, cam, pts = sm.synth_fuse_scene(rng, 300, 300, dup=1)
    r = Res(KF)
    # the points the oracle fuses come first, so that a one-point call is not an empty one
    _, free, _ = oracle_lib.OracleMatcher().fuse(KF, cam, pts, 3.0)
    order = np.argsort(free < 0, kind="stable")
    p = np.ascontiguousarray(pts[order][:n])
    skip = np.zeros(n, bool)
    skip[n // 2::7] = n > 1
    for sim3 in (False, True):
        want = _check(oracle_lib, [Job(r, cam), Job(r, cam, skip=skip)], p, 3.0, sim3)
        assert want[0][0] >= min(n, 20), want[0]
    r.close()


# ---------------------------------------------------------------- planted rules

FUSE = [c for c in P.all_cases() if c.entry in ("fuse", "fuse-sim3")]
MUST = ("depth-zero", "image-edge", "view-half", "window-edge", "level-gate", "chi2-stereo-7.8", "chi2-mono-5.99",
        "no-uright", "tie-first-wins", "flags")


def test_planted_families_present():
    names = [c.name for c in FUSE]
    assert any(c.entry == "fuse" for c in FUSE) and any(c.entry == "fuse-sim3" for c in FUSE)
    for fam in MUST:
        assert any(n.startswith(fam) for n in names), fam


def realised_sigma2(inv):
    """level_sigma2 for a planted mvInvLevelSigma2. The handle forms 1.0f / level_sigma2[l] as the reference
    does, and near 7.8 one step of level_sigma2 moves that quotient by two steps, so not every float is a
    quotient (7.8f is none). A level takes the level_sigma2 whose quotient is the planted value where one
    exists; otherwise the nearest quotient that stands on the same side of both chi-square constants (7.8,
    5.99, compared as double, the planted cases' e2 being 1). -> (level_sigma2, exact)."""
    out, exact = [], True
    for v in np.asarray(inv, np.float32):
        s0 = np.float32(1.0) / v
        cands = [s0]
        for _ in range(4):
            cands = [np.nextafter(cands[0], np.float32(0))] + cands + [np.nextafter(cands[-1], np.float32(np.inf))]
        side = lambda x: (float(x) > 7.8, float(x) > 5.99)   # noqa: E731
        ok = [s for s in cands if side(np.float32(1.0) / s) == side(v)]
        best = min(ok, key=lambda s: abs(float(np.float32(1.0) / s) - float(v)))
        exact = exact and np.float32(1.0) / best == v
        out.append(best)
    return np.asarray(out, np.float32), exact


@pytest.fixture(scope="module")
def strangers():
    """Two random keyframes unrelated to any planted case, as the jobs on either side of it."""
    rng = np.random.default_rng(5)
    out = []
    for n in (150, 90):
        K = sm.synth_frame(rng, n, stereo=True)
        out.append(Job(Res(K), sm.synth_kf_camera(rng)))
    yield out
    for j in out:
        j.res.close()


@pytest.mark.parametrize("case", FUSE, ids=repr)
def test_planted_rules(gpu, oracle_lib, strangers, case):
    """Every planted Fuse case as the middle job of three, between two unrelated keyframes that search the
    case's points as well: the case's row passes the case's own check (against the trace of the definition)
    and equals the oracle's row; where every planted invSigma2 is a quotient 1.0f / sigma2, the row also
    equals the oracle on the case exactly as planted."""
    c = case
    sim3 = c.entry == "fuse-sim3"
    sigma2, exact = realised_sigma2(c.inv_sigma2)
    k = Job(Res(c.F, sigma2), c.cam)
    jobs = [strangers[0], k, strangers[1]]
    n, bi, bd = _check(oracle_lib, jobs, c.pts, c.th, sim3)
    _, tr = P.run_definition(c)
    c.check(c, tr, (int(n[1]), bi[1], bd[1]))
    if exact:
        want = P.run_oracle(oracle_lib, c)
        assert n[1] == want[0]
        np.testing.assert_array_equal(bi[1], want[1])
        np.testing.assert_array_equal(bd[1], want[2])
    k.res.close()


# ---------------------------------------------------------------- device views and refusals

def test_device_view_create(gpu, oracle_lib):
    """A handle with its grid made from the device view of an extracted frame (keys, descriptors, mvuRight and
    scale factors copied device to device, the grids built from the view's keys) and one from the host copy
    of the same frame give the same rows, the oracle's."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_stereo
    from orb_slam3_ros_amd.matcher import Camera, current_frame_view
    from orb_slam3_ros_amd.synth import synth_stereo
    bf, fx = 0.110078 * 458.654, 458.654
    el, er = ORBextractor(1000, 1.2, 8, 20, 7), ORBextractor(1000, 1.2, 8, 20, 7)
    left, right = synth_stereo(5, 752, 480)
    (ml, kl, dl), _, ur, _, _ = frame_stereo(el, er, left, right, bf, fx)
    fid = _lib.load().orbfe_extractor_frame_id(el.handle)
    sf = np.asarray(el.GetScaleFactors(), np.float32)
    F = MatchFrame(kl, dl, (0.0, 752.0, 0.0, 480.0), sf, ur, bf)
    V = current_frame_view(F, el, fid)
    assert V is not None and V.N == F.N and F.N > 300 and (ur >= 0).sum() > 50
    rng = np.random.default_rng(8)
    cam = sm.synth_kf_camera(rng)
    c = Camera.make(cam.Tcw.rotation(), np.array(cam.Tcw.t[:], np.float64), cam.fx, cam.fy, cam.cx, cam.cy)
    pts = sm.synth_local_map_3d(rng, F, c, 600, copy_frac=0.6)
    pts["id"] = 20000 + np.arange(len(pts))
    dev, host = Res(F, handle_from=V), Res(F)
    assert dev.h.has_grid() and host.h.has_grid() and dev.h.N == F.N
    for sim3 in (False, True):
        n, bi, bd = _check(oracle_lib, [Job(dev, cam), Job(host, cam)], pts, 3.0, sim3)
        assert n[0] == n[1] >= 20
        np.testing.assert_array_equal(bi[0], bi[1])
        np.testing.assert_array_equal(bd[0], bd[1])
    dev.close()
    host.close()


def test_refusals_with_handles(gpu, oracle_lib, scene_jobs):
    """A handle with geometry but no grid, and bRight on a single-camera handle (or with sim3 on a two-camera
    one), are refused with ORBFE_E_ARG and the outputs keep their sentinel."""
    lib = _lib.load()
    scenes, pts, masks, jobs = scene_jobs
    j = jobs[0]
    geom_only = Res(j.res.K, grid=False)
    assert geom_only.h.has_geom and not geom_only.h.has_grid() and j.res.h.has_grid()
    rng = np.random.default_rng(3)
    two = Res(sm.synth_frame_two(rng, 60, 50))
    n = len(pts)

    def call(fj, sim3=0):
        bi, bd, nf = np.full(2 * n, 7, np.int32), np.full(2 * n, 7, np.int32), np.full(2, 7, np.int32)
        arr = (FuseJob * 2)()
        for c, x in enumerate((FuseJob.make(None), fj)):
            ctypes.memmove(ctypes.byref(arr, c * ctypes.sizeof(FuseJob)), ctypes.byref(x), ctypes.sizeof(FuseJob))
        rc = lib.orbfe_fuse_batch(arr, 2, pts.ctypes.data, n, 3.0, sim3, bi.ctypes.data, bd.ctypes.data, nf.ctypes.data)
        assert (bi == 7).all() and (bd == 7).all() and (nf == 7).all()
        return rc
    assert call(FuseJob.make(geom_only.h, j.cam)) == _lib.ORBFE_E_ARG
    assert call(FuseJob.make(j.res.h, j.cam, bRight=True)) == _lib.ORBFE_E_ARG
    assert call(FuseJob.make(two.h, j.cam, bRight=True), sim3=1) == _lib.ORBFE_E_ARG
    bad_model = FuseJob.make(j.res.h, j.cam)
    bad_model.model.type = 2
    assert call(bad_model) == _lib.ORBFE_E_ARG
    bad_pose = FuseJob.make(j.res.h, j.cam)
    bad_pose.cam.Tcw.kind = 2
    assert call(bad_pose) == _lib.ORBFE_E_ARG
    assert ORBmatcher.last_fuse_batch() == (0, 0, 0)
    # the Python wrapper's own refusals
    with pytest.raises(ValueError):
        ORBmatcher().FuseBatch([FuseJob.make(j.res.h, j.cam, skip=np.zeros(n - 1, bool))], pts)
    with pytest.raises(ValueError):
        ORBmatcher().FuseBatch([TriJob.make(None)], pts)
    closed = KeyFrameFeatures(j.res.K, FeatureVector({}), j.res.sigma2, grid=True)
    fj = FuseJob.make(closed, j.cam)
    closed.close()
    with pytest.raises(ValueError):
        ORBmatcher().FuseBatch([fj], pts)
    with pytest.raises(ValueError):
        FuseJob.make(closed, j.cam)
    geom_only.close()
    two.close()


def test_grid_handle_serves_the_other_batches(gpu, oracle_lib):
    """A handle with its grid is a handle with geometry: SearchForTriangulationBatch and SearchByBoWBatch give
    the rows they give on a geometry handle of the same arrays (GPU against GPU), which are the oracle's."""
    rng = np.random.default_rng(4100)
    K1, fv1, mp1, sg1, nbs = sm.synth_tri_scene(rng, 203, 2, 300, False)
    nb = nbs[0]
    k1g, k1 = KeyFrameFeatures(K1, fv1, sg1, grid=True), KeyFrameFeatures(K1, fv1, sg1)
    k2g, k2 = KeyFrameFeatures(nb.K, nb.fv, nb.sigma2, grid=True), KeyFrameFeatures(nb.K, nb.fv, nb.sigma2)
    assert k1g.has_grid() and k1g.has_geom and not k1.has_grid()
    m = ORBmatcher(0.6, True)
    rows = []
    for a, b in ((k1g, k2g), (k1, k2)):
        rows.append(m.SearchForTriangulationBatch(a, mp1, [TriJob.make(b, nb.mp, nb.F12, nb.ep)], False, False))
    no, oo = oracle_lib.OracleMatcher(0.6, True).search_for_triangulation(K1, mp1, fv1, nb.K, nb.mp, nb.fv, nb.F12, nb.ep,
                                                                          nb.sigma2, False, False)
    for nm, out in rows:
        assert nm[0] == no > 20
        np.testing.assert_array_equal(out[0], oo)
    mp2 = np.where(rng.random(nb.K.N) < 0.6, 5, -1).astype(np.int32)
    bows = [ORBmatcher(0.75, True).SearchByBoWBatch([h], [mp2], K1, fv1) for h in (k2g, k2)]
    no, oo = oracle_lib.OracleMatcher(0.75, True).search_by_bow(nb.K.keys, nb.K.desc, mp2, nb.fv, K1, fv1)
    for nm, out in bows:
        assert nm[0] == no
        np.testing.assert_array_equal(out[0], oo)
    for h in (k1g, k1, k2g, k2):
        h.close()
