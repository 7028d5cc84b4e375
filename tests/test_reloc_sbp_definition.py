"""CPU: tests/reloc_sbp_definition.py (the projection of SearchByProjection(F, KF), ORBmatcher.cc:1904-1939,
restated in numpy float32 scalars) pinned against the oracle's C++ before the GPU tests rely on it:
(a) against oracle.is_in_frustum where the two formulas coincide, (b) against the oracle's device-free
SearchByProjection(CurrentFrame, LastFrame) projection at rotated poses, (c) the non-vacuity
conditions of tests/test_gpu_sbp_kf_batch.py on the oracle alone, on that file's seeds."""
import numpy as np
import pytest

import reloc_sbp_definition as D
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import LAST_POINT_DTYPE, MP_IN_VIEW, Camera, CameraModel


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


@pytest.mark.parametrize("t", [(0.0, 0.0, 0.0), (0.3, -0.2, 0.1), (-1.5, 0.4, 2.0)])
def test_pure_translation_equals_is_in_frustum(om, t):
    """(a) R = I: Sophus' point action and isInFrustum's R * P + t are both P + t, so u, v, the bounds
    verdict, the distance verdict and the predicted level must equal Frame::isInFrustum's (view-cosine
    limit below -1, points in front of the camera)."""
    rng = np.random.default_rng(31)
    F = D.frame(rng, 200)
    cam = D.camera(np.eye(3), t)
    cd = D.candidate(rng, F, cam, 160)
    D.plant_rejections(rng, F, cd)
    pts = cd.points[cd.records(F)[3][:, 2] > 0].copy()   # in front of the camera
    pts["flags"] = 0
    pts["normal"] = 0    # viewCos = 0 for every point: above the limit
    rec, reason, _, xc = D.project(F, cam, pts, np.arange(len(pts)), np.zeros(len(pts), np.float32))
    fc = Camera.make(np.eye(3), t, D.FX, D.FY, D.CX, D.CY, 1.2, view_cos_limit=-2.0)
    assert np.array_equal(np.array(fc.Ow[:], np.float32), np.array(cam.Ow[:], np.float32))
    _, track = om.is_in_frustum(F, fc, pts)
    in_bounds = ~np.isin(reason, (D.LEFT, D.RIGHT, D.ABOVE, D.BELOW))
    assert (reason != D.NONFINITE).all() and (~in_bounds).sum() >= 4
    assert (reason == D.NEAR).sum() >= 1 and (reason == D.FAR).sum() >= 1
    # mTrackProjX / Y are written once the projection is inside the image
    written = ~((track["proj_x"] == -1) & (track["proj_y"] == -1))
    np.testing.assert_array_equal(written, in_bounds)
    np.testing.assert_array_equal(track["proj_x"][in_bounds].view(np.uint32), rec["u"][in_bounds].view(np.uint32))
    np.testing.assert_array_equal(track["proj_y"][in_bounds].view(np.uint32), rec["v"][in_bounds].view(np.uint32))
    np.testing.assert_array_equal((track["flags"] & MP_IN_VIEW) != 0, rec["valid"] == 1)
    ok = rec["valid"] == 1
    np.testing.assert_array_equal(track["scale_level"][ok], rec["octave"][ok])
    assert len(set(rec["octave"][ok].tolist())) >= 5


@pytest.mark.parametrize("kind", ["pinhole", "kb8"])
def test_rotated_pose_equals_the_oracle_projection(om, kind):
    """(b) rotated poses: u, v (and z) of the definition, packed into records and searched by
    sbp_lastframe, give the slots sbp_lastframe_pose gives from the same points and pose (its
    projection is the oracle's C++ pose_apply / cam_project)."""
    rng = np.random.default_rng(47)
    kb8 = kind == "kb8"
    F = D.frame(rng, 300, 512, 512) if kb8 else D.frame(rng, 300)
    model = (CameraModel.make("kb8", *sm.TUMVI_LEFT[:4], sm.TUMVI_LEFT[4]) if kb8
             else CameraModel.make("pinhole", D.FX, D.FY, D.CX, D.CY))
    for deg in (12.0, 33.0):
        R, t = D.rotation(rng.normal(size=3), deg), rng.normal(scale=0.4, size=3)
        cam = D.camera(R, t)
        cd = D.candidate(rng, F, cam, 200, model=model if kb8 else None)
        lp = np.zeros(200, LAST_POINT_DTYPE)
        lp["pos"], lp["desc"], lp["id"] = cd.points["pos"], cd.points["desc"], cd.points["id"]
        rec, _, _, xc = D.project(F, cam, cd.points, cd.kf_idx, cd.KF.keys["angle"], model if kb8 else None)
        lp["octave"], lp["angle"] = rec["octave"], rec["angle"]   # the predicted level as nLastOctave
        lp["observations"], lp["valid"] = 1, 1
        rec["valid"], rec["observations"] = 1, 1
        rec["invzc"] = (1.0 / xc[:, 2].astype(np.float64)).astype(np.float32)
        obs = np.zeros(F.N, np.int32)
        a, b = np.full(F.N, -1, np.int32), np.full(F.N, -1, np.int32)
        m = om.OracleMatcher(0.9, True)
        na = m.sbp_lastframe(F, a, obs, np.ascontiguousarray(rec), 7.0, False, False)
        nb = m.sbp_lastframe_pose(F, b, obs, lp, cam.Tcw, model, 7.0, False, False)
        assert na == nb and na >= 40
        np.testing.assert_array_equal(a, b)


def test_main_scene_is_not_vacuous(om):
    """(c) every candidate of the main case finds >= 20 matches under both thresholds, and every
    rejection path and both level clamps are present in the definition's reasons."""
    F, cands = D.scene_main()
    for cd in cands:
        for th, dist in ((10.0, 100), (3.0, 64)):
            for ori in (True, False):
                assert cd.expected(om, F, th, dist, ori)[0] >= 20
    _, reason, clamp, xc = cands[0].records(F)
    for r in (D.LEFT, D.RIGHT, D.ABOVE, D.BELOW, D.NEAR, D.FAR):
        assert (reason == r).sum() >= 1
    assert ((xc[:, 2] < 0) & (reason == D.OK)).sum() >= 2   # behind the camera, searched all the same
    assert (clamp == -1).sum() >= 1 and (clamp == 1).sum() >= 1
    assert max(abs(D.POSES[i][1]) for i in range(3)) >= 20.0


def test_rotation_and_contention_scenes_are_not_vacuous(om):
    F, cands = D.scene_rotation()
    assert cands[0].expected(om, F, 10.0, 100, True)[0] < cands[0].expected(om, F, 10.0, 100, False)[0]
    F, cands, (first, count) = D.scene_contention()
    assert count >= 8
    for ori in (True, False):
        n, row = cands[0].expected(om, F, 10.0, 100, ori)
        nr, rrow = D.reversed_block(cands[0], first, count).expected(om, F, 10.0, 100, ori)
        assert not np.array_equal(row, rrow)   # point order decides
        ids = cands[0].points["id"][first:first + count]
        assert np.isin(row, ids).sum() >= 8    # the later points took their next-best
    F, cands = D.scene_rows()
    a, b = (c.expected(om, F, 10.0, 100, True)[1] for c in cands)
    assert not np.array_equal(a, b)
