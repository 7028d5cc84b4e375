"""GPU parity of orbfe_search_by_projection_kf_batch (SearchByProjection(CurrentFrame, pKF, sFound, th,
ORBdist), ORBmatcher.cc:1889-2010, for the candidates of one Tracking::Relocalization sweep in one
launch, projection on the device). Every row and count is checked against the CPU: the projection's
definition in numpy float32 (tests/reloc_sbp_definition.py, pinned by test_reloc_sbp_definition.py)
gives each candidate's records, and OracleMatcher.sbp_kf on them the expected row. The GPU is never
compared with itself. Non-vacuity is asserted on the oracle's outputs."""
import numpy as np
import pytest

import reloc_sbp_definition as D
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures, MatchFrame, ORBmatcher

pytestmark = pytest.mark.gpu
SWEEPS = ((10.0, 100), (3.0, 64))   # Tracking.cc:3765, :3779


@pytest.fixture(scope="module")
def om(oracle_lib):
    return oracle_lib


def _handles(cands):
    """One resident keyframe per distinct KF object (an empty FeatureVector: only the angles are read)."""
    hs = {}
    for c in cands:
        if c is not None and id(c.KF) not in hs:
            hs[id(c.KF)] = KeyFrameFeatures(c.KF, FeatureVector({}))
    return hs


def _check(om, F, cands, th, dist, ori, Fcall=None, model=None, hs=None):
    """One batch call over cands (None: a skipped candidate) against the oracle per candidate."""
    own = hs is None
    hs = _handles(cands) if own else hs
    live = [c for c in cands if c is not None]
    some = live[0]
    mvp = np.stack([(some.row if c is None else c.row) for c in cands]).copy()
    before = mvp.copy()
    nm = ORBmatcher(0.9, ori).SearchByProjectionKeyFrameBatch(
        F if Fcall is None else Fcall, [None if c is None else hs[id(c.KF)] for c in cands],
        [(some if c is None else c).cam for c in cands], [None if c is None else c.points for c in cands],
        [None if c is None else c.kf_idx for c in cands], mvp, th, dist, model=model)
    assert nm.shape == (len(cands),) and nm.dtype == np.int32
    exp = []
    for i, c in enumerate(cands):
        if c is None or len(c.points) == 0:
            en, erow = 0, before[i]
        else:
            en, erow = c.expected(om, F, th, dist, ori)
        exp.append(en)
        assert nm[i] == en, (i, nm[i], en)
        np.testing.assert_array_equal(mvp[i], erow, err_msg=f"candidate {i}")
    if own:
        for h in hs.values():
            h.close()
    return np.asarray(exp), mvp


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("th,dist", SWEEPS)
def test_three_poses(gpu, om, th, dist, ori):
    """C = 3, distinct poses (one rotated by 25 degrees), every rejection path in candidate 0."""
    F, cands = D.scene_main()
    exp, _ = _check(om, F, cands, th, dist, ori)
    assert (exp >= 20).all()


def test_rejection_paths_are_present(om):
    _, reason, clamp, xc = (lambda F, cs: cs[0].records(F))(*D.scene_main())
    counts = {r: int((reason == r).sum()) for r in (D.LEFT, D.RIGHT, D.ABOVE, D.BELOW, D.NEAR, D.FAR)}
    assert all(v >= 1 for v in counts.values()), counts
    assert ((xc[:, 2] < 0) & (reason == D.OK)).sum() >= 2
    assert (clamp == -1).sum() >= 1 and (clamp == 1).sum() >= 1


def test_rows_are_independent(gpu, om):
    """The same pose, points and keyframe twice with different slots held beforehand."""
    F, cands = D.scene_rows()
    for th, dist in SWEEPS:
        exp, rows = _check(om, F, cands, th, dist, True)
        assert not np.array_equal(rows[0], rows[1]) and (exp >= 20).all()


def test_contention_follows_point_order(gpu, om):
    F, cands, (first, count) = D.scene_contention()
    rev = [D.reversed_block(cands[0], first, count), cands[1]]
    for ori in (True, False):
        _, rows = _check(om, F, cands, 10.0, 100, ori)
        _, rrows = _check(om, F, rev, 10.0, 100, ori)
        # (both equal the oracle, whose answers differ: test_reloc_sbp_definition.py)
        assert not np.array_equal(rows[0], rrows[0]) and np.array_equal(rows[1], rrows[1])


def test_rotation_filter_drops_bins(gpu, om):
    F, cands = D.scene_rotation()
    on, _ = _check(om, F, cands, 10.0, 100, True)
    off, _ = _check(om, F, cands, 10.0, 100, False)
    assert on[0] < off[0]


def test_skipped_empty_single_and_many(gpu, om):
    """A NULL candidate and one without points inside a batch, C = 1, and C = 33 tiny candidates."""
    F, cands = D.scene_tiny()
    empty = D.Candidate(cands[1].KF, cands[1].cam, cands[1].points[:0].copy(), cands[1].kf_idx[:0].copy(),
                        cands[1].row)
    mixed = [cands[0], None, cands[2], empty, None, cands[3]]
    for th, dist in SWEEPS:
        _check(om, F, mixed, th, dist, True)
        _check(om, F, cands[:1], th, dist, True)
        exp, _ = _check(om, F, cands, th, dist, True)
        assert len(exp) == 33 and exp.sum() >= 33
    hs = _handles(cands[:1])
    h = hs[id(cands[0].KF)]
    h.close()
    with pytest.raises(ValueError):
        _check(om, F, cands[:1], 10.0, 100, True, hs=hs)
    with pytest.raises(ValueError):
        ORBmatcher(0.9).SearchByProjectionKeyFrameBatch(F, [None], [cands[0].cam], [None, None], [None],
                                                        cands[0].row[None, :].copy(), 10.0, 100)


def test_malformed_slots_are_refused(gpu, om):
    """kf_idx not ascending, or beyond the keyframe: ORBFE_E_ARG, the rows untouched."""
    F, cands = D.scene_tiny(C=2)
    hs = _handles(cands)
    c = cands[0]
    for bad in (c.kf_idx[::-1].copy(), np.full_like(c.kf_idx, c.kf_idx[0]),
                np.append(c.kf_idx[:-1], c.KF.N).astype(np.int32), np.append(-1, c.kf_idx[1:]).astype(np.int32)):
        mvp = np.stack([c.row, cands[1].row]).copy()
        before = mvp.copy()
        with pytest.raises(_lib.OrbfeError):
            ORBmatcher(0.9).SearchByProjectionKeyFrameBatch(
                F, [hs[id(x.KF)] for x in cands], [x.cam for x in cands], [x.points for x in cands],
                [bad, cands[1].kf_idx], mvp, 10.0, 100)
        assert np.array_equal(mvp, before)
    for h in hs.values():
        h.close()


def test_device_view_of_an_extracted_frame(gpu, om):
    """cur as the device view of an extracted frame and as the host view of the same arrays."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_stereo
    from orb_slam3_ros_amd.matcher import current_frame_view
    from orb_slam3_ros_amd.synth import synth_stereo
    bf, fx = 0.110078 * 458.654, 458.654
    el, er = ORBextractor(1000, 1.2, 8, 20, 7), ORBextractor(1000, 1.2, 8, 20, 7)
    left, right = synth_stereo(5, 640, 480)
    (_, kl, dl), _, ur, _, _ = frame_stereo(el, er, left, right, bf, fx)
    fid = _lib.load().orbfe_extractor_frame_id(el.handle)
    F = MatchFrame(kl, dl, (0.0, 640.0, 0.0, 480.0), np.asarray(el.GetScaleFactors(), np.float32), ur, bf)
    assert 200 <= F.N <= 2048
    V = current_frame_view(F, el, fid)
    assert V is not None and V.N == F.N
    rng = np.random.default_rng(4800)
    cands = [D.candidate(rng, F, D.pose(i), 150) for i in range(3)]
    for th, dist in SWEEPS:
        a, _ = _check(om, F, cands, th, dist, True, Fcall=V)
        b, _ = _check(om, F, cands, th, dist, True)
        assert (a >= 20).all() and np.array_equal(a, b)
    el.close()
    er.close()


def test_kannala_brandt8_model(gpu, om):
    F, cands, model = D.scene_kb8()
    for ori in (True, False):
        exp, _ = _check(om, F, cands, 10.0, 100, ori, model=model)
        assert (exp >= 20).all()


def test_at_the_limits(gpu, om):
    """cur.N = 2048, n_pts = 2048, C = 2."""
    F, cands = D.scene_limits()
    exp, _ = _check(om, F, cands, 3.0, 64, True)
    assert (exp >= 1000).all()
