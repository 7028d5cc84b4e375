"""GPU parity of SearchByBoW on the planted cases of tests/sbow_patterns.py (each proved on the CPU to reach
the rule it names, tests/test_sbow_definition.py): every case through every form its variant has, every slot
and the return value equal to the C++ oracle's.

  SearchByBoW(KF, F) as planted                          k_bow_block (register and LDS node paths)
  SearchByBoW(KF, F), frame padded / keyframe padded     k_bow_nodes + k_bow_commit (keypoint angles)
  SearchByBoWBatch [KF, None, empty keyframe, padded KF] k_bow_batch for rows 0-2, k_bow_nodes + k_bow_commit
                                                         (the pack's angles) for row 3; F on the host and in HBM
  SearchByBoWKF, single and two-camera keyframes         k_bow_kfkf + k_bow_commit (keypoint angles), plain and
                                                         padded
  SearchByBoWKFBatch [KF2, None, padded KF2]             k_bow_kfkf_batch for row 0 (register and LDS node
                                                         paths), k_bow_kfkf + k_bow_commit (both packs' angles)
                                                         for row 2

k_bow_block, k_bow_batch and k_bow_kfkf_batch walk a node with the same bow_walk_node, under the KF-F rules
in the first two and the KF-KF rules in the third.

Padding is inert (sbow_patterns.pad_frame / pad_keyframe), so the expected slots of a padded run are the
planted run's. Which form ran is asserted, not supposed: the drivers record it (orbfe_matcher_last_bow_form,
orbfe_matcher_last_bow_batch, orbfe_matcher_last_bow_kf_batch: host records that touch no kernel), so a moved
LDS bound fails here instead of quietly testing one kernel twice.

Out of scope: SearchForTriangulation's node walk, the two-camera SearchByProjection forms, ComputeBoW.
"""
import ctypes

import numpy as np
import pytest

import sbow_patterns as P
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import DeviceMatchFrame, FeatureVector, KeyFrameFeatures, MatchFrame, ORBmatcher

pytestmark = pytest.mark.gpu

KFF = [c for c in P.all_cases() if c.kind == "kff"]
KFKF = [c for c in P.all_cases() if c.kind == "kfkf"]
# orbfe_matcher_last_bow_form (include/orbfe.h)
FORM_BLOCK, FORM_NODES, FORM_KFKF = 1, 2, 3


@pytest.fixture(scope="module")
def lib(gpu):
    return _lib.load()


def _batch_counts(lib):
    w = (ctypes.c_int32 * 3)()
    assert lib.orbfe_matcher_last_bow_batch(w) == _lib.ORBFE_OK
    return tuple(w)


def _kf_frame(side):
    return MatchFrame(side.keys, side.desc, P.BOUNDS, P.SF)


@pytest.mark.parametrize("case", KFF, ids=repr)
def test_kf_f_every_form(lib, oracle_lib, case):
    n_o, s_o = P.run_oracle(oracle_lib, case)
    m = ORBmatcher(case.nnratio, case.check_ori)
    for c, form in ((case, FORM_BLOCK), (P.pad_frame(case), FORM_NODES), (P.pad_keyframe(case), FORM_NODES)):
        n, s = m.SearchByBoW(c.a.keys, c.a.desc, c.a.mp, c.a.fv, c.F, c.b.fv)
        assert lib.orbfe_matcher_last_bow_form() == form, (c.name, lib.orbfe_matcher_last_bow_form())
        assert n == n_o, (c.name, n, n_o)
        np.testing.assert_array_equal(s[:case.b.N], s_o, err_msg=c.name)
        assert (s[case.b.N:] == -1).all(), c.name


@pytest.mark.parametrize("case", KFF, ids=repr)
def test_kf_f_batch(lib, gpu, oracle_lib, case):
    """[the case's keyframe, a discarded candidate, an empty keyframe, the padded keyframe] against the case's
    F, on the host and device-resident."""
    n_o, s_o = P.run_oracle(oracle_lib, case)
    big = P.pad_keyframe(case)
    empty = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), P.BOUNDS, P.SF)
    kfs = [KeyFrameFeatures(_kf_frame(case.a), case.a.fv), None, KeyFrameFeatures(empty, FeatureVector({})),
           KeyFrameFeatures(_kf_frame(big.a), big.a.fv)]
    mps = [case.a.mp, None, np.zeros(0, np.int32), big.a.mp]
    Fd = DeviceMatchFrame(case.F, gpu)
    Fd.c.device = 1   # orbfe_frame.device: keys and descriptors are HBM pointers (the device view)
    m = ORBmatcher(case.nnratio, case.check_ori)
    for F in (case.F, Fd):
        nm, rows = m.SearchByBoWBatch(kfs, mps, F, case.b.fv)
        assert _batch_counts(lib) == (1, 2, 1)
        assert nm.tolist() == [n_o, 0, 0, n_o]
        np.testing.assert_array_equal(rows[0], s_o)
        np.testing.assert_array_equal(rows[3], s_o)
        assert (rows[1:3] == -1).all()
    for k in kfs:
        if k is not None:
            k.close()


@pytest.mark.parametrize("case", KFKF, ids=repr)
def test_kf_kf(lib, oracle_lib, case):
    n_o, s_o = P.run_oracle(oracle_lib, case)
    m = ORBmatcher(case.nnratio, case.check_ori)
    for c in (case, P.pad_frame(case), P.pad_keyframe(case)):
        a, b = c.a, c.b
        n, s = m.SearchByBoWKF(a.keys, a.desc, a.mp, a.fv, b.keys, b.desc, b.mp, b.fv,
                               -1 if a.nleft is None else a.nleft, -1 if b.nleft is None else b.nleft)
        assert lib.orbfe_matcher_last_bow_form() == FORM_KFKF
        assert n == n_o, (c.name, n, n_o)
        np.testing.assert_array_equal(s[:case.a.N], s_o, err_msg=c.name)
        assert (s[case.a.N:] == -1).all(), c.name


def _kf_batch_form(a, b):
    """The form orbfe_search_by_bow_kf_batch gives candidate b against KF1 a (its host rules, with the LDS
    bound of sbow_patterns.kf_batch_lds): 0 one workgroup, 1 the empty row, 2 the multi-launch path."""
    shared = b is not None and set(a.fv.node_ids.tolist()) & set(b.fv.node_ids.tolist())
    if not shared or not int(a.fv.offsets[-1]) or not int(b.fv.offsets[-1]):
        return 1
    return 0 if P.fits_kf_batch(P.dims(a), P.dims(b)) else 2


@pytest.mark.parametrize("case", KFKF, ids=repr)
def test_kf_kf_batch(lib, oracle_lib, case):
    """[the case's KF2, a discarded candidate, the padded KF2] against the case's KF1 in one call. The
    candidates of this search are side b, which pad_frame pads; the form of each row is worked out on the CPU
    first and the padded row must be past the one-workgroup bound for the padding to be of use."""
    n_o, s_o = P.run_oracle(oracle_lib, case)
    a, big = case.a, P.pad_frame(case).b
    cands = [case.b, None, big]
    modes = [_kf_batch_form(a, b) for b in cands]
    assert modes == [0, 1, 2], (case.name, modes)   # else the padding no longer serves: fix it, not this line
    k1 = KeyFrameFeatures(_kf_frame(a), a.fv)
    kfs = [None if b is None else KeyFrameFeatures(_kf_frame(b), b.fv) for b in cands]
    nl = [-1 if b is None or b.nleft is None else b.nleft for b in cands]
    nm, rows = ORBmatcher(case.nnratio, case.check_ori).SearchByBoWKFBatch(
        k1, a.mp, kfs, [None if b is None else b.mp for b in cands], -1 if a.nleft is None else a.nleft, nl)
    w = np.zeros(3, np.int32)
    assert lib.orbfe_matcher_last_bow_kf_batch(w.ctypes.data) == _lib.ORBFE_OK
    assert w.tolist() == [modes.count(0), modes.count(1), modes.count(2)], (case.name, w, modes)
    assert nm.tolist() == [n_o, 0, n_o], (case.name, nm, n_o)
    np.testing.assert_array_equal(rows[0], s_o, err_msg=case.name)
    np.testing.assert_array_equal(rows[2], s_o, err_msg=case.name)
    assert (rows[1] == -1).all()
    for k in [k1] + kfs:
        if k is not None:
            k.close()
