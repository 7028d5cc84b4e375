"""CPU: the argument checks and trivial returns of orbfe_search_by_bow_kf_batch run before any device
call, so they answer on a machine without a GPU. A resident handle cannot be made here; the checks
that need one (nleft ranges, a NULL mp of a keyframe with features) are in
tests/test_gpu_bow_kf_batch.py::test_refusals_with_handles."""
import ctypes

import numpy as np

from orb_slam3_ros_amd import _lib

OK, E_ARG = _lib.ORBFE_OK, _lib.ORBFE_E_ARG


def test_symbols_are_exported(orbfe_lib):
    for name in ("orbfe_search_by_bow_kf_batch", "orbfe_matcher_last_bow_kf_batch", "orbfe_kfdb_detect_nbest"):
        assert getattr(orbfe_lib, name) is not None
    from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
    from orb_slam3_ros_amd.matcher import ORBmatcher
    assert callable(ORBmatcher.SearchByBoWKFBatch) and callable(KeyFrameDatabase.DetectNBestCandidates)


def test_trivial_returns_and_refusals(orbfe_lib):
    call = orbfe_lib.orbfe_search_by_bow_kf_batch
    out, nm = np.full(8, 7, np.int32), np.full(2, 7, np.int32)
    mp1 = np.zeros(8, np.int32)
    kfs, mps = (ctypes.c_void_p * 2)(), (ctypes.c_void_p * 2)()
    o, n = out.ctypes.data, nm.ctypes.data
    # no candidates: nothing to do, whatever the other arguments are
    assert call(None, None, -1, None, None, None, 0, o, n, 0.9, 1) == OK
    assert call(None, None, -1, None, None, None, -1, o, n, 0.9, 1) == E_ARG
    # NULL outputs (the handle argument is never dereferenced: the check comes first)
    assert call(1, mp1.ctypes.data, -1, kfs, mps, None, 2, None, n, 0.9, 1) == E_ARG
    assert call(1, mp1.ctypes.data, -1, kfs, mps, None, 2, o, None, 0.9, 1) == E_ARG
    assert call(1, mp1.ctypes.data, -1, kfs, mps, None, 0, None, None, 0.9, 1) == E_ARG
    # NULL query keyframe, NULL candidate tables
    assert call(None, mp1.ctypes.data, -1, kfs, mps, None, 2, o, n, 0.9, 1) == E_ARG
    assert call(None, mp1.ctypes.data, -1, None, mps, None, 2, o, n, 0.9, 1) == E_ARG
    assert call(None, mp1.ctypes.data, -1, kfs, None, None, 2, o, n, 0.9, 1) == E_ARG
    assert (out == 7).all() and (nm == 7).all()   # a refusal writes nothing


def test_last_form_record(orbfe_lib):
    w = np.full(3, 7, np.int32)
    assert orbfe_lib.orbfe_matcher_last_bow_kf_batch(None) == E_ARG
    out, nm = np.full(8, 7, np.int32), np.full(2, 7, np.int32)
    assert orbfe_lib.orbfe_search_by_bow_kf_batch(None, None, -1, None, None, None, -1, out.ctypes.data,
                                                  nm.ctypes.data, 0.9, 1) == E_ARG
    assert orbfe_lib.orbfe_matcher_last_bow_kf_batch(w.ctypes.data) == OK
    assert w.tolist() == [0, 0, 0]   # a refused call ran no form
