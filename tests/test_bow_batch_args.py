"""CPU: the argument checks and trivial returns of the resident-keyframe entry points
(orbfe_keyframe_destroy, orbfe_search_by_bow_batch) run before any device call, so they answer on a
machine without a GPU."""
import ctypes

import numpy as np

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import FeatureVector, MatchFrame
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE


def _frame(n=8):
    sf = np.asarray([1.0, 1.2], np.float32)
    return MatchFrame(np.zeros(n, KEYPOINT_DTYPE), np.zeros((n, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), sf)


def test_batch_trivial_returns(orbfe_lib):
    F, fv = _frame(), FeatureVector({3: [0, 1]})
    out, nm = np.full(8, 7, np.int32), np.full(1, 7, np.int32)
    call = orbfe_lib.orbfe_search_by_bow_batch
    assert call(None, None, 0, F.ref(), fv.ref(), out.ctypes.data, nm.ctypes.data, 0.75, 1) == _lib.ORBFE_OK
    assert (out == 7).all() and (nm == 7).all()   # nothing to write for no candidates
    assert call(None, None, -1, F.ref(), fv.ref(), out.ctypes.data, nm.ctypes.data, 0.75, 1) == _lib.ORBFE_E_ARG
    kfs, mps = (ctypes.c_void_p * 1)(), (ctypes.c_void_p * 1)()
    assert call(kfs, mps, 1, F.ref(), fv.ref(), None, nm.ctypes.data, 0.75, 1) == _lib.ORBFE_E_ARG
    assert call(kfs, mps, 1, F.ref(), fv.ref(), out.ctypes.data, None, 0.75, 1) == _lib.ORBFE_E_ARG
    assert call(None, mps, 1, F.ref(), fv.ref(), out.ctypes.data, nm.ctypes.data, 0.75, 1) == _lib.ORBFE_E_ARG
    assert call(kfs, mps, 1, None, fv.ref(), out.ctypes.data, nm.ctypes.data, 0.75, 1) == _lib.ORBFE_E_ARG


def test_batch_of_discarded_candidates_needs_no_device(orbfe_lib):
    """Every candidate NULL (pKF->isBad()): rows of -1 and zero counts, no device call."""
    F, fv = _frame(), FeatureVector({3: [0, 1]})
    out, nm = np.full((3, 8), 7, np.int32), np.full(3, 7, np.int32)
    kfs, mps = (ctypes.c_void_p * 3)(), (ctypes.c_void_p * 3)()
    rc = orbfe_lib.orbfe_search_by_bow_batch(kfs, mps, 3, F.ref(), fv.ref(), out.ctypes.data, nm.ctypes.data, 0.75, 1)
    assert rc == _lib.ORBFE_OK and (out == -1).all() and (nm == 0).all()


def test_keyframe_null_handle(orbfe_lib):
    orbfe_lib.orbfe_keyframe_destroy(None)   # a no-op: no device is touched
    assert orbfe_lib.orbfe_keyframe_n(None) == _lib.ORBFE_E_ARG


def test_keyframe_create_checks_before_the_device(orbfe_lib):
    """A refused FeatureVector never reaches the device."""
    F = _frame()
    h = ctypes.c_void_p()
    create = orbfe_lib.orbfe_keyframe_create
    assert create(F.ref(), FeatureVector({3: [0, 8]}).ref(), ctypes.byref(h)) == _lib.ORBFE_E_ARG   # index >= n
    assert h.value is None
    bad = FeatureVector({3: [0], 9: [1]})
    bad.node_ids[:] = [9, 3]
    assert create(F.ref(), bad.ref(), ctypes.byref(h)) == _lib.ORBFE_E_ARG
    off = FeatureVector({3: [0], 9: [1]})
    off.offsets[0] = 1
    assert create(F.ref(), off.ref(), ctypes.byref(h)) == _lib.ORBFE_E_ARG
    assert create(None, off.ref(), ctypes.byref(h)) == _lib.ORBFE_E_ARG
    assert create(F.ref(), FeatureVector({3: [0]}).ref(), None) == _lib.ORBFE_E_ARG
