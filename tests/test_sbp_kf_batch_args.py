"""CPU: the refusals and trivial returns of orbfe_search_by_projection_kf_batch come before any device
call and before any write to mvp, so they answer on a machine without a GPU (a device call would
return ORBFE_E_DEVICE here). The refusals that need a resident keyframe (malformed kf_idx) are in
tests/test_gpu_sbp_kf_batch.py; a handle of another device needs two devices and is not tested."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import (MAP_POINT_3D_DTYPE, CameraModel, KFCamera, MatchFrame, ORBmatcher, Pose)

SF = np.asarray([1.0, 1.2], np.float32)


def _frame(n=8, **kw):
    return MatchFrame(np.zeros(n, KEYPOINT_DTYPE), np.zeros((n, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), SF, **kw)


class _Args:
    """A well-formed call of C candidates without keyframes (every kfs[c] NULL), to be broken per case."""

    def __init__(self, C=2, n=8, n_pts=3):
        self.F = _frame(n)
        self.C = C
        self.kfs = (ctypes.c_void_p * C)()
        self.cams = (KFCamera * C)()
        for c in range(C):
            self.cams[c] = KFCamera.make(Pose.se3(np.eye(3), np.zeros(3)), 50.0, 50.0, 32.0, 24.0)
        self.points = [np.zeros(n_pts, MAP_POINT_3D_DTYPE) for _ in range(C)]
        self.idx = [np.arange(n_pts, dtype=np.int32) for _ in range(C)]
        self.pp = (ctypes.c_void_p * C)(*[p.ctypes.data for p in self.points])
        self.ip = (ctypes.c_void_p * C)(*[i.ctypes.data for i in self.idx])
        self.npts = np.full(C, n_pts, np.int32)
        self.mvp = np.full((C, n), 7, np.int32)
        self.nm = np.full(C, 7, np.int32)
        self.model = None

    def call(self, lib, **kw):
        a = dict(cur=self.F.ref(), kfs=self.kfs, cams=self.cams, model=self.model, pts=self.pp, idx=self.ip,
                 npts=self.npts.ctypes.data, C=self.C, mvp=self.mvp.ctypes.data, nm=self.nm.ctypes.data)
        a.update(kw)
        return lib.orbfe_search_by_projection_kf_batch(a["cur"], a["kfs"], a["cams"], a["model"], a["pts"], a["idx"],
                                                       a["npts"], a["C"], a["mvp"], a["nm"], 10.0, 100, 1)

    def untouched(self):
        return bool((self.mvp == 7).all())


def test_trivial_returns(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, C=0) == _lib.ORBFE_OK
    assert a.untouched() and (a.nm == 7).all()          # nothing to write for no candidates
    assert a.call(orbfe_lib, C=0, cur=None, kfs=None, mvp=None) == _lib.ORBFE_OK
    # every candidate skipped: zero counts, the rows untouched, no device call
    assert a.call(orbfe_lib) == _lib.ORBFE_OK
    assert a.untouched() and (a.nm == 0).all()


@pytest.mark.parametrize("null", ["cur", "kfs", "cams", "pts", "idx", "npts", "mvp", "nm"])
def test_null_pointers_are_refused(orbfe_lib, null):
    a = _Args()
    assert a.call(orbfe_lib, **{null: None}) == _lib.ORBFE_E_ARG
    assert a.untouched() and (a.nm == 7).all()


def test_bad_arguments_are_refused(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, C=-1) == _lib.ORBFE_E_ARG
    a.npts[1] = -1
    assert a.call(orbfe_lib) == _lib.ORBFE_E_ARG
    a = _Args()
    a.model = ctypes.pointer(CameraModel.make("pinhole", 50.0, 50.0, 32.0, 24.0))
    a.model.contents.type = 5
    assert a.call(orbfe_lib) == _lib.ORBFE_E_ARG
    # a two-camera current frame
    a = _Args()
    two = _frame(8, nleft=4)
    assert a.call(orbfe_lib, cur=two.ref()) == _lib.ORBFE_E_ARG
    # a frame without scale factors / keypoint arrays
    a = _Args()
    a.F.c.scale_factors = None
    assert a.call(orbfe_lib) == _lib.ORBFE_E_ARG
    a = _Args()
    a.F.c.keys = None
    assert a.call(orbfe_lib) == _lib.ORBFE_E_ARG
    assert a.untouched() and (a.nm == 7).all()


def test_capacity_limits_are_refused(orbfe_lib):
    """cur.N = 2049, n_pts = 2049 and a frame whose bounds do not fit the one-workgroup index:
    ORBFE_E_CAPACITY, reported to Python as OrbfeCapacityError, nothing written."""
    a = _Args(n=2049)
    assert a.call(orbfe_lib) == _lib.ORBFE_E_CAPACITY and a.untouched() and (a.nm == 7).all()
    assert _Args(n=2048).call(orbfe_lib) == _lib.ORBFE_OK
    a = _Args(n_pts=2049)
    assert a.call(orbfe_lib) == _lib.ORBFE_E_CAPACITY and a.untouched() and (a.nm == 7).all()
    assert _Args(n_pts=2048).call(orbfe_lib) == _lib.ORBFE_OK
    a = _Args()
    a.F.c.max_x = 70000.0   # blk_geom: image bounds beyond the bucket index
    assert a.call(orbfe_lib) == _lib.ORBFE_E_CAPACITY and a.untouched()
    # through the wrapper
    F = _frame(2049)
    mvp = np.full((1, 2049), 7, np.int32)
    cam = KFCamera.make(Pose.se3(np.eye(3), np.zeros(3)), 50.0, 50.0, 32.0, 24.0)
    with pytest.raises(_lib.OrbfeCapacityError):
        ORBmatcher(0.9).SearchByProjectionKeyFrameBatch(F, [None], [cam], [None], [None], mvp, 10.0, 100)
    assert (mvp == 7).all()


def test_wrapper_checks_its_arguments():
    F = _frame()
    cam = KFCamera.make(Pose.se3(np.eye(3), np.zeros(3)), 50.0, 50.0, 32.0, 24.0)
    m = ORBmatcher(0.9)
    with pytest.raises(ValueError):   # one entry per candidate
        m.SearchByProjectionKeyFrameBatch(F, [None, None], [cam], [None, None], [None, None],
                                          np.full((2, 8), -1, np.int32), 10.0, 100)
    with pytest.raises(ValueError):   # mvp must be [C, N] int32
        m.SearchByProjectionKeyFrameBatch(F, [None], [cam], [None], [None], np.full((1, 7), -1, np.int32), 10.0, 100)
    with pytest.raises(ValueError):
        m.SearchByProjectionKeyFrameBatch(F, [None], [cam], [None], [None], np.full((1, 8), -1, np.int64), 10.0, 100)
