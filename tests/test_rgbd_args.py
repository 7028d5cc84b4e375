"""CPU: the argument checks and trivial returns of the RGB-D entry points (orbfe_frame_rgbd,
orbfe_rgbd_stereo_batch) run before any device call and before the handle is read, so they answer on
a machine without a GPU. An extractor handle cannot be created without a device; the calls below pass
a zeroed placeholder block as the handle, which a correct check order never dereferences."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE, RGBDParams

W, H = 64, 48


@pytest.fixture(scope="module")
def handle():
    return ctypes.create_string_buffer(1 << 16)


def _params(ndist=5):
    return RGBDParams(517.3, 516.5, 31.8, 25.5, [0.26, -0.95, -0.005, 0.002, 1.16, 0, 0, 0, 0, 0, 0, 0][:ndist], 40.0,
                      1.0 / 5000.0)


class _Frame:
    """Well-formed arguments of orbfe_frame_rgbd; a test replaces one of them."""

    def __init__(self, handle):
        self.gray = np.zeros((H, W), np.uint8)
        self.depth = np.zeros((H, W), np.uint16)
        self.kps, self.kun = np.zeros(8, KEYPOINT_DTYPE), np.zeros(8, KEYPOINT_DTYPE)
        self.desc = np.zeros((8, 32), np.uint8)
        self.ur, self.dp = np.zeros(8, np.float32), np.zeros(8, np.float32)
        self.n = ctypes.c_int(7)
        self.p = _params()
        self.a = dict(h=handle, img=self.gray.ctypes.data, width=W, height=H, stride=W, depth=self.depth.ctypes.data,
                      depth_type=_lib.ORBFE_DEPTH_U16, depth_stride=2 * W, p=self.p.ref(), kps=self.kps.ctypes.data,
                      kun=self.kun.ctypes.data, desc=self.desc.ctypes.data, cap=8, n=ctypes.byref(self.n),
                      ur=self.ur.ctypes.data, dp=self.dp.ctypes.data)

    def call(self, lib, **over):
        a = dict(self.a, **over)
        return lib.orbfe_frame_rgbd(*[a[k] for k in ("h", "img", "width", "height", "stride", "depth", "depth_type",
                                                     "depth_stride", "p", "kps", "kun", "desc", "cap", "n", "ur", "dp")])


def test_frame_rgbd_null_arguments(orbfe_lib, handle):
    f = _Frame(handle)
    assert f.call(orbfe_lib, h=None) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, p=None) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, n=None) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, depth=None) == _lib.ORBFE_E_ARG
    assert f.n.value == 0   # *n is cleared as orbfe_extract clears it


@pytest.mark.parametrize("depth_type", [-1, 2, 5])
def test_frame_rgbd_bad_depth_type(orbfe_lib, handle, depth_type):
    assert _Frame(handle).call(orbfe_lib, depth_type=depth_type) == _lib.ORBFE_E_ARG


@pytest.mark.parametrize("ndist", [-1, 1, 3, 6, 7, 9, 11, 13, 14])
def test_frame_rgbd_bad_ndist(orbfe_lib, handle, ndist):
    f = _Frame(handle)
    f.p.c.ndist = ndist
    assert f.call(orbfe_lib) == _lib.ORBFE_E_ARG


def test_frame_rgbd_strides(orbfe_lib, handle):
    f = _Frame(handle)
    assert f.call(orbfe_lib, depth_stride=2 * W - 1) == _lib.ORBFE_E_ARG      # u16: one row is 2 W bytes
    assert f.call(orbfe_lib, depth_type=_lib.ORBFE_DEPTH_F32, depth_stride=4 * W - 1) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, depth_type=_lib.ORBFE_DEPTH_F32, depth_stride=2 * W) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, depth_stride=-4) == _lib.ORBFE_E_ARG
    assert f.call(orbfe_lib, stride=W - 1) == _lib.ORBFE_E_ARG


def test_frame_rgbd_empty_image(orbfe_lib, handle):
    """As orbfe_extract: ORBFE_E_EMPTY and *n = 0 (ORBextractor::operator() returns -1)."""
    f = _Frame(handle)
    for over in (dict(img=None), dict(width=0), dict(height=0), dict(width=-3)):
        f.n.value = 7
        assert f.call(orbfe_lib, **over) == _lib.ORBFE_E_EMPTY
        assert f.n.value == 0


class _Batch:
    def __init__(self, handle):
        self.ptrs = (ctypes.c_void_p * 2)(0x1000, 0x2000)   # never read: every call below returns first
        self.out = np.full((2, 8), 7.0, np.float32)
        self.p = _params()
        self.a = dict(h=handle, base=0, step=1, nframes=2, d_depth=self.ptrs, depth_type=_lib.ORBFE_DEPTH_U16,
                      pitch=2 * W, p=self.p.ref(), keys_un=None, ur=self.out.ctypes.data, dp=self.out.ctypes.data,
                      stream=None)

    def call(self, lib, **over):
        a = dict(self.a, **over)
        return lib.orbfe_rgbd_stereo_batch(*[a[k] for k in ("h", "base", "step", "nframes", "d_depth", "depth_type",
                                                            "pitch", "p", "keys_un", "ur", "dp", "stream")])


def test_batch_argument_checks(orbfe_lib, handle):
    b = _Batch(handle)
    assert b.call(orbfe_lib, h=None) == _lib.ORBFE_E_ARG
    assert b.call(orbfe_lib, p=None) == _lib.ORBFE_E_ARG
    assert b.call(orbfe_lib, nframes=-1) == _lib.ORBFE_E_ARG
    assert b.call(orbfe_lib, d_depth=None) == _lib.ORBFE_E_ARG
    for t in (-1, 2):
        assert b.call(orbfe_lib, depth_type=t) == _lib.ORBFE_E_ARG
    for nd in (-1, 3, 6, 13):
        b.p.c.ndist = nd
        assert b.call(orbfe_lib) == _lib.ORBFE_E_ARG
    assert (b.out == 7.0).all()


def test_batch_of_no_frames(orbfe_lib, handle):
    """nframes == 0 is ORBFE_OK with nothing written, whatever the pointers; the checks on the
    parameters still come first."""
    b = _Batch(handle)
    assert b.call(orbfe_lib, nframes=0) == _lib.ORBFE_OK
    assert b.call(orbfe_lib, nframes=0, d_depth=None, ur=None, dp=None) == _lib.ORBFE_OK
    assert b.call(orbfe_lib, nframes=0, depth_type=9) == _lib.ORBFE_E_ARG
    assert (b.out == 7.0).all()


def test_params_helper():
    p = RGBDParams(1, 2, 3, 4, [0.5, 0, 0, 0], 40.0, 0.25)
    assert ctypes.sizeof(p.c) == 4 * 4 + 12 * 4 + 4 + 4 + 4
    assert (p.c.fx, p.c.cy, p.c.ndist, p.c.bf, p.c.depth_factor) == (1.0, 4.0, 4, 40.0, 0.25)
    assert p.c.dist[0] == 0.5 and p.c.dist[11] == 0.0
    with pytest.raises(_lib.OrbfeError):
        RGBDParams(1, 2, 3, 4, [0.5, 0, 0])
