"""CPU: every refusal of orbfe_search_local_points_slabs comes before any device call and before any write
to its outputs, so it answers on a machine without a GPU (a device call would return ORBFE_E_DEVICE here).
The slab pointers are dummies: a refused call never reads them."""
import ctypes
import re

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import MAP_POINT_3D_DTYPE, Camera, CameraModel, LocalMapJob, MatchFrame

SF = np.asarray([1.0, 1.2], np.float32)
OK, E_ARG, E_CAP = _lib.ORBFE_OK, _lib.ORBFE_E_ARG, _lib.ORBFE_E_CAPACITY
CAM = Camera.make(np.eye(3), np.zeros(3), 50.0, 50.0, 32.0, 24.0)


def _max_points():
    src = open(_lib.HEADER_PATH).read()
    return int(re.search(r"#define ORBFE_LOCAL_BATCH_MAX_POINTS (\d+)", src).group(1))


class _Args:
    """A well-formed call of B frames over dummy slabs, to be broken per case."""

    def __init__(self, B=2, cap=8, n_pts=5):
        self.geom = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), SF)
        self.model = CameraModel.make("pinhole", 50.0, 50.0, 32.0, 24.0)
        self.B, self.cap = B, cap
        self.points = [np.zeros(n_pts, MAP_POINT_3D_DTYPE) for _ in range(B)]
        self.skip = [np.asarray([0, n_pts - 1], np.int32) for _ in range(B)]
        self.jobs = (LocalMapJob * B)()
        self.fill_jobs()
        self.dummy = np.zeros(64, np.uint8)
        self.mvp_in = np.full((B, cap), -1, np.int32)
        self.obs = np.zeros((B, cap), np.int32)
        self.mvp = np.full((B, cap), 7, np.int32)
        self.nm = np.full(B, 7, np.int32)
        self.ntm = np.full(B, 7, np.int32)
        self.nk = np.full(B, 7, np.int32)

    def fill_jobs(self):
        self.kept = [LocalMapJob.make(CAM, self.points[f], 3.0, self.skip[f], want_in_view=True) for f in range(self.B)]
        for f, j in enumerate(self.kept):
            j.in_view_flags[:] = 7
            self.jobs[f] = j

    def call(self, lib, **kw):
        d = self.dummy.ctypes.data
        a = dict(kps=d, desc=d, counts=d, cap=self.cap, base=0, step=1, ur=d, geom=self.geom.ref(), model=None,
                 jobs=self.jobs, B=self.B, mvp_in=self.mvp_in.ctypes.data, obs=self.obs.ctypes.data,
                 mvp=self.mvp.ctypes.data, nm=self.nm.ctypes.data, ntm=self.ntm.ctypes.data, nk=self.nk.ctypes.data)
        a.update(kw)
        return lib.orbfe_search_local_points_slabs(
            a["kps"], a["desc"], a["counts"], a["cap"], a["base"], a["step"], a["ur"], a["geom"], a["model"], a["jobs"],
            a["B"], a["mvp_in"], a["obs"], 0, 50.0, 0.8, a["mvp"], a["nm"], a["ntm"], a["nk"], None)

    def untouched(self):
        return bool((self.mvp == 7).all() and (self.nm == 7).all() and (self.ntm == 7).all() and (self.nk == 7).all()
                    and all((j.in_view_flags == 7).all() for j in self.kept))


def _last(lib):
    w = np.full(3, -9, np.int32)
    assert lib.orbfe_matcher_last_local_batch(w.ctypes.data) == OK
    return tuple(int(v) for v in w)


def test_symbols_are_declared_and_exported(orbfe_lib):
    src = open(_lib.HEADER_PATH).read()
    for name in ("orbfe_search_local_points_slabs", "orbfe_matcher_last_local_batch",
                 "orbfe_matcher_last_local_uploads"):
        assert hasattr(orbfe_lib, name), name
        assert re.search(r"\bint " + name + r"\(", src), name
    assert orbfe_lib.orbfe_matcher_last_local_batch(None) == E_ARG
    assert _max_points() >= 16384


def test_local_job_layout_matches_the_header():
    """orbfe_local_job: the header's field order and its 128 bytes, camera first."""
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct orbfe_local_job \{(.*?)\} orbfe_local_job;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in LocalMapJob._fields_] == ["cam", "pts", "n_pts", "skip", "n_skip", "th", "in_view"]
    assert ctypes.sizeof(LocalMapJob) == 128 and ctypes.sizeof(Camera) == 84
    assert [getattr(LocalMapJob, n).offset for n in names] == [0, 88, 96, 104, 112, 116, 120]
    assert MAP_POINT_3D_DTYPE.itemsize == 80


def test_trivial_returns(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, B=0) == OK and a.untouched()
    assert a.call(orbfe_lib, B=0, kps=None, geom=None, jobs=None, mvp=None, mvp_in=None) == OK
    assert _last(orbfe_lib) == (0, 0, 0)


@pytest.mark.parametrize("null", ["kps", "desc", "counts", "geom", "jobs", "mvp_in", "obs", "mvp", "nm", "ntm", "nk"])
def test_null_pointers_are_refused(orbfe_lib, null):
    a = _Args()
    assert a.call(orbfe_lib, **{null: None}) == E_ARG and a.untouched()


def test_bad_arguments_are_refused(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, B=-1) == E_ARG
    assert a.call(orbfe_lib, cap=0) == E_ARG and a.call(orbfe_lib, cap=-3) == E_ARG
    assert a.call(orbfe_lib, base=-1) == E_ARG and a.call(orbfe_lib, step=-1) == E_ARG
    a.jobs[1].n_pts = -1
    assert a.call(orbfe_lib) == E_ARG
    a.fill_jobs()
    a.jobs[1].n_skip = -1
    assert a.call(orbfe_lib) == E_ARG
    a.fill_jobs()
    a.jobs[0].pts = None                      # NULL pts with n_pts > 0
    assert a.call(orbfe_lib) == E_ARG
    a.fill_jobs()
    a.jobs[0].skip = None                     # NULL skip with n_skip > 0
    assert a.call(orbfe_lib) == E_ARG
    for bad in (-1, 5):                       # a skip index outside [0, n_pts)
        a.skip[1][1] = bad
        a.fill_jobs()
        assert a.call(orbfe_lib) == E_ARG
    a = _Args()
    a.model.type = 5
    assert a.call(orbfe_lib, model=ctypes.byref(a.model)) == E_ARG
    two = MatchFrame(np.zeros(8, KEYPOINT_DTYPE), np.zeros((8, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), SF, nleft=4)
    assert a.call(orbfe_lib, geom=two.ref()) == E_ARG
    a.geom.c.scale_factors = None
    assert a.call(orbfe_lib) == E_ARG
    a = _Args()
    a.geom.c.nlevels = 0
    assert a.call(orbfe_lib) == E_ARG
    assert a.untouched() and _last(orbfe_lib) == (0, 0, 0)


def test_capacity_limits_are_refused(orbfe_lib):
    a = _Args(n_pts=_max_points() + 1)
    assert a.call(orbfe_lib) == E_CAP and a.untouched()
    a = _Args()
    a.geom.c.max_x = 70000.0   # image bounds beyond the one-workgroup bucket index
    assert a.call(orbfe_lib) == E_CAP and a.untouched()
    # a bad argument is reported before a capacity limit
    a = _Args(n_pts=_max_points() + 1)
    a.jobs[0].n_pts = -1
    assert a.call(orbfe_lib) == E_ARG and a.untouched()


def test_wrapper_job_keeps_its_arrays():
    pts = np.zeros(4, MAP_POINT_3D_DTYPE)
    j = LocalMapJob.make(CAM, pts, 3.0, [1, 2], want_in_view=True)
    assert (j.n_pts, j.pts, j.n_skip) == (4, pts.ctypes.data, 2) and j._points is pts
    assert j.skip == j._skip.ctypes.data and j.in_view == j.in_view_flags.ctypes.data and len(j.in_view_flags) == 4
    k = LocalMapJob.make(CAM, None, 3.0)
    assert k.pts is None and k.skip is None and k.in_view is None and k.n_pts == 0 and k.in_view_flags is None
    assert LocalMapJob.make(CAM, pts[:0], 3.0, want_in_view=True).in_view is None
    with pytest.raises(ValueError):
        LocalMapJob.make(CAM, np.zeros(4, np.float32), 3.0)
