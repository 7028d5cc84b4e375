"""CPU: every refusal of orbfe_search_by_projection_lastframe_slabs comes before any device call and
before any write to its outputs, so it answers on a machine without a GPU (a device call would return
ORBFE_E_DEVICE here). The slab pointers are dummies: a refused call never reads them."""
import ctypes
import re

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import LAST_POINT_DTYPE, SIM3, CameraModel, MatchFrame, Pose, TrackJob

SF = np.asarray([1.0, 1.2], np.float32)
OK, E_ARG, E_CAP = _lib.ORBFE_OK, _lib.ORBFE_E_ARG, _lib.ORBFE_E_CAPACITY


class _Args:
    """A well-formed call of B frames over dummy slabs, to be broken per case."""

    def __init__(self, B=2, cap=8, n_pts=3):
        self.geom = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), SF)
        self.cam = CameraModel.make("pinhole", 50.0, 50.0, 32.0, 24.0)
        self.B, self.cap = B, cap
        self.points = [np.zeros(n_pts, LAST_POINT_DTYPE) for _ in range(B)]
        for p in self.points:
            p["valid"] = 1
        self.jobs = (TrackJob * B)()
        self.fill_jobs()
        self.dummy = np.zeros(64, np.uint8)
        self.mvp = np.full((B, cap), 7, np.int32)
        self.nm = np.full(B, 7, np.int32)
        self.nk = np.full(B, 7, np.int32)

    def fill_jobs(self):
        for f in range(self.B):
            self.jobs[f] = TrackJob.make(Pose.se3(np.eye(3), np.zeros(3)), self.points[f], 7.0)

    def call(self, lib, **kw):
        d = self.dummy.ctypes.data
        a = dict(kps=d, desc=d, counts=d, cap=self.cap, base=0, step=1, ur=d, geom=self.geom.ref(),
                 cam=ctypes.byref(self.cam), jobs=self.jobs, B=self.B, mvp=self.mvp.ctypes.data,
                 nm=self.nm.ctypes.data, nk=self.nk.ctypes.data)
        a.update(kw)
        return lib.orbfe_search_by_projection_lastframe_slabs(
            a["kps"], a["desc"], a["counts"], a["cap"], a["base"], a["step"], a["ur"], a["geom"], a["cam"], a["jobs"],
            a["B"], 1, a["mvp"], a["nm"], a["nk"], None)

    def untouched(self):
        return bool((self.mvp == 7).all() and (self.nm == 7).all() and (self.nk == 7).all())


def _last(lib):
    w = np.full(3, -9, np.int32)
    assert lib.orbfe_matcher_last_track_batch(w.ctypes.data) == OK
    return tuple(int(v) for v in w)


def test_symbols_are_exported(orbfe_lib):
    for name in ("orbfe_search_by_projection_lastframe_slabs", "orbfe_matcher_last_track_batch"):
        assert hasattr(orbfe_lib, name), name
    assert orbfe_lib.orbfe_matcher_last_track_batch(None) == E_ARG


def test_track_job_layout_matches_the_header():
    """orbfe_track_job: the header's field order and its 56 bytes, pose first."""
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct orbfe_track_job \{(.*?)\} orbfe_track_job;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in TrackJob._fields_] == ["Tcw", "pts", "n_pts", "th", "bForward", "bBackward"]
    assert ctypes.sizeof(TrackJob) == 56 and ctypes.sizeof(Pose) == 32
    assert [getattr(TrackJob, n).offset for n in names] == [0, 32, 40, 44, 48, 52]
    assert LAST_POINT_DTYPE.itemsize == 64


def test_trivial_returns(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, B=0) == OK and a.untouched()
    assert a.call(orbfe_lib, B=0, kps=None, geom=None, jobs=None, mvp=None) == OK
    assert _last(orbfe_lib) == (0, 0, 0)


@pytest.mark.parametrize("null", ["kps", "desc", "counts", "geom", "cam", "jobs", "mvp", "nm", "nk"])
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
    a.jobs[0].pts = None                      # NULL pts with n_pts > 0
    assert a.call(orbfe_lib) == E_ARG
    a.fill_jobs()
    for octave in (-1, 2):                    # a valid point's octave outside [0, nlevels)
        a.points[1]["octave"][2] = octave
        assert a.call(orbfe_lib) == E_ARG
    a = _Args()
    a.cam.type = 5
    assert a.call(orbfe_lib) == E_ARG
    a = _Args()
    two = MatchFrame(np.zeros(8, KEYPOINT_DTYPE), np.zeros((8, 32), np.uint8), (0.0, 64.0, 0.0, 48.0), SF, nleft=4)
    assert a.call(orbfe_lib, geom=two.ref()) == E_ARG
    a.geom.c.scale_factors = None
    assert a.call(orbfe_lib) == E_ARG
    a = _Args()
    a.jobs[1].Tcw = Pose.sim3(np.eye(3), np.zeros(3), 1.0)   # a pose that is not SE3
    assert a.jobs[1].Tcw.kind == SIM3 and a.call(orbfe_lib) == E_ARG
    assert a.untouched() and _last(orbfe_lib) == (0, 0, 0)


def test_capacity_limits_are_refused(orbfe_lib):
    a = _Args(n_pts=2049)
    assert a.call(orbfe_lib) == E_CAP and a.untouched()
    a = _Args()
    a.geom.c.max_x = 70000.0   # image bounds beyond the one-workgroup bucket index
    assert a.call(orbfe_lib) == E_CAP and a.untouched()
    # a bad argument is reported before a capacity limit
    a = _Args(n_pts=2049)
    a.jobs[0].n_pts = -1
    assert a.call(orbfe_lib) == E_ARG and a.untouched()


def test_wrapper_job_keeps_its_points():
    pts = np.zeros(4, LAST_POINT_DTYPE)
    j = TrackJob.make(Pose.se3(np.eye(3), np.zeros(3)), pts, 7.0, True, False)
    assert (j.n_pts, j.pts, j.bForward, j.bBackward) == (4, pts.ctypes.data, 1, 0) and j._points is pts
    assert TrackJob.make(j.Tcw, None, 7.0).pts is None and TrackJob.make(j.Tcw, pts[:0], 7.0).n_pts == 0
    with pytest.raises(ValueError):
        TrackJob.make(j.Tcw, np.zeros(4, np.float32), 7.0)
