"""CPU: every refusal of orbfe_search_by_bow_slabs comes before any device work and before any write to its
outputs, so it answers on a machine without a GPU (a device call would return ORBFE_E_DEVICE here). The slab
and bow pointers are dummies: a refused call never reads them. Two refusals need a keyframe handle, which only
a device can make (NULL kf_mp for a keyframe with features, a handle of another device): the first is in
tests/test_gpu_bow_slabs.py."""
import ctypes
import re

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import BowJob

OK, E_ARG, E_CAP = _lib.ORBFE_OK, _lib.ORBFE_E_ARG, _lib.ORBFE_E_CAPACITY


class _Args:
    """A well-formed call of J jobs with discarded keyframes over dummy slabs, to be broken per case."""

    def __init__(self, J=3, cap=8, nframes=2):
        self.J, self.cap, self.nframes = J, cap, nframes
        raw = np.zeros(256 + 16, np.uint8)
        self.dummy = raw[-raw.ctypes.data % 16:][:256]   # 16-byte aligned, as d_desc must be
        d = self.dummy.ctypes.data
        self.bows = _lib.BowBatchStruct(d, d, d, d, d, d)
        self.jobs = (BowJob * J)()
        for j in range(J):
            self.jobs[j].frame = j % nframes
        self.out = np.full((J, cap), 7, np.int32)
        self.nm = np.full(J, 7, np.int32)
        self.nk = np.full(J, 7, np.int32)

    def call(self, lib, **kw):
        d = self.dummy.ctypes.data
        a = dict(kps=d, desc=d, counts=d, cap=self.cap, base=0, step=1, bows=ctypes.byref(self.bows), jobs=self.jobs,
                 J=self.J, nframes=self.nframes, out=self.out.ctypes.data, nm=self.nm.ctypes.data,
                 nk=self.nk.ctypes.data)
        a.update(kw)
        return lib.orbfe_search_by_bow_slabs(a["kps"], a["desc"], a["counts"], a["cap"], a["base"], a["step"], a["bows"],
                                             a["jobs"], a["J"], a["nframes"], 0.7, 1, a["out"], a["nm"], a["nk"], None)

    def untouched(self):
        return bool((self.out == 7).all() and (self.nm == 7).all() and (self.nk == 7).all())


def _last(lib):
    w = np.full(4, -9, np.int32)
    assert lib.orbfe_matcher_last_bow_slabs(w.ctypes.data) == OK
    return tuple(int(v) for v in w)


def test_symbols_are_declared_and_exported(orbfe_lib):
    src = open(_lib.HEADER_PATH).read()
    for name in ("orbfe_search_by_bow_slabs", "orbfe_matcher_last_bow_slabs"):
        assert hasattr(orbfe_lib, name), name
        assert re.search(r"\bint " + name + r"\(", src), name
    assert orbfe_lib.orbfe_matcher_last_bow_slabs(None) == E_ARG


def test_bow_job_layout_matches_the_header():
    src = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct orbfe_bow_job \{(.*?)\} orbfe_bow_job;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"(\w+)\s*$", decl.strip())[0] for decl in body.split(";") if decl.strip()]
    assert names == [f[0] for f in BowJob._fields_] == ["frame", "kf", "kf_mp"]
    assert ctypes.sizeof(BowJob) == 24 and [getattr(BowJob, n).offset for n in names] == [0, 8, 16]


def test_no_jobs(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, J=0) == OK and a.untouched()
    assert a.call(orbfe_lib, J=0, jobs=None) == OK and a.untouched()   # NULL jobs is refused only with n_jobs > 0
    assert a.call(orbfe_lib, J=0, nframes=0) == OK
    assert _last(orbfe_lib) == (0, 0, 0, 0)


def test_negative_counts_are_refused(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, J=-1) == E_ARG and a.call(orbfe_lib, nframes=-1) == E_ARG
    assert a.call(orbfe_lib, J=0, nframes=-1) == E_ARG and a.untouched()


@pytest.mark.parametrize("null", ["kps", "desc", "counts", "bows", "jobs", "out", "nm", "nk"])
def test_null_pointers_are_refused(orbfe_lib, null):
    a = _Args()
    assert a.call(orbfe_lib, **{null: None}) == E_ARG and a.untouched()
    if null != "jobs":
        assert a.call(orbfe_lib, J=0, **{null: None}) == E_ARG   # also with nothing to do


@pytest.mark.parametrize("field", ["fv_node_ids", "fv_offsets", "fv_indices", "counts"])
def test_null_bow_rows_are_refused(orbfe_lib, field):
    a = _Args()
    setattr(a.bows, field, None)
    assert a.call(orbfe_lib) == E_ARG and a.untouched()


def test_bad_arguments_are_refused(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, cap=0) == E_ARG and a.call(orbfe_lib, cap=-3) == E_ARG
    assert a.call(orbfe_lib, base=-1) == E_ARG and a.call(orbfe_lib, step=-1) == E_ARG
    d = a.dummy.ctypes.data
    for off in (1, 4, 8):
        assert a.call(orbfe_lib, desc=d + off) == E_ARG   # d_desc is staged with 16-byte loads
    for bad in (-1, a.nframes, a.nframes + 5):
        a.jobs[1].frame = bad
        assert a.call(orbfe_lib) == E_ARG
    assert a.call(orbfe_lib, nframes=0) == E_ARG   # no frame is inside [0, 0)
    assert a.untouched() and _last(orbfe_lib) == (0, 0, 0, 0)


def test_capacity_limit_is_refused(orbfe_lib):
    a = _Args()
    assert a.call(orbfe_lib, cap=8193) == E_CAP and a.untouched()
    # a bad argument is reported before the capacity limit
    a.jobs[0].frame = -1
    assert a.call(orbfe_lib, cap=8193) == E_ARG and a.untouched()

