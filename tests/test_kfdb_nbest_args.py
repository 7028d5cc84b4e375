"""CPU: the argument checks and trivial returns of orbfe_kfdb_detect_nbest run before any device call,
so they answer on a machine without a GPU (keyframes with an empty BowVector need no device)."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib

OK, E_ARG = _lib.ORBFE_OK, _lib.ORBFE_E_ARG


@pytest.fixture
def db(orbfe_lib):
    h = ctypes.c_void_p()
    assert orbfe_lib.orbfe_kfdb_create(100, ctypes.byref(h)) == OK and h.value
    yield h
    orbfe_lib.orbfe_kfdb_destroy(h)


def _vec(ids):
    return np.array(ids, np.uint32), np.full(len(ids), 0.5, np.float64)


class Args:
    """A valid argument list; with(...) replaces entries by name."""

    def __init__(self, db):
        self.ids, self.w = _vec([1, 5, 9])
        self.con = np.array([3, 4], np.int32)
        self.bad = np.array([8], np.int32)
        self.loop, self.merge = np.full(3, 7, np.int32), np.full(3, 7, np.int32)
        self.nl, self.nm = ctypes.c_int32(-9), ctypes.c_int32(-9)
        self.base = dict(db=db, ids=self.ids.ctypes.data, w=self.w.ctypes.data, qn=3, con=self.con.ctypes.data, ncon=2,
                         map_id=0, bad=self.bad.ctypes.data, nbad=1, n=3, info=_lib.KF_INFO_FN(), ctx=None,
                         loop=self.loop.ctypes.data, nl=ctypes.byref(self.nl), merge=self.merge.ctypes.data,
                         nm=ctypes.byref(self.nm))

    def call(self, lib, **kw):
        a = dict(self.base, **kw)
        return lib.orbfe_kfdb_detect_nbest(*[a[k] for k in ("db", "ids", "w", "qn", "con", "ncon", "map_id", "bad",
                                                             "nbad", "n", "info", "ctx", "loop", "nl", "merge", "nm")])

    def untouched(self):
        return (self.loop == 7).all() and (self.merge == 7).all() and self.nl.value == -9 and self.nm.value == -9


def test_refusals(orbfe_lib, db):
    a = Args(db)
    assert orbfe_lib.orbfe_kfdb_add(db, 1, None, None, 0) == OK
    for kw in (dict(db=None), dict(nl=None), dict(nm=None), dict(loop=None), dict(merge=None), dict(n=-1),
               dict(ncon=-1), dict(nbad=-1), dict(con=None), dict(bad=None), dict(qn=-1), dict(ids=None), dict(w=None)):
        assert a.call(orbfe_lib, **kw) == E_ARG, kw
    for bad in ([5, 1, 9], [1, 1, 9], [1, 5, 100]):
        b, _ = _vec(bad)
        assert a.call(orbfe_lib, ids=b.ctypes.data) == E_ARG
    assert a.untouched()
    assert orbfe_lib.orbfe_kfdb_size(db) == 1


def test_trivial_returns(orbfe_lib, db):
    a = Args(db)
    # empty database
    assert a.call(orbfe_lib) == OK and (a.nl.value, a.nm.value) == (0, 0)
    # keyframes that can never share a word; connected ids that are absent are ignored
    assert orbfe_lib.orbfe_kfdb_add(db, 1, None, None, 0) == OK
    a.nl.value = a.nm.value = -9
    assert a.call(orbfe_lib) == OK and (a.nl.value, a.nm.value) == (0, 0)
    # empty query
    a.nl.value = a.nm.value = -9
    assert a.call(orbfe_lib, ids=None, w=None, qn=0) == OK and (a.nl.value, a.nm.value) == (0, 0)
    # n_candidates == 0 needs no arrays; no connected / bad lists need none either
    a.nl.value = a.nm.value = -9
    assert a.call(orbfe_lib, n=0, loop=None, merge=None, con=None, ncon=0, bad=None, nbad=0) == OK
    assert (a.nl.value, a.nm.value) == (0, 0)
    assert (a.loop == 7).all() and (a.merge == 7).all()


def test_python_wrapper_without_a_device(orbfe_lib):
    from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
    db = KeyFrameDatabase(50)
    db.add(2, (np.zeros(0, np.uint32), np.zeros(0)))
    q = (np.array([1, 2], np.uint32), np.array([0.5, 0.5]))
    loop, merge = db.DetectNBestCandidates(q, [2, 7], map_id=0, n=3, neighbours={2: [1]}, maps={2: 1}, bad_maps=[4])
    assert loop.dtype == np.int32 and len(loop) == 0 and len(merge) == 0
    with pytest.raises(_lib.OrbfeError):
        db.DetectNBestCandidates(q, [], n=-1)
    with pytest.raises(_lib.OrbfeError):
        db.DetectNBestCandidates((np.array([2, 1], np.uint32), np.array([0.5, 0.5])), [])
    db.close()
