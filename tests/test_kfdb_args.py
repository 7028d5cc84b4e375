"""CPU: the argument checks and trivial returns of the keyframe database (orbfe_kfdb_*) run before
any device call, so they answer on a machine without a GPU. Keyframes with an empty BowVector need no
device either, which is how the duplicate / absent id checks are reached here."""
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


def test_create_and_destroy(orbfe_lib):
    h = ctypes.c_void_p()
    assert orbfe_lib.orbfe_kfdb_create(0, ctypes.byref(h)) == E_ARG and h.value is None
    assert orbfe_lib.orbfe_kfdb_create(-5, ctypes.byref(h)) == E_ARG
    assert orbfe_lib.orbfe_kfdb_create(10, None) == E_ARG
    orbfe_lib.orbfe_kfdb_destroy(None)   # a no-op
    assert orbfe_lib.orbfe_kfdb_size(None) == E_ARG
    assert orbfe_lib.orbfe_kfdb_clear(None) == E_ARG
    assert orbfe_lib.orbfe_kfdb_erase(None, 0) == E_ARG


def test_add_checks(orbfe_lib, db):
    add = orbfe_lib.orbfe_kfdb_add
    ids, w = _vec([1, 5, 9])
    assert add(None, 0, ids.ctypes.data, w.ctypes.data, 3) == E_ARG
    assert add(db, -1, ids.ctypes.data, w.ctypes.data, 3) == E_ARG
    assert add(db, 0, ids.ctypes.data, w.ctypes.data, -1) == E_ARG
    assert add(db, 0, None, w.ctypes.data, 3) == E_ARG
    assert add(db, 0, ids.ctypes.data, None, 3) == E_ARG
    for bad in ([5, 1, 9], [1, 1, 9], [1, 5, 100]):   # descending, repeated, >= n_words
        b, _ = _vec(bad)
        assert add(db, 0, b.ctypes.data, w.ctypes.data, 3) == E_ARG
    assert orbfe_lib.orbfe_kfdb_size(db) == 0
    # an empty BowVector is legal and needs no device; the same id twice is not
    assert add(db, 4, None, None, 0) == OK
    assert add(db, 4, None, None, 0) == E_ARG
    assert add(db, 4, ids.ctypes.data, w.ctypes.data, 3) == E_ARG
    assert orbfe_lib.orbfe_kfdb_size(db) == 1


def test_erase_and_clear(orbfe_lib, db):
    assert orbfe_lib.orbfe_kfdb_erase(db, 3) == E_ARG    # absent
    assert orbfe_lib.orbfe_kfdb_erase(db, -1) == E_ARG
    for i in (3, 8):
        assert orbfe_lib.orbfe_kfdb_add(db, i, None, None, 0) == OK
    assert orbfe_lib.orbfe_kfdb_erase(db, 3) == OK
    assert orbfe_lib.orbfe_kfdb_erase(db, 3) == E_ARG
    assert orbfe_lib.orbfe_kfdb_size(db) == 1
    assert orbfe_lib.orbfe_kfdb_add(db, 3, None, None, 0) == OK    # erased ids may come back
    assert orbfe_lib.orbfe_kfdb_clear(db) == OK
    assert orbfe_lib.orbfe_kfdb_size(db) == 0
    assert orbfe_lib.orbfe_kfdb_erase(db, 8) == E_ARG


def _shared(lib, db, ids, w, n, cap=4, outs=None, n_out=True, mx=True):
    kf, words, sc, fl = (np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7, np.float32),
                         np.full(4, 7, np.uint8))
    no, m = ctypes.c_int32(-9), ctypes.c_int32(-9)
    p = [a.ctypes.data for a in (kf, words, sc, fl)] if outs is None else outs
    rc = lib.orbfe_kfdb_shared_words(db, ids.ctypes.data if ids is not None else None,
                                     w.ctypes.data if w is not None else None, n, p[0], p[1], p[2], p[3], cap,
                                     ctypes.byref(no) if n_out else None, ctypes.byref(m) if mx else None)
    untouched = all((a == 7).all() for a in (kf, words, sc, fl))
    return rc, no.value, m.value, untouched


def test_shared_words_checks(orbfe_lib, db):
    ids, w = _vec([1, 5, 9])
    assert _shared(orbfe_lib, None, ids, w, 3)[0] == E_ARG
    assert _shared(orbfe_lib, db, ids, w, -1)[0] == E_ARG
    assert _shared(orbfe_lib, db, None, w, 3)[0] == E_ARG
    assert _shared(orbfe_lib, db, ids, None, 3)[0] == E_ARG
    assert _shared(orbfe_lib, db, ids, w, 3, n_out=False)[0] == E_ARG
    assert _shared(orbfe_lib, db, ids, w, 3, mx=False)[0] == E_ARG
    assert _shared(orbfe_lib, db, ids, w, 3, cap=-1)[0] == E_ARG
    for k in range(4):
        outs = [1, 1, 1, 1]   # never dereferenced: the check comes first
        outs[k] = None
        assert _shared(orbfe_lib, db, ids, w, 3, outs=outs)[0] == E_ARG
    for bad in ([5, 1, 9], [1, 1, 9], [1, 5, 100]):
        b, _ = _vec(bad)
        assert _shared(orbfe_lib, db, b, w, 3)[0] == E_ARG


def test_empty_database_and_empty_query(orbfe_lib, db):
    ids, w = _vec([1, 5, 9])
    # empty database
    assert _shared(orbfe_lib, db, ids, w, 3) == (OK, 0, 0, True)
    # cap 0 with NULL arrays is enough for an empty result
    assert _shared(orbfe_lib, db, ids, w, 3, cap=0, outs=[None] * 4)[:3] == (OK, 0, 0)
    # keyframes that can never share a word
    assert orbfe_lib.orbfe_kfdb_add(db, 1, None, None, 0) == OK
    assert _shared(orbfe_lib, db, ids, w, 3) == (OK, 0, 0, True)
    # empty query
    assert _shared(orbfe_lib, db, None, None, 0) == (OK, 0, 0, True)


def test_detect_reloc_checks(orbfe_lib, db):
    call = orbfe_lib.orbfe_kfdb_detect_reloc
    ids, w = _vec([1, 5, 9])
    out, n = np.full(4, 7, np.int32), ctypes.c_int32(-9)
    nocb = _lib.KF_INFO_FN()
    a = (ids.ctypes.data, w.ctypes.data, 3, 0, nocb, None)
    assert call(None, *a, out.ctypes.data, 4, ctypes.byref(n)) == E_ARG
    assert call(db, *a, out.ctypes.data, 4, None) == E_ARG
    assert call(db, *a, None, 4, ctypes.byref(n)) == E_ARG
    assert call(db, *a, out.ctypes.data, -1, ctypes.byref(n)) == E_ARG
    assert call(db, None, w.ctypes.data, 3, 0, nocb, None, out.ctypes.data, 4, ctypes.byref(n)) == E_ARG
    assert call(db, ids.ctypes.data, w.ctypes.data, -1, 0, nocb, None, out.ctypes.data, 4, ctypes.byref(n)) == E_ARG
    b, _ = _vec([9, 5, 1])
    assert call(db, b.ctypes.data, w.ctypes.data, 3, 0, nocb, None, out.ctypes.data, 4, ctypes.byref(n)) == E_ARG
    assert n.value == -9 and (out == 7).all()
    # empty database, empty query: ORBFE_OK and zero candidates, also with cap 0 and no array
    assert call(db, *a, out.ctypes.data, 4, ctypes.byref(n)) == OK and n.value == 0
    n.value = -9
    assert call(db, *a, None, 0, ctypes.byref(n)) == OK and n.value == 0
    n.value = -9
    assert call(db, None, None, 0, 0, nocb, None, out.ctypes.data, 4, ctypes.byref(n)) == OK and n.value == 0
    assert (out == 7).all()


def test_python_wrapper_without_a_device(orbfe_lib):
    from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
    db = KeyFrameDatabase(50)
    db.add(2, (np.zeros(0, np.uint32), np.zeros(0)))
    assert len(db) == 1
    with pytest.raises(_lib.OrbfeError):
        db.add(2, (np.zeros(0, np.uint32), np.zeros(0)))
    with pytest.raises(_lib.OrbfeError):
        db.erase(3)
    with pytest.raises(ValueError):
        db.add(5, (np.zeros(2, np.uint32), np.zeros(3)))
    q = (np.array([1, 2], np.uint32), np.array([0.5, 0.5]))
    assert len(db.DetectRelocalizationCandidates(q)) == 0
    assert len(db.shared_words(q)[0]) == 0
    db.clear()
    assert len(db) == 0
    db.close()
    db.close()
