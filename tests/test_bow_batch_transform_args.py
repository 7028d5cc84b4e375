"""CPU: the argument checks and trivial returns of the batched ComputeBoW entry points
(orbfe_vocabulary_transform_batch, orbfe_frame_compute_bow, orbfe_kfdb_add_batch) come before any
device call, so they answer on a machine without a GPU; and the new symbols are exported with the
documented signatures. A vocabulary cannot be built without a device, so where a check needs a non-NULL
handle it gets a dummy address that is never dereferenced: the checks under test come first."""
import ctypes
import os
import re

import numpy as np
import pytest

from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import CFrame

OK, E_ARG, E_CAP = _lib.ORBFE_OK, _lib.ORBFE_E_ARG, _lib.ORBFE_E_CAPACITY
HDR = os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "orbfe.h")
DUMMY = 0x1000   # a non-NULL, suitably aligned address for pointers the checks never follow


def _batch(**kw):
    f = dict(bow_word_ids=DUMMY, bow_weights=DUMMY, fv_node_ids=DUMMY, fv_offsets=DUMMY, fv_indices=DUMMY,
             counts=DUMMY)
    f.update(kw)
    return _lib.BowBatchStruct(**f)


def test_transform_batch_checks(orbfe_lib):
    call = orbfe_lib.orbfe_vocabulary_transform_batch
    b = _batch()
    good = dict(voc=DUMMY, desc=DUMMY, counts=DUMMY, stride=2, nimg=4, cap=100, levelsup=4, out=ctypes.byref(b))

    def rc(**kw):
        a = dict(good)
        a.update(kw)
        return call(a["voc"], a["desc"], a["counts"], a["stride"], a["nimg"], a["cap"], a["levelsup"], a["out"], None)

    assert rc(voc=None) == E_ARG
    assert rc(desc=None) == E_ARG
    assert rc(counts=None) == E_ARG
    assert rc(out=None) == E_ARG
    assert rc(nimg=-1) == E_ARG
    assert rc(cap=0) == E_ARG
    assert rc(cap=-3) == E_ARG
    assert rc(stride=0) == E_ARG
    for field in ("bow_word_ids", "bow_weights", "fv_node_ids", "fv_offsets", "fv_indices", "counts"):
        assert rc(out=ctypes.byref(_batch(**{field: None}))) == E_ARG
    assert rc(desc=DUMMY + 1) == E_ARG                                          # descriptors are read as 32-bit words
    assert rc(out=ctypes.byref(_batch(bow_weights=DUMMY + 4))) == E_ARG           # doubles
    assert rc(cap=8193) == E_CAP
    assert rc(cap=8193, nimg=0) == E_CAP
    assert rc(cap=8193, nimg=-1) == E_ARG                                       # the argument errors come first
    assert rc(nimg=0) == OK
    assert rc(nimg=0, cap=8192, stride=1) == OK


def test_frame_compute_bow_checks(orbfe_lib):
    call = orbfe_lib.orbfe_frame_compute_bow
    desc = np.zeros((4, 32), np.uint8)
    bid, bw, fid, foff, fidx = (np.full(5, 7, np.uint32), np.full(5, 7.0), np.full(5, 7, np.uint32),
                                np.full(6, 7, np.int32), np.full(5, 7, np.uint32))
    nb, nf = ctypes.c_int32(-9), ctypes.c_int32(-9)
    F = CFrame()
    F.n, F.desc = 4, desc.ctypes.data
    outs = [bid.ctypes.data, bw.ctypes.data, ctypes.byref(nb), fid.ctypes.data, foff.ctypes.data, fidx.ctypes.data,
            ctypes.byref(nf)]
    assert call(None, ctypes.byref(F), 4, *outs) == E_ARG
    assert call(DUMMY, None, 4, *outs) == E_ARG
    for k in range(7):
        o = list(outs)
        o[k] = None
        assert call(DUMMY, ctypes.byref(F), 4, *o) == E_ARG
    F.n = -1
    assert call(DUMMY, ctypes.byref(F), 4, *outs) == E_ARG
    F.n, F.desc = 4, None
    assert call(DUMMY, ctypes.byref(F), 4, *outs) == E_ARG
    assert nb.value == -9 and nf.value == -9 and (foff == 7).all()


def test_kfdb_add_batch_checks(orbfe_lib):
    call = orbfe_lib.orbfe_kfdb_add_batch
    db = ctypes.c_void_p()
    assert orbfe_lib.orbfe_kfdb_create(100, ctypes.byref(db)) == OK
    ids = np.array([3, 4, 5], np.int32)
    b = _batch()
    assert call(None, DUMMY, ids.ctypes.data, ctypes.byref(b), 3, 50, None) == E_ARG
    assert call(db, None, ids.ctypes.data, ctypes.byref(b), 3, 50, None) == E_ARG
    assert call(db, DUMMY, None, ctypes.byref(b), 3, 50, None) == E_ARG
    assert call(db, DUMMY, ids.ctypes.data, None, 3, 50, None) == E_ARG
    assert call(db, DUMMY, ids.ctypes.data, ctypes.byref(b), -1, 50, None) == E_ARG
    assert call(db, DUMMY, ids.ctypes.data, ctypes.byref(b), 3, 0, None) == E_ARG
    for field in ("bow_word_ids", "bow_weights", "counts"):
        assert call(db, DUMMY, ids.ctypes.data, ctypes.byref(_batch(**{field: None})), 3, 50, None) == E_ARG
    dup = np.array([3, -1, 3], np.int32)   # an id twice in one batch (-1 may repeat: it skips)
    assert call(db, DUMMY, dup.ctypes.data, ctypes.byref(b), 3, 50, None) == E_ARG
    assert orbfe_lib.orbfe_kfdb_size(db) == 0
    orbfe_lib.orbfe_kfdb_destroy(db)


def test_python_wrappers_refuse_host_tensors(orbfe_lib):
    """transform_batch takes device tensors only; nothing is copied up behind the caller's back."""
    import torch
    from orb_slam3_ros_amd.vocabulary import ORBVocabulary
    voc = ORBVocabulary.__new__(ORBVocabulary)
    voc._h, voc._lib = None, orbfe_lib
    with pytest.raises(ValueError):
        voc.transform_batch(torch.zeros((2, 10, 32), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32))


def _decl(name):
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_and_signatures(orbfe_lib):
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("orbfe_vocabulary_transform_batch", "orbfe_frame_compute_bow", "orbfe_kfdb_add_batch"):
        assert hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == len(_decl(name))   # the ctypes binding has the header's arity
    assert _decl("orbfe_vocabulary_transform_batch") == [
        "const orbfe_vocabulary* voc", "const uint8_t* d_desc", "const int32_t* d_counts", "int32_t count_stride",
        "int32_t nimg", "int32_t cap", "int32_t levelsup", "const orbfe_bow_batch* out", "void* stream"]
    assert _decl("orbfe_frame_compute_bow") == [
        "const orbfe_vocabulary* voc", "const orbfe_frame* F", "int32_t levelsup", "uint32_t* bow_word_ids",
        "double* bow_weights", "int32_t* bow_n", "uint32_t* fv_node_ids", "int32_t* fv_offsets", "uint32_t* fv_indices",
        "int32_t* fv_n"]
    assert _decl("orbfe_kfdb_add_batch") == [
        "orbfe_kfdb* db", "const orbfe_vocabulary* voc", "const int32_t* kf_ids", "const orbfe_bow_batch* bows",
        "int32_t nimg", "int32_t cap", "void* stream"]
    # struct orbfe_bow_batch: six pointers, in the ctypes mirror's order
    src = open(HDR).read()
    body = re.search(r"typedef struct orbfe_bow_batch \{(.*?)\} orbfe_bow_batch;", src, flags=re.S).group(1)
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f[0] for f in _lib.BowBatchStruct._fields_]
    assert ctypes.sizeof(_lib.BowBatchStruct) == 6 * ctypes.sizeof(ctypes.c_void_p)
