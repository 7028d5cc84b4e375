"""GPU parity of ComputeBoW on the planted cases of tests/bow_patterns.py (each proved on the CPU to reach the
rule it names, tests/test_bow_definition.py). Every case goes through every form, and every form must equal
the definition (oracle/bow_definition.py) exactly: word ids, node ids, offsets and indices as integers,
weights as bytes. Expected values are computed once per module; the device is never compared with itself.

  ORBVocabulary.transform     k_bow_descend / k_bow_assemble (one thread per descriptor, serial assemble)
  transform_batch             k_bowb_descend / k_bowb_assemble: the case at the first, a middle and the last
                              image of a batch whose cap is no power of two, counts [nimg, 2] with garbage in
                              column 1, rows behind every count filled with a descriptor that would add a word
                              if read, and one image with a bad count (-1 or cap + 1) whose rows stay as they were
  compute_bow                 a host MatchFrame, a DeviceMatchFrame and a device view into a larger slab

Every form runs the case, then another image, then the case again on the same vocabulary and thread (stale
arena or LDS state would show in the second run).
"""
import ctypes

import numpy as np
import pytest

import bow_patterns as P
from kfdb_definition import KF, KeyFrameDatabaseDef
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd._lib import OrbfeCapacityError
from orb_slam3_ros_amd.matcher import CFrame, DeviceMatchFrame, MatchFrame
from orb_slam3_ros_amd.vocabulary import BowBatch

pytestmark = pytest.mark.gpu

CASES = P.all_cases()
SENT_I, SENT_W = 0x5A5A5A5A, -7.25


@pytest.fixture(scope="module")
def expected():
    """The definition's (BowVector, FeatureVector) of every case, computed once."""
    return {c.name: P.run_definition(c)[:2] for c in CASES}


@pytest.fixture(scope="module")
def vocs(gpu):
    """One device vocabulary per planted vocabulary, created at its first use."""
    made = {}

    def get(voc):
        if id(voc) not in made:
            made[id(voc)] = (voc, voc.device())
            assert made[id(voc)][1].n_nodes == voc.n_nodes
        return made[id(voc)][1]
    yield get
    for _, gv in made.values():
        gv.close()


def _same(got, want, name):
    (gb, gw), gfv = got
    (db, dw), (dfid, dfoff, dfidx) = want
    np.testing.assert_array_equal(gb, db, err_msg=name)
    assert np.asarray(gw).tobytes() == dw.tobytes(), (name, gw, dw)
    np.testing.assert_array_equal(gfv.node_ids, dfid, err_msg=name)
    np.testing.assert_array_equal(gfv.offsets, dfoff, err_msg=name)
    np.testing.assert_array_equal(gfv.indices[:len(dfidx)], dfidx, err_msg=name)


def _other(case):
    """Another image on the case's vocabulary: its features in reverse order and three random ones."""
    return np.concatenate([case.desc[::-1], P.randoms(len(case.name), 3)])


_frames = {}


def _frame(desc):
    """A synth_match frame of len(desc) keys with the planted descriptors in place of its own."""
    n = len(desc)
    if n not in _frames:
        _frames[n] = sm.synth_frame(np.random.default_rng(n), n, stereo=False)
    F = _frames[n]
    return MatchFrame(F.keys, desc, F.bounds, F.scale_factors)


class SlabView:
    """The descriptors as rows 1..n of a larger device slab (poisoned rows around them), behind a frame struct
    with the device flag set: what orbfe_frame_device_view hands out."""

    def __init__(self, F, device):
        import torch
        self.N = F.N
        slab = np.full((F.N + 2, 32), 0xA5, np.uint8)
        slab[1:-1] = F.desc
        self.slab = torch.from_numpy(slab).to(device)
        self.c = CFrame()
        ctypes.memmove(ctypes.byref(self.c), F.ref(), ctypes.sizeof(CFrame))
        self.c.desc = self.slab.data_ptr() + 32
        self.c.keys = None          # only n, desc and device are read
        self.c.device = 1

    def ref(self):
        return ctypes.byref(self.c)


def _forms(gpu, gv, levelsup):
    return {"transform": lambda d: gv.transform(d, levelsup),
            "compute_bow(host)": lambda d: gv.compute_bow(_frame(d), levelsup),
            "compute_bow(device)": lambda d: gv.compute_bow(DeviceMatchFrame(_frame(d), gpu), levelsup),
            "compute_bow(view)": lambda d: gv.compute_bow(SlabView(_frame(d), gpu), levelsup)}


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_case(gpu, expected, vocs, k):
    case = CASES[k]
    gv = vocs(case.voc)
    other = _other(case)
    want, want_other = expected[case.name], P.run_definition(case, desc=other)[:2]
    for name, run in _forms(gpu, gv, case.levelsup).items():
        _same(run(case.desc), want, f"{case.name} {name}")
        _same(run(other), want_other, f"{case.name} {name} (the other image)")
        _same(run(case.desc), want, f"{case.name} {name} (second run)")


def _bait(voc):
    """A kept leaf's own descriptor: read as a feature it would add to that word."""
    kept = [i for i in voc.leaves() if voc.w[i] > 0]
    return voc.desc[kept[len(kept) // 2]]


def _sentinel(gpu, nimg, cap, out=None):
    b = BowBatch(nimg, cap, gpu) if out is None else out
    for t in (b.bow_word_ids, b.fv_node_ids, b.fv_offsets, b.fv_indices, b.counts):
        t.fill_(SENT_I)
    b.bow_weights.fill_(SENT_W)
    return b


def _batch(gpu, gv, voc, images, counts, cap, levelsup, out):
    import torch
    d = np.empty((len(images), cap, 32), np.uint8)
    d[:] = _bait(voc)
    for i, f in enumerate(images):
        d[i, :len(f)] = f
    c = np.full((len(images), 2), -123456, np.int32)   # column 1: as monoIndex behind the extractor's counts
    c[:, 0] = counts
    res = gv.transform_batch(torch.from_numpy(d).to(gpu), torch.from_numpy(c).to(gpu), levelsup, out=out)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_case_batch(gpu, expected, vocs, k):
    case = CASES[k]
    gv = vocs(case.voc)
    other = _other(case)
    half = other[:max(1, len(other) // 2)]
    wants = {0: expected[case.name], 1: P.run_definition(case, desc=other)[:2], 3: expected[case.name],
             4: P.run_definition(case, desc=half)[:2], 5: expected[case.name]}
    cap = len(other) + 2
    if cap & (cap - 1) == 0:
        cap += 1
    images = [case.desc, other, case.desc, case.desc, half, case.desc]   # image 2 is the refused one
    counts = [len(f) for f in images]
    counts[2] = -1 if k % 2 else cap + 1
    out = _sentinel(gpu, 6, cap)
    for run in ("first run", "second run"):
        assert _batch(gpu, gv, case.voc, images, counts, cap, case.levelsup, out) is out
        cnt = out.counts.cpu().numpy()
        assert tuple(cnt[2]) == (-1, -1), (case.name, cnt[2])
        for t in (out.bow_word_ids, out.fv_node_ids, out.fv_offsets, out.fv_indices):
            assert (t[2].cpu().numpy() == SENT_I).all(), case.name
        assert (out.bow_weights[2].cpu().numpy() == SENT_W).all(), case.name
        for i, want in wants.items():
            assert tuple(cnt[i]) == (len(want[0][0]), len(want[1][0])), (case.name, i, cnt[i])
            assert int(out.fv_offsets[i, 0].cpu()) == 0
            _same(out.host(i), want, f"{case.name} image {i} ({run})")
        if run == "first run":   # another batch in between, then the same buffers again
            mid = _batch(gpu, gv, case.voc, [half, other], [len(half), len(other)], cap, case.levelsup, None)
            _same(mid.host(0), wants[4], f"{case.name} (the batch in between)")
            _same(mid.host(1), wants[1], f"{case.name} (the batch in between)")
            _sentinel(gpu, 6, cap, out)


@pytest.mark.parametrize("which", ["ragged", "chunked"])
def test_chain_into_keyframe_database(gpu, vocs, which):
    """transform_batch -> KeyFrameDatabase.add_batch -> shared_words against the same chain on the definition's
    BowVectors through KeyFrameDatabaseDef."""
    from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
    voc = P.chain_vocs()[which]
    gv = vocs(voc)
    rng = np.random.default_rng(len(which))
    images = [P.leaf_image(voc, 300 + i, int(n), random_every=4) for i, n in enumerate(rng.integers(5, 60, 8))]
    cap = 61
    ids = (rng.permutation(8) + 10).astype(np.int32)
    bows = _batch(gpu, gv, voc, images, [len(f) for f in images], cap, 1, None)
    db, ref = KeyFrameDatabase(gv.n_words), KeyFrameDatabaseDef(gv.n_words)
    db.add_batch(ids, bows)
    case = P.Case(which, voc, 1, images[0])
    defs = [P.run_definition(case, desc=f)[0] for f in images]
    for kid, bow in zip(ids, defs):
        ref.add(KF(int(kid), bow))
    assert len(db) == 8
    queries = defs[:2] + [P.run_definition(case, desc=P.leaf_image(voc, 400 + i, 40, random_every=3))[0] for i in range(2)]
    shared = 0
    for q in queries:
        g, r = db.shared_words(q), ref.shared_words(q)
        assert g[0].tolist() == r[0].tolist() and g[1].tolist() == r[1].tolist() and g[4] == r[4]
        assert g[3].tolist() == r[3].tolist() and g[2].tobytes() == r[2].tobytes()
        shared += len(r[0])
    assert shared > 8
    db.close()


def _raw(gv, n, call):
    """call(word ids, weights, &bow_n, node ids, offsets, indices, &fv_n) on sentinel-filled outputs of capacity
    n -> (rc, whether every output still holds its sentinel)."""
    bid, fid, fidx = (np.full(n, SENT_I, np.uint32) for _ in range(3))
    foff = np.full(n + 1, SENT_I, np.int32)
    bw = np.full(n, SENT_W, np.float64)
    nb, nf = ctypes.c_int32(-9), ctypes.c_int32(-9)
    rc = call(bid.ctypes.data, bw.ctypes.data, ctypes.byref(nb), fid.ctypes.data, foff.ctypes.data, fidx.ctypes.data,
              ctypes.byref(nf))
    clean = (all((a == SENT_I).all() for a in (bid, fid, fidx, foff)) and (bw == SENT_W).all() and
             nb.value == nf.value == -9)
    return rc, clean


def test_single_call_limit(gpu, vocs):
    """4096 descriptors are the single call's most; one more is a capacity error that writes nothing, and
    compute_bow takes it."""
    voc = P.group_voc(8)
    gv = vocs(voc)
    lib = _lib.load()
    f = P.leaf_image(voc, 500, 4097, random_every=2)
    case = P.Case("limit", voc, 1, f)
    _same(gv.transform(f[:4096], 1), P.run_definition(case, desc=f[:4096])[:2], "n = 4096")
    rc, clean = _raw(gv, 4097, lambda *o: lib.orbfe_vocabulary_transform(gv._h, f.ctypes.data, 4097, 1, *o))
    assert rc == _lib.ORBFE_E_CAPACITY and clean
    with pytest.raises(OrbfeCapacityError):
        gv.transform(f, 1)
    want = P.run_definition(case)[:2]
    _same(gv.compute_bow(_frame(f), 1), want, "n = 4097, compute_bow")
    _same(gv.transform(f[:4096], 1), P.run_definition(case, desc=f[:4096])[:2], "n = 4096 after the refusal")


@pytest.mark.parametrize("where", ["host", "device"])
def test_compute_bow_limit(gpu, vocs, where):
    """8193 descriptors are a capacity error in compute_bow, on a host frame and on a device frame, and nothing
    is written; the next call on the same thread is served."""
    voc = P.group_voc(8)
    gv = vocs(voc)
    lib = _lib.load()
    f = P.leaf_image(voc, 501, 8193, random_every=2)
    F = _frame(f)
    if where == "device":
        F = SlabView(F, gpu)
    rc, clean = _raw(gv, 8193, lambda *o: lib.orbfe_frame_compute_bow(gv._h, F.ref(), 1, *o))
    assert rc == _lib.ORBFE_E_CAPACITY and clean
    with pytest.raises(OrbfeCapacityError):
        gv.compute_bow(F, 1)
    small = P.Case("after", voc, 1, f[:100])
    _same(gv.compute_bow(_frame(f[:100]), 1), P.run_definition(small)[:2], "after the refusal")
