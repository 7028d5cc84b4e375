"""GPU parity of orbfe_kfdb_detect_nbest (KeyFrameDatabase::DetectNBestCandidates on the device
database) against the restatement in tests/place_recognition_definition.py: the loop and merge ids
compared with np.array_equal, in order. The GPU is never compared with itself."""
import numpy as np
import pytest

import kfdb_definition as kd
import place_recognition_definition as pr
from kfdb_definition import KF
from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
from place_recognition_definition import PlaceRecognitionDef

pytestmark = pytest.mark.gpu


class Pair:
    """The device database and the definition, fed the same calls."""

    def __init__(self, n_words, bows=None, neighbours=None, maps=None):
        self.g, self.d = KeyFrameDatabase(n_words), PlaceRecognitionDef(n_words)
        self.nbrs, self.maps = {}, {}
        for i, b in (bows or {}).items():
            self.add(i, b, (neighbours or {}).get(i, ()), (maps or {}).get(i, 0))

    def add(self, kf_id, bow, neighbours=(), map_id=0):
        self.g.add(kf_id, bow)
        self.d.add(KF(kf_id, bow, neighbours, map_id))
        self.nbrs[kf_id], self.maps[kf_id] = list(neighbours), map_id

    def erase(self, kf_id):
        self.g.erase(kf_id)
        self.d.erase(kf_id)

    def nbest(self, q, connected=(), map_id=0, n=3, bad_maps=()):
        got = self.g.DetectNBestCandidates(q, connected, map_id, n, self.nbrs, self.maps, bad_maps)
        exp = self.d.DetectNBestCandidates(q, connected, map_id, n, bad_maps)
        for g, e in zip(got, exp):
            assert g.dtype == np.int32 and np.array_equal(g, e), (got, exp)
        return exp[0].tolist(), exp[1].tolist()

    def reloc(self, q, map_id=0):
        got = self.g.DetectRelocalizationCandidates(q, map_id, self.nbrs, self.maps)
        exp = self.d.DetectRelocalizationCandidates(q, map_id)
        assert np.array_equal(got, exp), (got, exp)
        return exp.tolist()

    def close(self):
        self.g.close()


@pytest.mark.parametrize("n_words,n_kf", [(64, 40), (256, 300)])
def test_random_databases(gpu, n_words, n_kf):
    """Random BowVectors, neighbour lists (some longer than 10, some naming absent ids), two good maps
    and a bad one, random connected sets, n from 0 to 5; the per-keyframe scores carry over from query to
    query on both sides."""
    rng = np.random.default_rng(n_words + n_kf)
    bows, nbrs, maps = pr.random_scene(rng, n_words, n_kf, n_maps=3)
    p = Pair(n_words, bows, nbrs, maps)
    seen_loop = seen_merge = 0
    for k in range(12):
        q = bows[int(rng.integers(0, n_kf))] if k % 2 else kd.random_bow(rng, n_words, int(rng.integers(5, 40)))
        con = rng.choice(n_kf + 10, int(rng.integers(0, 20)), replace=False)
        loop, merge = p.nbest(q, con, map_id=int(rng.integers(0, 2)), n=k % 6, bad_maps=[2] if k % 3 else [])
        seen_loop += len(loop)
        seen_merge += len(merge)
    assert seen_loop > 5 and seen_merge > 5
    p.close()


def test_connected_keyframe_moves_the_gate(gpu):
    n_words, bows, q = pr.gate_fixture()
    p = Pair(n_words, bows)
    assert p.nbest(q) == ([0], [])
    assert p.nbest(q, [0]) == ([1, 2], [])
    assert p.nbest(q, [0, 999]) == ([1, 2], [])
    p.close()


def test_stable_order_and_independent_lists(gpu):
    n_words, bows, maps, q = pr.tie_fixture()
    p = Pair(n_words, bows, maps=maps)
    assert p.nbest(q, n=3) == ([10, 12, 14], [11, 13, 15])
    assert p.nbest(q, n=2) == ([10, 12], [11, 13])
    assert p.nbest(q, map_id=1, n=1) == ([11], [10])
    assert p.nbest(q, n=5) == ([10, 12, 14], [11, 13, 15])      # fewer than n available
    assert p.nbest(q, n=0) == ([], [])
    assert p.nbest(q, n=3, bad_maps=[1]) == ([10, 12, 14], [])  # a bad merge map
    assert p.nbest(q, map_id=7, n=2) == ([], [10, 11])          # merge full, loop never fills
    # erase followed by add: the keyframe moves to the back and its score starts from 0
    p.erase(10)
    p.add(10, bows[10], (), 0)
    assert p.nbest(q, n=3) == ([12, 14, 10], [11, 13, 15])
    p.close()


def test_one_list_full_while_the_other_is_short(gpu):
    bows = {k: pr.uniform(range(0, 8)) for k in range(5)}
    p = Pair(64, bows, maps={0: 0, 1: 0, 2: 0, 3: 1, 4: 0})
    assert p.nbest(pr.uniform(range(0, 8)), n=2) == ([0, 1], [3])
    p.close()


def test_dedupe_of_best_neighbours(gpu):
    n_words, bows, nbrs, q = pr.dedupe_fixture()
    p = Pair(n_words, bows, nbrs)
    assert p.nbest(q) == ([2, 3], [])
    assert p.nbest(q, [2]) == ([0, 1, 3], [])
    p.close()


def test_stale_score_and_interleaved_relocalisation(gpu):
    """Query A leaves mPlaceRecognitionScore on X; a relocalisation query in between neither sees it nor
    disturbs it; query B then reaches it through a neighbour. The relocalisation side's own stale score
    (kd.stale_score_fixture) stays intact across an N-best query likewise."""
    n_words, bows, nbrs, qa, qb = pr.stale_place_fixture()
    p = Pair(n_words, bows, nbrs)
    assert p.nbest(qa) == ([2], [])
    assert p.reloc(qb) == [0, 1]
    assert p.nbest(qb) == ([2, 0], [])
    p.close()
    n_words, bows, nbrs, qa, qb = kd.stale_score_fixture()
    p = Pair(n_words, bows, nbrs)
    assert p.reloc(qa) == [2]
    p.nbest(qb)
    p.nbest(qa)
    assert p.reloc(qb) == [0]   # X's mRelocScore from A still pushes keyframe 1 out
    p.close()


def test_ordered_sum(gpu):
    """kd.ordered_sum_fixture: the score is one left-to-right double chain. The last keyframe scores
    float 1.0 exactly that way and 1 + 2^-23 in any other order. A twin added before it shares the same
    102 words with terms -2, -2^-23 and exact zeros, so it scores float 1.0 in every order: with the
    right chain the two tie and keep the list order (twin first); any other chain puts the keyframe
    ahead of its twin."""
    n_words, q, kfs = kd.ordered_sum_fixture()
    p = Pair(n_words)
    z, twin = len(kfs) - 1, 100
    for i, b in enumerate(kfs[:-1]):
        p.add(i, b)
    z_ids = kfs[-1][0]
    p.add(twin, (z_ids, np.array([1.0, 2.0 ** -24] + [0.0] * (len(z_ids) - 2))))
    p.add(z, kfs[-1])
    loop, _ = p.nbest(q, n=len(kfs) + 1)
    assert p.d.kfs[z].mPlaceRecognitionScore == np.float32(1.0) == p.d.kfs[twin].mPlaceRecognitionScore
    assert loop.index(twin) + 1 == loop.index(z)
    p.close()


def test_callback_errors_and_bad_counts(gpu):
    from orb_slam3_ros_amd import _lib
    n_words, bows, nbrs, qa, qb = pr.stale_place_fixture()
    p = Pair(n_words, bows, nbrs)
    assert p.nbest(qa) == ([2], [])

    def boom(kf_id):
        raise KeyError(kf_id)
    with pytest.raises(KeyError):
        p.g.DetectNBestCandidates(qb, [], neighbours=boom)
    # the refused call committed nothing: X's score from A is still the only one
    assert p.nbest(qb) == ([2, 0], [])
    import ctypes
    ids, w = np.ascontiguousarray(qb[0], np.uint32), np.ascontiguousarray(qb[1], np.float64)
    loop, merge = np.full(3, 7, np.int32), np.full(3, 7, np.int32)
    nl, nm = ctypes.c_int32(-9), ctypes.c_int32(-9)
    cb = _lib.KF_INFO_FN(lambda ctx, kf_id, nb, mp: 11)
    rc = p.g._lib.orbfe_kfdb_detect_nbest(p.g._h, ids.ctypes.data, w.ctypes.data, len(ids), None, 0, 0, None, 0, 3, cb,
                                          None, loop.ctypes.data, ctypes.byref(nl), merge.ctypes.data, ctypes.byref(nm))
    assert rc == _lib.ORBFE_E_ARG and (loop == 7).all() and (merge == 7).all() and nl.value == nm.value == -9
    p.close()
