"""GPU parity of the keyframe database (orbfe_kfdb_*: KeyFrameDatabase::add / erase and
DetectRelocalizationCandidates with every BowVector resident in HBM) against the restatement in
tests/kfdb_definition.py. shared_words is compared on ids and order, words, the scored flags and the
scores byte for byte; DetectRelocalizationCandidates on the ids with np.array_equal. The GPU is
never compared with itself."""
import numpy as np
import pytest

import kfdb_definition as kd
from kfdb_definition import KF, KeyFrameDatabaseDef
from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase

pytestmark = pytest.mark.gpu

LDS_WORDS = 4096   # KFDB_LDS_WORDS: longer queries are read from global memory


class Pair:
    """The device database and the definition, fed the same calls."""

    def __init__(self, n_words):
        self.g, self.d = KeyFrameDatabase(n_words), KeyFrameDatabaseDef(n_words)
        self.nbrs, self.maps = {}, {}

    def add(self, kf_id, bow, neighbours=(), map_id=0):
        self.g.add(kf_id, bow)
        self.d.add(KF(kf_id, bow, neighbours, map_id))
        self.nbrs[kf_id], self.maps[kf_id] = list(neighbours), map_id

    def erase(self, kf_id):
        self.g.erase(kf_id)
        self.d.erase(kf_id)

    def shared(self, q):
        got, exp = self.g.shared_words(q), self.d.shared_words(q)
        np.testing.assert_array_equal(got[0], exp[0])   # ids and order
        np.testing.assert_array_equal(got[1], exp[1])   # mnRelocWords
        np.testing.assert_array_equal(got[3], exp[3])   # scored
        assert got[2].tobytes() == exp[2].tobytes(), (got[2], exp[2])
        assert got[4] == exp[4]
        return exp

    def detect(self, q, map_id=0):
        got = self.g.DetectRelocalizationCandidates(q, map_id, self.nbrs, self.maps)
        exp = self.d.DetectRelocalizationCandidates(q, map_id)
        assert got.dtype == np.int32 and np.array_equal(got, exp), (got, exp)
        return exp

    def both(self, q, map_id=0):
        return self.shared(q), self.detect(q, map_id)

    def close(self):
        self.g.close()


def _u(ids):
    return np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids))


@pytest.mark.parametrize("n_words,qn", [(64, 1), (64, 64), (1000, 1), (1000, 64), (1000, 1000),
                                        (6000, LDS_WORDS), (6000, LDS_WORDS + 1)])
def test_lengths_around_the_wave(gpu, n_words, qn):
    """Keyframe BowVectors of 1, 63, 64, 65, 129 and 1,000 words (as many as the word space holds)
    against queries of 1, 64 and 1,000 words and one query on each side of the LDS staging limit."""
    rng = np.random.default_rng(n_words + qn)
    p = Pair(n_words)
    for i, n in enumerate((1, 63, 64, 65, 129, 1000, 64, 1, 129)):
        p.add(i, kd.random_bow(rng, n_words, min(n, n_words)))
    q = kd.random_bow(rng, n_words, qn)
    ex, _ = p.both(q)
    if qn >= 64:
        assert len(ex[0]) >= 5 and ex[3].any()
    # a query made of one keyframe's own first word: found whatever the other lengths are
    ids, w = p.d.kfs[4].words, p.d.kfs[4].weights
    p.both((np.array(ids[:1], np.uint32), np.array(w[:1])))
    p.close()


def test_boundary_matches(gpu):
    p = Pair(1000)
    p.add(0, _u(list(range(100, 165))))           # 65 words: its last word is in the second wave step
    p.add(1, _u(list(range(300, 364))))
    # no shared word at all
    ex, cand = p.both(_u(list(range(500, 600))))
    assert len(ex[0]) == 0 and len(cand) == 0
    # exactly one shared word: the keyframe's last and the query's first
    ex, cand = p.both(_u(list(range(164, 264))))
    assert ex[0].tolist() == [0] and ex[1].tolist() == [1] and cand.tolist() == [0]
    ex, _ = p.both(_u(list(range(363, 463))))
    assert ex[0].tolist() == [1] and ex[1].tolist() == [1]
    # two identical L1-normalised vectors: the score is exactly 1
    rng = np.random.default_rng(5)
    b = (kd.random_bow(rng, 1000, 128)[0], np.full(128, 2.0 ** -7))   # every partial sum is exact
    p.add(2, b)
    ex, _ = p.both(b)
    at = ex[0].tolist().index(2)
    assert ex[1][at] == 128 and ex[3][at] and ex[2][at] == np.float32(1.0)
    p.close()


def test_ordered_sum(gpu):
    """Weights over six decades, not normalised, negative and zero ones, and the keyframe whose float
    score tells a left-to-right chain from any other order (tests/test_kfdb_definition.py)."""
    n_words, q, kfs = kd.ordered_sum_fixture()
    p = Pair(n_words)
    for i, b in enumerate(kfs):
        p.add(i, b)
    ex, _ = p.both(q)
    z = len(kfs) - 1
    at = ex[0].tolist().index(z)
    assert ex[3][at] and ex[2][at] == np.float32(1.0) and ex[3].sum() >= 4
    p.close()


def test_list_order(gpu):
    """40 keyframes added in shuffled id order, three erased from the middle, one re-added: ties on the
    first shared word are resolved by the add sequence."""
    rng = np.random.default_rng(40)
    n_words = 64
    p = Pair(n_words)
    order = rng.permutation(40)
    bows = {int(i): kd.random_bow(rng, n_words, int(rng.integers(3, 20))) for i in order}
    gone = [int(order[15]), int(order[20]), int(order[25])]
    # the keyframe that will come back shares its BowVector with two others, one added before and one
    # after it, and the query holds that vector's first word: all three tie on their first shared word
    bows[int(order[3])] = bows[int(order[30])] = bows[gone[1]]
    for i in order:
        p.add(int(i), bows[int(i)])
    q = kd.random_bow(rng, n_words, 24)
    if int(bows[gone[1]][0][0]) not in q[0].tolist():
        ids = np.sort(np.append(q[0][1:], bows[gone[1]][0][0])).astype(np.uint32)
        q = (ids, q[1])
    ex, _ = p.both(q)
    trio = [i for i in ex[0].tolist() if i in (int(order[3]), gone[1], int(order[30]))]
    assert trio == [int(order[3]), gone[1], int(order[30])]   # add order before the erase
    for i in gone:
        p.erase(i)
    ex, _ = p.both(q)
    assert not set(gone) & set(ex[0].tolist())
    p.add(gone[1], bows[gone[1]])
    ex, _ = p.both(q)
    first = {i: min(set(bows[i][0].tolist()) & set(q[0].tolist())) for i in ex[0].tolist()}
    firsts = [first[i] for i in ex[0].tolist()]
    assert firsts == sorted(firsts) and len(set(firsts)) < len(firsts)   # ties exist
    grp = [i for i in ex[0].tolist() if first[i] == first[gone[1]]]   # the re-added keyframe went to the back
    assert grp[-1] == gone[1] and grp.index(int(order[3])) < grp.index(int(order[30])) < len(grp) - 1
    assert len(p.g) == 38
    p.close()


def test_growth_and_compaction(gpu):
    """Past the initial arena capacity (32,768 words), then more than half erased: the survivors'
    results do not change, and new keyframes land behind them."""
    rng = np.random.default_rng(7)
    n_words = 1000
    p = Pair(n_words)
    q = kd.random_bow(rng, n_words, 300)
    for i in range(30):
        p.add(i, kd.random_bow(rng, n_words, 900))
    small = p.shared(q)
    for i in range(30, 80):                       # 72,000 words: two doublings
        p.add(i, kd.random_bow(rng, n_words, 900))
    ex = p.shared(q)
    assert len(ex[0]) == 80
    old = ex[0] < 30                              # the first 30 went through both reallocations
    assert ex[0][old].tolist() == small[0].tolist() and ex[1][old].tolist() == small[1].tolist()
    keep = [i for i in range(80) if i % 3 == 0]
    for i in range(80):
        if i not in keep:
            p.erase(i)                            # crosses the half-dead line several times
    ex2, _ = p.both(q)
    assert ex2[0].tolist() == [i for i in ex[0].tolist() if i in keep]
    m = np.isin(ex[0], keep)
    np.testing.assert_array_equal(ex2[1], ex[1][m])
    p.add(200, kd.random_bow(rng, n_words, 900))
    p.add(1, kd.random_bow(rng, n_words, 17))
    ex3, _ = p.both(q)
    assert set(ex3[0].tolist()) == set(keep) | {200, 1}
    p.g.clear()
    p.d = KeyFrameDatabaseDef(n_words)
    p.nbrs, p.maps = {}, {}
    assert len(p.g) == 0 and len(p.g.shared_words(q)[0]) == 0
    p.add(3, kd.random_bow(rng, n_words, 64))
    p.both(q)
    p.close()


def _stale(score_x_first):
    n_words, bows, nbrs, qa, qb = kd.stale_score_fixture()
    p = Pair(n_words)
    for i in sorted(bows):
        p.add(i, bows[i], nbrs.get(i, ()))
    if score_x_first:
        assert p.detect(qa).tolist() == [2]
    return p, qb


def test_stale_score(gpu):
    """Query A scores X. In query B, X shares one word and fails the gate but is a neighbour of a
    scored keyframe: the accumulated score includes X's score from A. A database in which X was never
    scored answers differently."""
    p, qb = _stale(True)
    ex = p.shared(qb)
    assert ex[0].tolist() == [0, 1, 2] and ex[3].tolist() == [True, True, False]
    assert p.detect(qb).tolist() == [0]
    p.close()
    fresh, qb = _stale(False)
    assert fresh.detect(qb).tolist() == [0, 1]
    # erase drops the entry's state: X erased and added again starts from 0
    p, qb = _stale(True)
    n_words, bows, _, _, _ = kd.stale_score_fixture()
    p.erase(2)
    p.add(2, bows[2])
    assert p.detect(qb).tolist() == [0, 1]
    p.close()
    fresh.close()


def test_covisibility(gpu):
    q = _u(list(range(10)))
    # two scored keyframes point to the same, strictly better, neighbour: one candidate. 99 is unknown.
    p = Pair(32)
    p.add(0, _u(list(range(9)) + [20]), [2, 99])
    p.add(1, _u(list(range(9)) + [21]), [2])
    p.add(2, _u(list(range(10))))
    assert p.detect(q).tolist() == [2]
    p.close()
    # an equal score does not replace pBestKF; the best keyframe of all sits in another map
    p = Pair(32)
    p.add(3, _u(list(range(9)) + [20]), [4])
    p.add(4, _u(list(range(9)) + [21]), [3])
    p.add(5, _u(list(range(10))), [3], map_id=1)
    assert p.detect(q).tolist() == [3, 4]
    assert p.detect(q, map_id=1).tolist() == [5]
    # a neighbour that is in the database but shares no word in this query is skipped
    p.add(6, _u([30, 31]), [])
    p.nbrs[3] = [6, 4]
    p.d.kfs[3].neighbours = [6, 4]
    assert p.detect(q).tolist() == [3, 4]
    p.close()


def test_info_callback(gpu):
    """info is asked at most once per keyframe id and query, callables work as dicts do, an exception
    inside it is re-raised after the call, and the cap protocol reports the needed count."""
    import ctypes
    from orb_slam3_ros_amd import _lib
    q = _u(list(range(10)))
    g = KeyFrameDatabase(32)
    for i in range(4):
        g.add(i, _u(list(range(9)) + [20 + i]))
    asked = []

    def nb(i):
        asked.append(i)
        return [(i + 1) % 4, (i + 2) % 4]

    got = g.DetectRelocalizationCandidates(q, 0, nb, lambda i: 0)
    assert sorted(asked) == [0, 1, 2, 3] and got.tolist() == [0, 1, 2, 3]

    def boom(i):
        raise KeyError("covisibility")

    with pytest.raises(KeyError):
        g.DetectRelocalizationCandidates(q, 0, boom)

    # a call whose callback failed commits nothing: keyframe 0's score from a first query survives a
    # failed second query that would have rescored it, and is read stale in a third
    h = KeyFrameDatabase(32)
    h.add(0, _u(list(range(10))))
    h.add(1, _u([0] + list(range(10, 19))))
    h.add(2, _u(list(range(10, 19)) + [19]))
    assert h.DetectRelocalizationCandidates(_u(list(range(10)))).tolist() == [0]     # 0 scored: 1.0
    with pytest.raises(KeyError):                                                    # would set 0 to 0.5
        h.DetectRelocalizationCandidates(_u(list(range(5)) + list(range(20, 25))), 0, boom)
    # 1 and 2 are scored (10 and 9 of 10 words: 1.0 and 0.9), 0 shares one word and fails the gate. 2's
    # neighbour 0 is read stale: with the first query's 1.0 it becomes 2's best keyframe (acc 1.9, and
    # 1's 1.0 falls under 0.75 * 1.9); with the failed query's 0.5 the answer would be [2]
    q3 = _u([0] + list(range(10, 19)))
    assert h.DetectRelocalizationCandidates(q3, 0, {2: [0]}).tolist() == [0]
    h.close()

    class Small(KeyFrameDatabase):   # a wrapper whose first capacity is too small: the cap protocol
        def __len__(self):
            return 1

    s = Small(32)
    for i in range(4):
        s.add(i, _u(list(range(9)) + [20 + i]))
    assert s.DetectRelocalizationCandidates(q).tolist() == [0, 1, 2, 3]
    assert s.shared_words(q)[0].tolist() == [0, 1, 2, 3]
    s.close()
    ids, w = q
    out, n = np.full(4, 7, np.int32), ctypes.c_int32(-1)
    rc = g._lib.orbfe_kfdb_detect_reloc(g._h, ids.ctypes.data, w.ctypes.data, 10, 0, _lib.KF_INFO_FN(), None,
                                        out.ctypes.data, 3, ctypes.byref(n))
    assert rc == _lib.ORBFE_E_ARG and n.value == 4 and (out == 7).all()
    kf, wd, sc, fl, mx = (np.full(4, 7, np.int32), np.full(4, 7, np.int32), np.full(4, 7, np.float32),
                          np.full(4, 7, np.uint8), ctypes.c_int32(-1))
    rc = g._lib.orbfe_kfdb_shared_words(g._h, ids.ctypes.data, w.ctypes.data, 10, kf.ctypes.data, wd.ctypes.data,
                                        sc.ctypes.data, fl.ctypes.data, 2, ctypes.byref(n), ctypes.byref(mx))
    assert rc == _lib.ORBFE_E_ARG and n.value == 4 and mx.value == -1
    assert all((a == 7).all() for a in (kf, wd, sc, fl))
    g.close()


def test_end_to_end_relocalisation(gpu, oracle_lib):
    """ComputeBoW -> add for 30 keyframes; a perturbed copy of one of them queries the database; the
    candidates go into SearchByBoWBatch over their resident features. The true keyframe is among
    them and its row equals the oracle's SearchByBoW."""
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.matcher import KeyFrameFeatures, ORBmatcher
    from orb_slam3_ros_amd.vocabulary import L1_NORM, TF_IDF, ORBVocabulary, synth_vocabulary
    rng = np.random.default_rng(30)
    par, leaf, desc, w = synth_vocabulary(rng, 10, 4)
    voc = ORBVocabulary.from_arrays(10, 4, L1_NORM, TF_IDF, par, leaf, desc, w)
    p = Pair(voc.n_words)
    kfs, fvs, feats = [], [], []
    for i in range(30):
        K = sm.synth_frame(rng, 400, stereo=False)
        bow, fv = voc.transform(K.desc, 4)
        p.add(i, bow)
        kfs.append(K)
        fvs.append(fv)
        feats.append(KeyFrameFeatures(K, fv))
    true = 17
    F, _ = sm.perturbed_frame(rng, kfs[true], rot=10.0, flip_p=0.03, drop=0.1)
    fbow, ffv = voc.transform(F.desc, 4)
    p.shared(fbow)
    cand = p.detect(fbow)
    assert true in cand.tolist()
    mps = [np.arange(kfs[c].N, dtype=np.int32) for c in cand]
    nm, rows = ORBmatcher(0.75, True).SearchByBoWBatch([feats[c] for c in cand], mps, F, ffv)
    at = cand.tolist().index(true)
    no, oo = oracle_lib.OracleMatcher(0.75, True).search_by_bow(kfs[true].keys, kfs[true].desc, mps[at], fvs[true], F,
                                                               ffv)
    assert nm[at] == no and no >= 15 and np.array_equal(rows[at], oo)
    for h in feats:
        h.close()
    p.close()
    voc.close()
