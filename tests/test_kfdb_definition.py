"""CPU: hand-worked cases for tests/kfdb_definition.py, the restatement the GPU keyframe database is
compared with (KeyFrameDatabase.cc:39-66,733-845, ScoringObject.cpp:23-68)."""
import numpy as np

import kfdb_definition as kd
from kfdb_definition import KF, KeyFrameDatabaseDef

F32 = np.float32


def _bow(pairs):
    return np.array([p[0] for p in pairs], np.uint32), np.array([p[1] for p in pairs], np.float64)


def test_three_keyframes_by_hand():
    db = KeyFrameDatabaseDef(16)
    db.add(KF(7, _bow([(2, 0.5), (5, 0.5)])))
    db.add(KF(3, _bow([(1, 0.25), (2, 0.25), (5, 0.25), (9, 0.25)])))
    db.add(KF(4, _bow([(9, 1.0)])))
    q = _bow([(1, 0.5), (2, 0.25), (9, 0.25)])
    ids, words, scores, scored, mx = db.shared_words(q)
    # word 1: [3]; word 2: [7, 3]; word 9: [3, 4]  ->  3, 7, 4
    assert ids.tolist() == [3, 7, 4]
    assert words.tolist() == [3, 1, 1]
    assert mx == 3   # minCommonWords = int(2.4f) = 2: only keyframe 3 is scored
    assert scored.tolist() == [True, False, False]
    # keyframe 3: words 1, 2, 9: (|.5-.25| - .5 - .25) + (0 - .25 - .25) + (0 - .25 - .25) = -1.5 -> 0.75
    chain = 0.0
    for t in (abs(0.5 - 0.25) - 0.5 - 0.25, abs(0.25 - 0.25) - 0.25 - 0.25, abs(0.25 - 0.25) - 0.25 - 0.25):
        chain += t
    assert chain == -1.5
    assert scores.tobytes() == np.array([0.75, 0, 0], np.float32).tobytes()
    assert db.kfs[3].mRelocScore == F32(0.75) and db.kfs[7].mRelocScore == F32(0)
    assert db.DetectRelocalizationCandidates(q).tolist() == [3]


def test_min_common_words_gate():
    """int(maxCommonWords * 0.8f): 4 -> 3, 5 -> 4, 10 -> 8, and the gate is strictly greater."""
    for mx, mn in ((4, 3), (5, 4), (10, 8)):
        assert int(F32(mx) * F32(0.8)) == mn
        db = KeyFrameDatabaseDef(32)
        u = lambda n: (np.arange(n, dtype=np.uint32), np.full(n, 1.0 / n))   # noqa: E731
        db.add(KF(0, u(mx)))
        db.add(KF(1, u(mn + 1)))
        db.add(KF(2, u(mn)))
        ids, words, _, scored, got = db.shared_words(u(mx))
        assert got == mx and ids.tolist() == [0, 1, 2] and words.tolist() == [mx, mn + 1, mn]
        assert scored.tolist() == [True, True, False]


def test_erase_then_add_moves_to_the_back():
    db = KeyFrameDatabaseDef(8)
    b = _bow([(3, 1.0)])
    for i in (0, 1, 2):
        db.add(KF(i, b))
    assert db.shared_words(b)[0].tolist() == [0, 1, 2]
    db.erase(0)
    assert db.shared_words(b)[0].tolist() == [1, 2]
    db.add(KF(0, b))
    assert db.shared_words(b)[0].tolist() == [1, 2, 0]


def _stale_db(score_x_first):
    n_words, bows, nbrs, qa, qb = kd.stale_score_fixture()
    db = KeyFrameDatabaseDef(n_words)
    for i in sorted(bows):
        db.add(KF(i, bows[i], nbrs.get(i, ())))
    if score_x_first:
        assert db.DetectRelocalizationCandidates(qa).tolist() == [2]
        assert db.kfs[2].mRelocScore == F32(1)
    return db, qb


def test_stale_score_is_read():
    db, qb = _stale_db(True)
    ids, words, scores, scored, mx = db.shared_words(qb)
    assert ids.tolist() == [0, 1, 2] and words.tolist() == [10, 9, 1] and mx == 10
    assert scored.tolist() == [True, True, False]
    assert scores[:2].tolist() == [F32(1.0), F32(0.9)]
    assert db.kfs[2].mRelocScore == F32(1)   # not rewritten: X failed the gate
    # accScore(0) = 1 + X's stale 1 = 2, accScore(1) = 0.9 < 0.75 * 2
    assert db.DetectRelocalizationCandidates(qb).tolist() == [0]
    fresh, qb = _stale_db(False)
    # X never scored: accScore(0) = 1, accScore(1) = 0.9 > 0.75
    assert fresh.DetectRelocalizationCandidates(qb).tolist() == [0, 1]


def test_ordered_sum_fixture_is_order_sensitive():
    """Summing the same terms in reverse gives another double for at least one keyframe (and another
    float score), so a tree or atomic sum on the device cannot pass the GPU test by luck."""
    _, q, kfs = kd.ordered_sum_fixture()
    differs = 0
    for b in kfs:
        terms = kd.shared_terms(q[0].tolist(), q[1].tolist(), b[0].tolist(), b[1].tolist())
        assert len(terms) > 40
        fwd = 0.0
        for t in terms:
            fwd += t
        rev = 0.0
        for t in reversed(terms):
            rev += t
        assert -fwd / 2.0 == kd.l1_score(q[0].tolist(), q[1].tolist(), b[0].tolist(), b[1].tolist())
        differs += fwd != rev
    assert differs >= 1
    # the last keyframe: the order reaches the float score (its terms span more than one wave's 64 lanes)
    assert len(terms) == 102
    assert fwd == -(2.0 + 2.0 ** -23) and F32(-fwd / 2.0) == F32(1.0)
    assert F32(-rev / 2.0) == F32(1.0) + F32(2.0 ** -23)
    pair = 0.0   # a pairwise tree over the same terms
    level = list(terms)
    while len(level) > 1:
        level = [sum(level[i:i + 2]) for i in range(0, len(level), 2)]
    pair = level[0]
    assert F32(-pair / 2.0) != F32(-fwd / 2.0)
    chunks = sum(terms[:64]) + sum(terms[64:])   # per-64 partial sums, then combined
    assert F32(-chunks / 2.0) != F32(-fwd / 2.0)


def test_covisibility_tail():
    u = lambda ids: (np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids)))   # noqa: E731
    q = u(list(range(10)))
    # 0 and 1 both point to 2, the best; 3 (equal score to its neighbour 4) keeps itself; 5 is in another map
    db = KeyFrameDatabaseDef(32)
    db.add(KF(0, u(list(range(9)) + [20]), [2, 99]))
    db.add(KF(1, u(list(range(9)) + [21]), [2]))
    db.add(KF(2, u(list(range(10)))))
    assert db.DetectRelocalizationCandidates(q).tolist() == [2]
    db2 = KeyFrameDatabaseDef(32)
    db2.add(KF(3, u(list(range(9)) + [20]), [4]))
    db2.add(KF(4, u(list(range(9)) + [21]), [3]))
    db2.add(KF(5, u(list(range(10))), [3], map_id=1))   # accScore 1.9, the best of all, but in map 1
    assert db2.DetectRelocalizationCandidates(q).tolist() == [3, 4]
    assert db2.DetectRelocalizationCandidates(q, map_id=1).tolist() == [5]
