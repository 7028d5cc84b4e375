"""CPU: tests/place_recognition_definition.py (the restatement of DetectNBestCandidates the GPU tests
compare against) pinned on cases worked out by hand."""
import numpy as np

import place_recognition_definition as pr
from kfdb_definition import F32, KF
from place_recognition_definition import PlaceRecognitionDef, uniform


def _lists(res):
    return res[0].tolist(), res[1].tolist()


def test_connected_keyframe_moves_the_gate():
    n_words, bows, q = pr.gate_fixture()
    db = pr.build(PlaceRecognitionDef, n_words, bows)
    # maximum 10 words: gate int(10 * 0.8f) = 8, keyframe 1 (8 words) is not above it
    assert _lists(db.DetectNBestCandidates(q, [])) == ([0], [])
    assert db.kfs[1].mPlaceRecognitionScore == 0 and db.kfs[0].mPlaceRecognitionScore == F32(1.0)
    # 0 connected: maximum 8, gate int(6.4) = 6, both 8 and 7 words pass; 1 shares more mass
    assert _lists(db.DetectNBestCandidates(q, [0])) == ([1, 2], [])
    # identical vectors of 10 words at 0.1 share 8 (7) words: score 0.8 (0.7) up to rounding
    assert abs(float(db.kfs[1].mPlaceRecognitionScore) - 0.8) < 1e-6
    assert abs(float(db.kfs[2].mPlaceRecognitionScore) - 0.7) < 1e-6
    # a connected id that is not in the database is ignored
    assert _lists(db.DetectNBestCandidates(q, [0, 999])) == ([1, 2], [])


def test_equal_scores_keep_list_order_and_lists_fill_independently():
    n_words, bows, maps, q = pr.tie_fixture()
    db = pr.build(PlaceRecognitionDef, n_words, bows, maps=maps)
    # list order = add order 10..15; maps 0, 1, 0, 1, 0, 1
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=3)) == ([10, 12, 14], [11, 13, 15])
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=2)) == ([10, 12], [11, 13])
    assert _lists(db.DetectNBestCandidates(q, [], map_id=1, n=1)) == ([11], [10])
    # fewer than n available
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=5)) == ([10, 12, 14], [11, 13, 15])
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=0)) == ([], [])
    # a bad merge map, and a query map nobody is in
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=3, bad_maps=[1])) == ([10, 12, 14], [])
    assert _lists(db.DetectNBestCandidates(q, [], map_id=7, n=2)) == ([], [10, 11])
    # erase then add moves a keyframe to the back of every word's list
    db.erase(10)
    db.add(KF(10, bows[10], (), 0))
    assert db.kfs[10].mPlaceRecognitionScore == 0
    assert _lists(db.DetectNBestCandidates(q, [], map_id=0, n=3)) == ([12, 14, 10], [11, 13, 15])


def test_loop_full_while_merge_is_short():
    """One list full, the walk goes on for the other; a same-map keyframe met while loop is full is
    marked seen and dropped."""
    bows = {k: uniform(range(0, 8)) for k in range(5)}
    maps = {0: 0, 1: 0, 2: 0, 3: 1, 4: 0}
    db = pr.build(PlaceRecognitionDef, 64, bows, maps=maps)
    assert _lists(db.DetectNBestCandidates(uniform(range(0, 8)), [], map_id=0, n=2)) == ([0, 1], [3])


def test_best_neighbour_substitution_is_deduplicated():
    n_words, bows, nbrs, q = pr.dedupe_fixture()
    db = pr.build(PlaceRecognitionDef, n_words, bows, neighbours=nbrs)
    # scores: 2 -> 1.0, 0 and 1 -> 0.9, 3 -> 9 of its 12 words at 1/12 against 0.1: 0.75.
    # accScore: 0 and 1 -> 1.9 (pBestKF 2), 2 -> 1.0 (itself), 3 -> its own: sorted 0, 1, 2, 3 -> 2, 2, 2, 3
    assert _lists(db.DetectNBestCandidates(q, [], n=3)) == ([2, 3], [])
    # with 2 connected it carries no stamp: the neighbours do not count it
    assert _lists(db.DetectNBestCandidates(q, [2], n=3)) == ([0, 1, 3], [])


def test_stale_score_reaches_a_later_query():
    n_words, bows, nbrs, qa, qb = pr.stale_place_fixture()
    db = pr.build(PlaceRecognitionDef, n_words, bows, neighbours=nbrs)
    fresh = pr.build(PlaceRecognitionDef, n_words, bows, neighbours=nbrs)
    assert _lists(fresh.DetectNBestCandidates(qb, [])) == ([0, 1], [])
    assert _lists(db.DetectNBestCandidates(qa, [])) == ([2], [])
    assert db.kfs[2].mPlaceRecognitionScore == F32(1.0)
    # X (one shared word, gate 8) is not scored in B but stamped: 1's accScore is 0.9 + 1.0 and its
    # pBestKF is X itself
    assert _lists(db.DetectNBestCandidates(qb, [])) == ([2, 0], [])
    assert db.kfs[2].mPlaceRecognitionScore == F32(1.0)


def test_relocalisation_state_is_apart():
    n_words, bows, nbrs, qa, qb = pr.stale_place_fixture()
    db = pr.build(PlaceRecognitionDef, n_words, bows, neighbours=nbrs)
    db.DetectNBestCandidates(qa, [])
    assert db.kfs[2].mRelocScore == 0
    assert db.DetectRelocalizationCandidates(qb).tolist() == [0, 1]   # no stale reloc score: both above 0.75 * best
    assert db.kfs[2].mPlaceRecognitionScore == F32(1.0) and db.kfs[0].mRelocScore == F32(1.0)
    assert _lists(db.DetectNBestCandidates(qb, [])) == ([2, 0], [])


def test_empty_cases():
    db = PlaceRecognitionDef(64)
    assert _lists(db.DetectNBestCandidates(uniform([1, 2]), [])) == ([], [])
    db.add(KF(0, uniform([1, 2])))
    assert _lists(db.DetectNBestCandidates((np.zeros(0, np.uint32), np.zeros(0)), [])) == ([], [])
    assert _lists(db.DetectNBestCandidates(uniform([5, 6]), [])) == ([], [])
    assert _lists(db.DetectNBestCandidates(uniform([1, 2]), [0])) == ([], [])   # the only sharer is connected
