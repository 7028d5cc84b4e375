"""CPU: the C++ twin of the keyframe database (tests/native/kfdb_cpu.cpp: std::list, std::map,
std::vector<list>, the CPU baseline of tools/kfdb_timing.py) against tests/kfdb_definition.py on the
fixtures the GPU tests use: ids and order, words, scored flags, scores byte for byte, candidates."""
import numpy as np
import pytest

import kfdb_definition as kd
from kfdb_definition import KF, KeyFrameDatabaseDef, KeyFrameDatabaseNative


class Pair:
    def __init__(self, n_words):
        self.n, self.d = KeyFrameDatabaseNative(n_words), KeyFrameDatabaseDef(n_words)

    def add(self, kf_id, bow, neighbours=(), map_id=0):
        self.n.add(KF(kf_id, bow, neighbours, map_id))
        self.d.add(KF(kf_id, bow, neighbours, map_id))

    def erase(self, kf_id):
        self.n.erase(kf_id)
        self.d.erase(kf_id)

    def both(self, q, map_id=0):
        got, exp = self.n.shared_words(q), self.d.shared_words(q)
        for k in (0, 1, 3):
            np.testing.assert_array_equal(got[k], exp[k])
        assert got[2].tobytes() == exp[2].tobytes() and got[4] == exp[4]
        c, e = self.n.DetectRelocalizationCandidates(q, map_id), self.d.DetectRelocalizationCandidates(q, map_id)
        assert np.array_equal(c, e), (c, e)
        return exp, e


@pytest.fixture
def pair():
    made = []

    def make(n_words):
        made.append(Pair(n_words))
        return made[-1]
    yield make
    for p in made:
        p.n.close()


def test_ordered_sum(pair):
    n_words, q, kfs = kd.ordered_sum_fixture()
    p = pair(n_words)
    for i, b in enumerate(kfs):
        p.add(i, b)
    ex, _ = p.both(q)
    at = ex[0].tolist().index(len(kfs) - 1)
    assert ex[3][at] and ex[2][at] == np.float32(1.0)


def test_stale_score(pair):
    n_words, bows, nbrs, qa, qb = kd.stale_score_fixture()
    p = pair(n_words)
    for i in sorted(bows):
        p.add(i, bows[i], nbrs.get(i, ()))
    assert p.both(qa)[1].tolist() == [2]
    assert p.both(qb)[1].tolist() == [0]
    fresh = pair(n_words)
    for i in sorted(bows):
        fresh.add(i, bows[i], nbrs.get(i, ()))
    assert fresh.both(qb)[1].tolist() == [0, 1]


def test_list_order_and_random_databases(pair):
    rng = np.random.default_rng(40)
    for n_words, qn in ((64, 24), (1000, 300)):
        p = pair(n_words)
        order = [int(i) for i in rng.permutation(40)]
        bows = {i: kd.random_bow(rng, n_words, int(rng.integers(3, min(n_words, 400) // 3))) for i in order}
        for i in order:
            p.add(i, bows[i], [int(x) for x in rng.choice(45, 4, replace=False)], int(rng.integers(0, 2)))
        q = kd.random_bow(rng, n_words, qn)
        p.both(q)
        for i in (order[15], order[20], order[25]):
            p.erase(i)
        p.both(q, map_id=1)
        p.add(order[20], bows[order[20]])
        ex, _ = p.both(q)
        assert order[20] in ex[0].tolist()
        p.both(kd.random_bow(rng, n_words, 1))
        assert p.n.detect_reps(q, 3) == len(p.d.DetectRelocalizationCandidates(q))


def test_covisibility(pair):
    u = lambda ids: (np.array(ids, np.uint32), np.full(len(ids), 1.0 / len(ids)))   # noqa: E731
    q = u(list(range(10)))
    p = pair(32)
    p.add(0, u(list(range(9)) + [20]), [2, 99])   # 99 is not in the table
    p.add(1, u(list(range(9)) + [21]), [2])
    p.add(2, u(list(range(10))))
    assert p.both(q)[1].tolist() == [2]
    p = pair(32)
    p.add(3, u(list(range(9)) + [20]), [4])
    p.add(4, u(list(range(9)) + [21]), [3])
    p.add(5, u(list(range(10))), [3], map_id=1)
    assert p.both(q)[1].tolist() == [3, 4]
    assert p.both(q, map_id=1)[1].tolist() == [5]
