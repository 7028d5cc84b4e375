"""CPU: the planted ComputeBoW cases (tests/bow_patterns.py) through the definition
(oracle/bow_definition.py) and the C++ oracle. For every case: the oracle's word ids, weight bytes, node ids,
offsets and indices equal the definition's, and the definition's trace shows that the rule the case names
decided (the case's own `check`). Where a case is marked order-sensitive, summing in another order gives other
weight bytes, so a case that stopped telling the orders apart fails here. The tie cases show, in the trace,
two children at the winning distance at the named positions and the lowest index as the winner. The same
comparison runs on seeded random images over full trees. No case is skipped."""
import numpy as np
import pytest

import bow_patterns as P
from oracle import bow_definition as bd
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.vocabulary import synth_vocabulary

CASES = P.all_cases()


def _same(defn, ora, name):
    (db, dw), (dfid, dfoff, dfidx), _ = defn
    (ob, ow), (ofid, ofoff, ofidx) = ora
    np.testing.assert_array_equal(ob, db, err_msg=name)
    assert ow.tobytes() == dw.tobytes(), (name, ow, dw)
    np.testing.assert_array_equal(ofid, dfid, err_msg=name)
    np.testing.assert_array_equal(ofoff, dfoff, err_msg=name)
    np.testing.assert_array_equal(ofidx, dfidx, err_msg=name)


def test_chain_orders():
    """The three summation orders on addends whose sum depends on them."""
    xs = [1e16, 1.0, 1.0, -1e16, 1.0]
    assert bd.chain(xs) == 1.0 and bd.chain(xs, "sorted") == 0.0 and bd.chain(xs, "pairwise") == 0.0
    assert bd.chain([1e16, -1e16, 1.0, 1.0], "pairwise") == 2.0 and bd.chain([1e16, 1.0, 1.0, -1e16], "pairwise") == 0.0
    assert bd.chain([0.1] * 10, start=0.0) != bd.chain([0.1] * 10, "pairwise", start=0.0)
    assert bd.chain([2.5]) == 2.5 and bd.chain([], start=0.0) == 0.0
    with pytest.raises(ValueError):
        bd.chain(xs, "reversed")


def test_case_inventory():
    names = {c.name for c in CASES}
    need = ["distance-0", "distance-256-all", "distance-255-vs-256", "chunks-9-children", "chunks-130-children",
            "tie-across-chunk-edge", "tie-across-chunk-edge-G64", "best-in-last-chunk", "tie-first-of-two-chunks",
            "arity-1-chain", "ragged-arity", "levelsup-ge-L", "levelsup-ge-L-plus-2", "levelsup-0",
            "unflagged-childless-node-tfidf", "unflagged-childless-node-idf", "dot-product-tf-divides-by-words",
            "idf-keeps-first", "l2-norm-bytes", "word-sum-order", "single-word-all-features-64",
            "single-word-all-features-1025", "kept-equals-n", "every-feature-own-word", "bin-ragged",
            "bin-trailing-bytes", "bin-k-20"]
    for rule in ("tie-first-last", "tie-adjacent", "best-is-last"):
        need += [f"{rule}-G{G}" for G in (4, 8, 16, 32, 64)] + [f"{rule}-G{G}-full" for G in (4, 16, 32, 64)]
    need += [f"leaf-above-L-levelsup-{ls}" for ls in (0, 1, 2, 3, 4, 6)]
    need += [f"{r}-{w}" for w in ("tfidf", "idf") for r in ("weight-zero", "weight-negative", "weight-minus-zero",
                                                           "weight-nan", "weight-denormal-min", "all-stopped",
                                                           "one-kept-of-many")]
    need += [f"weighting-{w}-{s}" for w in ("tfidf", "tf", "idf", "binary") for s in ("l1", "l2", "dot")]
    need += [f"norm-order-{n}" for n in (63, 64, 65, 128, 129)]
    need += [f"kept-{m}" for m in (1, 1023, 1024, 1025, 2047, 2048, 2049)]
    need += [f"n-{n}-G{G}" for n in (1, 2, 63, 64, 65) for G in (4, 8, 16, 32, 64)]
    for n in need:
        assert n in names, n
    assert len(need) == len(set(need)) == len(CASES), sorted(names - set(need))
    # the declared k of the tie cases gives the group width their name carries (the power of two >= k, 4..64)
    ks = {(G, "-full" if full else ""): k for G, k, full in [(G, k, 0) for G, k in P.GROUPS] + [(G, G, 1) for G in P.FULL]}
    assert sorted(ks.values()) == [2, 4, 8, 10, 16, 20, 32, 33, 64]
    for c in CASES:
        if c.name.startswith(("tie-first-last-G", "tie-adjacent-G", "best-is-last-G")):
            G = int(c.name.split("-G")[1].split("-")[0])
            assert c.voc.k == ks[(G, "-full" if c.name.endswith("-full") else "")] and G // 2 < max(c.voc.k, 3) <= G
    sens = {c.name for c in CASES if c.sens}
    assert sens == {"word-sum-order", "single-word-all-features-64", "single-word-all-features-1025"} | {
        f"norm-order-{n}" for n in (63, 64, 65, 128, 129)}
    # tiny vocabularies and images: a count in the name is the only licence for more
    for c in CASES:
        assert c.voc.n_nodes <= 5000 and c.voc.L <= 4, c.name
        assert c.n <= 2100, c.name
        assert c.n <= 100 or any(ch.isdigit() for ch in c.name.split("-G")[0]) or c.name in (
            "kept-equals-n", "every-feature-own-word"), (c.name, c.n)
        assert c.voc.k ** (c.voc.L + 1) < 2 ** 31, c.name   # the loaders' `int expected`


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case(oracle_lib, case):
    defn = P.run_definition(case)
    _same(defn, P.run_oracle(oracle_lib, case), case.name)
    case.check(case, defn[2])
    (ids, w), (fid, foff, fidx), tr = defn
    assert len(tr["f"]) == case.n and len(foff) == len(fid) + 1 and int(foff[-1]) == len(fidx)
    assert len(fidx) == sum(f["kept"] for f in tr["f"])
    if case.sens:
        other = [P.run_definition(case, order)[0] for order in ("sorted", "pairwise")]
        assert all(np.array_equal(o[0], ids) for o in other)
        assert any(o[1].tobytes() != w.tobytes() for o in other), "no other order changes the bytes any more"


TIES = [c for c in CASES if c.name.startswith(("tie-", "distance-256-all"))]


@pytest.mark.parametrize("case", TIES, ids=repr)
def test_tie_positions(case):
    """At every level of the planted feature's walk at least two children share the winning distance, the
    positions are the ones the name says, and the lowest index won."""
    tr = P.run_definition(case)[2]
    f = tr["f"][0]
    assert len(f["levels"]) == 2
    for lv in f["levels"]:
        best = min(lv["dist"])
        at = [j for j, d in enumerate(lv["dist"]) if d == best]
        assert len(at) >= 2 and lv["tie"] and lv["won"] == at[0] and f["path"][f["levels"].index(lv)] == lv["children"][at[0]]
    a = len(f["levels"][0]["children"])
    top = [j for j, d in enumerate(f["levels"][0]["dist"]) if d == min(f["levels"][0]["dist"])]
    if case.name.startswith("tie-first-last"):
        assert top == [0, a - 1]
    elif case.name.startswith("tie-adjacent"):
        assert len(top) == 2 and top[1] == top[0] + 1
    elif case.name == "tie-across-chunk-edge":
        assert top == [3, 4]          # G = 4: the last lane of one chunk, the first of the next
    elif case.name == "tie-across-chunk-edge-G64":
        assert top == [63, 64, 128]
    elif case.name == "tie-first-of-two-chunks":
        assert top == [0, 4]
    elif case.name == "distance-256-all":
        assert top == [0, 1, 2, 3] and min(f["levels"][0]["dist"]) == 256


@pytest.mark.parametrize("k,L", [(2, 4), (10, 4), (20, 2)])
def test_random_images(oracle_lib, k, L):
    """Seeded random images over full trees, every weighting and scoring in turn: definition == oracle."""
    rng = np.random.default_rng(10 * k + L)
    par, leaf, desc, w = synth_vocabulary(rng, k, L, stop_frac=0.1)
    combos = [(P.L1_NORM, P.TF_IDF), (P.DOT_PRODUCT, P.TF), (P.L2_NORM, P.IDF), (P.L1_NORM, P.BINARY)]
    for i, (scoring, weighting) in enumerate(combos):
        voc = P.Voc(k, L, scoring, weighting, (par, leaf, desc, w))
        f = rng.integers(0, 256, (150, 32), dtype=np.uint8)
        f[:75] = sm.flip_bits(rng, desc[rng.integers(1, len(desc), 75)], 0.08)
        case = P.Case(f"random-{k}-{L}-{i}", voc, (4, 0, 2, 6)[i], f)
        defn = P.run_definition(case)
        _same(defn, P.run_oracle(oracle_lib, case), case.name)
        assert len(defn[0][0]) > 10


def test_loader_definition(oracle_lib):
    """parse_bin reads what save_bin wrote, stops at the expected node count, and refuses what the reference does."""
    case = next(c for c in CASES if c.name == "bin-ragged")
    rv = P.ragged_voc()
    for a, b in zip(case.voc.args(), rv.args()):
        assert np.array_equal(a, b)
    assert bd.parse_bin(P.save_bin(21, 2, 0, 0, rv.par, rv.leaf, rv.desc, rv.w)) is None
    assert oracle_lib.OracleVocabulary.from_bin(P.save_bin(21, 2, 0, 0, rv.par, rv.leaf, rv.desc, rv.w)) is None
