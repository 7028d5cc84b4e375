"""Planted ComputeBoW cases: one rule of TemplatedVocabulary::transform (TemplatedVocabulary.h:1139-1206,
:1229-1270) or of the kernels' own thresholds per case, at the value where it decides. Each case carries a
`check(case, trace)` that proves from the trace of oracle/bow_definition.py that the rule it names decided;
order-sensitive cases (`sens`) must come out with other weight bytes under another summation order.

Two ways of planting a vocabulary, both with exact distances:
  sized   every node is the base descriptor B with a chosen number of bits flipped, so the feature B has a
          chosen distance to every node of the tree (descent ties, distance extremes, chunk edges);
  coded   a child is its parent with the 64-bit block of its level set to the child's code, so a leaf's own
          descriptor walks to that leaf (distance to the right child: a constant; to a sibling: that constant
          plus the distance of the two codes). Images over many words are made of leaf descriptors.

all_cases() -> [Case]; Case: name, voc (Voc: k, L, scoring, weighting and the arrays of
ORBVocabulary.from_arrays; blob: the binary file the loader cases go through), levelsup, desc (uint8 [n, 32]),
check, sens.
"""
import functools
import math
import struct

import numpy as np

from oracle import bow_definition as bd
from orb_slam3_ros_amd.vocabulary import save_bin

TF_IDF, TF, IDF, BINARY = bd.TF_IDF, bd.TF, bd.IDF, bd.BINARY
L1_NORM, L2_NORM, DOT_PRODUCT = bd.L1_NORM, bd.L2_NORM, bd.DOT_PRODUCT
WNAME = {TF_IDF: "tfidf", TF: "tf", IDF: "idf", BINARY: "binary"}
SNAME = {L1_NORM: "l1", L2_NORM: "l2", DOT_PRODUCT: "dot"}
GROUPS = ((4, 2), (8, 8), (16, 10), (32, 20), (64, 33))   # (G, the smallest declared k that gives it)
FULL = (4, 16, 32, 64)                                     # k = G as well, where the line above leaves lanes idle
SIZES = (1, 2, 63, 64, 65)
NORM_WORDS = (63, 64, 65, 128, 129)
KEPT = (1, 1023, 1024, 1025, 2047, 2048, 2049)
LEAF_ABOVE_LEVELSUP = (0, 1, 2, 3, 4, 6)
BEST, FAR = 40, 100


def base_desc(seed):
    return np.random.default_rng(9000 + seed).integers(0, 256, 32, dtype=np.uint8)


def flip(desc, bits):
    """desc with the given bit positions flipped."""
    b = np.unpackbits(desc)
    b[np.asarray(list(bits), int)] ^= 1
    return np.packbits(b)


def away(desc, d, salt=0):
    """desc at Hamming distance exactly d; another salt, another set of bits (67 is coprime to 256)."""
    assert 0 <= d <= 256
    return flip(desc, {(salt * 37 + 67 * t) % 256 for t in range(d)})


def away_many(desc, ds, salts):
    """away(desc, ds[i], salts[i]) for every i, as rows."""
    ds, salts, t = np.asarray(ds, int), np.asarray(salts, int), np.arange(256)
    cols = (salts[:, None] * 37 + 67 * t[None, :]) % 256
    on = t[None, :] < ds[:, None]
    bits = np.zeros((len(ds), 256), np.uint8)
    bits[np.nonzero(on)[0], cols[on]] = 1
    return np.packbits(bits, axis=1) ^ np.asarray(desc, np.uint8)[None, :]


class Builder:
    def __init__(self):
        self.par, self.leaf, self.desc, self.w = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def add(self, parent, desc, leaf=1, w=1.0):
        self.par.append(parent)
        self.leaf.append(leaf)
        self.desc.append(np.asarray(desc, np.uint8))
        self.w.append(w)
        return len(self.par) - 1

    def arrays(self):
        return (np.array(self.par, np.int32), np.array(self.leaf, np.uint8), np.array(self.desc, np.uint8),
                np.array(self.w, np.float64))


class Voc:
    def __init__(self, k, L, scoring, weighting, arrays, blob=None):
        self.k, self.L, self.scoring, self.weighting = k, L, scoring, weighting
        self.par, self.leaf, self.desc, self.w = arrays
        self.blob = blob
        self._oracle = None

    @classmethod
    def from_blob(cls, blob):
        """The tree as the definition's loadFromBinFile reads it; the device and the oracle load the bytes."""
        k, L, s, w, par, leaf, desc, wt = bd.parse_bin(blob)
        return cls(k, L, s, w, (par, leaf, desc, wt), blob)

    def args(self):
        return self.k, self.L, self.scoring, self.weighting, self.par, self.leaf, self.desc, self.w

    def variant(self, scoring, weighting, w=None):
        return Voc(self.k, self.L, scoring, weighting, (self.par, self.leaf, self.desc, self.w if w is None else w))

    @property
    def n_nodes(self):
        return len(self.par)

    def children(self, p):
        return [int(i) for i in np.flatnonzero(self.par[1:] == p) + 1]

    def leaves(self):
        has = np.zeros(self.n_nodes, bool)
        has[self.par[1:]] = True
        return [i for i in range(1, self.n_nodes) if not has[i]]

    def word(self, node):
        return int(self.leaf[1:node + 1].astype(bool).sum()) - 1 if self.leaf[node] else 0

    def device(self):
        from orb_slam3_ros_amd.vocabulary import ORBVocabulary
        return ORBVocabulary.from_bin(self.blob) if self.blob is not None else ORBVocabulary.from_arrays(*self.args())

    def oracle(self, oracle_lib):
        if self._oracle is None:
            O = oracle_lib.OracleVocabulary
            self._oracle = O.from_bin(self.blob) if self.blob is not None else O.from_arrays(*self.args())
        return self._oracle


class Case:
    def __init__(self, name, voc, levelsup, desc, check=None, sens=False):
        self.name, self.voc, self.levelsup, self.sens = name, voc, levelsup, sens
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.check = check or (lambda c, tr: None)

    @property
    def n(self):
        return len(self.desc)

    def __repr__(self):
        return self.name


def run_definition(case, order="feature", desc=None):
    return bd.py_transform(*case.voc.args(), case.desc if desc is None else desc, case.levelsup, order)


def run_oracle(oracle_lib, case):
    return case.voc.oracle(oracle_lib).transform(case.desc, case.levelsup)


def leaf_weight(i):
    return 0.25 + (i * 0.6180339887) % 5.0


def randoms(seed, n):
    return np.random.default_rng(5000 + seed).integers(0, 256, (n, 32), dtype=np.uint8)


# ---- sized trees: the feature B has a chosen distance to every node ----
def sized_voc(k, B, d1, d2, L=2):
    """Root with len(d1) children at distances d1 from B; each of them has len(d2) leaves at distances d2."""
    a1, a2 = len(d1), len(d2)
    n = 1 + a1 + a1 * a2
    ids = np.arange(n)
    par = np.concatenate([[0], np.zeros(a1, int), np.repeat(1 + np.arange(a1), a2)]).astype(np.int32)
    ds = np.concatenate([[0], d1, np.tile(d2, a1)])
    salt = np.concatenate([[0], np.arange(a1), ids[1 + a1:]])
    desc = away_many(B, ds, salt)
    desc[0] = 0
    leaf = (ids > a1).astype(np.uint8)
    w = np.where(ids > a1, [leaf_weight(i) for i in ids], 0.0)
    assert all(np.array_equal(desc[i], away(B, int(ds[i]), int(salt[i]))) for i in (1, a1, n - 1))
    return Voc(k, L, L1_NORM, TF_IDF, (par, leaf, desc, w))


def dists(a, best):
    """a distances, FAR and more, with BEST (or the given value) at the positions of `best`."""
    d = [FAR + (j * 7) % 50 for j in range(a)]
    for j, v in (best.items() if isinstance(best, dict) else {j: BEST for j in best}.items()):
        d[j] = v
    return d


def sized_image(B, seed):
    r = randoms(seed, 2)
    return np.stack([B, B, r[0], B, r[1]])


def winners_check(levels):
    """levels: per tree level (the positions at the winning distance, that distance). The lowest index won."""
    def check(c, tr):
        f = tr["f"][0]
        assert len(f["levels"]) == len(levels)
        for lv, (pos, d) in zip(f["levels"], levels):
            at = [j for j, x in enumerate(lv["dist"]) if x == min(lv["dist"])]
            assert at == sorted(pos) and min(lv["dist"]) == d, (c.name, at, pos, min(lv["dist"]))
            assert lv["won"] == min(pos) and lv["tie"] == (len(pos) > 1), c.name
        assert f["kept"] and all(tr["f"][i] is f for i in (1, 3))
    return check


def _tie_cases():
    out = []
    ks = [(G, k, "") for G, k in GROUPS] + [(G, G, "-full") for G in FULL]
    for G, k, tag in ks:
        a = k
        rules = {"tie-first-last": [0, a - 1], "tie-adjacent": [(a - 1) // 2, (a - 1) // 2 + 1], "best-is-last": [a - 1]}
        for r, (name, pos) in enumerate(rules.items()):
            B = base_desc(100 * G + 10 * len(tag) + r)
            voc = sized_voc(k, B, dists(a, pos), dists(a, pos))
            out.append(Case(f"{name}-G{G}{tag}", voc, 1, sized_image(B, G + r), winners_check([(pos, BEST)] * 2)))
    return out


def _distance_cases():
    out = []
    B = base_desc(1)
    out.append(Case("distance-0", sized_voc(4, B, dists(4, {2: 0}), dists(4, {1: 0})), 1, sized_image(B, 1),
                    winners_check([([2], 0), ([1], 0)])))
    B = base_desc(2)
    out.append(Case("distance-256-all", sized_voc(4, B, [256] * 4, [256] * 4), 1, sized_image(B, 2),
                    winners_check([([0, 1, 2, 3], 256)] * 2)))
    B = base_desc(3)
    out.append(Case("distance-255-vs-256", sized_voc(4, B, [256, 256, 256, 255], [256, 255, 256, 256]), 1,
                    sized_image(B, 3), winners_check([([3], 255), ([1], 255)])))
    return out


def _chunk_cases():
    """Nodes with more children than the group has lanes: declared k = 4 (G = 4) with 9 children, declared
    k = 64 with 130."""
    out = []

    def one(name, k, seed, p1, p2, a1, a2):
        B = base_desc(200 + seed)
        l1 = p1 if isinstance(p1, dict) else {j: BEST for j in p1}
        l2 = p2 if isinstance(p2, dict) else {j: BEST for j in p2}
        voc = sized_voc(k, B, dists(a1, l1), dists(a2, l2))
        w1 = [j for j, v in l1.items() if v == min(l1.values())]
        w2 = [j for j, v in l2.items() if v == min(l2.values())]

        def check(c, tr, w1=w1, w2=w2):
            winners_check([(w1, BEST), (w2, BEST)])(c, tr)
            G = 4 if c.voc.k <= 4 else 64
            assert len(tr["f"][0]["levels"][0]["children"]) > G
        out.append(Case(name, voc, 1, sized_image(B, 200 + seed), check))

    # a near miss one lane earlier and in the first chunk, the best in a later chunk
    one("chunks-9-children", 4, 0, {6: BEST, 5: BEST + 1, 0: BEST + 2}, {5: BEST, 1: BEST + 1}, 9, 9)
    one("tie-across-chunk-edge", 4, 1, [3, 4], [7, 8], 9, 9)
    one("best-in-last-chunk", 4, 2, {8: BEST, 0: BEST + 1, 4: BEST + 1}, {8: BEST, 7: BEST + 1}, 9, 9)
    one("tie-first-of-two-chunks", 4, 3, [0, 4], [1, 5, 8], 9, 9)
    one("chunks-130-children", 64, 4, {129: BEST, 64: BEST + 1, 0: BEST + 2}, [1], 130, 2)
    one("tie-across-chunk-edge-G64", 64, 5, [63, 64, 128], [0, 1], 130, 2)
    return out


# ---- coded trees: a leaf's descriptor walks to that leaf ----
def coded_voc(k, L, arity, seed, scoring=L1_NORM, weighting=TF_IDF, weight=None, flag=None):
    """arity(path) -> number of children of the node reached by the child indices `path` (0: a leaf).
    weight(node id, path) / flag(node id, path) default to leaf_weight and 1 for childless nodes."""
    rng = np.random.default_rng(seed)
    codes = {}

    def code(level, j):
        while (level, j) not in codes:
            c = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()
            if c not in [v for (lv, _), v in codes.items() if lv == level]:
                codes[(level, j)] = c
        return np.frombuffer(codes[(level, j)], np.uint8)

    b = Builder()
    paths = {0: ()}
    todo = [0]
    while todo:   # breadth first, DBoW2's node order
        nxt = []
        for p in todo:
            path = paths[p]
            for j in range(arity(path)):
                d = b.desc[p].copy()
                d[8 * len(path):8 * len(path) + 8] = code(len(path), j)
                cp = path + (j,)
                i = len(b.par)
                kids = len(cp) < 4 and arity(cp) > 0
                b.add(p, d, leaf=0 if kids else (1 if flag is None else flag(i, cp)),
                      w=0.0 if kids else (leaf_weight(i) if weight is None else weight(i, cp)))
                paths[i] = cp
                if kids:
                    nxt.append(i)
        todo = nxt
    v = Voc(k, L, scoring, weighting, b.arrays())
    v.paths = paths
    return v


def full(k, L):
    return lambda path: k if len(path) < L else 0


def near(rng, d, nbits=3):
    """d with nbits of its last 64 bits flipped: the blocks the codes use stay as they are for L <= 3."""
    return flip(d, 192 + rng.choice(64, nbits, replace=False))


def leaf_image(voc, seed, n, pool=None, random_every=0):
    rng = np.random.default_rng(seed)
    pool = voc.leaves() if pool is None else pool
    f = voc.desc[rng.choice(pool, n)].copy()
    if random_every:
        r = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        f[random_every - 1::random_every] = r[random_every - 1::random_every]
    return f


@functools.lru_cache(None)
def ragged_voc():
    """1 to 5 children mixed in one tree of depth 3 (declared k = 5)."""
    v = coded_voc(5, 3, lambda p: 0 if len(p) == 3 else 1 + (2 * sum(p) + 3 * len(p)) % 5 if p else 5, 11)
    ar = {len(v.children(i)) for i in range(v.n_nodes)}
    assert ar == {0, 1, 2, 3, 4, 5}
    return v


@functools.lru_cache(None)
def chunked_voc():
    """Declared k = 4 with a 9-child root whose children have 1 to 9 children: every chunk count of G = 4."""
    return coded_voc(4, 2, lambda p: 9 if not p else (p[0] + 1 if len(p) == 1 else 0), 12)


@functools.lru_cache(None)
def leaf_above_voc():
    """L = 4, k = 3, with a leaf at depth 1 (path 0) and one at depth 2 (path 1, 0)."""
    return coded_voc(3, 4, lambda p: 0 if p in ((0,), (1, 0)) or len(p) == 4 else 3, 13)


def _shape_cases():
    out = []
    b = Builder()
    rng = np.random.default_rng(21)
    p = 0
    for lv in range(4):
        p = b.add(p, rng.integers(0, 256, 32, dtype=np.uint8), leaf=1 if lv == 3 else 0, w=1.75 if lv == 3 else 0.0)

    def chain_check(c, tr):
        for f in tr["f"]:
            assert f["path"] == [1, 2, 3, 4] and f["nid"] == 2 and all(len(lv["children"]) == 1 for lv in f["levels"])
    out.append(Case("arity-1-chain", Voc(2, 4, L1_NORM, TF_IDF, b.arrays()), 2, randoms(21, 6), chain_check))

    rv = ragged_voc()

    def ragged_check(c, tr):
        seen = {len(lv["children"]) for f in tr["f"] for lv in f["levels"]}
        assert seen == {1, 2, 3, 4, 5}, seen
    out.append(Case("ragged-arity", rv, 1, leaf_image(rv, 22, 90, random_every=5), ragged_check))

    def root_check(c, tr):
        assert all(f["nid"] == 0 and not f["nid_unset"] for f in tr["f"])
    out.append(Case("levelsup-ge-L", rv, 3, leaf_image(rv, 23, 40, random_every=4), root_check))
    out.append(Case("levelsup-ge-L-plus-2", rv, 5, leaf_image(rv, 24, 40, random_every=4), root_check))

    def leaf_check(c, tr):
        assert all(f["nid"] == f["leaf"] and not f["nid_unset"] for f in tr["f"])
    out.append(Case("levelsup-0", rv, 0, leaf_image(rv, 25, 40, random_every=4), leaf_check))

    lv = leaf_above_voc()
    shallow = [i for i in lv.leaves() if len(lv.paths[i]) < 4]
    assert sorted(len(lv.paths[i]) for i in shallow) == [1, 2]
    img = np.concatenate([lv.desc[lv.leaves()], lv.desc[shallow], randoms(26, 6)])
    for ls in LEAF_ABOVE_LEVELSUP:
        def above_check(c, tr, ls=ls):
            nid_level = 4 - ls
            for f in tr["f"]:
                depth = len(f["path"])
                assert f["nid_unset"] == (nid_level > depth), (c.name, depth)
                assert f["nid"] == (0 if nid_level <= 0 or nid_level > depth else f["path"][nid_level - 1])
            depths = {len(f["path"]) for f in tr["f"] if f["kept"]}
            assert {1, 2, 4} <= depths
            unset = sum(f["nid_unset"] for f in tr["f"])
            assert (unset > 0) == (ls in (0, 1, 2)), (c.name, unset)
        out.append(Case(f"leaf-above-L-levelsup-{ls}", lv, ls, img, above_check))
    return out


@functools.lru_cache(None)
def unflagged_arrays():
    """Root with 3 children. Child 0 has the true word 0 (0.75), an unflagged childless node A (2.5) and word 1;
    child 1 is itself childless and unflagged (B, 1e-3); child 2 has words 2..4. -> (voc, A, B, word-0 leaf)."""
    v = coded_voc(3, 2, lambda p: 0 if p == (1,) or len(p) == 2 else 3, 14)
    par, leaf, desc, w = v.par, v.leaf.copy(), v.desc, v.w.copy()
    top = v.children(0)
    under0 = v.children(top[0])
    A, Bn, w0 = under0[1], top[1], under0[0]
    leaf[A] = leaf[Bn] = 0
    w[A], w[Bn], w[w0] = 2.5, 1e-3, 0.75
    return (par, leaf, desc, w), A, Bn, w0, v.children(top[2])[1]


def _unflagged_cases():
    arrays, A, Bn, w0, other = unflagged_arrays()
    out = []
    for weighting in (TF_IDF, IDF):
        voc = Voc(3, 2, L1_NORM, weighting, arrays)
        assert voc.word(w0) == 0 and voc.word(A) == 0 and voc.word(Bn) == 0
        img = voc.desc[[A, w0, Bn, other, A]]

        def check(c, tr, voc=voc):
            assert [f["leaf"] for f in tr["f"]] == [A, w0, Bn, other, A]
            assert tr["words"][0] == [2.5, 0.75, 1e-3, 2.5] and all(f["kept"] for f in tr["f"])
            assert not c.voc.leaf[A] and not c.voc.leaf[Bn] and tr["f"][2]["path"] == [Bn]
            (ids, wt), _, _ = run_definition(c)
            raw = (2.5 + 0.75 + 1e-3 + 2.5) if c.voc.weighting == TF_IDF else 2.5
            ow = float(c.voc.w[other])
            assert ids.tolist() == [0, c.voc.word(other)] and wt[0] == raw / (raw + ow)
        out.append(Case(f"unflagged-childless-node-{WNAME[weighting]}", voc, 1, img, check))
    voc = Voc(3, 2, L1_NORM, IDF, arrays)

    def first_check(c, tr):
        assert tr["words"][0] == [1e-3, 0.75, 2.5]
        (ids, wt), _, _ = run_definition(c)
        assert wt[0] == 1e-3 / (1e-3 + float(c.voc.w[other]))   # the first feature's weight, not word 0's own
    out.append(Case("idf-keeps-first", voc, 1, voc.desc[[Bn, w0, other, A]], first_check))
    return out


# ---- stop rules ----
STOP_W = [0.0, -1.5, -0.0, float("nan"), 5e-324, 2.0, 3.0, 0.7]


def _stop_cases():
    out = []
    base = coded_voc(8, 1, full(8, 1), 15, weight=lambda i, p: STOP_W[p[0]])
    lf = base.children(0)
    plans = {"weight-zero": [5, 0, 6, 0, 5], "weight-negative": [1, 5, 1], "weight-minus-zero": [2, 6, 2, 7],
             "weight-nan": [3, 5, 3, 3], "weight-denormal-min": [4, 5, 4], "all-stopped": [0, 1, 2, 3, 0, 1],
             "one-kept-of-many": [(0, 1, 2, 3)[i % 4] for i in range(17)] + [6] + [(3, 2, 1, 0)[i % 4] for i in range(22)]}
    for weighting in (TF_IDF, IDF):
        voc = base.variant(L1_NORM, weighting)
        for name, plan in plans.items():
            def check(c, tr, plan=plan, name=name):
                kept = [i for i, j in enumerate(plan) if j >= 4]
                assert [i for i, f in enumerate(tr["f"]) if f["kept"]] == kept
                assert [f["path"] for f in tr["f"]] == [[lf[j]] for j in plan]
                (ids, wt), (fid, foff, fidx), _ = run_definition(c)
                assert sorted(fidx.tolist()) == kept and int(foff[-1]) == len(kept)
                assert ids.tolist() == sorted({j for j in plan if j >= 4})
                if name == "all-stopped":
                    assert len(ids) == 0 and len(fid) == 0 and foff.tolist() == [0]
                if name == "weight-denormal-min":
                    assert 4 in tr["words"] and tr["words"][4][0] == 5e-324 > 0
                if name == "one-kept-of-many":
                    assert ids.tolist() == [6] and wt.tolist() == [1.0] and fidx.tolist() == [17]
            out.append(Case(f"{name}-{WNAME[weighting]}", voc, 0, base.desc[[lf[j] for j in plan]], check))
    return out


# ---- weighting x scoring ----
def _weighting_cases():
    out = []
    base = coded_voc(3, 2, full(3, 2), 16)
    lf = base.leaves()
    plan = [0, 4, 4, 7, 0, 4, 2]                         # 7 features, 4 words, repeats
    img = np.concatenate([base.desc[[lf[j] for j in plan]], randoms(16, 2)])
    ones = np.where(base.w > 0, 1.0, 0.0)
    for weighting in (TF_IDF, TF, IDF, BINARY):
        for scoring in (L1_NORM, L2_NORM, DOT_PRODUCT):
            voc = base.variant(scoring, weighting, ones if weighting in (TF, BINARY) else None)
            out.append(Case(f"weighting-{WNAME[weighting]}-{SNAME[scoring]}", voc, 1, img))

    def dot_check(c, tr):
        (ids, wt), _, _ = run_definition(c)
        counts = {w: len(a) for w, a in tr["words"].items()}
        assert len(tr["f"]) == 7 and len(ids) == 4 and [counts[int(i)] for i in ids] == [2, 1, 3, 1]
        assert wt.tolist() == [2 / 4, 1 / 4, 3 / 4, 1 / 4]          # /= v.size(), not /= n
    out.append(Case("dot-product-tf-divides-by-words", base.variant(DOT_PRODUCT, TF, ones), 1, img[:7], dot_check))

    def l2_check(c, tr):
        (ids, wt), _, _ = run_definition(c)
        sums = []
        for i in ids:
            s = 0.0
            for a in tr["words"][int(i)]:
                s += a
            sums.append(s)
        norm = 0.0
        for s in sums:
            norm += s * s
        norm = math.sqrt(norm)
        assert len(ids) == 4 and wt.tobytes() == np.array([s / norm for s in sums]).tobytes()
        assert float(np.abs(wt).sum()) != 1.0   # not the L1 norm
    out.append(Case("l2-norm-bytes", base.variant(L2_NORM, TF_IDF), 1, img[:7], l2_check))
    return out


# ---- ordered sums ----
def decades(seed, n):
    return 10.0 ** np.random.default_rng(seed).uniform(-8.0, 8.0, n)


@functools.lru_cache(None)
def shared_word_voc(scoring):
    """Root (declared k = 10) with 20 children: child 0 the true word 0 (1.0), children 1..17 childless and
    unflagged (they share word 0) with weights over 16 decades, children 18 and 19 words 1 and 2."""
    w = decades(31, 20)
    w[0] = 1.0
    return coded_voc(10, 1, full(20, 1), 17, scoring=scoring, weight=lambda i, p: float(w[p[0]]),
                     flag=lambda i, p: 0 if 1 <= p[0] <= 17 else 1)


def _order_cases():
    out = []
    voc = shared_word_voc(L1_NORM)
    kids = voc.children(0)

    def ws_check(c, tr):
        a = tr["words"][0]
        assert len(a) >= 50 and max(a) / min(a) > 1e14 and set(tr["words"]) == {0, 1, 2}
    out.append(Case("word-sum-order", voc, 0, leaf_image(voc, 32, 64), ws_check, sens=True))
    for nb in NORM_WORDS:
        # word 0: 1.0 (three features: 3.0); words 1..nb-2: distinct weights just under 2^-53, each less than
        # half an ulp of the chain's accumulator, so the reference's left-to-right chain absorbs every one and
        # any order that adds two of them to each other first keeps them; the last word (0.375) is added exactly
        w = np.array([1.0] + [2.0 ** -53 * (1.0 - j / 1024.0) for j in range(1, nb - 1)] + [0.375])
        v = coded_voc(10, 1, full(nb, 1), 100 + nb, weight=lambda i, p, w=w: float(w[p[0]]))
        rng = np.random.default_rng(nb)
        kids = v.children(0)
        img = v.desc[np.concatenate([rng.permutation(kids), [kids[0], kids[0]]])]

        def check(c, tr, nb=nb):
            assert len(tr["words"]) == nb == len(tr["norm"]) and tr["norm"][0] == 3.0
            assert run_definition(c)[0][1][0] == 3.0 / 3.375   # the chain's norm is 3.375 exactly
        out.append(Case(f"norm-order-{nb}", v, 0, img, check, sens=True))
    vd = shared_word_voc(DOT_PRODUCT)
    for n in (64, 1025):
        def check(c, tr, n=n):
            assert list(tr["words"]) == [0] and len(tr["words"][0]) == n and tr["norm"] is None
        out.append(Case(f"single-word-all-features-{n}", vd, 0, leaf_image(vd, 33 + n, n, pool=kids[:18]), check,
                        sens=True))
    return out


# ---- assemble thresholds ----
@functools.lru_cache(None)
def wide_voc():
    """Root (declared k = 10) with 48 leaves: words 0..39 kept, 40..47 stopped."""
    w = np.random.default_rng(51).uniform(0.1, 6.0, 48)
    w[40:] = 0.0
    return coded_voc(10, 1, full(48, 1), 18, weight=lambda i, p: float(w[p[0]]))


def kept_counts(m):
    """Features per word 0..39 summing to m. m >= 1023: word 0 takes the keys [0, 1020) and word 1 the next 11,
    so its run lies across the thread ranges around key 1024 (R = 1, 2, 3 keys per thread)."""
    c = np.zeros(40, int)
    if m < 1023:
        c[5] = m
        return c
    c[0], c[1] = 1020, min(11, m - 1020)
    rest = m - c[0] - c[1]
    rng = np.random.default_rng(m)
    for w in rng.integers(2, 40, rest):
        c[w] += 1
    return c


def _assemble_cases():
    out = []
    voc = wide_voc()
    kids = voc.children(0)
    for m in KEPT:
        c = kept_counts(m)
        plan = np.concatenate([np.repeat(np.arange(40), c), 40 + np.arange(37) % 8])
        plan = np.random.default_rng(60 + m).permutation(plan)

        def check(cs, tr, m=m, c=c):
            kept = [f["word"] for f in tr["f"] if f["kept"]]
            assert len(kept) == m and len(tr["f"]) == m + 37
            keys = sorted(kept)
            if m == 2049:   # word 1's run is the sorted keys 1020..1030
                assert keys[1019] == 0 and keys[1020:1031] == [1] * 11 and keys[1031] > 1
            assert [len(tr["words"].get(w, [])) for w in range(40)] == c.tolist()
        out.append(Case(f"kept-{m}", voc, 0, voc.desc[[kids[j] for j in plan]], check))

    def all_kept(c, tr):
        assert all(f["kept"] for f in tr["f"]) and len(tr["f"]) == 300
    out.append(Case("kept-equals-n", voc, 0, leaf_image(voc, 61, 300, pool=kids[:40]), all_kept))
    big = coded_voc(33, 2, lambda p: 33 if not p else (32 if len(p) == 1 else 0), 19)
    lf = big.leaves()
    assert len(lf) == 1056
    pick = np.random.default_rng(62).permutation(lf)[:1025]

    def own_word(c, tr):
        assert len(tr["words"]) == 1025 and all(len(a) == 1 for a in tr["words"].values())
    out.append(Case("every-feature-own-word", big, 1, big.desc[pick], own_word))
    return out


# ---- sizes: a partly filled descent block for every group width ----
@functools.lru_cache(None)
def group_voc(G):
    k, L = {4: (2, 4), 8: (8, 2), 16: (10, 2), 32: (20, 2), 64: (33, 2)}[G]
    return coded_voc(k, L, full(k, L), 70 + G)


def _size_cases():
    out = []
    for G, _ in GROUPS:
        voc = group_voc(G)
        for n in SIZES:
            rng = np.random.default_rng(1000 * G + n)
            img = leaf_image(voc, 80 + G + n, n, random_every=3)
            if n > 1:
                img[0] = near(rng, img[0])

            def check(c, tr, n=n):
                assert len(tr["f"]) == n
            out.append(Case(f"n-{n}-G{G}", voc, 1, img, check))
    return out


# ---- the loader ----
def _loader_cases():
    out = []
    rv = ragged_voc()
    blob = save_bin(*rv.args())
    v = Voc.from_blob(blob)
    expected = (5 ** 4 - 1) // 4

    def ragged_check(c, tr, expected=expected):
        assert c.voc.n_nodes < expected and c.voc.n_nodes == ragged_voc().n_nodes
    out.append(Case("bin-ragged", v, 1, leaf_image(rv, 91, 60, random_every=5), ragged_check))

    small = coded_voc(2, 2, full(2, 2), 92)
    assert small.n_nodes == 7
    F = base_desc(92)
    tail = struct.pack("<iB", 0, 1) + bytes(F) + struct.pack("<d", 9.0)   # a third child of the root, equal to F
    v = Voc.from_blob(save_bin(*small.args()) + tail + tail)
    img = np.concatenate([F[None], small.desc[small.leaves()], F[None]])

    def tail_check(c, tr):
        assert c.voc.n_nodes == 7 and len(c.voc.blob) == 16 + 45 * 8
        assert all(len(f["levels"][0]["children"]) == 2 and min(f["levels"][0]["dist"]) > 0 for f in tr["f"][:1])
    out.append(Case("bin-trailing-bytes", v, 1, img, tail_check))

    k20 = coded_voc(20, 2, full(20, 2), 93)
    v = Voc.from_blob(save_bin(*k20.args()))

    def k20_check(c, tr):
        assert c.voc.n_nodes == 421 and c.voc.k == 20
    out.append(Case("bin-k-20", v, 1, leaf_image(k20, 94, 50, random_every=4), k20_check))
    return out


@functools.lru_cache(None)
def all_cases():
    cases = (_tie_cases() + _distance_cases() + _chunk_cases() + _shape_cases() + _unflagged_cases() + _stop_cases() +
             _weighting_cases() + _order_cases() + _assemble_cases() + _size_cases() + _loader_cases())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def chain_vocs():
    """The vocabularies of the transform_batch -> KeyFrameDatabase chain: one ragged, one chunked."""
    return {"ragged": ragged_voc(), "chunked": chunked_voc()}
