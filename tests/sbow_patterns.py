"""Planted SearchByBoW scenes: every acceptance rule of SearchByBoW(KF, F) (single- and two-camera F) and
SearchByBoW(KF1, KF2) at the value where it decides. Each case names its rule and carries a
`check(case, trace, slots, n)` that proves from the trace of oracle/sbow_definition.py that this rule
decided; float-sensitive cases are marked `sens`: the definition's double evaluation must give other slots.

Descriptors are planted (sbp_patterns.base_desc / flip): a keyframe feature is a base descriptor, its
candidates are that descriptor with chosen bits flipped, the flipped bits dealt round-robin over the eight
32-bit words, so every Hamming distance is chosen and every word carries part of it. A case is a handful of
nodes of a few features; sub-scenes that must not interact sit in nodes of their own.

kind "kff": side a = the keyframe, side b = the frame F (b.nleft: F.Nleft); slots are F's, values a.mp.
kind "kfkf": side a = KF1, side b = KF2 (a.nleft / b.nleft: NLeft); slots are KF1's, values b.mp.

pad_frame / pad_keyframe append inert features to side b / side a (features in no node, and features with
map point -1 in nodes the other side does not have) until the one-workgroup forms no longer fit; the sizes
come from the drivers' own bounds, restated in block_lds / batch_lds / kf_batch_lds.
"""
import numpy as np

from oracle import sbow_definition as bd
from oracle import sbp_definition as sd
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import FeatureVector, MatchFrame
from sbp_patterns import BOUNDS, PLANS, SF, _plan_bins, base_desc, flip

f32 = np.float32
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)
EQ_PAIR = {0.6: (6, 10), 0.7: (21, 30), 0.75: (30, 40), 0.8: (40, 50), 0.9: (36, 40)}   # (float)d1 == r * (float)d2
FLOAT_PAIRS = ((30, 50), (15, 25), (27, 45))   # at 0.6: accepted in float, rejected with 0.6 as a double
# node ids near the top of a k = 10, L = 6 vocabulary's range ((10^7 - 1) / 9 nodes), never contiguous;
# the pad nodes of either side lie between them and are shared with nobody
NODE0, STEP, PAD_F, PAD_KF, NODE_END = 1_000_003, 97, 31, 53, 1_111_111
ORDER = [w * 32 + j for j in range(32) for w in range(8)]   # bit k of a planted set lies in word k % 8


def node_id(j):
    assert NODE0 + STEP * j < NODE_END
    return NODE0 + STEP * j


class Bits:
    """Fresh bit positions of one base descriptor, dealt over the eight words."""

    def __init__(self, start=0):
        self.k = start

    def take(self, n):
        assert self.k + n <= 256
        out = ORDER[self.k:self.k + n]
        self.k += n
        return out


def at(b, d, start=0):
    """b with d bits flipped, spread over the eight words: Hamming distance d from b."""
    return flip(b, ORDER[start:start + d])


class Side:
    """A keyframe or frame under construction. nleft fixed in advance: left features take indices from 0,
    right features from nleft; unused left indices are filled with features in no node."""

    def __init__(self, mp0, nleft=None):
        self.mp0, self.nleft = mp0, nleft
        self.feats = {}          # index -> (desc, angle, mp)
        self.nodes = {}          # node id -> [index, ...] in walk order
        self.nl = 0
        self.nr = nleft if nleft is not None else 0

    def feat(self, desc, node=None, angle=0.0, mp=None, right=False):
        if right:
            i = self.nr
            self.nr += 1
        else:
            i = self.nl
            self.nl += 1
            assert self.nleft is None or i < self.nleft
        self.feats[i] = (desc, f32(angle), self.mp0 + i if mp is None else mp)
        if node is not None:
            self.nodes.setdefault(node, []).append(i)
        return i

    def build(self):
        n = max(self.nl, self.nr) if self.nleft is None else max(self.nr, self.nleft)
        rng = np.random.default_rng(self.mp0)
        keys = np.zeros(n, KEYPOINT_DTYPE)
        keys["x"], keys["y"] = rng.uniform(20, 700, n), rng.uniform(20, 440, n)
        keys["size"], keys["response"], keys["class_id"] = 31.0, 20.0, -1
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.mp = np.full(n, -1, np.int32)
        for i, (d, a, m) in self.feats.items():
            self.desc[i], keys["angle"][i], self.mp[i] = d, a, m
        self.keys = keys
        self.fv = FeatureVector(self.nodes)
        return self

    @property
    def N(self):
        return len(self.keys)


class Case:
    def __init__(self, name, rule, kind, a, b, nnratio, check_ori, check, sens=False):
        self.name, self.rule, self.kind, self.a, self.b = name, rule, kind, a.build(), b.build()
        self.nnratio, self.check_ori, self.check, self.sens = nnratio, check_ori, check, sens
        self.frame()

    def frame(self):
        """Side b as the MatchFrame of the KF-F form."""
        b = self.b
        self.F = MatchFrame(b.keys, b.desc, BOUNDS, SF, nleft=b.nleft) if self.kind == "kff" else None

    def __repr__(self):
        return self.name

    def matched(self, slots, ia, ib):
        return slots[ib] == self.a.mp[ia] if self.kind == "kff" else slots[ia] == self.b.mp[ib]

    def free(self, slots, ia, ib):
        return slots[ib] == -1 if self.kind == "kff" else slots[ia] == -1


WIDE = 18


class Scene:
    def __init__(self, kind, nnratio=0.75, check_ori=True, nleft=None, nleft_a=None):
        self.kind, self.nnratio, self.check_ori = kind, nnratio, check_ori
        self.a, self.b = Side(1000, nleft_a), Side(2000 if kind == "kfkf" else 0, nleft)
        self.j = 0

    def node(self):
        self.j += 1
        return node_id(3 * self.j)

    def duel(self, seed, dists, right=(), angle_a=0.0, angle_b=0.0, wide=False):
        """A node of its own: one keyframe feature and candidates at the given distances, in that order.
        wide: WIDE far candidates more (distance 150 and up, left ones), so that the node takes the kernels'
        path for nodes of more than 16 candidates; the planted ones sit at its end."""
        nd, b = self.node(), base_desc(seed)
        ia = self.a.feat(b, nd, angle_a)
        if wide:
            for k in range(WIDE):
                self.b.feat(at(b, 150 + k), nd, angle_b)
        ibs = [self.b.feat(at(b, d), nd, angle_b, right=k in right) for k, d in enumerate(dists)]
        return ia, ibs

    def case(self, name, rule, check, sens=False):
        pre = "kk-" if self.kind == "kfkf" else ""
        return Case(pre + name, rule, self.kind, self.a, self.b, self.nnratio, self.check_ori, check, sens)


def th_low(kind):
    """The largest accepted best distance: bestDist1 <= TH_LOW (KF, F), bestDist1 < TH_LOW (KF, KF)."""
    return bd.TH_LOW if kind == "kff" else bd.TH_LOW - 1


# ---------------------------------------------------------------- distance, ratio
def distance_edge(kind, d, wide=False):
    s = Scene(kind, nnratio=0.9)
    ia, (ib, _) = s.duel(1, [d, 120], wide=wide)
    ok = d <= th_low(kind)

    def check(case, tr, slots, n):
        t = tr["kf"][ia]
        assert (t["bd1"], t["bd2"], t["best"]) == (d, 120, ib) and bd.ratio_passes(d, 120, 0.9)
        assert t["rule"] == ("accepted" if ok else "distance")
        assert case.matched(slots, ia, ib) if ok else case.free(slots, ia, ib)
        assert n == int(ok)
    return s.case(f"distance-{d}" + "-wide" * wide, f"bestDist1 {'<=' if kind == 'kff' else '<'} TH_LOW", check)


def ratio_cases(kind, r, wide=False):
    """(float)d1 == r * (float)d2 exactly: the strict < rejects; one step below is accepted, one above rejected."""
    s = Scene(kind, nnratio=r)
    d1, d2 = EQ_PAIR[r]
    assert f32(d1) == f32(f32(r) * f32(d2)) and d1 + 1 <= th_low(kind)
    exp = []
    for k, d in enumerate((d1, d1 - 1, d1 + 1)):
        ia, (ib, _) = s.duel(10 + k, [d, d2], wide=wide)
        exp.append((ia, ib, d, d == d1 - 1))

    def check(case, tr, slots, n):
        for ia, ib, d, ok in exp:
            t = tr["kf"][ia]
            assert (t["bd1"], t["bd2"], t["best"]) == (d, d2, ib)
            assert t["rule"] == ("accepted" if ok else "ratio")
            assert case.matched(slots, ia, ib) if ok else case.free(slots, ia, ib)
        assert n == 1
    return s.case(f"ratio-{r}" + "-wide" * wide, "(float)bestDist1 < mfNNratio * (float)bestDist2, strict", check)


def ratio_float(kind, wide=False):
    s = Scene(kind, nnratio=0.6)
    exp = [s.duel(20 + k, [d1, d2], wide=wide) + (d1, d2) for k, (d1, d2) in enumerate(FLOAT_PAIRS)]

    def check(case, tr, slots, n):
        for ia, (ib, _), d1, d2 in exp:
            t = tr["kf"][ia]
            assert (t["bd1"], t["bd2"], t["rule"]) == (d1, d2, "accepted") and case.matched(slots, ia, ib)
            assert not bd.ratio_passes(d1, d2, 0.6, double=True)
        assert n == len(exp)
    return s.case("ratio-0.6-float" + "-wide" * wide, "the product mfNNratio * (float)bestDist2 in float", check, sens=True)


def lone_candidate(kind, r):
    s = Scene(kind, nnratio=r)
    d = th_low(kind)
    ia, (ib,) = s.duel(30, [d])

    def check(case, tr, slots, n):
        t = tr["kf"][ia]
        assert (t["bd1"], t["bd2"], t["rule"]) == (d, 256, "accepted") and case.matched(slots, ia, ib) and n == 1
    return s.case(f"lone-candidate-{r}", "bestDist2 stays 256 with one free candidate", check)


def best_tie_rejected(kind):
    """Two candidates at the best distance: bestDist2 == bestDist1, the ratio test rejects, both stay free and
    the node's next keyframe feature takes one of them."""
    s = Scene(kind)
    nd, b, bits = s.node(), base_desc(40), Bits()
    S0, S1, X = bits.take(20), bits.take(20), bits.take(10)
    k0 = s.a.feat(b, nd)
    k1 = s.a.feat(flip(b, S1 + X), nd)
    f0, f1 = s.b.feat(flip(b, S0), nd), s.b.feat(flip(b, S1), nd)

    def check(case, tr, slots, n):
        t0, t1 = tr["kf"][k0], tr["kf"][k1]
        assert (t0["bd1"], t0["bd2"], t0["best"], t0["rule"]) == (20, 20, f0, "ratio")
        assert (t1["bd1"], t1["bd2"], t1["best"], t1["rule"]) == (10, 50, f1, "accepted")
        if kind == "kff":
            assert slots[f0] == -1 and slots[f1] == case.a.mp[k1]
        else:
            assert slots[k0] == -1 and slots[k1] == case.b.mp[f1]
        assert n == 1
    return s.case("best-tie-rejected", "a tie at the best fails the ratio test for any mfNNratio < 1", check)


# ---------------------------------------------------------------- the "already matched" chain
def ladder(kind, m):
    """Four keyframe features contend for four candidates f0..f3 of one node of m candidates (the others
    are far). Distances (T = 12 private bits per candidate, D = 12 + s - 2u):
        k0: f0 10, others 34             takes f0
        k1: f1 12, f0 14, others 36      12 vs 14 fails the ratio; f0 is gone, 12 vs 36 passes: takes f1
        k2: f1 8, f2 16, others 32       its best f1 is taken: accepts its former second best f2
        k3: f3 20, f2 22, far ones 133+  20 vs 22 fails; f2 is gone, 20 vs 133 passes: takes f3
    """
    s = Scene(kind)
    nd, b, bits = s.node(), base_desc(50), Bits()
    T = [bits.take(12) for _ in range(4)]
    G = bits.take(100)
    g = bits.take(6)
    plan = [({0: 12}, 10), ({1: 12, 0: 11}, 1), ({1: 12, 2: 8}, 0), ({3: 12, 2: 11}, 9)]
    K = []
    for u, x in plan:
        own = [p for i, c in u.items() for p in T[i][:c]] + bits.take(x)
        K.append(s.a.feat(flip(b, own), nd))
    pos = {0: 0, m // 2: 1, m - 2: 2, m - 1: 3}   # the rungs' positions in the node: first, middle, last two
    assert len(pos) == 4
    f = [None] * 4
    for p in range(m):
        if p in pos:
            f[pos[p]] = s.b.feat(flip(b, T[pos[p]]), nd)
        else:
            s.b.feat(flip(b, G + [g[k] for k in range(6) if (p >> k) & 1]), nd)
    want = [(10, 34, 0), (12, 36, 1), (16, 32, 2), (20, 133, 3)]

    def check(case, tr, slots, n):
        ham = lambda k, i: bd._ham(case.a.desc[K[k]], case.b.desc[f[i]])   # noqa: E731
        assert len(case.b.nodes[nd]) == m
        for k, (d1, d2, i) in enumerate(want):
            t = tr["kf"][K[k]]
            assert (t["bd1"], t["bd2"], t["best"], t["rule"]) == (d1, d2, f[i], "accepted"), (k, t)
            assert case.matched(slots, K[k], f[i])
        # k1 and k3 pass only because their rival was removed; k2's best was taken
        assert ham(1, 0) == 14 and not bd.ratio_passes(12, 14, case.nnratio) and case.matched(slots, K[0], f[0])
        assert ham(3, 2) == 22 and not bd.ratio_passes(20, 22, case.nnratio)
        assert ham(2, 1) == 8 < tr["kf"][K[2]]["bd1"]
        assert n == 4
    return s.case(f"ladder-{m}", "a taken candidate is skipped: bestDist2 and the best change", check)


def node_size(kind, m):
    """A node of m candidates, the winner in the last position, the runner-up in the first, the indices
    descending along the node."""
    s = Scene(kind)
    nd, b = s.node(), base_desc(60 + m)
    ia = s.a.feat(b, nd)
    dist = [30] + [60 + p for p in range(1, m - 1)] + [10] if m > 1 else [10]
    idx = [s.b.feat(at(b, d)) for d in reversed(dist)][::-1]   # position p holds index idx[p]
    s.b.nodes[nd] = idx

    def check(case, tr, slots, n):
        k = list(case.b.fv.node_ids).index(nd)
        assert idx == sorted(idx, reverse=True) and list(case.b.fv.indices[case.b.fv.offsets[k]:case.b.fv.offsets[k + 1]]) == idx
        t = tr["kf"][ia]
        assert (t["bd1"], t["bd2"], t["best"], t["rule"]) == (10, 30 if m > 1 else 256, idx[-1], "accepted")
        assert case.matched(slots, ia, idx[-1]) and n == 1
    return s.case(f"node-size-{m}", "every position of a node is scored, partly filled quads included", check)


def mp_skip(kind, side):
    """side a: a keyframe feature without a map point would have taken the candidate, the next one takes it.
    side b (KF-KF): a KF2 feature without a map point at distance 0 is no candidate."""
    s = Scene(kind)
    nd, b = s.node(), base_desc(70)
    if side == "a":
        k0 = s.a.feat(at(b, 5), nd, mp=-1)
        k1 = s.a.feat(at(b, 10), nd)
        f0, f1 = s.b.feat(b, nd), s.b.feat(at(b, 50), nd)
    else:
        k0 = k1 = s.a.feat(b, nd)
        s.b.feat(b, nd, mp=-1)
        f0, f1 = s.b.feat(at(b, 10), nd), s.b.feat(at(b, 50), nd)

    def check(case, tr, slots, n):
        if side == "a":
            assert tr["kf"][k0]["skip"] == "mp" and tr["kf"][k0]["best"] == -1
        t = tr["kf"][k1]
        assert (t["bd1"], t["best"], t["rule"]) == (10, f0, "accepted") and case.matched(slots, k1, f0) and n == 1
    return s.case("mp-skip" if side == "a" else "mp2-skip", "a NULL / bad map point is skipped", check)


def empty_node(kind):
    s = Scene(kind)
    e1, e2 = s.node(), s.node()
    s.a.nodes[e1], s.b.nodes[e1] = [], []
    s.a.feat(base_desc(80), e1)            # shared node, the other side's list empty
    s.a.nodes[e2], s.b.nodes[e2] = [], []
    s.b.feat(base_desc(80), e2)            # shared node, the keyframe's list empty
    ia, (ib, _) = s.duel(81, [10, 40])     # the last node of both lists

    def check(case, tr, slots, n):
        assert tr["nodes"] == [e1, e2, tr["kf"][ia]["node"]]
        last = [int(fv.node_ids[-1]) == tr["nodes"][-1] for fv in (case.a.fv, case.b.fv)]
        assert all(last) if "+" not in case.name else any(last)   # padding adds nodes to one side
        assert tr["kf"][0]["rule"] == "none" and tr["kf"][ia]["rule"] == "accepted"
        assert case.matched(slots, ia, ib) and n == 1
    return s.case("empty-node", "empty lists in shared nodes; the last node of both lists", check)


def join(kind):
    """260 shared one-pair nodes; unpaired nodes at the front, in the middle and at the end of either side,
    each holding an exact copy of a feature the other side has in a shared node."""
    s = Scene(kind)
    lone = {0: "a", 1: "b", 2: "a", 100: "b", 101: "b", 102: "a", 200: "a", 201: "a", 202: "b", 297: "b", 298: "a",
            299: "a"}
    exp, intr, shared = [], [], []

    def near(j):   # the nearest shared node: the next one, at the end the one before
        k = j
        while k in lone:
            k += 1
        return k if k < 300 else max(i for i in range(300) if i not in lone)
    for j in range(300):
        nd, b = node_id(3 * j + (j % 3)), base_desc(1000 + j)
        if j in lone:
            side = s.a if lone[j] == "a" else s.b
            intr.append((lone[j], side.feat(base_desc(1000 + near(j)), nd)))
            continue
        shared.append(nd)
        d = j % 40 + 1
        exp.append((s.a.feat(b, nd), s.b.feat(at(b, d, start=j % 200), nd), d))
    assert len(shared) > 256 and shared[-1] > NODE_END - 25000

    def check(case, tr, slots, n):
        assert tr["nodes"] == shared
        for ia, ib, d in exp:
            assert tr["kf"][ia]["bd1"] == d and tr["kf"][ia]["bd2"] == 256 and case.matched(slots, ia, ib)
        for side, i in intr:
            if side == "a":
                assert i not in tr["kf"] and (kind == "kff" or slots[i] == -1)
            elif kind == "kff":
                assert slots[i] == -1
        assert n == len(exp) == len(shared)
    return s.case("join", "the lower_bound walk pairs exactly the node ids present on both sides", check)


def unlisted(kind):
    s = Scene(kind)
    b = base_desc(90)
    ia, (ib, _) = s.duel(90, [10, 40])
    ua = s.a.feat(at(b, 10))   # a copy of the accepted candidate, in no node
    ub = s.b.feat(b)           # a copy of the keyframe feature, in no node

    def check(case, tr, slots, n):
        assert ua not in tr["kf"] and tr["kf"][ia]["best"] == ib and case.matched(slots, ia, ib) and n == 1
        assert slots[ub if kind == "kff" else ua] == -1
    return s.case("unlisted", "a feature in no node takes part in nothing", check)


# ---------------------------------------------------------------- rotation
def rotation(kind, pname, check_ori):
    s = Scene(kind, check_ori=check_ori)
    plan = PLANS[pname]
    exp = []
    for j, (aq, ak, bn) in enumerate(plan):
        ia, (ib,) = s.duel(200 + j, [3], angle_a=aq, angle_b=ak)
        exp.append((ia, ib, bn))
    if not plan:   # zero non-empty bins: candidates that miss the distance rule
        for j in range(3):
            s.duel(200 + j, [120], angle_a=90.0)
    bins = _plan_bins(plan)
    keep = sd.py_three_maxima(bins)

    def check(case, tr, slots, n):
        assert (tr["bins"], tr["kept_bins"]) == ((bins, keep) if check_ori else (None, None))
        for ia, ib, bn in exp:
            kept = (not check_ori) or bn in keep
            assert tr["kf"][ia]["rule"] == ("accepted" if kept else "dropped bin")
            assert tr["kf"][ia]["bin"] == (bn if check_ori else None)
            assert case.matched(slots, ia, ib) if kept else case.free(slots, ia, ib)
        assert n == (sum(bins[b] for b in keep if b >= 0) if check_ori else len(plan))
    sens = check_ori and (pname.startswith("tenth") or pname == "half-way")
    return s.case(f"rot-{pname}-ori{int(check_ori)}", "rot * (1.0f / 30) in float, max < 0.1f * (float)max1", check, sens)


# ---------------------------------------------------------------- two-camera F
NL = 40


def right_inside_left(wide=False):
    """The right best at exactly 50 is written, at 51 it is not (the left one is written both times)."""
    s = Scene("kff", nleft=NL)
    ia, (l0, _, r0, _) = s.duel(100, [10, 40, 50, 60], right=(2, 3), wide=wide)
    ib, (l1, _, r1, _) = s.duel(99, [10, 40, 51, 60], right=(2, 3), wide=wide)

    def check(case, tr, slots, n):
        t = tr["kf"][ia]
        assert (t["bd1"], t["bd1R"], t["rule"], t["ruleR"]) == (10, 50, "accepted", "accepted")
        assert slots[l0] == slots[r0] == case.a.mp[ia] and r0 >= NL > l0
        t = tr["kf"][ib]
        assert (t["bd1"], t["bd1R"], t["rule"], t["ruleR"]) == (10, 51, "accepted", "distance")
        assert slots[l1] == case.a.mp[ib] and slots[r1] == -1 and n == 3
    return s.case("right-inside-left" + "-wide" * wide, "bestDist1R <= TH_LOW inside bestDist1 <= TH_LOW", check)


def right_needs_left():
    s = Scene("kff", nleft=NL)
    ia, (l0, r0) = s.duel(101, [51, 0], right=(1,))     # the left's best is 51
    ib, (r1,) = s.duel(102, [0], right=(0,))            # no left candidate at all
    nd, b = s.node(), base_desc(103)                    # the only left candidate is taken by the feature before
    k0, k1 = s.a.feat(b, nd), s.a.feat(at(b, 20), nd)
    l2, r2 = s.b.feat(at(b, 2), nd), s.b.feat(at(b, 60), nd, right=True)

    def check(case, tr, slots, n):
        for i, r in ((ia, r0), (ib, r1)):
            assert tr["kf"][i]["bd1R"] == 0 and tr["kf"][i]["ruleR"] == "left distance" and slots[r] == -1
        assert tr["kf"][ia]["bd1"] == 51 and tr["kf"][ib]["bd1"] == 256 and slots[l0] == -1
        assert slots[l2] == case.a.mp[k0] and tr["kf"][k0]["ruleR"] == "distance"
        t = tr["kf"][k1]
        assert (t["bd1"], t["bd1R"], t["ruleR"]) == (256, 40, "left distance") and slots[r2] == -1 and n == 1
    return s.case("right-needs-left", "the right side is looked at only inside bestDist1 <= TH_LOW", check)


def right_ignores_ratio():
    s = Scene("kff", nleft=NL)
    ia, (l0, l1, r0, r1) = s.duel(104, [20, 21, 30, 31], right=(2, 3))

    def check(case, tr, slots, n):
        t = tr["kf"][ia]
        assert (t["bd1"], t["bd2"], t["rule"]) == (20, 21, "ratio") and slots[l0] == slots[l1] == -1
        assert (t["bd1R"], t["bd2R"], t["ruleR"]) == (30, 31, "accepted") and not bd.ratio_passes(30, 31, case.nnratio)
        assert slots[r0] == case.a.mp[ia] and slots[r1] == -1 and n == 1
    return s.case("right-ignores-ratio", "the right ratio test is disabled (|| true)", check)


def right_tie():
    """Two right candidates at the best right distance: the earlier position wins, which holds the larger
    index. Nodes of 5 and of 20 candidates, the left one first, the right ones' indices descending."""
    s = Scene("kff", nleft=NL)
    exp = []
    for m, p1, p2 in ((5, 2, 3), (20, 6, 17)):   # the tie's positions: lanes 2 and 3; lane 2 before lane 1
        nd, b = s.node(), base_desc(105 + m)
        ia = s.a.feat(b, nd)
        left = s.b.feat(at(b, 10), nd)
        desc = {p: flip(b, ORDER[8 * p:8 * p + 15]) if p in (p1, p2) else at(b, 70 + p, start=100) for p in range(1, m)}
        rs = [s.b.feat(desc[p], right=True) for p in reversed(range(1, m))][::-1]   # rs[p - 1]: position p
        s.b.nodes[nd] += rs
        exp.append((ia, left, rs[p1 - 1], rs[p2 - 1]))

    def check(case, tr, slots, n):
        for ia, left, first, second in exp:
            t = tr["kf"][ia]
            assert first > second and (t["bd1R"], t["bd2R"], t["bestR"], t["ruleR"]) == (15, 15, first, "accepted")
            assert bd._ham(case.a.desc[ia], case.b.desc[second]) == 15
            assert slots[first] == slots[left] == case.a.mp[ia] and slots[second] == -1
        assert n == 4
    return s.case("right-tie", "strict <: the first of equal right candidates in node order wins", check)


def nleft_edge(mode):
    """mid: the candidates at indices nleft - 1 and nleft are a left and a right one (read as two left ones
    the ratio test fails: 10 vs 12). 0: every candidate is a right one, nothing is written. n: every one left."""
    if mode == "mid":
        s = Scene("kff", nleft=1)
        ia, (l0, r0) = s.duel(110, [10, 12], right=(1,))
    else:
        s = Scene("kff", nleft=0 if mode == "0" else 2)
        ia, (l0, r0) = s.duel(110, [10, 12], right=(0, 1) if mode == "0" else ())

    def check(case, tr, slots, n):
        t = tr["kf"][ia]
        assert case.b.nleft == {"mid": 1, "0": 0, "n": 2}[mode] and (l0, r0) == (0, 1) and case.F.nleft == case.b.nleft
        if mode == "mid":
            assert (t["bd1"], t["bd2"], t["bd1R"], t["rule"], t["ruleR"]) == (10, 256, 12, "accepted", "accepted")
            assert not bd.ratio_passes(10, 12, case.nnratio) and slots[0] == slots[1] == case.a.mp[ia] and n == 2
        elif mode == "0":
            assert (t["bd1"], t["bd1R"], t["bd2R"], t["ruleR"]) == (256, 10, 12, "left distance") and n == 0
            assert slots[0] == slots[1] == -1
        else:
            assert (t["bd1"], t["bd2"], t["bd1R"], t["rule"]) == (10, 12, 256, "ratio") and n == 0
    return s.case("nleft-edge" + {"mid": "", "0": "-0", "n": "-n"}[mode], "realIdxF < F.Nleft is the left side", check)


def rot_two_entries():
    """Keyframe features that match a left and a right feature enter the histogram twice. Bins by entries:
    2: 5, 11: 4, 5: 3, 9: 3 -> kept {2, 11, 5}; counted once per keyframe feature: 2: 3, 11: 3, 5: 3, 9: 3 ->
    kept {2, 5, 9}."""
    s = Scene("kff", nleft=NL)
    exp = []
    for j, (bl, br) in enumerate([(2, 2), (2, 2), (2, 11), (11, None), (11, None), (11, None), (5, None), (5, None),
                                  (5, None), (9, None), (9, None), (9, None)]):
        nd, b = s.node(), base_desc(120 + j)
        ia = s.a.feat(b, nd, angle=f32(30.0 * bl))
        il = s.b.feat(at(b, 3), nd, angle=0.0)
        ir = None
        if br is not None:   # rot = 30 bl - a == 30 br
            ir = s.b.feat(at(b, 5), nd, angle=f32(30.0 * (bl - br) % 360.0), right=True)
        exp.append((ia, il, ir, bl, br))
    keep = {2, 11, 5}

    def check(case, tr, slots, n):
        assert tr["kept_bins"] == keep and [tr["bins"][b] for b in (2, 11, 5, 9)] == [5, 4, 3, 3]
        assert any(tr["kf"][ia]["bin"] != tr["kf"][ia]["binR"] is not None for ia, *_ in exp)
        for ia, il, ir, bl, br in exp:
            t = tr["kf"][ia]
            assert (t["bin"], t["binR"]) == (bl, br)
            assert slots[il] == (case.a.mp[ia] if bl in keep else -1)
            assert ir is None or slots[ir] == (case.a.mp[ia] if br in keep else -1)
        assert n == 12
    return s.case("rot-two-entries", "a left and a right match of one keyframe feature are two histogram entries", check)


# ---------------------------------------------------------------- two-camera keyframes (KF, KF)
def right_skipped(which):
    """1: the KF1 feature at index NLeft is skipped (it would have taken the candidate), the one at NLeft - 1
    takes it. 2: the KF2 feature at index NLeft (distance 0) is no candidate, the one at NLeft - 1 is."""
    s = Scene("kfkf", nleft_a=2 if which == 1 else None, nleft=2 if which == 2 else None)
    nd, b = s.node(), base_desc(130)
    if which == 1:
        s.a.feat(base_desc(131))
        k1 = s.a.feat(at(b, 10), nd)
        k0 = s.a.feat(b, right=True)
        s.a.nodes[nd].insert(0, k0)
        f0, f1 = s.b.feat(b, nd), s.b.feat(at(b, 60), nd)
    else:
        k0 = k1 = s.a.feat(b, nd)
        s.b.feat(base_desc(131))
        f0 = s.b.feat(at(b, 10), nd)
        fr = s.b.feat(b, right=True)
        s.b.nodes[nd].insert(0, fr)
        f1 = s.b.feat(at(b, 60), nd, right=True)

    def check(case, tr, slots, n):
        if which == 1:
            assert (k1, k0, case.a.nleft) == (1, 2, 2) and tr["kf"][k0]["skip"] == "right" and slots[k0] == -1
        else:
            assert (f0, fr, case.b.nleft) == (1, 2, 2) and tr["kf"][k1]["bd2"] == 256
        t = tr["kf"][k1]
        assert (t["bd1"], t["best"], t["rule"]) == (10, f0, "accepted") and slots[k1] == case.b.mp[f0] and n == 1
    return s.case(f"right-skipped-{which}", "indices from NLeft on are skipped in a two-camera keyframe", check)


# ---------------------------------------------------------------- padding
LDS_MAX = 150 * 1024   # orbfe_search_by_bow: blds <= 150 * 1024; orbfe_search_by_bow_batch: lds_max
F_MAX = 4096           # MT_BOW_FR * MT_BOW_NT
KP = KEYPOINT_DTYPE.itemsize


def _a(b, to):
    return (b + to - 1) // to * to


def dims(side, add=0):
    """(features, nodes, listed indices) of a side, or of what _padded makes of it."""
    listed = add // 2
    return side.N + add, len(side.fv.node_ids) + (listed + 3) // 4, int(side.fv.offsets[-1]) + listed


def block_lds(da, db, npairs):
    """orbfe_search_by_bow's blds: the uploads from the node pairs to F's descriptors (each at a multiple of
    256), then 4 bytes per F feature and 16."""
    (an, ann, ai), (bn, bnn, bi) = da, db
    ups = [npairs * 8, (ann + 1) * 4, ai * 4, (bnn + 1) * 4, bi * 4, an * 4, an * 32, an * KP]
    return _a(sum(_a(u, 256) for u in ups) + bn * 32, 16) + bn * 4 + 16


def _pack(d):
    """Bytes of orbfe_keyframe_create's pack: node ids, CSR offsets, CSR indices, angles, descriptors."""
    n, nn, ni = d
    return _a(nn * 4, 16) + _a((nn + 1) * 4, 16) + _a(ni * 4, 16) + _a(n * 4, 16) + n * 32


def batch_lds(da, db):
    """bow_batch_lds + 16 of candidate a against frame b (orbfe_keyframe_create's pack layout)."""
    (an, ann, ai), (bn, bnn, bi) = da, db
    nvec_fm = _a(_a(bnn * 4, 256) + _a((bnn + 1) * 4, 256) + bi * 4, 16) // 16
    return (nvec_fm + 2 * bn + _pack(da) // 16 + (an + 3) // 4) * 16 + bn * 4 + 16


def kf_batch_lds(da, db):
    """kf_bow_batch_lds + 16 of KF1 a against candidate b: both packs, both handle arrays, 4 bytes per KF1
    feature and a byte per KF2 feature."""
    an, bn = da[0], db[0]
    return (_pack(da) // 16 + _pack(db) // 16 + (an + 3) // 4 + (bn + 3) // 4) * 16 + an * 4 + _a(bn, 16) + 16


def fits_block(da, db, npairs):
    return block_lds(da, db, npairs) <= LDS_MAX and db[0] <= F_MAX


def fits_batch(da, db):
    return batch_lds(da, db) <= LDS_MAX and db[0] <= F_MAX


def fits_kf_batch(da, db):
    return kf_batch_lds(da, db) <= LDS_MAX and da[0] <= F_MAX


def _npairs(case):
    return len(set(case.a.fv.node_ids.tolist()) & set(case.b.fv.node_ids.tolist()))


def _padded(side, add, off):
    """side + add inert features: every other one in no node, the others four to a node with map point -1,
    the nodes' ids between, below and above the case's (shared with nobody)."""
    rng = np.random.default_rng(add)
    p = object.__new__(Side)
    p.__dict__.update(side.__dict__)
    n0 = side.N
    keys = np.zeros(add, KEYPOINT_DTYPE)
    keys["x"], keys["y"], keys["angle"] = rng.uniform(20, 700, add), rng.uniform(20, 440, add), rng.uniform(0, 360, add)
    keys["size"], keys["response"], keys["class_id"] = 31.0, 20.0, -1
    p.keys = np.concatenate([side.keys, keys])
    p.desc = np.concatenate([side.desc, rng.integers(0, 256, (add, 32), dtype=np.uint8)])
    p.mp = np.concatenate([side.mp, np.full(add, -1, np.int32)])
    p.nodes = {k: list(v) for k, v in side.nodes.items()}
    listed = np.arange(n0 + 1, n0 + add, 2)
    for q in range(0, len(listed), 4):
        p.nodes[NODE0 - 1940 + STEP * (q // 4) + off] = [int(i) for i in listed[q:q + 4]]
    assert max(p.nodes) < NODE_END
    p.fv = FeatureVector(p.nodes)
    assert dims(p) == dims(side, add)
    return p


def _with(case, tag, a=None, b=None):
    c = object.__new__(Case)
    c.__dict__.update(case.__dict__)
    c.name = case.name + tag
    if a is not None:
        c.a = a
    if b is not None:
        c.b = b
        c.frame()
    return c


def _grow(case, side):
    """The smallest multiple of 64 features to add to a side so that no one-workgroup form takes the case."""
    add, np_ = 0, _npairs(case)
    while True:
        da, db = dims(case.a, add if side == "a" else 0), dims(case.b, add if side == "b" else 0)
        if not fits_block(da, db, np_) and not (side == "a" and fits_batch(da, db)):
            return add
        add += 64


_ADD = {}


def pad_keyframe(case):
    """Side a grown until neither orbfe_search_by_bow's nor the batch's one-workgroup form takes it against
    the plain frame. One size for all cases of a kind (the largest any needs)."""
    add = _ADD.get("a")
    if add is None:
        add = _ADD["a"] = max(_grow(c, "a") for c in all_cases())
    return _with(case, "+kf", a=_padded(case.a, add, PAD_KF))


def pad_frame(case):
    """Side b grown until orbfe_search_by_bow's one-workgroup form does not take it against the plain keyframe."""
    add = _ADD.get("b")
    if add is None:
        add = _ADD["b"] = max(_grow(c, "b") for c in all_cases())
    return _with(case, "+frame", b=_padded(case.b, add, PAD_F))


# ---------------------------------------------------------------- the list
LADDER_SIZES = (6, 17, 35)
NODE_SIZES = (1, 3, 4, 5, 16, 17, 33)


def _build():
    out = []
    for kind in ("kff", "kfkf"):
        out += [distance_edge(kind, th_low(kind)), distance_edge(kind, th_low(kind) + 1)]
        out += [ratio_cases(kind, r) for r in RATIOS] + [ratio_float(kind)]
        out += [lone_candidate(kind, r) for r in RATIOS] + [best_tie_rejected(kind)]
        out += [ladder(kind, m) for m in LADDER_SIZES] + [node_size(kind, m) for m in NODE_SIZES]
        out += [mp_skip(kind, "a"), empty_node(kind), join(kind), unlisted(kind)]
        for pname in PLANS:
            out += [rotation(kind, pname, True), rotation(kind, pname, False)]
    # the edges again in nodes of more than 16 candidates: the kernels' other node path restates them
    out += [distance_edge("kff", 50, True), distance_edge("kff", 51, True), ratio_float("kff", True),
            right_inside_left(True)] + [ratio_cases("kff", r, True) for r in RATIOS]
    out += [right_inside_left(), right_needs_left(), right_ignores_ratio(), right_tie(), nleft_edge("mid"),
            nleft_edge("0"), nleft_edge("n"), rot_two_entries()]
    out += [mp_skip("kfkf", "b"), right_skipped(1), right_skipped(2)]
    assert len({c.name for c in out}) == len(out)
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


# ---------------------------------------------------------------- running a case
def run_definition(case, double=False):
    """-> (nmatches, slots, trace) by oracle/sbow_definition.py."""
    a, b = case.a, case.b
    if case.kind == "kff":
        return bd.py_sbow_kf_f(a.keys["angle"], a.desc, a.mp, a.fv, b.keys["angle"], b.desc, b.fv, b.nleft,
                               case.nnratio, case.check_ori, double)
    return bd.py_sbow_kf_kf(a.keys["angle"], a.desc, a.mp, a.fv, a.nleft, b.keys["angle"], b.desc, b.mp, b.fv,
                            b.nleft, case.nnratio, case.check_ori, double)


def run_oracle(oracle_lib, case):
    """-> (nmatches, slots) by the C++ oracle."""
    a, b = case.a, case.b
    om = oracle_lib.OracleMatcher(case.nnratio, case.check_ori)
    if case.kind == "kff":
        return om.search_by_bow(a.keys, a.desc, a.mp, a.fv, case.F, b.fv)
    return om.search_by_bow_kf(a.keys, a.desc, a.mp, a.fv, b.keys, b.desc, b.mp, b.fv,
                               -1 if a.nleft is None else a.nleft, -1 if b.nleft is None else b.nleft)
