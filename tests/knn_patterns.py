"""Planted descriptors for the kNN + ratio stage of ComputeStereoFishEyeMatches (Frame.cc:1126-1151): every
rule of knnMatch(k = 2) and of the ratio test at the value where it decides, and every place where the
kernels split the train rows (k_knn2's 256-row LDS chunks, the W wave ranges of k_knn2_batch<W>).

A case is (name, L, R, ratio, check): queries, train rows, the ratio and a `check(case, trace, train, dist,
ngood)` that proves on the trace of oracle/knn_definition.py that the case reaches what its name says. No
descriptor is random except the filler rows, which are seeded and which the checks confirm to be far.

Two constructions:

  exact pair   R = {0, a row of `delta` bits}; a query of d0 bits outside that row's support is at exactly
               (d0, d0 + delta). All pairs of one delta share a train set, so a case holds several queries.
  block code   train row j has b_j bits set in a block of its own; a query with x_j bits inside block j and y
               bits in no block is at |q| + b_j - 2 x_j from row j, so the query chooses its best row, its
               second row and both distances. Rows outside the code are fillers of >= 100 bits.

A Frame embeds a case into the slab layout of the batched kernels (counts = (n, monoIndex), [cap][32]
descriptors) at a chosen monoL, monoR and cap, with poison around it: the train side's rows outside
[monoR, nR) are copies of the queries, the query side's rows outside [monoL, nL) copies of train rows, so a
kernel that reads or answers a row it should not shows a distance-0 match. pack() lays the frames of one
launch into two slabs or into one interleaved slab.
"""
from fractions import Fraction

import numpy as np

from oracle import knn_definition as kd

ORDER = [w * 32 + j for j in range(32) for w in range(8)]   # bit k of a planted set lies in word k % 8
RATIO = 0.7                                  # the reference's ratio
RATIOS = (0.5, 0.6, 0.75, 0.8, 0.9, 1.0)     # the others the API is driven at
# a pair at (0.5, 0.75, 1.0: exact) or next to equality with float32(ratio), planted with its neighbours
EQ_PAIR = {0.5: (64, 128), 0.6: (60, 100), 0.75: (96, 128), 0.8: (80, 100), 0.9: (90, 100), 1.0: (128, 128)}
CAPS = (64, 100, 2048, 2112, 4096)          # the issue's caps; 512 only hosts the mid-sized cases
FIT_CAPS = (64, 100, 512, 2048)
GEOMS = ((0, 0), (1, 3), (63, 1), (64, 64), (65, 63), (5, 65), (0, 7))   # (monoL, monoR) dealt over the cases
MT_NT, KNN_Q = 256, 64                      # k_knn2's chunk, k_knn2_batch's queries per block


def row(positions):
    """The 32-byte descriptor with exactly these bit positions set (position p: word p // 32, bit p % 32)."""
    bits = np.zeros(256, np.uint8)
    bits[list(positions)] = 1
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


def fillers(n, seed):
    """n seeded rows of at least 100 set bits, pairwise different."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for r in out:   # top up the rare light row
        while kd.hamming(r, np.zeros(32, np.uint8)) < 100:
            r[rng.integers(0, 32)] = 0xFF
    return out


def exact_passes(d0, d1, ratio):
    """d0 < d1 * float32(ratio) in exact arithmetic (what the double product of two floats of <= 9 and 24
    significant bits is)."""
    return Fraction(d0) < Fraction(d1) * Fraction(float(np.float32(ratio)))


def wave_ranges(nt, W):
    """k_knn2_batch<W>'s split of the train rows over its W waves."""
    return [(nt * w // W, nt * (w + 1) // W) for w in range(W)]


class Case:
    def __init__(self, name, group, L, R, ratio, check, **facts):
        self.name, self.group, self.ratio, self.check = name, group, float(ratio), check
        self.L = np.ascontiguousarray(L, np.uint8).reshape(-1, 32)
        self.R = np.ascontiguousarray(R, np.uint8).reshape(-1, 32)
        self.facts = facts   # what the check compares the trace with

    def __repr__(self):
        return self.name


# ---- exact pairs -------------------------------------------------------------------------------------------
def _check_pairs(case, trace, train, dist, ngood):
    pairs = case.facts["pairs"]
    assert len(trace) == len(pairs)
    for (d0, d1, t0, t1, rule), (p0, p1) in zip(trace, pairs):
        assert (d0, d1) == (p0, p1), (case.name, (d0, d1), (p0, p1))
        assert t0 == case.facts["best"] and t1 == 1 - t0
        assert rule == ("pass" if exact_passes(p0, p1, case.ratio) else "ratio-reject"), (case.name, p0, p1, rule)


def pair_case(name, group, ratio, delta, d0s):
    """All of (d0, d0 + delta) for d0 in d0s against one two-row train set; the nearer row comes first for
    an even delta and second for an odd one (for delta 0 the rows are equal and the earlier one is best)."""
    far = row(ORDER[:delta])
    near_first = delta % 2 == 0
    R = [np.zeros(32, np.uint8), far] if near_first else [far, np.zeros(32, np.uint8)]
    L = [row(ORDER[delta:delta + d0]) for d0 in d0s]
    return Case(name, group, L, R, ratio, _check_pairs, pairs=[(d0, d0 + delta) for d0 in d0s],
                best=0 if near_first else 1)


def ladder_pairs():
    """The pairs the ratio ladder at 0.7 must hold (integer arithmetic: passes iff 10 d0 < 7 d1)."""
    want = set()
    for d1 in range(2, 257):
        d0 = (7 * d1 + 9) // 10 - 1          # the largest d0 with 10 d0 < 7 d1
        want |= {(d0, d1), (d0 + 1, d1)}
    for k in range(1, 26):
        want |= {(7 * k - 1, 10 * k), (7 * k, 10 * k), (7 * k + 1, 10 * k)}
    want |= {(0, 0), (0, 1), (179, 256), (180, 256)} | {(d, d) for d in (1, 50, 128, 256)}
    return want


def disagreement(ratio):
    """The pairs 0 <= d0 <= d1 <= 256 on which the float product or the double literal decide otherwise than
    the kernels' rule."""
    return {(a, b) for b in range(257) for a in range(b + 1)
            if len({kd.ratio_passes(a, b, ratio, v) for v in kd.VARIANTS}) > 1}


def ratio_pairs(ratio):
    d0, d1 = EQ_PAIR[ratio]
    near = {(d0 - 1, d1), (d0, d1)} | ({(d0 + 1, d1)} if d0 < d1 else set())
    return disagreement(ratio) | near


def _pair_cases(group, ratio, pairs):
    by_delta = {}
    for d0, d1 in sorted(pairs):
        by_delta.setdefault(d1 - d0, []).append(d0)
    return [pair_case(f"{group}-delta{delta}", group, ratio, delta, d0s) for delta, d0s in sorted(by_delta.items())]


# ---- block code --------------------------------------------------------------------------------------------
class BlockCode:
    """nt train rows; code_rows[k] is a code row of sizes[k] bits in its own block, every other row a filler."""

    def __init__(self, nt, code_rows, sizes, seed):
        assert len(code_rows) == len(sizes) and len(set(code_rows)) == len(code_rows)
        self.nt, self.code_rows, self.sizes = nt, list(code_rows), list(sizes)
        self.blocks, k = [], 0
        for b in sizes:
            self.blocks.append(ORDER[k:k + b])
            k += b
        self.free = ORDER[k:]
        self.R = fillers(nt, seed) if nt else np.zeros((0, 32), np.uint8)
        for r, blk in zip(self.code_rows, self.blocks):
            assert 0 <= r < nt
            self.R[r] = row(blk)

    def query(self, A, B, da, db):
        """A query whose best is code row A at da and whose second is code row B at db (da <= db; on da == db
        the earlier row must be A), every other code row strictly farther than db."""
        ia, ib = self.code_rows.index(A), self.code_rows.index(B)
        ba, bb = self.sizes[ia], self.sizes[ib]
        assert da < db or (da == db and A < B)
        for xa in range(ba, -1, -1):
            for xb in range(bb, -1, -1):
                for y in range(len(self.free) + 1):
                    w = xa + xb + y
                    if w + ba - 2 * xa == da and w + bb - 2 * xb == db and \
                            all(w + b > db for i, b in enumerate(self.sizes) if i not in (ia, ib)):
                        return row(self.blocks[ia][:xa] + self.blocks[ib][:xb] + self.free[:y])
        raise AssertionError(f"no query for rows {A},{B} at ({da},{db}) with sizes {ba},{bb}")


def _check_plan(case, trace, train, dist, ngood):
    plan = case.facts["plan"]
    assert len(trace) == len(plan)
    for i, ((d0, d1, t0, t1, rule), want) in enumerate(zip(trace, plan)):
        assert (d0, d1, t0, t1) == want, (case.name, i, (d0, d1, t0, t1), want)
        assert rule == ("pass" if exact_passes(d0, d1, case.ratio) else "ratio-reject")
        assert t0 < len(case.R) and (train[i] == t0 if rule == "pass" else train[i] == -1)


def code_case(name, group, nt, code_rows, sizes, wants, seed, ratio=0.7, repeat=None, dups=()):
    """wants: [(A, B, da, db)]. dups: [(A, B)]: row B becomes a copy of code row A before the queries are
    made (a tie at any distance, 0 included). repeat: the number of queries, the wants taken cyclically."""
    code = BlockCode(nt, code_rows, sizes, seed)
    for a, b in dups:
        code.R[b] = code.R[a]
    L, plan = [], []
    for A, B, da, db in wants:
        if (A, B) in dups:   # the query lies da from row A and so from its copy
            ia = code.code_rows.index(A)
            assert da == db and da <= len(code.free)
            L.append(row(code.blocks[ia] + code.free[:da]))
        else:
            L.append(code.query(A, B, da, db))
        plan.append((da, db, A, B))
    if repeat is not None:
        idx = [i % len(L) for i in range(repeat)]
        L, plan = [L[i] for i in idx], [plan[i] for i in idx]
    return Case(name, group, L, code.R, ratio, _check_plan, plan=plan)


def _sizes(n, variant):
    """Block sizes of n code rows: "b" all 4 (every pair can hold (5, 9)), "a" / "c" 4 or 5 by bit 0 / bit 1
    of the row's number (pairs of rows of different size can hold (6, 7))."""
    return [4 + {"a": k % 2, "b": 0, "c": (k // 2) % 2}[variant] for k in range(n)]


def _all_pairs(code_rows, sizes):
    wants = []
    for i, A in enumerate(code_rows):
        for j, B in enumerate(code_rows):
            if i != j:
                wants.append((A, B, 5, 9) if (sizes[i] - sizes[j]) % 2 == 0 else (A, B, 6, 7))
    return wants


MERGE_NT = sorted({nt for W in (4, 16) for nt in (2, 3, W - 1, W, W + 1, 4 * W + 3)})   # 2 3 4 5 15 16 17 19 67


def _edge_rows(nt):
    """For a train set too large for one code: the rows at the ends of the wave ranges of both W."""
    rows = {0, nt - 1}
    for W in (4, 16):
        rg = [r for r in wave_ranges(nt, W) if r[1] > r[0]]
        for a, b in (rg[0], rg[1], rg[len(rg) // 2], rg[-1]):
            rows |= {a, b - 1}
    return sorted(rows)


def merge_cases():
    out = []
    for nt in MERGE_NT:
        rows = list(range(nt)) if nt <= 19 else _edge_rows(nt)
        for v in "abc":
            sizes = _sizes(len(rows), v)
            if v != "b" and len(set(sizes)) == 1:
                continue
            out.append(code_case(f"merge-nt{nt}-{v}", "merge", nt, rows, sizes, _all_pairs(rows, sizes), 100 + nt))
    return out


def tie_cases():
    """The best distance twice, everything else far: rejected, at distance 0 too."""
    out = []
    for W in (4, 16):
        nt = 4 * W + 3
        rg = wave_ranges(nt, W)
        spots = {"same": (rg[1][0], rg[1][0] + 1), "adjacent": (rg[W // 2][1] - 1, rg[W // 2][1]),
                 "first-last": (0, nt - 1)}
        for where, (A, B) in spots.items():
            wa = [w for w, (a, b) in enumerate(rg) if a <= A < b][0]
            wb = [w for w, (a, b) in enumerate(rg) if a <= B < b][0]
            assert {"same": wa == wb, "adjacent": wb == wa + 1, "first-last": (wa, wb) == (0, W - 1)}[where]
            for d in (0, 5):
                out.append(code_case(f"tie-W{W}-{where}-d{d}", "tie", nt, [A, B], [4, 4], [(A, B, d, d)],
                                     200 + W + d, dups=[(A, B)]))
            # equally near but different rows (no copy): d = y + 4 for any x, here 5
            out.append(code_case(f"tie-W{W}-{where}-distinct", "tie", nt, [A, B], [4, 4], [(A, B, 5, 5)], 230 + W))
    for A, B in ((255, 256), (0, 511)):
        for d in (0, 5):
            out.append(code_case(f"tie-knn2-{A}-{B}-d{d}", "tie", 512, [A, B], [4, 4], [(A, B, d, d)], 260 + d,
                                 dups=[(A, B)]))
    return out


def _check_few(case, trace, train, dist, ngood):
    assert len(case.R) < 2 and ngood == 0 and (train == -1).all() and (dist == -1).all()
    assert all(t[4] == "few-train" for t in trace)
    if len(case.R) == 1:
        assert trace[0][:3] == (0, kd.INF, 0)   # the first query is the train row itself


def small_cases():
    code = BlockCode(3, [0, 1, 2], [4, 4, 4], 300)
    q = [code.R[0], code.query(0, 1, 5, 9), code.query(1, 2, 5, 9)]
    none = np.zeros((0, 32), np.uint8)
    return [Case("train-0", "small", q, none, 0.7, _check_few),
            Case("train-1", "small", q, code.R[:1], 0.7, _check_few),
            code_case("queries-0", "small", 3, [0, 1, 2], [4, 4, 4], [], 300),
            code_case("queries-1", "small", 3, [0, 1, 2], [4, 4, 4], [(2, 0, 5, 9)], 300)]


def chunk_cases():
    """k_knn2's 256-row chunks of the train rows and 256-query blocks."""
    out = []
    for nr in (255, 256, 257, 512, 513):
        rows = sorted({r for r in (0, 254, 255, 256, 257, 511, 512, nr - 1) if r < nr})
        sizes = _sizes(len(rows), "a")
        out.append(code_case(f"chunk-nr{nr}", "chunk", nr, rows, sizes, _all_pairs(rows, sizes), 400 + nr))
    # the all-zero query: its best is the last row (4 bits), its second row 0 (8 bits); rows past nr of the
    # second chunk's LDS are zero-filled and must not be scanned
    code = BlockCode(257, [0, 256], [8, 4], 460)
    out.append(Case("chunk-zero-query", "chunk", [np.zeros(32, np.uint8), code.query(0, 256, 6, 10)], code.R, 0.7,
                    _check_plan, plan=[(4, 8, 256, 0), (6, 10, 0, 256)]))
    for nl in (1, 255, 256, 257):
        rows, sizes = list(range(5)), _sizes(5, "a")
        out.append(code_case(f"chunk-nl{nl}", "chunk", 5, rows, sizes, _all_pairs(rows, sizes), 470, repeat=nl))
    return out


def big_train_case():
    """cap = 4096 with nR = 4096: code rows at the ends of the W = 4 and W = 16 ranges of 4096 rows."""
    rows = [0, 255, 256, 1023, 1024, 2047, 2048, 3839, 3840, 4095]
    sizes = _sizes(len(rows), "a")
    return code_case("big-train-4096", "geometry", 4096, rows, sizes, _all_pairs(rows, sizes), 500)


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        cs = _pair_cases("ladder-0.7", 0.7, ladder_pairs())
        for r in RATIOS:
            cs += _pair_cases(f"ratio-{r}", r, ratio_pairs(r))
        cs += tie_cases() + merge_cases() + small_cases() + chunk_cases() + [big_train_case()]
        assert len({c.name for c in cs}) == len(cs)
        _CASES = cs
    return _CASES


def case(name):
    return next(c for c in all_cases() if c.name == name)


def planted_pairs(group):
    """The (d0, d1) the exact-pair cases of a group say they plant (their checks prove it)."""
    return {p for c in all_cases() if c.group == group for p in c.facts["pairs"]}


def run_definition(c, variant="kernel"):
    trace = []
    t, d, n = kd.knn_ratio(c.L, c.R, c.ratio, variant, trace)
    return t, d, n, trace


# ---- slab embedding ----------------------------------------------------------------------------------------
def _poison(cap, src):
    if len(src) == 0:
        return np.full((cap, 32), 0x5A, np.uint8)
    return src[np.arange(cap) % len(src)].copy()


class Frame:
    """A case at (monoL, monoR, cap): counts and [cap][32] descriptors of its left and its right image."""

    def __init__(self, c, monoL, monoR, cap):
        self.case, self.monoL, self.monoR, self.cap = c, monoL, monoR, cap
        self.nL, self.nR = monoL + len(c.L), monoR + len(c.R)
        assert self.nL <= cap and self.nR <= cap, (c.name, monoL, monoR, cap)
        self.name = f"{c.name}@L{monoL}-R{monoR}-cap{cap}"
        self._built = self._want = None

    def __repr__(self):
        return self.name

    def built(self):
        """(counts_l, desc_l, counts_r, desc_r)."""
        if self._built is None:
            c = self.case
            dl, dr = _poison(self.cap, c.R), _poison(self.cap, c.L)
            dl[self.monoL:self.nL] = c.L
            dr[self.monoR:self.nR] = c.R
            self._built = (np.array([self.nL, self.monoL], np.int32), dl, np.array([self.nR, self.monoR], np.int32), dr)
        return self._built

    def expected(self, oracle_lib):
        """(l2r [cap], dist [cap], ngood) by the C++ oracle on the frame's own bytes, computed once."""
        if self._want is None:
            self._want = oracle_frame(oracle_lib, *self.built(), self.cap, self.case.ratio)
        return self._want


def oracle_frame(oracle_lib, cl, dl, cr, dr, cap, ratio):
    """knn_definition.knn_frame with the C++ oracle in the place of knn_ratio."""
    nL, monoL, nR, monoR = int(cl[0]), int(cl[1]), int(cr[0]), int(cr[1])
    l2r, dist = np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    if nL > monoL:
        _, t, d = oracle_lib.stereo_knn_ratio(dl[monoL:nL], dr[monoR:max(nR, monoR)], ratio)
        l2r[monoL:nL] = np.where(t >= 0, t + monoR, -1)
        dist[monoL:nL] = d
    return l2r, dist, int((l2r >= 0).sum())


def fit_cap(c, monoL, monoR, caps=FIT_CAPS):
    return next(k for k in caps if monoL + len(c.L) <= k and monoR + len(c.R) <= k)


GEOMETRY_BASE = "merge-nt5-a"   # 20 queries over 5 train rows


def geometry_frames():
    """The slot geometry: monoL / monoR off and on multiples of 64, one query and none, query blocks below
    monoL, across monoL, across nL and past nL, every cap."""
    g, one, zero = case(GEOMETRY_BASE), case("queries-1"), case("queries-0")
    out = []
    for cap in CAPS:
        for monoL, monoR in ((0, 0), (1, 65), (63, 64), (64, 1), (65, 63)):
            if monoL + len(g.L) <= cap:
                out.append(Frame(g, monoL, min(monoR, cap - len(g.R)), cap))
        room = min(cap - 1, 70)
        out += [Frame(one, room, 2, cap), Frame(zero, room, 0, cap), Frame(one, 0, 0, cap)]   # nL-1, nL, a lone row
    # the > 64 KB launches on other cases: a tie across the first and last range, empty ranges, a long scan
    for cap in (2112, 4096):
        for name in ("tie-W16-first-last-d0", "tie-W4-adjacent-d5", "merge-nt2-a", "merge-nt67-a", "train-1",
                     "chunk-nr513", "chunk-zero-query"):
            out.append(Frame(case(name), 65, cap - 600, cap))
    out.append(Frame(case("big-train-4096"), 3, 0, 4096))
    return out


_FRAMES = None


def all_frames():
    """Every case once, at a (monoL, monoR) dealt from GEOMS and the smallest cap that holds it, and the
    geometry frames."""
    global _FRAMES
    if _FRAMES is None:
        fr = []
        for i, c in enumerate(c for c in all_cases() if c.name != "big-train-4096"):
            monoL, monoR = GEOMS[i % len(GEOMS)]
            # a launch has one ratio: the few cases of another ratio than 0.7 share one cap
            fr.append(Frame(c, monoL, monoR, fit_cap(c, monoL, monoR, FIT_CAPS if c.ratio == RATIO else FIT_CAPS[1:])))
        _FRAMES = fr + geometry_frames()
    return _FRAMES


def frames_by_cap():
    out = {}
    for f in all_frames():
        out.setdefault(f.cap, []).append(f)
    return out


def launch_groups():
    """{(cap, ratio): frames}: what one launch can hold."""
    out = {}
    for f in all_frames():
        out.setdefault((f.cap, f.case.ratio), []).append(f)
    return out


ADDRESSINGS = ("separate", "interleaved")


def pack(frames, addressing):
    """The frames of one launch laid into slabs. "separate": the left images in a slab of len + 3 images from
    image 2 on, the right images every second image of a slab of 2 len + 1. "interleaved": one slab, left
    image 2 f, right image 2 f + 1. Images that belong to no frame are full of copies of the first frame's
    queries and claim cap rows. Returns (counts_l, desc_l, counts_r, desc_r, (lbase, lstep, rbase, rstep));
    in the interleaved form both sides are the same arrays."""
    n, cap = len(frames), frames[0].cap
    assert all(f.cap == cap for f in frames)
    spare = _poison(cap, frames[0].case.L)

    def slab(nimg):
        return np.tile(np.array([cap, 0], np.int32), (nimg, 1)), np.tile(spare, (nimg, 1, 1))

    if addressing == "separate":
        (cl, dl), (cr, dr), adr = slab(n + 3), slab(2 * n + 1), (2, 1, 0, 2)
    else:
        cl, dl = slab(2 * n + 1)
        cr, dr, adr = cl, dl, (0, 2, 1, 2)
    for f, fr in enumerate(frames):
        a, b, c, d = fr.built()
        li, ri = adr[0] + f * adr[1], adr[2] + f * adr[3]
        cl[li], dl[li], cr[ri], dr[ri] = a, b, c, d
    return cl, dl, cr, dr, adr


def launches(frames, nframes):
    """The frames of one cap cut into launches of nframes: consecutive frames, the last launch filled from the
    start of the list, so that within a launch neighbouring frames differ whenever the list has two frames."""
    m = len(frames)
    return [[frames[(s + k) % m] for k in range(nframes)] for s in range(0, m, nframes)]
