"""Planted ComputeStereoMatches cases: image pairs, keypoint records and descriptors built so that one
branch of k_stereo / k_stereo_cut decides the answer, each with a CPU precondition asserted from the
trace of oracle/stereo_definition.py before anything runs on the GPU (the pattern of octree_patterns.py).

Two kinds of image pair, both 320 x 264 (8 levels at 1.2: level 7 is 89 x 74, one pixel above the 73 the
engine's cell grid needs, and still admits legal keys; 320 columns hold a row of 130 distinct candidates):
  tex     smooth noise; right = left moved 8 px (uR = uL - 8) plus +-3 of independent noise, so the window
          search of a true match finds sums around 200 instead of 0 and the median cut keeps it
  patch   a grid of 11 x 11 left windows and 11 x 21 right strips around level-0 keys, written pixel by
          pixel so that all 11 sums are chosen integers: a ramp of slope 7 gives SAD(k) = 847 |k - k0|,
          `a` subtracted from the strip's column 5 adds a to every shift <= 5, `b` added to column 15 adds
          b to every shift >= 5: SAD(4) = 847 + a, SAD(5) = a + b, SAD(6) = 847 + b

Two larger tex pairs serve one path each: TALL (1152 x 2048, the bitonic ordering) and COARSE (1168 x 1168
with 5 levels at 2.0, the binary-search fallback of the row table).

Every planted key is one the extractor can emit (validate()): integer level coordinates in
[19, w_l - 19) x [19, h_l - 19) times scale[l] in float32. The one exception is the right key of
`edge-reject`, labelled OUTSIDE the extractor's domain: a negative column, which the iniu < 0 test
rejects before any pixel is read.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np

import fast_patterns as fp
from oracle import stereo_definition as sd

F32 = np.float32
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
NLEVELS, SCALE, NFEAT = 8, 1.2, 1200
EDGE = 19            # EDGE_THRESHOLD: the extractor emits keys at least 19 px inside their level
SHIFT = 8            # disparity of the tex pair
U = 847              # 121 x 7: the ramp's SAD per shift


class Geom:
    def __init__(self, w, h, yoff=0, nlevels=NLEVELS, factor=SCALE):
        self.w, self.h, self.yoff, self.nlevels, self.factor = w, h, yoff, nlevels, factor
        s, self.scale, self.inv = F32(1.0), [], []
        for l in range(nlevels):
            if l:
                s = F32(np.float64(s) * np.float64(F32(factor)))
            self.scale.append(s)
            self.inv.append(F32(1.0) / s)
        self.sizes = fp.level_sizes(w, h, nlevels, factor)

    def legal(self, l, x, y):
        w, h = self.sizes[l]
        return EDGE <= x < w - EDGE and EDGE <= y < h - EDGE


SMALL = Geom(320, 264)
# More than 1983 rows: the bitonic / binary-search ordering. 1152 wide, not narrower: at 1024 x 2048 the
# detection area of every level is less than half as wide as high, DistributeOctTree's root column count
# round(width / height) is 0 and the reference extractor itself divides by it.
TALL = Geom(1152, 2048, yoff=1730)
# A second pyramid, 5 levels at 2.0: level 4 has scale 16, so the row band of one of its keys spans 64
# rows and k_stereo's row-start table (rows from -32) no longer covers row - maxspan of a left key on
# rows 19 .. 31. 1168 = 16 x 73: level 4 is 73 x 73, the smallest level the cell grid accepts.
COARSE = Geom(1168, 1168, nlevels=5, factor=2.0)
PAIR_GEOM = {"tex": SMALL, "patch": SMALL, "tall": TALL, "coarse": COARSE}


# ---- images -------------------------------------------------------------------------------------
_IMAGES = {}


def _texture(g, seed):
    rng = np.random.default_rng(seed)
    lo = rng.integers(40, 216, (g.h // 4 + 3, g.w // 4 + 3)).astype(np.float64)
    up = np.kron(lo, np.ones((4, 4)))
    sm = sum(up[dy:dy + g.h + 8, dx:dx + g.w + 8] for dy in range(4) for dx in range(4)) / 16.0
    base = np.clip(sm[:g.h, :g.w + SHIFT] + rng.integers(-6, 7, (g.h, g.w + SHIFT)), 0, 255)
    right = np.clip(base[:, SHIFT:] + rng.integers(-3, 4, (g.h, g.w)), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(base[:, :g.w].astype(np.uint8)), right   # right(x) = left(x + 8): uR = uL - 8


def ramp_windows(k0=5, a=0, b=0):
    """(left 11 x 11, right 11 x 21): SAD(k) = U |k - k0| + (a if k <= 5) + (b if k >= 5)."""
    r = np.tile(50 + 7 * np.arange(21), (11, 1)).astype(np.int64)
    lw = r[:, k0:k0 + 11].copy()
    for tot, col, sign in ((a, 5, -1), (b, 15, 1)):
        per = np.full(11, tot // 11)
        per[:tot % 11] += 1
        assert per.max() <= 84
        r[:, col] += sign * per
    assert r.min() >= 0 and r.max() <= 255
    return lw.astype(np.uint8), r.astype(np.uint8)


def periodic_windows():
    """Period 4 along x: the sums vanish at shifts 3 and 7."""
    p = np.array([40, 200, 90, 150])
    r = np.tile(p[np.arange(21) % 4], (11, 1))
    return r[:, 3:14].astype(np.uint8), r.astype(np.uint8)


def flat_windows():
    return np.full((11, 11), 100, np.uint8), np.full((11, 21), 100, np.uint8)


# The patch pool: name -> (windows, disparity of the planted right key). Pool entries "s<value>" are
# ramps whose winning sum is that value, split evenly (delta about 0) unless said otherwise.
POOL = {
    "tie-3-7": (periodic_windows(), 4), "flat": (flat_windows(), 4),
    "min-at--5": (ramp_windows(k0=0), 4), "min-at-+5": (ramp_windows(k0=10), 4),
    "delta-0": (ramp_windows(a=60, b=60), 4), "delta-+half": (ramp_windows(a=U, b=0), 4),
    "delta--half": (ramp_windows(a=0, b=U - 1), 4),
    # a > b: deltaR > 0, the match moves right and the disparity shrinks; a < b the other way
    "disp-0": (ramp_windows(a=40, b=40), 0), "disp-0-neg": (ramp_windows(a=40, b=10), 0),
    "disp-0-pos": (ramp_windows(a=10, b=40), 0),
    "disp-32": (ramp_windows(a=40, b=40), 32), "disp-32-below": (ramp_windows(a=40, b=10), 32),
    "disp-32-above": (ramp_windows(a=10, b=40), 32),
}
SAD_POOL = [0, 0, 0, 0, 0, 0, 1, 2, 3, 10, 20, 21, 22, 50, 99, 100, 100, 100, 101, 104, 105, 110, 150, 200, 209, 210, 210,
            211, 218, 219, 220, 221, 230, 231, 254, 255, 255, 255, 256, 256, 256, 257, 300, 400, 500, 535, 536, 537, 538,
            539, 600, 10, 10]
PATCH_AT = {}   # name -> (cx, cy) of the left key, filled by _patch_pair


def _patch_pair(g, seed):
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (g.h, g.w), dtype=np.uint8)
    right = rng.integers(0, 256, (g.h, g.w), dtype=np.uint8)
    used_l, used_r = np.zeros((g.h, g.w), bool), np.zeros((g.h, g.w), bool)
    names = list(POOL) + [f"s{v}#{i}" for i, v in enumerate(SAD_POOL)]
    slot = 0
    for name in names:
        if name in POOL:
            (lw, rw), dsp = POOL[name]
        else:
            v = int(name[1:].split("#")[0])
            (lw, rw), dsp = ramp_windows(a=v // 2, b=v - v // 2), 4
        while True:   # next free grid cell whose right strip fits
            cy, cx = 24 + 12 * (slot // 5), 64 + 48 * (slot % 5)
            slot += 1
            assert cy + 5 < g.h - EDGE
            if cx - dsp - 10 >= 3 and not used_r[cy, cx - dsp - 10:cx - dsp + 11].any():
                break
        assert g.legal(0, cx, cy) and g.legal(0, cx - dsp, cy)
        assert not used_l[cy - 5:cy + 6, cx - 5:cx + 6].any() and not used_r[cy - 5:cy + 6, cx - dsp - 10:cx - dsp + 11].any()
        left[cy - 5:cy + 6, cx - 5:cx + 6] = lw
        right[cy - 5:cy + 6, cx - dsp - 10:cx - dsp + 11] = rw
        used_l[cy - 5:cy + 6, cx - 5:cx + 6] = True
        used_r[cy - 5:cy + 6, cx - dsp - 10:cx - dsp + 11] = True
        PATCH_AT[name] = (cx, cy, dsp)
    return left, right


def images(pair):
    """(left, right) of a pair name: 'tex', 'patch', 'tall', 'coarse'."""
    if pair not in _IMAGES:
        _IMAGES[pair] = {"tex": lambda: _texture(SMALL, 11), "patch": lambda: _patch_pair(SMALL, 12),
                         "tall": lambda: _texture(TALL, 13), "coarse": lambda: _texture(COARSE, 14)}[pair]()
    return _IMAGES[pair]


# ---- keys and descriptors -----------------------------------------------------------------------
def make_key(g, l, x, y):
    k = np.zeros((), KEYPOINT_DTYPE)
    k["x"], k["y"] = F32(x) * g.scale[l], F32(y) * g.scale[l]
    k["size"], k["angle"] = F32(31.0) * g.scale[l], F32((x * 37 + y * 11) % 360)
    k["response"], k["octave"], k["class_id"] = F32(20 + (x + y) % 60), l, -1
    return k


class Build:
    """Accumulates the planted keys of one case. Level coordinates are kept for validate()."""

    def __init__(self, name, g=SMALL):
        self.g, self.rng = g, np.random.default_rng(zlib.crc32(name.encode()))
        self.k = {"L": [], "R": []}
        self.d = {"L": [], "R": []}
        self.lv = {"L": [], "R": []}   # (level, x, y) or None for a key outside the extractor's domain

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flip(self, d, k):
        bits = np.unpackbits(d)
        bits[self.rng.permutation(256)[:k]] ^= 1
        return np.packbits(bits)

    def add(self, side, l, x, y, d=None):
        self.k[side].append(make_key(self.g, l, x, y))
        self.d[side].append(self.desc() if d is None else d)
        self.lv[side].append((l, x, y))
        return len(self.k[side]) - 1

    def add_raw(self, side, x, y, octave, d):
        """A key OUTSIDE the extractor's domain (edge-reject only)."""
        k = make_key(self.g, octave, 30, 30)
        k["x"], k["y"] = F32(x), F32(y)
        self.k[side].append(k)
        self.d[side].append(d)
        self.lv[side].append(None)
        return len(self.k[side]) - 1

    def pair(self, l, x, y, dx, flips, dy=0):
        """A left key and its right key dx level pixels to the left, `flips` descriptor bits apart."""
        d = self.desc()
        return self.add("L", l, x, y, d), self.add("R", l, x - dx, y + dy, self.flip(d, flips))

    def fill_right(self, n, rows, x0=EDGE, step=2, l=0):
        """n right keys with random descriptors on the given level rows, distinct columns."""
        out, w = [], self.g.sizes[l][0]
        per = (w - EDGE - x0 + step - 1) // step
        assert n <= per * len(rows)
        for i in range(n):
            out.append(self.add("R", l, x0 + step * (i % per), rows[i // per]))
        return out

    def arrays(self, side):
        k = np.array(self.k[side], KEYPOINT_DTYPE) if self.k[side] else np.zeros(0, KEYPOINT_DTYPE)
        d = np.array(self.d[side], np.uint8).reshape(-1, 32)
        return k, d


@dataclass(eq=False)
class StereoCase:
    name: str
    pair: str
    b: Build
    bf: float
    fx: float
    pre: object
    layout: tuple | None = None        # (extra pitch, base offset) of the caller's images
    outside: str | None = None         # why a key lies outside the extractor's domain
    tie_last: bool = False             # the reference also holds the definition's wrong tie rule
    _ref: dict = field(default_factory=dict)

    def __repr__(self):
        return self.name

    @property
    def g(self):
        return self.b.g

    def keys(self):
        return self.b.arrays("L") + self.b.arrays("R")


def case(name, b, pre, pair="tex", bf=32.0, fx=64.0, **kw):
    return StereoCase(name, pair, b, bf, fx, pre, **kw)


def validate(c, cap):
    """Every key is legal (or labelled outside), counts fit the capacity, keys of a side are distinct."""
    for side in "LR":
        k, _ = c.b.arrays(side)
        assert len(k) <= cap, f"{c.name}: {len(k)} {side} keys over the capacity {cap}"
        seen = set()
        for rec, lv in zip(k, c.b.lv[side]):
            if lv is None:
                assert c.outside and side == "R", f"{c.name}: unlabelled key outside the extractor's domain"
                assert 0 <= int(rec["octave"]) < c.g.nlevels and 0 <= int(rec["y"]) < c.g.h and rec["x"] <= -1.0
                continue
            l, x, y = lv
            assert c.g.legal(l, x, y), f"{c.name}: {side} key {lv} outside [19, w - 19) x [19, h - 19)"
            assert rec["octave"] == l and rec["x"] == F32(x) * c.g.scale[l] and rec["y"] == F32(y) * c.g.scale[l]
            assert lv not in seen, f"{c.name}: duplicate {side} key {lv}"
            seen.add(lv)


def check_windows(c, tr):
    """Every window the definition read lies inside its level with the margin of the kernel's aligned
    dword loads (3 bytes before, 7 after the 21 columns)."""
    for kt in tr.keys:
        if kt.window:
            l, r0, c0l, c0r = kt.window
            w, h = c.g.sizes[l]
            assert r0 >= 0 and r0 + 11 <= h and c0l >= 3 and c0l + 16 <= w and c0r >= 3 and c0r + 28 <= w, (c.name, kt.window)


# ---- references ---------------------------------------------------------------------------------
_ORACLES = {}


def oracles(pair, oracle_lib):
    """The oracle's two extractors holding the pyramids of a pair (one extraction per distinct image)."""
    if pair not in _ORACLES:
        left, right = images(pair)
        g = PAIR_GEOM[pair]
        ol = oracle_lib.OracleExtractor(NFEAT, g.factor, g.nlevels, 20, 7)
        orr = oracle_lib.OracleExtractor(NFEAT, g.factor, g.nlevels, 20, 7)
        ol(left)
        orr(right)
        pl = [ol.pyramid_level(l) for l in range(g.nlevels)]
        pr = [orr.pyramid_level(l) for l in range(g.nlevels)]
        _ORACLES[pair] = (ol, orr, pl, pr, ol.level_info())
    return _ORACLES[pair]


def definition(c, oracle_lib, **kw):
    _, _, pl, pr, info = oracles(c.pair, oracle_lib)
    kl, dl, kr, dr = c.keys()
    return sd.stereo_match(pl, pr, info["scale"], info["inv_scale"], kl, dl, kr, dr, c.bf, c.fx, **kw)


def reference(c, oracle_lib):
    """{'oracle': (uR, depth, n), 'def': (uR, depth, n, trace)} of a case, computed once, never modified."""
    if not c._ref:
        ol, orr = oracles(c.pair, oracle_lib)[:2]
        kl, dl, kr, dr = c.keys()
        c._ref["oracle"] = oracle_lib.stereo_match(ol, orr, kl, dl, kr, dr, c.bf, c.fx)
        c._ref["def"] = definition(c, oracle_lib)
        if c.tie_last:
            c._ref["def-tie-last"] = definition(c, oracle_lib, tie_last=True)
    return c._ref


def capacity(oracle_lib, g=SMALL):
    """The engine's keypoint capacity per image from the reference's level budgets and root columns."""
    ora = oracle_lib.OracleExtractor(NFEAT, g.factor, g.nlevels, 20, 7)
    budget = [int(v) for v in ora.level_info()["per_level"]]
    ora.close()
    n_ini = [int(sd.round_half_away(F32(w - 2 * 16) / F32(h - 2 * 16))) for w, h in g.sizes]   # root columns
    return sum(max(b + 3, 4 * k) for b, k in zip(budget, n_ini))


# The engine's capacity per geometry (Geom objects hash by identity; there is one of each). The values
# are written out, not computed at import, because capacity() needs the oracle library: they are asserted
# against capacity() on the CPU and against the engine on the GPU. SMALL and TALL happen to agree: the
# level budgets are the same and every level has one root column.
CAP = {SMALL: 1224, TALL: 1224, COARSE: 1215}


# ---- preconditions ------------------------------------------------------------------------------
def outcomes(tr):
    return [k.outcome for k in tr.keys]


def bands_of(c):
    """(bands, maxspan): the row band of every right key and the widest one, the kernel's `maxspan`."""
    kr = c.keys()[2]
    bands = [sd.band(k["y"], int(k["octave"]), c.g.scale) for k in kr]
    return bands, max(hi - lo for lo, hi in bands)


def scan_pos(c, i_l, i_r):
    """(lowest, highest) position that right key i_r can have in the kernel's scan of left key i_l. The scan
    visits the records whose first band row lies in [row - maxspan, row], ordered by that row; records that
    share a first row come in an order the counting sort's atomics decide, so i_r lies anywhere among them."""
    bands, maxspan = bands_of(c)
    row = int(c.keys()[0]["y"][i_l])
    own = bands[i_r][0]
    assert row - maxspan <= own <= row
    before = sum(1 for lo, _ in bands if row - maxspan <= lo < own)
    return before, before + sum(1 for lo, _ in bands if lo == own) - 1


def scan_rank(c, i_l, i_r):
    return scan_pos(c, i_l, i_r)[0]


def trips_of(c, i_l, i_r):
    """The 64-stride trips (first, last) in which the scan of left key i_l can meet right key i_r."""
    lo, hi = scan_pos(c, i_l, i_r)
    return lo // 64, hi // 64


def pre_outcomes(*want):
    def pre(c, ref):
        got = outcomes(ref["def"][3])
        assert got[:len(want)] == list(want), f"{c.name}: outcomes {got[:len(want)]}, wanted {want}"
    return pre


def pre_trip(first_rank):
    def pre(c, ref):
        tr = ref["def"][3].keys[0]
        assert tr.ncand >= first_rank + 1 and tr.outcome == "accepted", (tr.ncand, tr.outcome)
        assert tr.best_idx == c.best and scan_rank(c, 0, c.best) >= first_rank
        # the decoy's band starts on a row of its own, below every other record's: it is scanned first
        assert scan_pos(c, 0, c.decoy) == (0, 0)
    return pre


def pre_tie(c, ref):
    """Each left key has two passing candidates on the best distance, and keeping the last instead of the
    first changes its answer. Where in the scan the two sit is asserted from the bounds of scan_pos():
    (left key, lower right index, higher right index) per entry."""
    tr = ref["def"][3]
    alt = ref["def-tie-last"]
    for i, kt in enumerate(tr.keys):
        assert kt.nties == 2 and kt.best_dist < sd.TH_ORB, (c.name, i, kt.nties, kt.best_dist)
        assert ref["def"][0][i] != alt[0][i], f"{c.name}: key {i} answers the same under either tie rule"
    for i_l, first, second in c.within + [c.across, c.cross_later, c.later]:
        assert first < second and tr.keys[i_l].best_idx == first, (c.name, i_l, first, second)
    for i_l, first, second in c.within:      # one trip, whatever order the sort leaves them in
        assert trips_of(c, i_l, first) == trips_of(c, i_l, second) and len(set(trips_of(c, i_l, first))) == 1
    i_l, first, second = c.across            # the lower index in an earlier trip
    assert trips_of(c, i_l, first)[1] < trips_of(c, i_l, second)[0]
    i_l, first, second = c.cross_later       # the lower index in a later trip
    assert trips_of(c, i_l, first)[0] > trips_of(c, i_l, second)[1]
    i_l, first, second = c.later             # one trip, the lower index sorted later
    assert trips_of(c, i_l, first) == trips_of(c, i_l, second) and len(set(trips_of(c, i_l, first))) == 1
    assert scan_pos(c, i_l, first)[0] > scan_pos(c, i_l, second)[1]


# ---- cases: candidate scan ----------------------------------------------------------------------
def row_candidates(n, g=SMALL, pad_to=None):
    """One left key whose row holds n candidates: the true match, planted FIRST in right-index order, sorts
    after all others (its band starts on the key's row), past the first 64 (n = 65) or 128 (n = 130); a
    decoy 6 bits worse than the match is the only record whose band starts on row y - 4, the lowest, so it
    is the first record scanned."""
    b = Build(f"row-{n}", g)
    y = 100 + g.yoff
    d = b.desc()
    b.add("L", 0, 250, y, d)
    best = b.add("R", 0, 250 - SHIFT, y + 2, b.flip(d, 3))
    decoy = b.add("R", 0, 250 - 61, y - 2, b.flip(d, 9))
    b.fill_right(n - 2, [y - 1, y], x0=EDGE + 1)
    if pad_to:
        b.fill_right(pad_to - n, [y + 40, y + 41])
    c = case(f"row-{n}-candidates" + ("-tall" if g is TALL else ""), b, pre_trip(64 if n < 130 else 128), pair="tall" if g is TALL else "tex", fx=100.0, bf=50.0)
    c.best, c.decoy = best, decoy
    return c


def tie_case(g=SMALL, pad_to=None):
    b = Build("tie", g)
    y = 60 + g.yoff

    def tied(x, yy, dy_true, dy_decoy, true_first):
        d = b.desc()
        i_l = b.add("L", 0, x, yy, d)
        order = [(x - SHIFT, yy + dy_true), (x - 70, yy + dy_decoy)]
        if not true_first:
            order.reverse()
        return i_l, [b.add("R", 0, px, py, b.flip(d, 6)) for px, py in order]
    # tied() returns the left index and the two right indices in planting order: (lower, higher)
    # within one trip, the true match first and second
    w1, w1r = tied(200, y, 0, 0, True)
    w2, w2r = tied(230, y, 0, 0, False)
    # across trips: 70 records sort between the bands that start on rows yb - 4 and yb
    yb = y + 60
    a_l, a_r = tied(200, yb, -2, 2, True)     # the lower index starts its band 4 rows earlier
    x_l, x_r = tied(240, yb, 2, -2, True)     # the lower index starts its band 4 rows later: it sorts later
    b.fill_right(70, [yb - 1], x0=EDGE + 1)
    # same trip, lower index sorted later
    yc = y + 100
    l_l, l_r = tied(210, yc, 2, -2, True)
    if pad_to:
        b.fill_right(pad_to - len(b.k["R"]), [y + 20, y + 21])
    c = case("tie-first-iR-wins" + ("-tall" if g is TALL else ""), b, pre_tie, pair="tall" if g is TALL else "tex", fx=100.0, bf=50.0,
             tie_last=True)
    c.within = [(w1, *w1r), (w2, *w2r)]
    c.across, c.cross_later, c.later = (a_l, *a_r), (x_l, *x_r), (l_l, *l_r)
    return c


def dist_case(name, flips, want):
    b = Build(name)
    for i, f in enumerate(flips):
        b.pair(0, 100 + 40 * i, 50 + 12 * i, SHIFT, f)

    def pre(c, ref):
        tr = ref["def"][3]
        assert [k.best_dist for k in tr.keys] == [min(f, 100) for f in flips]
        assert outcomes(tr) == want, outcomes(tr)
    return case(name, b, pre)


def octave_case(name, right_octave, rx, ry, want_filtered):
    """A level-3 left key at (60, 50) -> (103.68, 86.4); one right key, 8 px to the left, on another octave."""
    b = Build(name)
    d = b.desc()
    b.add("L", 3, 60, 50, d)
    b.add("R", right_octave, rx, ry, b.flip(d, 4))

    def pre(c, ref):
        kt = ref["def"][3].keys[0]
        assert kt.ncand == 1 and kt.nfiltered == want_filtered, (kt.ncand, kt.nfiltered)
        assert (kt.outcome == "no-filtered") == (want_filtered == 0)
    return case(name, b, pre)


def _ulp_pairs(g, want):
    """(left level, left column, right level, right column) one octave apart whose image columns are equal
    in exact arithmetic (6 a' = 5 b') and right - left = `want` ulps in float32."""
    for l in range(0, NLEVELS - 1):
        for m in range(4, 40):
            a, bb = 6 * m, 5 * m
            if not (g.legal(l, a, 30) and g.legal(l + 1, bb, 30)):
                continue
            for left, right in (((l, a), (l + 1, bb)), ((l + 1, bb), (l, a))):
                x, z = F32(left[1]) * g.scale[left[0]], F32(right[1]) * g.scale[right[0]]
                if int(z.view(np.int32)) - int(x.view(np.int32)) == want:
                    return left + right
    raise AssertionError("no float32 column pair found")


def _row_on(g, l, row):
    """A legal y on level l whose image row (int)(y scale) is `row`."""
    for y in range(EDGE, g.sizes[l][1] - EDGE):
        if int(F32(y) * g.scale[l]) == row:
            return y
    return None


def max_u_case(name, ulps, want_filtered):
    """uR against maxU = uL: a left key on level l and a right key one octave up whose columns are equal in
    exact arithmetic and `ulps` apart in float32."""
    g = SMALL
    ll, a, lr, bb = _ulp_pairs(g, ulps)
    b = Build(name)
    d = b.desc()
    yr = 30
    row = int(F32(yr) * g.scale[lr])
    yl = _row_on(g, ll, row) or _row_on(g, ll, row + 1)
    b.add("L", ll, a, yl, d)
    b.add("R", lr, bb, yr, b.flip(d, 2))

    def pre(c, ref):
        kl, _, kr, _ = c.keys()
        kt = ref["def"][3].keys[0]
        diff = int(kr["x"].view(np.int32)[0]) - int(kl["x"].view(np.int32)[0])
        assert diff == ulps and kt.ncand == 1 and kt.nfiltered == want_filtered, (diff, kt.ncand, kt.nfiltered)
    return case(name, b, pre)


def min_u_case(name, which):
    """uR against minU = uL - maxD, maxD = fx exactly (bf = fx, mb = 1): fx = uL - uR is exact, so uR == minU;
    one ulp more (less) of fx moves minU above (below) uR."""
    b = Build(name)
    d = b.desc()
    b.add("L", 0, 200, 80, d)    # 90 and 110 share a binade, so 200 - fx is exact for fx one ulp off 90 too
    b.add("R", 0, 110, 80, b.flip(d, 2))
    fx = {"equal": F32(90.0), "above": np.nextafter(F32(90.0), F32(0)), "below": np.nextafter(F32(90.0), F32(180))}[which]

    def pre(c, ref):
        kt = ref["def"][3].keys[0]
        max_d, mb = sd.search_bounds(c.bf, c.fx)
        assert mb == 1 and max_d == F32(c.fx)
        min_u, u_r = F32(F32(200.0) - max_d), F32(110.0)
        if which == "equal":
            assert min_u == u_r and kt.nfiltered == 1
        elif which == "above":   # the smallest float above uR
            assert min_u == np.nextafter(u_r, F32(np.inf)) and kt.nfiltered == 0 and kt.outcome == "no-filtered"
        else:
            assert min_u == np.nextafter(u_r, F32(-np.inf)) and kt.nfiltered == 1
    return case(name, b, pre, bf=float(fx), fx=float(fx))


def candidates_none():
    b = Build("none")
    b.pair(0, 150, 60, SHIFT, 2, dy=3)    # band 61 .. 65 of the right key misses row 60
    b.pair(0, 150, 120, SHIFT, 2, dy=-3)
    return case("candidates-none", b, pre_outcomes("no-candidates", "no-candidates"))


def candidates_all_filtered():
    b = Build("filtered")
    d = b.desc()
    b.add("L", 0, 150, 60, d)
    b.add("R", 0, 151, 60, b.flip(d, 1))      # uR > uL
    b.add("R", 0, 150 - 65, 61, b.flip(d, 1))  # uR < uL - maxD (64)
    b.add("R", 2, 100, 42, b.flip(d, 1))      # octave + 2, row band 57.6 .. 63.4
    b.add("L", 7, 40, 30, d)                  # uL 143.3: a level-7 key with level-0 .. 5 candidates only
    b.add("R", 5, 50, 43, b.flip(d, 1))

    def pre(c, ref):
        k0, k1 = ref["def"][3].keys
        assert k0.ncand == 3 and k0.nfiltered == 0 and k1.ncand >= 1 and k1.nfiltered == 0
        assert outcomes(ref["def"][3]) == ["no-filtered"] * 2
    return case("candidates-all-filtered", b, pre)


def band_edge(levels=(0, 3, 7), g=SMALL, name="band-edge"):
    """Per level one right key; left keys of the levels around it on the first and last row of its band and
    on the rows just outside."""
    b = Build(name, g)
    plan = []
    for l in levels:
        w, h = g.sizes[l]
        found = None
        def reach(row):
            for ll in (l, l - 1, l + 1):
                if 0 <= ll < NLEVELS:
                    yl = _row_on(g, ll, row)
                    if yl is not None:
                        return ll, yl
            return None
        for yr in range(EDGE, h - EDGE):
            lo, hi = sd.band(F32(yr) * g.scale[l], l, g.scale)
            # the rows just outside: the nearest ones that a legal left key of these levels can lie on
            below = next((r for r in (lo - 1, lo - 2, lo - 3) if reach(r)), None)
            above = next((r for r in (hi + 1, hi + 2, hi + 3) if reach(r)), None)
            if below is not None and above is not None and reach(lo) and reach(hi):
                found = (yr, lo, hi, {r: reach(r) for r in (below, lo, hi, above)})
                break
        assert found, f"no band-edge rows on level {l}"
        yr, lo, hi, rows = found
        xr = (w // 2)
        d = b.desc()
        i_r = b.add("R", l, xr, yr, d)
        u_r = F32(xr) * g.scale[l]
        for k, row in enumerate(sorted(rows)):
            ll, yl = rows[row]
            xl = int(np.ceil(float(u_r + F32(SHIFT) + F32(3 * k)) / float(g.scale[ll])))   # distinct, right of uR
            b.add("L", ll, xl, yl, b.flip(d, 1 + k))
            plan.append((l, row, row in (lo, hi), i_r))

    def pre(c, ref):
        tr = ref["def"][3]
        kr = c.keys()[2]
        for kt, (l, row, inside, i_r) in zip(tr.keys, plan):
            own = sd.band(kr["y"][i_r], l, c.g.scale)
            assert kt.row == row and (own[0] <= row <= own[1]) == inside
            if inside:
                assert kt.nfiltered >= 1 and kt.best_idx == i_r, (l, row, kt.ncand, kt.nfiltered, kt.best_idx)
            else:
                assert kt.best_idx != i_r
    return case(name, b, pre, pair="tall" if g is TALL else "tex")


ST_ROFF = 32   # orbfe_kernels.hip: the row-start table of k_stereo covers rows -ST_ROFF .. height + ST_ROFF


def row_table_fallback():
    """k_stereo reads the scan bounds of a left key from its row-start table only when
    row - maxspan >= -ST_ROFF, else it binary-searches the sorted keys (`!tab`). maxspan is the widest band
    of ANY right key of the frame: one level-4 key of the COARSE pyramid (scale 16, band of 64 rows) puts
    every left key on rows 19 .. 31 on the binary search, rows 32 and 33 stay on the table. One left key
    per row 19 .. 33 with its match 2 rows below, on or 2 rows above it; 70 right keys on rows 19 and 20
    put the match of row 21 into the second 64-stride trip; two ties on the best distance on fallback rows,
    the first-planted candidate the true match in one and the decoy in the other."""
    g = COARSE
    b = Build("row-table-fallback", g)
    wide = b.add("R", 4, 30, 30)            # (480, 480): band 448 .. 512
    fill = b.fill_right(70, [19, 20], x0=EDGE + 1)
    rows = list(range(19, 34))
    match = {}
    for r in rows:
        dy = 2 if r in (19, 21) else (0, -2, 2)[(r - 20) % 3]
        i_l, i_r = b.pair(0, 300 + 40 * (r - 19), r, SHIFT, 3, dy=dy)
        match[i_l] = i_r
    ties = []
    for x, r, true_first in ((940, 24, True), (1000, 28, False)):
        d = b.desc()
        i_l = b.add("L", 0, x, r, d)
        order = [(x - SHIFT, r + 1), (x - 75, r - 1)]
        if not true_first:
            order.reverse()
        ties.append((i_l, *[b.add("R", 0, px, py, b.flip(d, 6)) for px, py in order]))
    far = b.fill_right(40, [60, 61], x0=EDGE + 1)   # records past every left row: the upper bound is inside the list

    def pre(c, ref):
        tr, alt = ref["def"][3], ref["def-tie-last"]
        kl, _, kr, _ = c.keys()
        bands, maxspan = bands_of(c)
        assert maxspan == bands[wide][1] - bands[wide][0] == 64 > EDGE + ST_ROFF
        assert min(lo for lo, _ in bands) >= -ST_ROFF      # no bin of the counting sort is clamped
        fallback = [i for i in range(len(kl)) if int(kl["y"][i]) - maxspan < -ST_ROFF]
        table = [i for i in range(len(kl)) if i not in fallback]
        assert sorted({tr.keys[i].row for i in fallback}) == list(range(19, 32)) and sorted({tr.keys[i].row for i in table}) == [32, 33]
        for i in range(len(kl)):
            kt = tr.keys[i]
            # the bounds either path must give: jlo = 0 (no band starts below row - maxspan), jhi = the
            # number of bands that start on or above the key's row, inside the list
            assert sum(1 for lo, _ in bands if lo < kt.row - maxspan) == 0
            jhi = sum(1 for lo, _ in bands if lo <= kt.row)
            assert kt.ncand >= 1 and kt.ncand <= jhi < len(kr) - len(far), (i, kt.row, kt.ncand, jhi)
            if i in match:   # (a tie won by its decoy goes on to a window search that finds no minimum)
                assert kt.best_idx == match[i] and kt.outcome in ("accepted", "cut"), (i, kt.row, kt.outcome)
        assert sum(tr.keys[i].outcome == "accepted" for i in fallback) >= 10
        i21 = next(i for i in match if tr.keys[i].row == 21)
        assert trips_of(c, i21, match[i21])[0] == 1
        for i_l, first, second in ties:
            assert i_l in fallback and tr.keys[i_l].nties == 2 and tr.keys[i_l].best_idx == first < second
            assert ref["def"][0][i_l] != alt[0][i_l]
    return case("row-table-fallback", b, pre, pair="coarse", fx=100.0, bf=50.0, tie_last=True)


# ---- cases: SAD search on the patch pair ---------------------------------------------------------
def patch_case(name, patches, pre, flips=2, **kw):
    images("patch")
    b = Build(name)
    for p in patches:
        cx, cy, dsp = PATCH_AT[p]
        b.pair(0, cx, cy, dsp, flips)
    return case(name, b, pre, pair="patch", **kw)


def pre_sads(outcome, **want):
    def pre(c, ref):
        kt = ref["def"][3].keys[0]
        assert kt.outcome == outcome, f"{c.name}: {kt.outcome} {kt.sads} {kt.bestinc} {kt.delta}"
        for k, v in want.items():
            got = getattr(kt, k)
            assert (v(got) if callable(v) else got == v), f"{c.name}: {k} = {got} ({kt.sads})"
    return pre


def sad_cases():
    pad = ["s100#15"]   # a second accepted match keeps the median above zero
    out = [
        patch_case("sad-tie-first-shift", ["tie-3-7"] + pad, pre_sads(
            "accepted", bestinc=-2, sads=lambda s: s[3] == s[7] == min(s) and sorted(s)[1] == min(s))),
        patch_case("sad-min-at-minus5", ["min-at--5"] + pad, pre_sads("inc-at-end", bestinc=-5)),
        patch_case("sad-min-at-plus5", ["min-at-+5"] + pad, pre_sads("inc-at-end", bestinc=5)),
        patch_case("sad-flat", ["flat"] + pad, pre_sads("inc-at-end", bestinc=-5, sads=[0] * 11)),
        patch_case("delta-zero", ["delta-0"] + pad, pre_sads("accepted", bestinc=0, delta=F32(0))),
        patch_case("delta-plus-half", ["delta-+half"] + pad, pre_sads(
            "accepted", bestinc=0, delta=F32(0.5), sads=lambda s: s[5] == s[6] == U and s[4] == 2 * U)),
        # -0.5 itself needs d1 == d2, which the first strict minimum excludes: d1 = d2 + 1 is the closest
        patch_case("delta-minus-half", ["delta--half"] + pad, pre_sads(
            "accepted", bestinc=0, sads=lambda s: s[4] == s[5] + 1, delta=lambda v: F32(-0.5) < v < F32(-0.49))),
        patch_case("disparity-zero-clamped", ["disp-0"] + pad, pre_sads("clamped", bestinc=0, delta=F32(0))),
        patch_case("disparity-zero-from-above", ["disp-0-pos"] + pad, pre_sads("accepted", delta=lambda v: v < 0)),
        patch_case("disparity-negative", ["disp-0-neg"] + pad, pre_sads("disparity-out", delta=lambda v: v > 0)),
        patch_case("disparity-just-below-maxD", ["disp-32-below"] + pad, pre_sads("accepted", delta=lambda v: v > 0),
                   bf=16.0, fx=32.0),
        patch_case("disparity-at-maxD", ["disp-32"] + pad, pre_sads("disparity-out", delta=F32(0)), bf=16.0, fx=32.0),
        patch_case("disparity-just-above-maxD", ["disp-32-above"] + pad, pre_sads("disparity-out", delta=lambda v: v < 0),
                   bf=16.0, fx=32.0),
    ]
    return out


def window_alignment(layout=None, name="window-alignment"):
    """Left and right window start columns on all four byte alignments, on level 0 and on level 2, over
    consecutive rows."""
    b = Build(name)
    for l, dx in ((0, SHIFT), (2, 6)):
        n = 0
        for i in range(4):
            for j in range(4):
                x = 60 + 4 * (n % 8) * 4 + i
                y = 40 + 7 * n
                n += 1
                if b.g.legal(l, x, y) and b.g.legal(l, x - dx - j, y):
                    d = b.desc()
                    b.add("L", l, x, y, d)
                    b.add("R", l, x - dx - j, y, b.flip(d, 3))

    def pre(c, ref):
        tr = ref["def"][3]
        for l in (0, 2):
            got = {(k.window[2] & 3, k.window[3] & 3) for k in tr.keys if k.window and k.window[0] == l}
            assert len(got) == 16, f"{c.name}: level {l} reaches {len(got)} of 16 alignment pairs"
        assert sum(o == "accepted" for o in outcomes(tr)) >= 12
    return case(name, b, pre, layout=layout)


def edge_reject():
    """OUTSIDE the extractor's domain: a right key on column -3. With a legal left key every legal right
    candidate has uR <= uL, hence endu <= w_l - 9; only a negative column reaches the rejection."""
    b = Build("edge")
    d = b.desc()
    b.add("L", 0, 40, 60, d)
    b.add_raw("R", -3.0, 60.0, 0, b.flip(d, 2))
    b.pair(0, 150, 100, SHIFT, 2)
    return case("edge-reject", b, pre_outcomes("window-out", "accepted"),
                outside="right key 0 has column -3: rejected by iniu < 0 before any pixel is read")


# ---- cases: the median cut -----------------------------------------------------------------------
def median_case(name, sads, median, cut, th=None):
    """Matches with the given winning sums (pool entries); the median and the sums cut are asserted."""
    pool = {}
    for i, v in enumerate(SAD_POOL):
        pool.setdefault(v, []).append(f"s{v}#{i}")
    names = [pool[v].pop(0) for v in sads]

    def pre(c, ref):
        tr = ref["def"][3]
        assert [k.sad for k in tr.keys] == list(sads), [k.sad for k in tr.keys]
        assert tr.n == len(sads) and tr.median == F32(median), (tr.n, tr.median)
        assert sorted(k.sad for k in tr.keys if k.outcome == "cut") == sorted(cut), (tr.th_dist, outcomes(tr))
        if th is not None:
            assert tr.th_dist == F32(th)
    return patch_case(name, names, pre)


def median_cases():
    return [
        median_case("median-zero", [0, 0, 0, 100, 0, 300], 0, [0, 0, 0, 0, 100, 300], th=0),
        median_case("n-1", [100], 100, []),
        median_case("n-1-zero", [0], 0, [0]),
        median_case("n-2", [100, 255], 255, []),               # index 1 of 2: the larger
        median_case("n-2-zero", [0, 0], 0, [0, 0]),
        median_case("n-even", [10, 20, 50, 100], 50, []),      # index 2 of 4
        median_case("n-even-cut", [10, 20, 21, 50], 21, [50]),
        median_case("n-odd", [100, 10, 300, 20, 50], 50, [300]),
        # 255 is the last entry of high-byte bin 0, 256 the first of bin 1
        # (thDist 535.5 against 537.6: the sums 536 and 537 tell the two medians apart)
        median_case("median-bin-last", [100, 255, 255, 535, 536], 255, [536]),
        median_case("median-bin-first", [100, 255, 256, 537, 538], 256, [538]),
        median_case("median-bin-first-alone", [254, 255, 256, 257, 600], 256, [600]),
        # thDist = fl(fl(1.5f 1.4f) 10) = 21 exactly, rounded up from 20.999999: 20 stays, 21 goes (equality is a cut)
        median_case("cut-boundary", [3, 10, 10, 10, 20, 21, 22], 10, [21, 22], th=21),
        # fl(fl(1.5f 1.4f) 100) = 209.99998: 209 stays, 210 goes
        median_case("cut-boundary-below-integer", [99, 100, 100, 100, 209, 210, 211], 100, [210, 211], th=209.99998),
        median_case("all-equal-distances", [100, 100, 100], 100, []),
    ]


# ---- cases: counts -------------------------------------------------------------------------------
def generic_keys(b, n, nr=None, levels=range(NLEVELS)):
    """n distinct left keys over the levels with a right key 8 px to the left (where legal), 0-7 bits apart."""
    g, seen = b.g, set()
    while len(b.k["L"]) < n:
        l = int(b.rng.choice(list(levels)))
        w, h = g.sizes[l]
        x, y = int(b.rng.integers(EDGE, w - EDGE)), int(b.rng.integers(EDGE, h - EDGE))
        if (l, x, y) in seen:
            continue
        seen.add((l, x, y))
        d = b.desc()
        b.add("L", l, x, y, d)
        xr = x - int(round(SHIFT / float(g.scale[l])))
        if g.legal(l, xr, y) and (nr is None or len(b.k["R"]) < nr):
            b.add("R", l, xr, y, b.flip(d, int(b.rng.integers(0, 8))))


def count_case(n, nr=None, name=None):
    b = Build(name or f"N-{n}")
    generic_keys(b, n, nr)
    if nr is not None and len(b.k["R"]) < nr:   # top up with level-0 keys
        have, i = set(b.lv["R"]), 0
        while len(b.k["R"]) < nr:
            lv = (0, EDGE + i % 280, 150 + i // 280)
            i += 1
            if lv not in have:
                b.add("R", *lv)

    def pre(c, ref):
        kl, _, kr, _ = c.keys()
        assert len(kl) == n and (nr is None or len(kr) == nr)
        if n >= 15 and (nr is None or nr >= 15):
            assert ref["def"][2] >= n // 4, f"{c.name}: only {ref['def'][2]} matches"
    return case(name or f"N-{n}", b, pre)


def skewed_work():
    """The first 16 left keys see 130 candidates each, the other 240 none."""
    b = Build("skew")
    fill = b.fill_right(130, [100, 101], x0=EDGE + 1)
    for i in range(16):
        src = fill[3 + 8 * i]
        l, x, y = b.lv["R"][src]
        b.add("L", 0, x + SHIFT, 100 + i % 2, b.flip(b.d["R"][src], i % 5))
    for i in range(240):
        b.add("L", 0, EDGE + i, 40 + (i % 3))

    def pre(c, ref):
        tr = ref["def"][3]
        assert all(k.ncand == 130 for k in tr.keys[:16]) and all(k.ncand == 0 for k in tr.keys[16:])
        assert sum(o in ("accepted", "cut") for o in outcomes(tr)[:16]) >= 12
    return case("skewed-work", b, pre)


# ---- the case list -------------------------------------------------------------------------------
_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = [
            row_candidates(65), row_candidates(130), tie_case(),
            dist_case("dist-74", [74, 3], ["accepted", "accepted"]), dist_case("dist-75", [75, 3], ["dist>=75", "accepted"]),
            dist_case("dist-99-100", [99, 100, 3], ["dist>=75", "dist>=75", "accepted"]),
            octave_case("octave-minus-1", 2, 66, 60, 1), octave_case("octave-plus-1", 4, 46, 42, 1),
            octave_case("octave-plus-2", 5, 38, 35, 0),
            max_u_case("uR-equals-maxU", 0, 1), max_u_case("uR-one-ulp-above-maxU", 1, 0),
            max_u_case("uR-one-ulp-below-maxU", -1, 1),
            min_u_case("uR-equals-minU", "equal"), min_u_case("uR-one-ulp-below-minU", "above"),
            min_u_case("uR-one-ulp-above-minU", "below"),
            candidates_none(), candidates_all_filtered(), band_edge(),
        ] + sad_cases() + [
            window_alignment(), window_alignment(layout=(13, 3), name="level0-odd-pitch"), edge_reject(),
        ] + median_cases() + [count_case(n) for n in (0, 1, 15, 16, 17, 512, 513, 1025)] + [
            count_case(40, 0, "Nr-0"), count_case(40, 1, "Nr-1"), count_case(300, CAP[SMALL] - 1, "Nr-cap-minus-1"),
            skewed_work(),
        ]
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


_TALL = None


def tall_cases():
    """The tall pair (1152 x 2048): right counts of a power of two plus one, a power of two, and one."""
    global _TALL
    if _TALL is None:
        _TALL = [row_candidates(130, TALL, pad_to=257), tie_case(TALL, pad_to=128), band_edge((0,), TALL, "band-edge-tall")]
    return _TALL


_COARSE = None


def coarse_cases():
    """The COARSE pair (1168 x 1168, 5 levels at 2.0): the binary-search fallback of the row table."""
    global _COARSE
    if _COARSE is None:
        _COARSE = [row_table_fallback()]
    return _COARSE


def fillers(pair):
    """Frames for the spare slots of a batch: one without left keys, one without right keys."""
    out = []
    for name, n, nr in (("filler-N-0", 0, 20), ("filler-Nr-0", 40, 0)):
        b = Build(name)
        generic_keys(b, 40, nr)
        if n == 0:
            b.k["L"], b.d["L"], b.lv["L"] = [], [], []
        out.append(case(f"{name}-{pair}", b, lambda c, ref: None, pair=pair))
    return out
