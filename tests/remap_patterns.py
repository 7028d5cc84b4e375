"""Planted inputs for the rectification kernels (k_remap, k_undistort): every builder of PATTERNS
returns (src, mapx, mapy, note) with a source of at most 64 x 48 and an output of at most 64 x 32,
built from seeds. PRE holds, per pattern, the CPU assertion (through
oracle/remap_definition.classify_groups, the kernel's fast-path rule as its comment states it)
that the inputs reach what the pattern is named for; sweep_coverage() counts what the window sweep
reaches as a whole. Nothing here predicts a byte: expected pixels come from remap_linear_def.

Source bytes are random with planted runs of 0 and 255, so a wrong or swapped weight shows.
"""
import numpy as np

from oracle import remap_definition as rd

SW, SH = 64, 48
FRACTIONS = (0, 1, 16, 31)


def up4(v):
    return (v + 3) // 4 * 4


def source(seed, sw=SW, sh=SH):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    for i in range(max(4, sh // 2)):   # horizontal and vertical runs of 0 and 255
        y, x, n = int(rng.integers(0, sh)), int(rng.integers(0, sw)), int(rng.integers(2, 9))
        if i % 3 == 2:
            s[y:y + n, x] = 255 * (i & 1)
        else:
            s[y, x:x + n] = 255 * (i & 1)
    return s


def variant(src, k):
    """Image k of a batch: distinct bytes, the same size."""
    return src if k == 0 else np.ascontiguousarray(np.roll(src, (k, 2 * k + 1), (0, 1)) ^ np.uint8(17 * k))


def _affine(dw, dh, a, s, b, t, cxy=0.0, cyx=0.0):
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    return (a + s * x + cxy * y).astype(np.float32), (b + t * y + cyx * x).astype(np.float32)


# ---- window sweep -------------------------------------------------------------------------------
SWEEP_SCALES = (0.25, 0.5, 1.0, 1.5, 2.0, 2.25, 2.34)
SWEEP_T = (0.5, 1.0, 1.5, 2.25)


def window_sweep(s, phase):
    """mx = a + s x, my = b + t y. For s < 1 the map ends across the right edge (four pixels share
    a column pair there: the window runs past sw with every sample inside); for s >= 1 it starts at
    column `phase` and runs off the right edge. At s = 2 the group's last pair sits at
    d = (off_0 & 3) + 6; at 2.25 and 2.34 the fraction decides between 6 and 7 group by group."""
    dw = 64 if s <= 1 else min(64, up4(int(SW / s) + 3))
    a = (SW - s * dw + phase - 1.7) if s < 1 else phase + 0.3
    mx, my = _affine(dw, 16, a, s, 0.4 + phase, SWEEP_T[phase])
    return source(100 + phase), mx, my, f"window sweep s = {s}, a = {a:g}"


def mirrored(phase):
    """s = -1: the pairs run right to left, d < 0 unless off_0 & 3 == 3 (then d = 3, 2, 1, 0: fast)."""
    mx, my = _affine(64, 16, 60.3 + phase, -1.0, 1.6 + phase, 1.0)
    return source(110 + phase), mx, my, f"mirrored, a = {60.3 + phase:g}"


def rotated(sign):
    """A rotation by 0.09 rad: pixel 3 of some groups samples the next (sign > 0: d > 6) or the
    previous (sign < 0: d < 0) source row."""
    c, s = np.cos(0.09), sign * np.sin(0.09)
    y, x = np.mgrid[0:24, 0:48].astype(np.float64)
    mx = 6.3 + c * x - s * y
    my = (3.2 if sign > 0 else 9.2) + s * x + c * y
    return source(120 + (sign > 0)), mx.astype(np.float32), my.astype(np.float32), f"rotated {sign:+d}"


SWEEP = {f"sweep-s{s}-p{p}": (lambda s=s, p=p: window_sweep(s, p)) for s in SWEEP_SCALES for p in range(4)}
SWEEP.update({f"mirrored-p{p}": (lambda p=p: mirrored(p)) for p in range(4)})
SWEEP.update({"rotated+": lambda: rotated(1), "rotated-": lambda: rotated(-1)})


def sweep_coverage():
    """Over the whole sweep (sources 4-byte aligned, pitch = 64): fast groups per off_0 & 3, fast
    groups whose largest d is exactly 6, and groups per failing clause."""
    fast, d6, fail = [0] * 4, 0, {}
    for build in SWEEP.values():
        src, mx, my, _ = build()
        for row in rd.classify_groups(src.shape[1], src.shape[0], up4(src.shape[1]), mx, my, True):
            for g in row:
                if g.verdict == rd.FAST:
                    fast[g.phase] += 1
                    d6 += g.dmax == 6
                else:
                    fail[g.verdict] = fail.get(g.verdict, 0) + 1
    return fast, d6, fail


def _groups(src, mx, my, pitch=None, aligned=True):
    sh, sw = src.shape
    return rd.classify_groups(sw, sh, up4(sw) if pitch is None else pitch, mx, my, aligned)


def _flat(rows):
    return [g for row in rows for g in row]


def pre_sweep(src, mx, my):
    v = {g.verdict for g in _flat(_groups(src, mx, my))}
    assert rd.FAST in v or rd.D_BIG in v or rd.D_NEG in v, v


def pre_mirrored(src, mx, my):
    g = _flat(_groups(src, mx, my))
    phase = {rd.fixed_point(mx[0, 0])[0] & 3}
    if phase == {3}:
        assert sum(k.verdict == rd.FAST and k.dmax == 3 for k in g) >= 10
    else:
        assert sum(k.verdict == rd.D_NEG for k in g) >= 10


def pre_rotated(src, mx, my):
    g = _flat(_groups(src, mx, my))
    want = rd.D_BIG if my[0, 47] > my[0, 0] else rd.D_NEG
    # the row change, not the column step, is what fails: the columns of a group span 4 at most
    far = [k for k in g if k.verdict == want and (k.dmax > 32 or want == rd.D_NEG)]
    assert len(far) >= 10 and sum(k.verdict == rd.FAST for k in g) >= 10


# ---- right edge ---------------------------------------------------------------------------------
EDGE_WIDTHS = (8, 9, 10, 11, 12, 13, 16, 17)
EDGE_OVER = {8: 0, 9: 3, 10: 2, 11: 1, 12: 0, 13: 3, 16: 0, 17: 3}   # base + 8 - sw at s = 1, sx_0 = sw - 5


def right_edge(sw):
    """dw = 8. Rows 0-3 (s = 1): the last group's first column is sw - 5 - (y % 4), its last sample
    column sw - 1 at most. Rows 4-7 (s = 0.5): four pixels over columns sw - 4 - (y % 4) and the
    next one. Every sample of those groups is inside; the 8-byte window ends at sw or up to 4 past."""
    sh, dw, dh = 6, 8, 8
    y, x = np.mgrid[0:dh, 0:dw].astype(np.float64)
    k = y % 4
    mx = np.where(y < 4, sw - 9 - k + 0.4 + x, sw - 5.6 - k + 0.5 * x)
    my = 0.5 + 0.5 * y
    return source(200 + sw, sw, sh), mx.astype(np.float32), my.astype(np.float32), f"right edge sw = {sw}"


def pre_right_edge(src, mx, my):
    sw = src.shape[1]
    rows = _groups(src, mx, my)
    last = [row[1] for row in rows]
    assert all(g.verdict in (rd.FAST, rd.WINDOW) for g in last), [g.verdict for g in last]   # every sample inside
    e = EDGE_OVER[sw]
    assert last[0].over == e and last[0].verdict == (rd.WINDOW if e else rd.FAST), last[0]
    assert any(g.verdict == rd.WINDOW for g in last)
    assert {g.over for g in last if g.verdict == rd.WINDOW} <= {1, 2, 3, 4}


# ---- bottom edge --------------------------------------------------------------------------------
def bottom_edge():
    """Output row y samples source row sh - 4 + y: row 2 has its second row on the last source row
    (fast), row 3 has S10 and S11 outside (guarded), rows 4 and 5 are below the source."""
    sw, sh = 24, 10
    mx, my = _affine(16, 6, 1.6, 1.0, sh - 4 + 0.37, 1.0)
    return source(300, sw, sh), mx, my, "bottom edge"


def pre_bottom_edge(src, mx, my):
    sh = src.shape[0]
    rows = _groups(src, mx, my)
    assert [rd.fixed_point(my[y, 0])[0] for y in range(6)] == [sh - 4, sh - 3, sh - 2, sh - 1, sh, sh + 1]
    assert all(g.verdict == rd.FAST for g in rows[2]) and all(g.verdict == rd.OUTSIDE for g in rows[3])


# ---- border ring --------------------------------------------------------------------------------
RING_SW, RING_SH = 12, 10
RING_POS = [(px, py) for py in (-1, 0, 1) for px in (-1, 0, 1)] + [(-2, 0), (2, 2)]   # 2 / -2: wholly outside


def _ring_coord(p, size):
    return {-2: -2, -1: -1, 0: 3, 1: size - 1, 2: size}[p]


def border_ring():
    """An all-255 source. Row r puts pixels 2-3 of every group at position RING_POS[r] (left / inside
    / right x above / inside / below, then two positions wholly outside) and pixels 0-1 inside at
    (3, 3); group 4 iy + ix carries the fractions (FRACTIONS[ix], FRACTIONS[iy]) / 32."""
    dh, dw = len(RING_POS), 64
    mx, my = np.zeros((dh, dw)), np.zeros((dh, dw))
    for r, (px, py) in enumerate(RING_POS):
        for g in range(16):
            fx, fy = FRACTIONS[g % 4] / 32, FRACTIONS[g // 4] / 32
            mx[r, 4 * g:4 * g + 2], my[r, 4 * g:4 * g + 2] = 3 + fx, 3 + fy
            mx[r, 4 * g + 2:4 * g + 4] = _ring_coord(px, RING_SW) + fx
            my[r, 4 * g + 2:4 * g + 4] = _ring_coord(py, RING_SH) + fy
    return np.full((RING_SH, RING_SW), 255, np.uint8), mx.astype(np.float32), my.astype(np.float32), "border ring"


def ring_closed_form(mx, my):
    """(255 * inside_weight_sum + 2**14) >> 15 per pixel, the weights written out here."""
    out = np.zeros(mx.shape, np.uint8)
    for y in range(mx.shape[0]):
        for x in range(mx.shape[1]):
            (sx, fx), (sy, fy) = rd.fixed_point(mx[y, x]), rd.fixed_point(my[y, x])
            wx = [(32 - fx) * (0 <= sx < RING_SW), fx * (0 <= sx + 1 < RING_SW)]
            wy = [(32 - fy) * (0 <= sy < RING_SH), fy * (0 <= sy + 1 < RING_SH)]
            out[y, x] = (255 * 32 * (wx[0] + wx[1]) * (wy[0] + wy[1]) + 2 ** 14) >> 15
    return out


def pre_border_ring(src, mx, my):
    rows = _groups(src, mx, my)
    for r, (px, py) in enumerate(RING_POS):
        want = rd.FAST if (px, py) == (0, 0) else rd.OUTSIDE
        assert all(g.verdict == want for g in rows[r]), (r, px, py)
    cf = ring_closed_form(mx, my)
    assert (cf[4] == 255).all() and (cf[-2:, 2::4] == 0).all() and len(np.unique(cf)) >= 8


# ---- rounding -----------------------------------------------------------------------------------
def _ticks(ks, js):
    return [k + (2 * j + 1) / 64 for k in ks for j in js]


AROUND = [-1 - 1 / 64, -1.0, -1 + 1 / 64, -1 / 64, 0.0]
# float32 holds 1/64 up to 2**17 and 1/32 up to 2**18: the first two coordinates are rounded when
# they become float32 (the product with 32 itself is a scaling by a power of two: always exact),
# the third is an exact half tick at X = 2**22. All three clamp to sx = 32767: outside, 0.
LARGE = [2.0 ** 18 + 33 / 64, -(2.0 ** 18) + 31 / 64, 2.0 ** 17 + 1 / 64, -(2.0 ** 17) - 3 / 64]


def rounding():
    """Coordinates k + (2 j + 1) / 64: exactly half a fixed-point tick (half goes to even, >> floors),
    k negative and positive, on x across the columns and on y down the rows."""
    xs = _ticks((-2, -1, 0, 1, 7, 30, 62), (0, 1, 15, 16, 30, 31)) + AROUND + LARGE + [5.25]
    ys = _ticks((-1, 0, 3, 46), (0, 15, 16, 31)) + AROUND + LARGE[:3]
    assert len(xs) == 52 and len(ys) == 24
    mx = np.broadcast_to(np.array(xs, np.float32)[None, :], (len(ys), len(xs))).copy()
    my = np.broadcast_to(np.array(ys, np.float32)[:, None], (len(ys), len(xs))).copy()
    return source(400), mx, my, "rounding"


def pre_rounding(src, mx, my):
    halves = [float(v) * 32 for v in mx[0, :42]] + [float(v) * 32 for v in my[:16, 0]]
    assert all(h - np.floor(h) == 0.5 for h in halves)
    assert sum(rd.sat_int(v) % 2 == 0 for v in mx[0, :42]) == 42    # every half went to the even tick
    assert [rd.sat_int(v) for v in AROUND] == [-32, -32, -32, 0, 0]   # -32.5 -> -32, -31.5 -> -32, -0.5 -> 0
    assert rd.fixed_point(-1 / 64) == (0, 0) and rd.fixed_point(-3 / 64) == (-1, 30)
    assert float(np.float32(LARGE[0])) != LARGE[0] and float(np.float32(LARGE[2])) == LARGE[2]
    assert rd.fixed_point(LARGE[0])[0] == 32767 and rd.fixed_point(LARGE[1])[0] == -32768


# ---- saturation ---------------------------------------------------------------------------------
SPECIALS = [1e9, -1e9, 3e38, -3e38, float("inf"), float("-inf"), 2.0 ** 26, -(2.0 ** 26), float("nan")]


def saturation():
    """Every special planted on x, on y and on both (NaN also against +-inf), one per group, at lane
    group % 4, among ordinary pixels. Source column 0 and row 0 are 255: a NaN converted to 0
    instead of INT_MIN would sample them."""
    src = source(500, 24, 16)
    src[0, :] = 255
    src[:, 0] = 255
    mx, my = _affine(16, 8, 2.3, 1.0, 2.6, 1.0)
    nan, inf = float("nan"), float("inf")
    plants = ([(v, None) for v in SPECIALS] + [(None, v) for v in SPECIALS] + [(v, v) for v in SPECIALS] +
              [(nan, inf), (-inf, nan), (nan, 2.0), (3.0, nan), (0.0, nan)])
    assert len(plants) == 32
    with np.errstate(all="ignore"):
        for g, (vx, vy) in enumerate(plants):
            y, x = g // 4, 4 * (g % 4) + g % 4
            if vx is not None:
                mx[y, x] = vx
            if vy is not None:
                my[y, x] = vy
    return src, mx, my, "saturation"


def pre_saturation(src, mx, my):
    bad = ~(np.isfinite(mx) & np.isfinite(my)) | (np.abs(mx) > 1e6) | (np.abs(my) > 1e6)
    assert bad.sum() == 32 and (bad.reshape(8, 4, 4).sum(2) == 1).all()      # one per group
    assert {int(v) for v in np.argwhere(bad)[:, 1] % 4} == {0, 1, 2, 3}
    for v in SPECIALS:
        assert rd.fixed_point(v)[0] == -32768   # INT_MIN >> 5, clamped
    assert rd.sat_int(2.0 ** 26 - 4) == 2 ** 31 - 128 and rd.sat_int(-(2.0 ** 26)) == rd.INT_MIN


# ---- layouts ------------------------------------------------------------------------------------
LAYOUT_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9)
LAYOUT_BATCHES = (1, 7, 8, 9, 17)


def layout(dw):
    """A 20 x 12 source and a dw x 5 output whose groups are fast where whole and aligned."""
    mx, my = _affine(dw, 5, 1.3, 1.0, 0.7, 1.5, cxy=1.25)
    return source(600 + dw, 20, 12), mx, my, f"layout dw = {dw}"


def pre_layout(src, mx, my):
    dw = mx.shape[1]
    g = _flat(_groups(src, mx, my))
    assert sum(k.verdict == rd.PARTIAL for k in g) == (5 if dw % 4 else 0)
    assert sum(k.verdict == rd.FAST for k in g) == 5 * (dw // 4)
    assert all(k.verdict == rd.UNALIGNED for k in _flat(_groups(src, mx, my, pitch=21)) if k.phase is not None)
    assert all(k.verdict == rd.UNALIGNED for k in _flat(_groups(src, mx, my, aligned=False)) if k.phase is not None)


def partial_at_origin(dw):
    """dw < 4: the only group of each row is partial and its pixels sample source row 0, columns
    0-3, where the lanes past dw (map entries read as 0: offset 0) would pass every other clause of
    the fast-path rule. Only the group being partial keeps it off the fast path."""
    mx, my = _affine(dw, 4, 0.3, 1.0, 0.4, 0.15)
    return source(700 + dw, 20, 12), mx, my, f"partial group at the origin, dw = {dw}"


def pre_partial(src, mx, my):
    assert all(g.verdict == rd.PARTIAL for g in _flat(_groups(src, mx, my)))
    pad = np.zeros((mx.shape[0], 4), np.float32)   # the kernel's view: lanes past dw read 0
    px, py = pad.copy(), pad.copy()
    px[:, :mx.shape[1]], py[:, :mx.shape[1]] = mx, my
    assert all(g.verdict == rd.FAST for g in _flat(_groups(src, px, py)))


PATTERNS = dict(SWEEP)
PATTERNS.update({f"partial-origin-dw{dw}": (lambda dw=dw: partial_at_origin(dw)) for dw in (1, 2, 3)})
PATTERNS.update({f"right-edge-sw{sw}": (lambda sw=sw: right_edge(sw)) for sw in EDGE_WIDTHS})
PATTERNS.update({"bottom-edge": bottom_edge, "border-ring": border_ring, "rounding": rounding, "saturation": saturation})
PATTERNS.update({f"layout-dw{dw}": (lambda dw=dw: layout(dw)) for dw in LAYOUT_WIDTHS})


def pre(name):
    for prefix, fn in (("sweep", pre_sweep), ("mirrored", pre_mirrored), ("rotated", pre_rotated),
                       ("right-edge", pre_right_edge), ("bottom-edge", pre_bottom_edge), ("border-ring", pre_border_ring),
                       ("rounding", pre_rounding), ("saturation", pre_saturation), ("layout", pre_layout),
                       ("partial", pre_partial)):
        if name.startswith(prefix):
            return fn
    raise KeyError(name)


_BUILT = {}


def built(name):
    """(src, mapx, mapy, note) of a pattern, built once; read-only arrays."""
    if name not in _BUILT:
        src, mx, my, note = PATTERNS[name]()
        for a in (src, mx, my):
            a.setflags(write=False)
        assert src.shape[0] <= SH and src.shape[1] <= SW and mx.shape[0] <= 32 and mx.shape[1] <= 64, name
        _BUILT[name] = (src, mx, my, note)
    return _BUILT[name]


_EXPECTED = {}


def expected(name, k=0):
    """remap_linear_def of the pattern's batch image k, computed once."""
    if (name, k) not in _EXPECTED:
        src, mx, my, _ = built(name)
        e = rd.remap_linear_def(variant(src, k), mx, my)
        e.setflags(write=False)
        _EXPECTED[name, k] = e
    return _EXPECTED[name, k]


# ---- undistort ----------------------------------------------------------------------------------
UNDIST_K = (458.654, 457.296, 367.215, 248.375)
UNDIST_DIST = {
    0: (),
    4: (-1.5, 0.3, 0.01, -0.02),            # 1 + k1 r2 + k2 r2^2 < 0 for r2 in (0.79, 4.21): the icdist < 0 break
    5: (-0.28, 0.07, 2e-4, 1.8e-5, 0.01),
    8: (0.5, -0.3, 1e-3, -2e-3, 0.1, 0.4, -0.2, 0.05),
    12: (-0.28, 0.07, 2e-4, 1.8e-5, 0.01, 0.02, -0.01, 0.003, 0.004, -0.003, -0.002, 0.005),   # s1..s4 non-zero
}
UNDIST_COUNTS = (1, 255, 256, 257)


def undistort_points():
    """257 points (float32): a radial sweep through the normalised radii 0.3 .. 1.3 (under the
    4-coefficient set: no break, a break at an iteration >= 1 just inside r2 = 0.79, a break at
    iteration 0 beyond it), random points, and the special points first and across the 255 / 256
    boundary."""
    rng = np.random.default_rng(7)
    fx, fy, cx, cy = UNDIST_K
    nan, inf = float("nan"), float("inf")
    special = [[cx, cy], [0, 0], [1e6, -1e6], [-1e6, 1e6], [nan, 100.0], [100.0, nan], [inf, 50.0], [60.0, -inf],
               [nan, nan], [751, 479]]
    r = np.linspace(0.3, 1.3, 160)
    ang = rng.uniform(0, 2 * np.pi, 160)
    sweep = np.stack([cx + fx * r * np.cos(ang), cy + fy * r * np.sin(ang)], 1)
    rnd = np.stack([rng.uniform(-20, 772, 87), rng.uniform(-20, 500, 87)], 1)
    pts = np.concatenate([np.array(special[:4]), sweep, rnd, np.array(special[4:])]).astype(np.float32)
    pts[0] = [np.float32(cx), np.float32(cy)]
    assert pts.shape == (257, 2)
    pts.setflags(write=False)
    return pts
