"""Seeded adversarial geometries and images for ComputePyramid's three builders, and the CPU
preconditions that prove each case reaches the branch it is named for. Shared by
tests/test_resize_definition.py (CPU) and tests/test_gpu_pyramid_adversarial.py (GPU); nothing here
touches a GPU or the C++ oracle.

A case is a PCase(name, img, scale, nlevels, lanes, branch, pre); pre(case) asserts the case's
precondition from the tables of oracle/resize_definition.py and from this module's own statement
of the host's launch rules:

  tiled resize (k_resize)       tiles of rz_rows x rz_cols output pixels, shrunk from 24 x 128 (rows by
                                1, columns by 4) until every tile's source window fits 32 rows and,
                                from (sx[x0] & ~3) to min(sx[x1 - 1] + 2, sw) rounded up to 16, 176
                                bytes; four vertically adjacent tiles per block
  row-streamed (k_resize_s)     strips of 256 columns x chunks of 48 rows (4 rows below 16 images), 5
                                source rows in flight. Allowed when, in every group of four output
                                columns starting at a multiple of 4, sx - (sx of the first & ~3), less
                                2 for the third and fourth column, lies in [0, 6], and every output
                                row reads rows (s - 1, s), unclipped, for distinct s
  dispatch                      fewer than 16 images and one-launch tiles present: the one-launch
                                pyramid; else per level the row-streamed resize when allowed and (for
                                level 1) the caller's pitch and pointers are multiples of 4; else
                                the tiled resize

Whether the one-launch tiles exist is read from the engine, not restated here (expected_builders
takes it as an argument).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

from oracle import resize_definition as rd

ONE_LAUNCH, ROW_STREAMED, TILED = 1, 2, 3
RZ_TR, RZ_TC, RZ_SR, RZ_SCB, RZ_TPB = 24, 128, 32, 176, 4
RS_COLS, RS_ROWS, RS_ROWS_SMALL, RS_D = 256, 48, 4, 5
SMALL_BATCH = 16
MIN_SIDE = 2 * 16 + 35 + 6     # 2 ORBFE_MINB + ORBFE_CELL + 6: the smallest level side the engine accepts
MAX_W, MAX_H = 640, 225        # no case image is larger


@dataclass
class PCase:
    name: str
    img: np.ndarray
    scale: float
    nlevels: int
    lanes: int
    branch: str
    pre: Callable | None = None
    nfeat: int = 300

    def __repr__(self):
        return self.name

    def tables(self, lanes=None):
        h, w = self.img.shape
        return rd.pyramid_tables(w, h, self.scale, self.nlevels, self.lanes if lanes is None else lanes)

    def sizes(self):
        h, w = self.img.shape
        return rd.level_sizes(w, h, self.scale, self.nlevels)


# ---- the host's rules, restated -----------------------------------------------------------------
def _round_up(v, m):
    return (v + m - 1) // m * m


def rs_columns_ok(t):
    sx, w = t["sx"], t["dw"]
    for xq in range(0, w, 4):
        base = int(sx[xq]) & ~3
        for q in range(min(4, w - xq)):
            off = int(sx[xq + q]) - base - (2 if q >= 2 else 0)
            if off < 0 or off > 6:
                return False
    return True


def rs_rows_ok(t):
    s0, s1 = t["sy0"], t["sy1"]
    return bool((s1 == s0 + 1).all() and (s1[1:] != s1[:-1]).all())


def rs_ok(t):
    return rs_columns_ok(t) and rs_rows_ok(t)


def tile_shape(t):
    """(rz_rows, rz_cols) of the tiled resize."""
    sx, s0, s1, w, h, sw = t["sx"], t["sy0"], t["sy1"], t["dw"], t["dh"], t["sw"]

    def rows_fit(tr):
        return all(int(s1[min(y0 + tr, h) - 1]) - int(s0[y0]) + 1 <= RZ_SR for y0 in range(0, h, tr))

    def cols_fit(tc):
        for x0 in range(0, w, tc):
            x1 = min(x0 + tc, w)
            sc0, sc1 = int(sx[x0]) & ~3, min(int(sx[x1 - 1]) + 2, sw)
            if _round_up(sc1 - sc0, 16) > RZ_SCB:
                return False
        return True

    tr, tc = RZ_TR, RZ_TC
    while tr > 1 and not rows_fit(tr):
        tr -= 1
    while tc > 4 and not cols_fit(tc):
        tc -= 4
    assert rows_fit(tr) and cols_fit(tc)
    return tr, tc


def level_facts(t, rows=RS_ROWS):
    """Launch geometry of one level under both chained builders."""
    w, h = t["dw"], t["dh"]
    tr, tc = tile_shape(t)
    col_tiles, row_tiles = -(-w // tc), -(-h // tr)
    chunks = -(-h // rows)
    src_rows = []
    for c in range(chunks):
        y0, y1 = c * rows, min((c + 1) * rows, h)
        src_rows.append(int(t["sy1"][y1 - 1]) - int(t["sy0"][y0]) + 1)
    return dict(w=w, h=h, sw=t["sw"], sh=t["sh"], rs_ok=rs_ok(t), rs_cols=rs_columns_ok(t), rs_rows=rs_rows_ok(t),
                rz_rows=tr, rz_cols=tc, col_tiles=col_tiles, row_tiles=row_tiles, block_rows=-(-row_tiles // RZ_TPB),
                tile_x0=[int(t["sx"][x0]) & ~3 for x0 in range(0, w, tc)], tile_sx0=[int(t["sx"][x0]) for x0 in range(0, w, tc)],
                strips=-(-w // RS_COLS), last_strip=w - (w - 1) // RS_COLS * RS_COLS, chunks=chunks,
                last_chunk=h - (chunks - 1) * rows, chunk_src_rows=src_rows, simd_end=t["simd_end"], xmax=t["xmax"])


def facts(case, rows=RS_ROWS):
    return [None] + [level_facts(t, rows) for t in case.tables()[1:]]


def aligned4(pitch, offsets=(0,)):
    return pitch % 4 == 0 and all(o % 4 == 0 for o in offsets)


def expected_builders(tabs, nimg, aligned, tiles):
    """Builder of every level >= 1 for a batch of nimg images whose pitch and pointers are (not) all
    multiples of 4; tiles = the engine's one-launch tile count for the geometry (0: it has none)."""
    if nimg < SMALL_BATCH and tiles > 0:
        return [ONE_LAUNCH] * (len(tabs) - 1)
    return [ROW_STREAMED if rs_ok(tabs[l]) and (l > 1 or aligned) else TILED for l in range(1, len(tabs))]


def expected_rs_rows(nimg):
    return RS_ROWS_SMALL if nimg < SMALL_BATCH else RS_ROWS


# ---- images -------------------------------------------------------------------------------------
def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def coded(w, h):
    """Upper half f(x), lower half g(y), of periods 251 and 241 with steps 29 and 31: neighbouring
    columns (rows) differ by 29 (31) grey levels, so a source column or row that is off by one shows,
    and its value names it."""
    img = np.zeros((h, w), np.uint8)
    img[: h // 2] = ((np.arange(w) * 29 + 11) % 251).astype(np.uint8)[None, :]
    img[h // 2:] = ((np.arange(h - h // 2) * 31 + 7) % 241).astype(np.uint8)[:, None]
    return img


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def stripes(w, h):
    return np.broadcast_to(((np.arange(w) & 1) * 255).astype(np.uint8), (h, w)).copy()


def constant(w, h, v=255):
    return np.full((h, w), v, np.uint8)


def mixed(seed, w, h):
    """Noise blocks, the coded pattern and saturated squares: keys on most levels."""
    rng = np.random.default_rng(seed)
    img = coded(w, h)
    for _ in range(5):
        bw, bh = min(40, w // 2), min(40, h // 2)
        x, y = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
        img[y:y + bh, x:x + bw] = rng.integers(0, 256, (bh, bw))
    for _ in range(8):
        x, y = int(rng.integers(4, w - 12)), int(rng.integers(4, h - 12))
        img[y:y + 7, x:x + 7] = int(rng.integers(0, 2)) * 255
    return img


def variant(img, k):
    """The k-th distinct companion of a case image in a batch: k = 0 is the image itself; the others
    are rolled, every second one inverted, every third one noise, each tagged with k on one row."""
    if k == 0:
        return img
    h, w = img.shape
    if k % 3 == 2:
        v = noise(7000 + 31 * k + w + h, w, h)
    else:
        v = np.roll(img, (5 * k, 3 * k), (0, 1))
        if k % 2:
            v = 255 - v
    v = v.copy()
    v[(7 * k) % h] = (v[(7 * k) % h].astype(np.int32) + 16 * k + 1).astype(np.uint8)
    return v


# ---- preconditions ------------------------------------------------------------------------------
def _legal(case):
    h, w = case.img.shape
    assert w <= MAX_W and h <= MAX_H, f"{case.name}: {w}x{h} above {MAX_W}x{MAX_H}"
    for lw, lh in case.sizes():
        assert lw >= MIN_SIDE and lh >= MIN_SIDE, f"{case.name}: level {lw}x{lh} below {MIN_SIDE}"


def pre_tiled_chain(col_tiles):
    def pre(case):
        f = facts(case)[1]
        assert not f["rs_cols"], f"{case.name}: the column rule holds"
        assert f["rz_rows"] < RZ_TR and f["rz_cols"] < RZ_TC and f["col_tiles"] == col_tiles, f
        assert all(x > 0 for x in f["tile_x0"][1:])
    return pre


def pre_rs_last_true(case):
    """Exact 2:1: the column rule holds with byte-pair offsets {0, 2, 4}; the same base at the next
    scale factors of the list (2.5, 2.6, 3.0) breaks it."""
    f = facts(case)[1]
    assert f["rs_ok"] and f["sw"] == 2 * f["w"] and f["sh"] == 2 * f["h"], f
    t = case.tables()[1]
    offs = {int(t["sx"][x]) - (int(t["sx"][x & ~3]) & ~3) - (2 if x & 2 else 0) for x in range(f["w"])}
    assert offs == {0, 2, 4}, offs
    for s in (2.5, 2.6, 3.0):
        (w0, h0), (w1, h1) = rd.level_sizes(f["sw"], f["sh"], s, 2)
        assert not rs_columns_ok(rd.tables(w0, h0, w1, h1, 16)), s


def pre_tiled_unaligned(odd_start):
    """Level 1 is row-streamable, so only an unaligned input sends it to the tiled resize; there the
    tiles are shrunk in rows and there are column tiles with x0 > 0 (odd_start: whose first source
    column is no multiple of 4)."""
    def pre(case):
        f = facts(case)[1]
        assert f["rs_ok"] and f["rz_rows"] < RZ_TR and f["col_tiles"] >= 2, f
        assert any(s & 3 for s in f["tile_sx0"][1:]) == odd_start, f"{case.name}: tile source starts {f['tile_sx0']}"
        assert not aligned4(form_pitch(case.img.shape[1], "d"), (1,))
    return pre


def pre_two_strips(case):
    f = facts(case)[1]
    assert f["rs_ok"] and f["strips"] == 2 and f["last_strip"] < RS_COLS and f["w"] % 4 == 3, f


def pre_chunks(n):
    def pre(case):
        f = facts(case)[1]
        assert f["rs_ok"] and f["chunks"] == n and f["last_chunk"] < RS_ROWS, f
    return pre


def pre_simd(kind):
    def pre(case):
        for f in facts(case)[1:]:
            w, e = f["w"], f["simd_end"]
            if kind == "full":
                assert e == w and case.lanes > 0, (w, e)
            elif kind == "small":
                assert 1 <= w - e <= 3, (w, e)
            elif kind == "large":
                assert w - e == 32, (w, e)
            elif kind == "scalar":
                assert e == 0 and case.lanes == 0
            elif kind == "whole-step-only":
                assert case.lanes == 64 and e == 64 and w < 96, (w, e)
    return pre


def pre_same_width(case):
    (w0, h0), (w1, h1) = case.sizes()[:2]
    assert w1 == w0 and h1 != h0, (w0, h0, w1, h1)
    t = case.tables()[1]
    assert (t["sx"] == np.arange(w0)).all() and (t["a1"] == 0).all() and t["xmax"] == w0 - 1


def pre_equal_level(level):
    def pre(case):
        s = case.sizes()
        assert s[level] == s[level - 1], s
        f = facts(case)[level]
        # the last row's second source row is clipped: not row-streamable, and every form but the
        # one-launch pyramid builds the copy with the tiled resize
        assert f["rs_cols"] and not f["rs_rows"] and f["xmax"] == f["w"] - 1, f
    return pre


def pre_deep(case):
    h, w = case.img.shape
    assert case.nlevels == 12 and min(case.sizes()[-1]) == MIN_SIDE, case.sizes()
    assert min(rd.level_sizes(w - 1, h - 1, case.scale, 12)[-1]) < MIN_SIDE


def pre_block_rows(case):
    f = facts(case)[1]
    assert f["h"] > 96 and f["row_tiles"] > RZ_TPB and f["block_rows"] >= 2, f


def pre_constant(case):
    for lanes in rd.LANES:
        for lv in rd.pyramid(case.img, case.scale, case.nlevels, lanes):
            assert (lv == case.img[0, 0]).all()


def pre_rounding_split(case):
    assert case.lanes == 16
    vec = rd.pyramid(case.img, case.scale, 2, 16)[1]
    sca = rd.pyramid(case.img, case.scale, 2, 0)[1]
    t = case.tables()[1]
    w, e = t["dw"], t["simd_end"]
    assert w - 16 < e < w, (w, e)
    d = vec != sca
    assert d[:, : w - 16].any() and d[:, w - 16: e].any(), "the two rounding forms agree on one side"
    assert (vec[:, e:] == sca[:, e:]).all()
    allvec = rd.resize_with(case.img, dict(t, simd_end=w))
    assert (allvec[:, e:] != vec[:, e:]).any(), "the tail columns do not separate the forms"


def pre_saturating(case):
    """0 / 255 neighbours: horizontal sums up to at least 255 * 1536, spread over half the range or more."""
    t = case.tables()[1]
    H = rd.horizontal(case.img, t)
    assert H.max() >= 255 * 1536 and H.max() - H.min() >= 255 * 1024, (H.min(), H.max())


# ---- run forms ----------------------------------------------------------------------------------
FORMS = ("a", "b", "c", "d")
FORM_IMAGES = {"a": 1, "b": 2, "c": 16, "d": 16}


def form_pitch(w, form):
    """a: the host call's tight rows; b, c: the width rounded up to 64; d: w + 1, or w + 3 where w + 1
    is a multiple of 4."""
    if form == "a":
        return w
    if form in ("b", "c"):
        return _round_up(w, 64)
    return w + 1 if (w + 1) % 4 else w + 3


def form_offset(form):
    return 1 if form == "d" else 0


def form_builders(case, form, tiles):
    w = case.img.shape[1]
    al = aligned4(form_pitch(w, form), (form_offset(form),))
    return expected_builders(case.tables(), FORM_IMAGES[form], al, tiles)


# ---- the cases ----------------------------------------------------------------------------------
def deep_base(scale=1.1, nlevels=12):
    """Smallest square base whose top level is still legal."""
    n = MIN_SIDE
    while min(rd.level_sizes(n, n, scale, nlevels)[-1]) < MIN_SIDE:
        n += 1
    return n


def _chain(*pres):
    def pre(case):
        _legal(case)
        for p in pres:
            p(case)
    return pre


def cases():
    C = []

    def add(name, img, scale, nlevels, lanes, branch, *pres):
        C.append(PCase(name, img, scale, nlevels, lanes, branch, _chain(*pres)))

    # scale factors past the row-streamed rule: the tiled resize builds the level in every chained form
    add("tiled-225x225-s3.0", coded(225, 225), 3.0, 2, 16, "rs_ok false; rz_rows, rz_cols shrunk; 2 column tiles",
        pre_tiled_chain(2))
    add("tiled-640x225-s3.0", noise(11, 640, 225), 3.0, 2, 16, "rs_ok false; 4 column tiles", pre_tiled_chain(4))
    add("tiled-230x225-s2.6", mixed(12, 230, 225), 2.6, 2, 8, "rs_ok false just past the rule's edge", pre_tiled_chain(2))
    add("tiled-225x225-s2.5", noise(13, 225, 225), 2.5, 2, 32, "rs_ok false just past the rule's edge", pre_tiled_chain(2))
    add("streamed-304x152-s2.0", noise(14, 304, 152), 2.0, 2, 0, "rs_ok true at its last scale factor; exact 2:1",
        pre_rs_last_true)
    # level 1 of a row-streamable geometry from unaligned input (form d)
    add("unaligned-300x150-s2.0", coded(300, 150), 2.0, 2, 16, "tiled level 1 from unaligned input, rz_rows < 24",
        pre_tiled_unaligned(False))
    add("unaligned-330x110-s1.5", mixed(15, 330, 110), 1.5, 2, 16, "tiled level 1 from unaligned input, rz_rows < 24; tile source start not on a dword",
        pre_tiled_unaligned(True))
    add("strips-330x107-s1.2", mixed(16, 330, 107), 1.2, 3, 16, "two k_resize_s strips, the second partial, w = 3 mod 4",
        pre_two_strips)
    # chunks of 48 rows (no legal level has fewer than 73 rows, so never one chunk)
    add("chunks2-120x100-s1.2", noise(17, 120, 100), 1.2, 2, 16, "two 48-row chunks, the last partial", pre_chunks(2))
    add("chunks3-100x150-s1.2", coded(100, 150), 1.2, 2, 8, "three 48-row chunks, the last partial", pre_chunks(3))
    add("blockrows-150x130-s1.2", mixed(18, 150, 130), 1.2, 2, 16, "level height > 96: two block rows of k_resize in form d",
        pre_block_rows)
    # the rounding split
    add("simd-full-115x96-s1.2", noise(19, 115, 96), 1.2, 2, 16, "simd_end == w", pre_simd("full"))
    add("simd-w-minus-1-116x97-s1.2", noise(20, 116, 97), 1.2, 2, 16, "simd_end == w - 1", pre_simd("small"))
    add("simd-w-minus-32-115x100-s1.2", noise(21, 115, 100), 1.2, 2, 64, "simd_end == w - 32, the largest tail", pre_simd("large"))
    add("simd-64-only-100x100-s1.2", noise(22, 100, 100), 1.2, 2, 64, "lanes 64, one whole step and no half step",
        pre_simd("whole-step-only"))
    add("scalar-133x107-s1.2", noise(23, 133, 107), 1.2, 3, 0, "lanes 0: everything scalar", pre_simd("scalar"))
    add("rounding-split-133x107-s1.2", noise(24, 133, 107), 1.2, 2, 16, "both rounding forms inside the last 16 columns",
        pre_rounding_split)
    # equal-size levels
    add("same-width-100x130-s1.004", mixed(25, 100, 130), 1.004, 2, 16, "width equal to the previous level's, height not",
        pre_same_width)
    add("equal-level1-100x100-s1.004", mixed(26, 100, 100), 1.004, 2, 16, "level 1 equal to level 0", pre_equal_level(1))
    add("equal-level2-140x140-s1.004", mixed(27, 140, 140), 1.004, 3, 32, "level 2 equal to level 1", pre_equal_level(2))
    n = deep_base()
    add(f"deep-{n}x{n}-s1.1-12", mixed(28, n, n), 1.1, 12, 16, "12 levels: deep source cones", pre_deep)
    # contents with the largest sums
    add("checkerboard-133x107-s1.2", checkerboard(133, 107), 1.2, 2, 16, "0 / 255 checkerboard", pre_saturating)
    add("stripes-150x110-s1.5", stripes(150, 110), 1.5, 2, 8, "vertical 0 / 255 stripes", pre_saturating)
    add("constant-255-133x107-s1.2", constant(133, 107), 1.2, 3, 16, "constant 255, vector rounding", pre_constant)
    add("constant-255-scalar-225x225-s3.0", constant(225, 225), 3.0, 2, 0, "constant 255, scalar rounding, tiled", pre_constant)
    # level widths: with the cases above, every residue mod 16 (coverage asserted over the set)
    for k, (w, h, lanes) in enumerate(RESIDUE_GEOMETRIES):
        add(f"width-{w}x{h}-s1.1-l{lanes}", mixed(40 + k, w, h) if k % 2 else noise(40 + k, w, h), 1.1, 3, lanes,
            "level widths and chunk source-row counts over all residues")
    return C


RESIDUE_GEOMETRIES = [(99, 121, 8), (103, 117, 32), (107, 131, 64), (113, 126, 0), (118, 139, 16)]


def coverage(all_cases):
    """Over the set: level widths mod 4 and mod 16, and the source-row counts mod 5 of the 48-row
    chunks of row-streamable levels."""
    w4, w16, r5 = set(), set(), set()
    for c in all_cases:
        for f in facts(c)[1:]:
            w4.add(f["w"] % 4)
            w16.add(f["w"] % 16)
            if f["rs_ok"]:
                r5.update(n % RS_D for n in f["chunk_src_rows"])
    return w4, w16, r5
