"""GPU parity of the row-streamed resize's packed remainder strip (k_resize_s, DESIGN.md "Pyramid:
the builders' branches and the cases that reach them"): every pyramid level of every image of a
16-image device batch, bit-exact against the CPU oracle, on geometries chosen so that the levels
reach every place the packed form can go wrong; and the same images through the one-image host
call, and as device batches of 1 and 2 with the one-launch pyramid switched off
(orbfe_debug_chained_pyramid), so that k_resize_s itself runs at the small-batch shapes (4 rows per
wave), where the launch arithmetic must keep the packed form out.

A level whose width is no multiple of 256 ends in a remainder strip of r = ceil((w mod 256) / 4)
lanes; with r <= 32 a wave takes that strip of G = min(64 // r, 512 // 48) consecutive 48-row chunks.
The (width, r, G, chunks) table of every case is computed here from the level-size formula, printed,
compared with what the engine reports it launched (orbfe_debug_copy what = 7), and the set of cases
is asserted to contain the named ones, so a geometry change cannot silently empty the test.
"""
import numpy as np
import pytest

import pyramid_patterns as pp
from oracle import resize_definition as rd
from test_gpu_input_layout import _Batch, _device_batch

pytestmark = pytest.mark.gpu

SCALE, LANES, NIMG = 1.2, 16, 16
PK_ROWS = 512   # RS_PK_ROWS: table rows a packed wave keeps in LDS
# (w, h, levels): widths of levels 1.. -> r
GEOMETRIES = [
    (154, 170, 4),   # 128, 107, 89: r = 32, 27, 23; no full strip; 128 = simd_end (no scalar tail); 3 chunks, G = 2
    (462, 150, 4),   # 385, 321, 267: r = 33 (full form), 17, 3 (G = 10 > the level's 2 chunks)
    (310, 150, 3),   # 258, 215: r = 1 (G = 10 > 3 chunks; the scalar tail reaches back into the full strip), 54 (full form)
    (406, 150, 3),   # 338, 282: r = 21 (G = 3), 7
    (105, 150, 3),   # 88, 73: r = 22 (G = 2), 19
    (314, 580, 2),   # 262 x 483: r = 2, 11 chunks over the capped G = 10 (64 // 2 = 32): two packed waves, one group in the second
]


def level_table(w, h, nlevels, rows=pp.RS_ROWS):
    """Per level >= 1: dict(l, w, h, r, G, chunks, full, packed, simd_end) under the packed-form rules."""
    tabs = rd.pyramid_tables(w, h, SCALE, nlevels, LANES)
    out = []
    for l, (lw, lh) in enumerate(rd.level_sizes(w, h, SCALE, nlevels)):
        if l == 0:
            continue
        r = (lw % pp.RS_COLS + 3) // 4
        G = min(64 // r, PK_ROWS // rows) if r else 0
        chunks, strips = -(-lh // rows), -(-lw // pp.RS_COLS)
        pk = G >= 2
        out.append(dict(l=l, w=lw, h=lh, r=r, G=G, chunks=chunks, full=(strips - 1 if pk else strips) * chunks,
                        packed=-(-chunks // G) if pk else 0, simd_end=tabs[l]["simd_end"], rs_ok=pp.rs_ok(tabs[l])))
    return out


TABLES = {g: level_table(*g) for g in GEOMETRIES}


def test_geometries_reach_every_packed_case():
    """CPU: the per-level tables contain the cases this file is for."""
    rows = [t for g in GEOMETRIES for t in TABLES[g]]
    for g in GEOMETRIES:
        print(g, [(t["w"], t["r"], t["G"], t["chunks"]) for t in TABLES[g]])
    assert all(t["rs_ok"] for t in rows), "every level must be row-streamable"
    by_r = {t["r"]: t for t in rows}
    for r in (1, 3, 21, 22, 32, 33):
        assert r in by_r, f"no level with r = {r}"
    for r in (1, 3):   # more groups than the level has chunks: trailing groups idle
        assert by_r[r]["G"] > by_r[r]["chunks"] and by_r[r]["packed"] == 1
    assert (by_r[21]["G"], by_r[22]["G"]) == (3, 2) and 64 - 3 * 21 > 0 and 64 - 2 * 22 > 0   # lanes past G r idle
    assert by_r[32]["G"] == 2 and by_r[32]["packed"] > 0 and by_r[33]["G"] == 1 and by_r[33]["packed"] == 0
    pk = [t for t in rows if t["packed"]]
    # a short last chunk sharing a wave with full chunks, in a wave count G does not divide
    assert any(t["chunks"] % t["G"] and t["h"] % pp.RS_ROWS and t["chunks"] > t["G"] for t in pk)
    assert any(t["h"] % pp.RS_ROWS and t["G"] >= t["chunks"] > 1 for t in pk)
    # the scalar-tail columns inside the remainder strip; no scalar tail at all; none of the strip's columns vector
    strip0 = lambda t: t["w"] // pp.RS_COLS * pp.RS_COLS
    assert any(strip0(t) < t["simd_end"] < t["w"] for t in pk)
    assert any(t["simd_end"] == t["w"] for t in pk)
    assert any(t["simd_end"] <= strip0(t) for t in pk)
    assert any(t["full"] == 0 for t in pk) and any(t["full"] > 0 for t in pk)
    assert any(t["l"] == 1 for t in pk), "a packed level 1: the source is the caller's image"
    # the cap on G at work: fewer chunks per wave than 64 // r, and more than one packed wave because of it
    assert any(t["G"] == PK_ROWS // pp.RS_ROWS < 64 // t["r"] and t["packed"] >= 2 and t["chunks"] % t["G"] for t in pk)
    # the small-batch shapes: every geometry has a level the large-batch rule would pack
    for g in GEOMETRIES:
        assert any(t["packed"] for t in level_table(*g, rows=pp.RS_ROWS_SMALL)), g


@pytest.fixture(scope="module")
def references(oracle_lib):
    """Per geometry, once: 16 distinct images and the oracle's pyramids. Never modified."""
    cache = {}

    def get(g):
        if g not in cache:
            w, h, nlevels = g
            base, refs = pp.mixed(300 + w, w, h), []
            for k in range(NIMG):
                img = pp.variant(base, k)
                ora = oracle_lib.OracleExtractor(300, SCALE, nlevels, 20, 7, resize_simd_lanes=LANES)
                ora(img)
                refs.append(dict(img=img, pyr=[ora.pyramid_level(l) for l in range(nlevels)]))
                ora.close()
            cache[g] = refs
        return cache[g]
    return get


def _launched(ext, nlevels):
    """Per level >= 1: (builder, [r, G, full items, packed items]) of the last call."""
    return [(b, pk) for b, _, pk in _launched_rows(ext, nlevels)]


def _launched_rows(ext, nlevels):
    """Per level >= 1: (builder, rs_rows as launched, [r, G, full items, packed items])."""
    out = []
    for l in range(1, nlevels):
        info, geo, pk = np.zeros(4, np.int32), np.zeros(6, np.int32), np.zeros(4, np.int32)
        assert ext._lib.orbfe_debug_copy(ext.handle, 5, 0, l, info.ctypes.data, 16) == 4
        assert ext._lib.orbfe_debug_copy(ext.handle, 6, 0, l, geo.ctypes.data, 24) == 6
        assert ext._lib.orbfe_debug_copy(ext.handle, 7, 0, l, pk.ctypes.data, 16) == 4
        out.append((int(info[1]), int(geo[2]), [int(v) for v in pk]))
    return out


def _check_levels(ext, image, ref, nlevels, what):
    for l in range(nlevels):
        pg, want = ext.pyramid_level(l, image=image), ref["pyr"][l]
        assert pg.shape == want.shape, f"{what} level {l}: size {pg.shape} vs {want.shape}"
        bad = np.argwhere(pg != want)
        assert bad.size == 0, (f"{what} level {l}: {len(bad)} px differ from the oracle, first (y, x) {bad[:4].tolist()}: "
                               f"gpu {[int(pg[y, x]) for y, x in bad[:4]]} vs {[int(want[y, x]) for y, x in bad[:4]]}")


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_packed_batch(geom, gpu, references):
    """A batch of 16 (the large-batch launch shapes), pitch rounded up to 64: level 1 is built from the
    caller's images at the caller's pitch, the others from the pyramid."""
    import torch
    w, h, nlevels = geom
    refs, pitch = references(geom), (w + 63) // 64 * 64
    dev, ptrs = _device_batch([r["img"] for r in refs], pitch, 0, 0xFF)
    b = _Batch(NIMG, gpu, w, h, 300, SCALE, nlevels, LANES, lap=(0, 0))
    try:
        b.run(ptrs, pitch)
        torch.cuda.synchronize()
        for t, (builder, pk) in zip(TABLES[geom], _launched(b.ext, nlevels)):
            print(geom, "level", t["l"], "width", t["w"], "launched r, G, full, packed:", pk)
            assert builder == pp.ROW_STREAMED, f"{geom} level {t['l']}: builder {builder}"
            want = [t["r"], t["G"], t["full"], t["packed"]] if t["packed"] else [0, 0, t["full"], 0]
            assert pk == want, f"{geom} level {t['l']}: launched {pk}, the table says {want}"
        for i in range(NIMG):
            _check_levels(b.ext, i, refs[i], nlevels, f"{geom} image {i} of {NIMG}:")
    finally:
        b.close()
    del dev


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_one_image_is_never_packed(geom, gpu, references):
    """The same images one at a time through the host call (the small-batch launch shapes): whichever
    builder takes the level, no packed item is launched, and the levels are the oracle's."""
    from orb_slam3_ros_amd.extractor import ORBextractor
    w, h, nlevels = geom
    refs = references(geom)
    ext = ORBextractor(300, SCALE, nlevels, 20, 7)
    try:
        ext.set_opencv_model(LANES, 0)
        for i in (0, 5):
            ext(refs[i]["img"].copy(), None, (0, 0))
            for l, (builder, pk) in enumerate(_launched(ext, nlevels), 1):
                assert pk[0] == pk[1] == pk[3] == 0, f"{geom} level {l}: one image launched packed items {pk} (builder {builder})"
            _check_levels(ext, 0, refs[i], nlevels, f"{geom} host call, image {i}:")
    finally:
        ext.close()


@pytest.mark.parametrize("nimg", (1, 2))
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[0]}x{g[1]}-{g[2]}")
def test_small_batch_row_streamed_is_never_packed(geom, nimg, gpu, references):
    """Device batches of 1 and 2 on an aligned pitch with the one-launch pyramid switched off: every
    level is built by k_resize_s at 4 rows per wave, one wave per strip and chunk (the packed form is
    for batches of 16 and more, and every geometry here has a level that rule would pack), and the
    levels are the oracle's."""
    import torch
    w, h, nlevels = geom
    refs, pitch = references(geom), (w + 63) // 64 * 64
    dev, ptrs = _device_batch([r["img"] for r in refs[:nimg]], pitch, 0, 0xFF)
    b = _Batch(nimg, gpu, w, h, 300, SCALE, nlevels, LANES, lap=(0, 0))
    try:
        assert b.ext._lib.orbfe_debug_chained_pyramid(b.ext.handle, 1) == 0
        b.run(ptrs, pitch)
        torch.cuda.synchronize()
        small = level_table(w, h, nlevels, rows=pp.RS_ROWS_SMALL)
        for t, (builder, rows, pk) in zip(small, _launched_rows(b.ext, nlevels)):
            strips, chunks = -(-t["w"] // pp.RS_COLS), -(-t["h"] // pp.RS_ROWS_SMALL)
            assert builder == pp.ROW_STREAMED, f"{geom} B = {nimg} level {t['l']}: builder {builder}, not the row-streamed resize"
            assert rows == pp.RS_ROWS_SMALL, f"{geom} B = {nimg} level {t['l']}: rs_rows {rows}"
            assert pk == [0, 0, strips * chunks, 0], f"{geom} B = {nimg} level {t['l']}: launched {pk}"
        for i in range(nimg):
            _check_levels(b.ext, i, refs[i], nlevels, f"{geom} B = {nimg} chained, image {i}:")
    finally:
        b.close()
    del dev
