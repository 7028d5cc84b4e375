"""GPU parity of ComputePyramid's three builders on the adversarial geometries and images of
tests/pyramid_patterns.py, bit-exact against the CPU oracle and against the plain-Python definition
of oracle/resize_definition.py (the two are held together on the same cases by
tests/test_resize_definition.py, so a difference here is the device's).

Every case runs in four forms:

  a  the one-image host call (tight rows: pitch = width)
  b  a device batch of 2, pitch rounded up to 64
  c  a device batch of 16, pitch rounded up to 64
  d  a device batch of 16, pitch w + 1 (w + 3 where w + 1 is a multiple of 4), the base pointer one
     byte off a 256-byte boundary, random bytes in the padding

Batches hold distinct images (pyramid_patterns.variant). For every image and level: the size, the
pixels against both references, and the final keypoints and descriptors against the oracle. For
every level: the builder the engine reports (orbfe_debug_copy what = 5) against the expectation the
pattern module derives from the definition's tables and its own statement of the dispatch rules,
and the level's resize geometry (what = 6: tile shape, row-streamed rows per wave, simd_end, xmax,
pitch) against the same tables. The caller's buffer, padding included, must be unchanged. Each
case's CPU precondition is asserted before anything touches the GPU.
"""
import numpy as np
import pytest

import pyramid_patterns as pp
from oracle import resize_definition as rd
from test_gpu_fast_adversarial import check_outputs
from test_gpu_input_layout import _Batch, _device_batch

pytestmark = pytest.mark.gpu

CASES = pp.cases()
NAMES = {pp.ONE_LAUNCH: "k_pyramid", pp.ROW_STREAMED: "k_resize_s", pp.TILED: "k_resize"}
SEEN = {}   # (builder, level 1 or "2+") -> the first (case, form) whose read-back showed it
NO_TILES = []   # (case, form, builders) of the small batches whose geometry has no one-launch tiles
SHRUNK = {}  # "rows" / "cols" -> the first (case, form) whose what = 6 read-back showed a shrunk tile


@pytest.fixture(scope="module")
def references(oracle_lib):
    """Per case, on demand and once: the 16 batch images with the definition's and the oracle's
    pyramids and the oracle's outputs. Never modified."""
    cache = {}

    def get(case):
        if case.name not in cache:
            refs = []
            for k in range(16):
                img = pp.variant(case.img, k)
                ora = oracle_lib.OracleExtractor(case.nfeat, case.scale, case.nlevels, 20, 7, resize_simd_lanes=case.lanes)
                mono, kp, desc = ora(img)
                refs.append(dict(img=img, mono=mono, kp=kp, desc=desc, pyr=[ora.pyramid_level(l) for l in range(case.nlevels)],
                                 dpyr=rd.pyramid(img, case.scale, case.nlevels, case.lanes)))
                ora.close()
            cache[case.name] = refs
        return cache[case.name]
    return get


def _check_levels(ext, image, ref, nlevels, what):
    for l in range(nlevels):
        pg = ext.pyramid_level(l, image=image)
        for name, want in (("oracle", ref["pyr"][l]), ("definition", ref["dpyr"][l])):
            assert pg.shape == want.shape, f"{what} level {l}: size {pg.shape} vs {name} {want.shape}"
            bad = np.argwhere(pg != want)
            assert bad.size == 0, (f"{what} level {l}: {len(bad)} px differ from the {name}, first (y, x) {bad[:4].tolist()}: "
                                   f"gpu {[int(pg[y, x]) for y, x in bad[:4]]} vs {[int(want[y, x]) for y, x in bad[:4]]}")


def _read_path(ext, nlevels):
    """what = 5 and what = 6 of every level >= 1: (tiles, [builder], [rs_ok], aligned, [geometry])."""
    built, fits, geo, tiles, al0 = [], [], [], 0, 0
    for l in range(1, nlevels):
        info, g6 = np.zeros(4, np.int32), np.zeros(6, np.int32)
        assert ext._lib.orbfe_debug_copy(ext.handle, 5, 0, l, info.ctypes.data, 16) == 4
        assert ext._lib.orbfe_debug_copy(ext.handle, 6, 0, l, g6.ctypes.data, 24) == 6
        tiles, al0 = int(info[0]), int(info[3])
        built.append(int(info[1]))
        fits.append(int(info[2]))
        geo.append([int(v) for v in g6])
    return tiles, built, fits, al0, geo


def _check_path(case, form, ext, pitch, offset):
    what = f"{case.name} form {form}:"
    tabs, facts = case.tables(), pp.facts(case)
    tiles, built, fits, al0, geo = _read_path(ext, case.nlevels)
    assert al0 == int(pp.aligned4(pitch, (offset,))), f"{what} aligned read back {al0}, pitch {pitch}, offset {offset}"
    assert fits == [int(f["rs_ok"]) for f in facts[1:]], f"{what} row-streamable per level {fits}"
    want = pp.form_builders(case, form, tiles)
    assert built == want, (f"{what} levels built by {[NAMES[b] for b in built]}, expected {[NAMES[b] for b in want]} "
                           f"({tiles} one-launch tiles)")
    nimg = pp.FORM_IMAGES[form]
    for l in range(1, case.nlevels):
        rz_rows, rz_cols, rs_rows, simd_end, xmax, lpitch = geo[l - 1]
        f, t = facts[l], tabs[l]
        assert (simd_end, xmax) == (t["simd_end"], t["xmax"]), f"{what} level {l}: simd_end, xmax {simd_end}, {xmax} vs {t['simd_end']}, {t['xmax']}"
        assert (rz_rows, rz_cols) == (f["rz_rows"], f["rz_cols"]), f"{what} level {l}: tile {rz_rows} x {rz_cols} vs {f['rz_rows']} x {f['rz_cols']}"
        assert rs_rows == (pp.expected_rs_rows(nimg) if built[l - 1] == pp.ROW_STREAMED else 0), f"{what} level {l}: rs_rows {rs_rows}"
        assert lpitch == (f["w"] + 15) // 16 * 16
        SEEN.setdefault((built[l - 1], 1 if l == 1 else "2+"), (case.name, form))
        if built[l - 1] == pp.TILED:
            if rz_rows < pp.RZ_TR:
                SHRUNK.setdefault("rows", (case.name, form))
            if rz_cols < pp.RZ_TC:
                SHRUNK.setdefault("cols", (case.name, form))
    if tiles == 0 and nimg < pp.SMALL_BATCH:   # the chained builders at the small-batch launch shapes
        NO_TILES.append((case.name, form, [NAMES[b] for b in built]))
    return tiles, built


def _run_host(case, refs):
    from orb_slam3_ros_amd.extractor import ORBextractor
    ref = refs[0]
    img = ref["img"].copy()
    ext = ORBextractor(case.nfeat, case.scale, case.nlevels, 20, 7)
    try:
        ext.set_opencv_model(case.lanes, 0)
        mono, kp, desc = ext(img, None, (0, 0))
        assert np.array_equal(img, ref["img"]), "the host call changed its input"
        _check_path(case, "a", ext, img.shape[1], 0)
        _check_levels(ext, 0, ref, case.nlevels, f"{case.name} form a:")
        check_outputs(mono, kp, desc, ref, f"{case.name} form a:")
    finally:
        ext.close()


def _run_batch(case, form, refs, device):
    import torch
    h, w = case.img.shape
    nimg, pitch, offset = pp.FORM_IMAGES[form], pp.form_pitch(w, form), pp.form_offset(form)
    imgs = [refs[i]["img"] for i in range(nimg)]
    dev, ptrs = _device_batch(imgs, pitch, offset, "random" if form == "d" else 0xFF, seed=len(case.name))
    before = dev.cpu().numpy().copy()
    b = _Batch(nimg, device, w, h, case.nfeat, case.scale, case.nlevels, case.lanes, lap=(0, 0))
    try:
        outs = b.run(ptrs, pitch)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), before), f"{case.name} form {form}: the call changed the caller's buffer"
        _check_path(case, form, b.ext, pitch, offset)
        for i in range(nimg):
            what = f"{case.name} form {form} image {i} of {nimg}:"
            _check_levels(b.ext, i, refs[i], case.nlevels, what)
            check_outputs(*outs[i], refs[i], what)
    finally:
        b.close()
    del dev


@pytest.mark.parametrize("form", pp.FORMS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_pyramid_case(case, form, gpu, references):
    case.pre(case)   # CPU: the geometry and the image reach the branch the case is named for
    refs = references(case)
    for r in refs[:1]:   # the references agree on the case image before the GPU is asked
        assert all(np.array_equal(a, d) for a, d in zip(r["pyr"], r["dpyr"])), f"{case.name}: oracle and definition differ"
    if form == "a":
        _run_host(case, refs)
    else:
        _run_batch(case, form, refs, gpu)


WITNESSES = [("strips-330x107-s1.2", "b"), ("strips-330x107-s1.2", "c"), ("tiled-225x225-s3.0", "c"),
             ("equal-level2-140x140-s1.004", "c")]


def test_every_builder_built_level_1_and_above(gpu, references):
    """Over the run, each builder built a level 1 and a level >= 2 and the tiled resize ran with its
    tile shrunk in rows and in columns. The read-backs of the cases above are collected as they run;
    when this test runs without them, it runs the four witnesses itself."""
    def missing():
        return [(NAMES[b], lv) for b in NAMES for lv in (1, "2+") if (b, lv) not in SEEN]
    if missing() or len(SHRUNK) < 2:
        by_name = {c.name: c for c in CASES}
        for name, form in WITNESSES:
            _run_batch(by_name[name], form, references(by_name[name]), gpu)
    print("builders seen:", {f"{NAMES[k[0]]} level {k[1]}": v for k, v in SEEN.items()})
    print("shrunk tiles:", SHRUNK, "; small batches without one-launch tiles:", NO_TILES)
    assert not missing(), f"never built: {missing()}"
    assert "rows" in SHRUNK and "cols" in SHRUNK, SHRUNK
