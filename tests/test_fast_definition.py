"""CPU: the definitional FAST-9/16 (oracle/fast_definition.py, numpy, written from the definition)
against the C++ oracle's restated cv::FAST, bit-exact: single regions, then the per-cell loop on the
adversarial pattern images of tests/fast_patterns.py. Also every precondition of those patterns
(each image reaches the branch it is named for) and the coverage of the geometry list, all from
the definition and the grid arithmetic alone. tests/test_gpu_fast_adversarial.py runs the same
cases on the GPU.
"""
import numpy as np
import pytest

import fast_patterns as fp
from oracle import fast_definition as fd

THRESHOLDS = (0, 7, 20, 254, 255)
STRADDLE = np.array([0, 7, 8, 20, 21, 234, 235, 255], np.uint8)
KINDS = ("full", "low", "binary", "straddle")


def _oro_fast(oracle_lib, roi, th):
    L = oracle_lib.lib()
    roi = np.ascontiguousarray(roi, np.uint8)
    out = np.zeros(roi.size, oracle_lib.KEYPOINT_DTYPE)
    n = L.oro_fast(roi.ctypes.data, roi.shape[1], roi.shape[0], roi.shape[1], th, out.ctypes.data, len(out))
    assert 0 <= n <= len(out)
    return [(int(k["x"]), int(k["y"]), int(k["response"])) for k in out[:n]]


def _region(rng, kind, h, w):
    if kind == "full":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "low":
        return rng.integers(100, 130, (h, w), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    return rng.choice(STRADDLE, (h, w))


@pytest.mark.parametrize("kind", KINDS)
def test_fast9_matches_oracle(kind, oracle_lib):
    """60 seeded regions per content kind (240 in all), sides 7-60 (both extremes included), five
    thresholds each: the (x, y, score) lists are equal including their order."""
    rng = np.random.default_rng(KINDS.index(kind))
    sides = [(7, 7), (7, 60), (60, 7), (60, 60), (8, 9)] + [tuple(rng.integers(7, 61, 2)) for _ in range(55)]
    total = 0
    for h, w in sides:
        roi = _region(rng, kind, int(h), int(w))
        for th in THRESHOLDS:
            ref, got = _oro_fast(oracle_lib, roi, th), fd.fast9(roi, th)
            assert got == ref, f"{kind} {h}x{w} th {th}: first difference {next((a, b) for a, b in zip(got + [None], ref + [None]) if a != b)}"
            total += len(ref)
    assert total > 100


def test_fast9_known_answers():
    """The definition itself on hand-checked regions (no oracle): an isolated impulse of contrast c
    has M = c; equal neighbours tie; contrast 1 at threshold 0 scores 0 and is never kept."""
    roi = np.full((15, 15), 50, np.uint8)
    roi[7, 7] = 71
    assert fd.fast9(roi, 20) == [(7, 7, 20)] and fd.fast9(roi, 21) == []
    roi[7, 7] = 29
    assert fd.fast9(roi, 20) == [(7, 7, 20)] and fd.fast9(roi, 21) == []
    roi[7, 8] = 29
    assert fd.fast9(roi, 20) == []
    roi[7, 8] = 28
    assert fd.fast9(roi, 20) == [(8, 7, 21)]
    roi[:] = 50
    roi[7, 7] = 51
    assert fd.fast9(roi, 0) == []
    roi[:] = 0
    roi[3, 3] = roi[11, 11] = 255   # the first and last pixel FAST looks at
    assert fd.fast9(roi, 254) == [(3, 3, 254), (11, 11, 254)] and fd.fast9(roi, 255) == []
    roi[2, 7] = 255                 # outside the frame
    assert fd.fast9(roi, 254) == [(3, 3, 254), (11, 11, 254)]
    assert fd.fast9(np.zeros((6, 20), np.uint8), 0) == []


CASES = fp.content_cases() + fp.geometry_cases()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_cell_keys_match_oracle(case, oracle_lib):
    """Level 0 (the input image: no resize model enters) of every pattern image: the oracle's raw keys,
    binned into the grid, equal the definitional cell loop cell by cell, order included."""
    ora = oracle_lib.OracleExtractor(case.nfeat, case.scale, 1, case.ini, case.min)
    ora(case.img)
    raw = ora.debug_keys(0, 0)
    ora.close()
    h, w = case.img.shape
    counts_o, lists_o = fd.bin_keys(raw["x"], raw["y"], raw["response"], w, h)
    counts_d, lists_d = fd.cell_keys(case.img, case.ini, case.min)
    assert [k for l in lists_o for k in l] == [(int(x), int(y), int(s)) for x, y, s in
                                               zip(raw["x"], raw["y"], raw["response"])], "binning keeps the cell-major order"
    assert np.array_equal(counts_o, counts_d), f"per-cell counts: oracle {counts_o.tolist()} definition {counts_d.tolist()}"
    for c, (lo, ld) in enumerate(zip(lists_o, lists_d)):
        assert lo == ld, f"cell {c}"


@pytest.mark.parametrize("case", [c for c in CASES if c.pre], ids=repr)
def test_preconditions(case):
    case.pre(case)


def test_cases_fit_the_engine():
    """Every level of every case is at least 73 px on each side and wide enough for the octree's
    initial nodes (round(width / height) >= 1)."""
    for case in CASES + fp.pyramid_cases():
        h, w = case.img.shape
        for lw, lh in fp.level_sizes(w, h, case.nlevels, case.scale):
            assert lw >= 73 and lh >= 73, (case.name, lw, lh)
            assert round((lw - 32) / (lh - 32)) >= 1, (case.name, lw, lh)


def test_level_sizes_match_oracle(oracle_lib):
    for case in fp.pyramid_cases() + [c for c in CASES if c.nlevels > 1][:3]:
        ora = oracle_lib.OracleExtractor(case.nfeat, case.scale, case.nlevels, case.ini, case.min)
        ora(case.img)
        h, w = case.img.shape
        got = [ora.pyramid_level(l).shape[::-1] for l in range(case.nlevels)]
        ora.close()
        assert got == fp.level_sizes(w, h, case.nlevels, case.scale), case.name


def test_geometry_list_coverage():
    """The geometry list reaches every shape-dependent path of the detector, by grid arithmetic alone."""
    levels = [(w, h, lw, lh) for w, h, nl in fp.GEOMETRIES for lw, lh in fp.level_sizes(w, h, nl)]
    facts = [fp.geometry_facts(lw, lh) for _, _, lw, lh in levels]
    cells = [c for f in facts for c in f["cells"]]
    # a single cell of 60-69 px both ways, and the jump to two cells of 35
    assert any(f["n_cols"] == 1 and f["n_rows"] == 1 and 60 <= f["w_cell"] <= 69 and 60 <= f["h_cell"] <= 69 for f in facts)
    assert fp.geometry_facts(101, 101)["w_cell"] == 69 and fp.geometry_facts(102, 102)["w_cell"] == 35
    assert (101, 101, 1) in fp.GEOMETRIES and (102, 102, 1) in fp.GEOMETRIES and (73, 73, 1) in fp.GEOMETRIES
    assert fp.geometry_facts(73, 73)["n_cols"] == 1 and fp.geometry_facts(73, 73)["w_cell"] == 41
    # one row with several columns, and the reverse
    assert any(f["n_rows"] == 1 and f["n_cols"] >= 3 for f in facts)
    assert any(f["n_cols"] == 1 and f["n_rows"] >= 3 for f in facts)
    # odd widths of every residue mod 4 (level 0 is the caller's image: pitch == width in these tests)
    assert {w % 4 for w, _, _ in fp.GEOMETRIES} == {0, 1, 2, 3}
    # all four realignments of a cell's first column
    assert {c["realign"] for c in cells} == {0, 1, 2, 3}
    # the compile-time LDS stride of 48 bytes and the generic path (64 and 80 bytes)
    assert {c["stride"] for c in cells} == {48, 64, 80}
    # cells whose rows run past the register prefetch window, and cells that fit it
    assert any(c["rows"] > c["prefetch_rows"] for c in cells) and any(c["rows"] <= c["prefetch_rows"] for c in cells)
    # clipped last columns / rows: a detection width that is no multiple of 4, of every residue
    assert {c["dw"] % 4 for c in cells} == {0, 1, 2, 3}
