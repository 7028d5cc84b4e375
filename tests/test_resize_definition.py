"""The plain-Python cv::resize / ComputePyramid of oracle/resize_definition.py against the C++ oracle
(oro_resize level by level, OracleExtractor.pyramid_level for the chain) on every case of
tests/pyramid_patterns.py under all five lane counts, against known answers, and against wrong
variants of itself: each variant must change a pixel of at least one case image, which shows that the
case set would catch that mistake in a kernel. CPU only.
"""
import numpy as np
import pytest

import pyramid_patterns as pp
from oracle import resize_definition as rd

CASES = pp.cases()


# ---- preconditions and coverage of the set ------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_reaches_its_branch(case):
    case.pre(case)


def test_set_coverage():
    w4, w16, r5 = pp.coverage(CASES)
    assert w4 == set(range(4)) and w16 == set(range(16)), f"level widths mod 4 {sorted(w4)}, mod 16 {sorted(w16)}"
    assert r5 == set(range(pp.RS_D)), f"chunk source-row counts mod {pp.RS_D}: {sorted(r5)}"
    f = [pp.facts(c) for c in CASES]
    chunks = {lv["chunks"] for c in f for lv in c[1:] if lv["rs_ok"]}
    assert {2, 3} <= chunks and 1 not in chunks
    assert any(lv["strips"] == 2 for c in f for lv in c[1:])
    assert {c.lanes for c in CASES} == set(rd.LANES)


def test_unreachable_geometries():
    """What the smallest legal level side (73) rules out, and the listed geometry it moves."""
    # one 48-row chunk, and a level narrower than 64 under lanes = 64 (simd_end from the half step only)
    assert pp.MIN_SIDE > pp.RS_ROWS and pp.MIN_SIDE > 64
    assert rd.simd_end(63, 64) == 32 and rd.simd_end(73, 64) == 64 and rd.simd_end(96, 64) == 64 and rd.simd_end(97, 64) == 96
    # 330 x 107 at scale 1.5 has a 71-row level 1: the case runs at 330 x 110 (73 rows, same tiles)
    assert rd.level_sizes(330, 107, 1.5, 2)[1] == (220, 71) and rd.level_sizes(330, 110, 1.5, 2)[1] == (220, 73)
    a, b = rd.tables(330, 107, 220, 71), rd.tables(330, 110, 220, 73)
    assert pp.tile_shape(a) == pp.tile_shape(b) == (20, 116)
    # a level >= 2 past the row-streamed column rule (scale factor >= 2.5) needs 73 * 2.5^2 = 457 rows
    assert rd.level_sizes(pp.MAX_W, pp.MAX_H, 2.5, 3)[2][1] < pp.MIN_SIDE


# ---- against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_definition_matches_oracle(case, oracle_lib):
    L = oracle_lib.lib()
    for lanes in rd.LANES:
        pyr = rd.pyramid(case.img, case.scale, case.nlevels, lanes)
        ora = oracle_lib.OracleExtractor(case.nfeat, case.scale, case.nlevels, 20, 7, resize_simd_lanes=lanes)
        ora(case.img)
        for l in range(case.nlevels):
            po = ora.pyramid_level(l)
            assert po.shape == pyr[l].shape, f"lanes {lanes} level {l}: {pyr[l].shape} vs oracle {po.shape}"
            bad = np.argwhere(po != pyr[l])
            assert bad.size == 0, f"lanes {lanes} level {l}: {len(bad)} px differ from the oracle, first {bad[:3].tolist()}"
            if l:
                src = np.ascontiguousarray(pyr[l - 1])
                out = np.zeros_like(pyr[l])
                L.oro_resize(src.ctypes.data, src.shape[1], src.shape[0], out.ctypes.data, out.shape[1], out.shape[0], lanes)
                bad = np.argwhere(out != pyr[l])
                assert bad.size == 0, f"lanes {lanes} level {l}: {len(bad)} px differ from oro_resize, first {bad[:3].tolist()}"
        ora.close()


# ---- known answers ------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", rd.LANES)
@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_constant_stays_constant(value, lanes):
    for (w, h), (dw, dh) in [((133, 107), (111, 89)), ((225, 225), (75, 75)), ((100, 130), (100, 129)), ((96, 80), (73, 79))]:
        out = rd.resize(pp.constant(w, h, value), dw, dh, lanes)
        assert out.shape == (dh, dw) and (out == value).all(), (value, lanes, w, h, np.unique(out))


def test_equal_size_is_a_copy():
    img = pp.noise(1, 97, 83)
    for lanes in rd.LANES:
        assert np.array_equal(rd.resize(img, 97, 83, lanes), img)
    # and the generic tables of an equal-size level are the identity with xmax = w - 1
    t = rd.tables(97, 83, 97, 83)
    assert (t["sx"] == np.arange(97)).all() and (t["a0"] == 2048).all() and (t["a1"] == 0).all() and t["xmax"] == 96
    assert (t["sy0"] == np.arange(83)).all() and t["sy1"][-1] == 82 and (t["b1"] == 0).all()
    for lanes in rd.LANES:
        assert np.array_equal(rd.resize_with(img, dict(t, simd_end=rd.simd_end(97, lanes))), img)


def test_exact_half_is_the_rounded_mean():
    img = pp.noise(2, 152, 148)
    a = img.astype(np.int64)
    want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(rd.resize(img, 76, 74, 0), want.astype(np.uint8))
    t = rd.tables(152, 148, 76, 74, 0)
    assert (t["a0"] == 1024).all() and (t["a1"] == 1024).all() and (t["b0"] == 1024).all() and t["xmax"] == 76


def test_simd_end_rule():
    for lanes in (8, 16, 32, 64):
        for w in range(1, 300):
            e = rd.simd_end(w, lanes)
            assert e % (lanes // 2) == 0 and 0 <= w - e <= lanes // 2, (w, lanes, e)
            assert (e + lanes // 2 < w) is False
    assert [rd.simd_end(w, 16) for w in (96, 97, 104, 105, 111, 112)] == [96, 96, 96, 104, 104, 112]
    assert rd.simd_end(100, 0) == 0


# ---- sensitivity: wrong variants of the definition ----------------------------------------------
def _pyramid_with(case, level_fn):
    """The case's pyramid with every level >= 1 built by level_fn(src, tables)."""
    out = [case.img]
    for (dw, dh) in case.sizes()[1:]:
        sh, sw = out[-1].shape
        out.append(level_fn(out[-1], dict(rd.tables(sw, sh, dw, dh, case.lanes), lanes=case.lanes)))
    return out


def v_scalar_everywhere(src, t):
    return rd.resize_with(src, dict(t, simd_end=0))


def v_vector_everywhere(src, t):
    return rd.resize_with(src, dict(t, simd_end=t["dw"]))


def v_no_half_step(src, t):
    lanes = t["lanes"]
    return rd.resize_with(src, dict(t, simd_end=t["dw"] // lanes * lanes if lanes else 0))


def v_right_neighbour_clamped_early(src, t):
    """sx + 1 clamped to sw - 2 instead of sw - 1."""
    S = src.astype(np.int64)
    H = S[:, t["sx"]] * t["a0"] + S[:, np.minimum(t["sx"] + 1, t["sw"] - 2)] * t["a1"]
    H[:, t["xmax"]:] = S[:, t["sx"][t["xmax"]:]] * rd.ONE
    H0, H1 = H[t["sy0"]], H[t["sy1"]]
    b0, b1 = t["b0"][:, None], t["b1"][:, None]
    out = rd.round_scalar(H0, H1, b0, b1)
    e = t["simd_end"]
    out[:, :e] = rd.round_vector(H0[:, :e], H1[:, :e], b0, b1)
    return out.astype(np.uint8)


def v_row_shift_at_48(src, t):
    sy0, sy1 = t["sy0"].copy(), t["sy1"].copy()
    for y in range(pp.RS_ROWS, t["dh"], pp.RS_ROWS):   # a chunk's first row takes the previous row's sources
        sy0[y], sy1[y] = sy0[y - 1], sy1[y - 1]
    return rd.resize_with(src, dict(t, sy0=sy0, sy1=sy1))


def v_truncated_coefficients(src, t):
    sx, fx = rd._axis(t["dw"], t["sw"])
    fx = np.where((sx < 0) | (sx >= t["sw"] - 1), np.float32(0), fx)
    sy, fy = rd._axis(t["dh"], t["sh"])
    one, k = np.float32(1), np.float32(rd.ONE)
    tr = lambda v: np.trunc(v.astype(np.float32)).astype(np.int64)
    return rd.resize_with(src, dict(t, a0=tr((one - fx) * k), a1=tr(fx * k), b0=tr((one - fy) * k), b1=tr(fy * k)))


def v_last_tile_unmasked(src, t):
    """The tiled resize with the last column tile's window starting at sx[x0] instead of sx[x0] & ~3
    while the columns are still addressed relative to the masked start."""
    _, tc = pp.tile_shape(t)
    x0 = (t["dw"] - 1) // tc * tc
    sx = t["sx"].copy()
    if x0 > 0:
        sx[x0:] = np.minimum(sx[x0:] + (int(sx[x0]) & 3), t["sw"] - 1)
    return rd.resize_with(src, dict(t, sx=sx))


VARIANTS = {"scalar-everywhere": v_scalar_everywhere, "vector-everywhere": v_vector_everywhere,
            "no-half-step": v_no_half_step, "right-neighbour-clamped-early": v_right_neighbour_clamped_early,
            "row-shift-at-48": v_row_shift_at_48, "truncated-coefficients": v_truncated_coefficients,
            "last-tile-unmasked": v_last_tile_unmasked}


@pytest.fixture(scope="module")
def definition_pyramids():
    return {c.name: rd.pyramid(c.img, c.scale, c.nlevels, c.lanes) for c in CASES}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_cases_separate_wrong_variant(name, definition_pyramids):
    fn = VARIANTS[name]
    hit = []
    for c in CASES:
        got = _pyramid_with(c, fn)
        want = definition_pyramids[c.name]
        if any(c.sizes()[l] == c.sizes()[l - 1] for l in range(1, c.nlevels)):
            continue   # the definition copies an equal-size level; the variants always resample
        if any((g != w).any() for g, w in zip(got, want)):
            hit.append(c.name)
    print(f"{name}: separated by {len(hit)} cases: {hit}")
    assert hit, f"no case image separates the variant {name}"


def test_unmodified_variant_harness_is_the_definition(definition_pyramids):
    """_pyramid_with and the tables reproduce the definition when nothing is changed (so a variant's
    difference is the variant's)."""
    for c in CASES:
        if any(c.sizes()[l] == c.sizes()[l - 1] for l in range(1, c.nlevels)):
            continue
        got = _pyramid_with(c, rd.resize_with)
        assert all(np.array_equal(g, w) for g, w in zip(got, definition_pyramids[c.name])), c.name
