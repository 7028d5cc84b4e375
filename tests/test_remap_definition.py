"""The plain definition of oracle/remap_definition.py (cv::remap INTER_LINEAR, cv::undistortPoints)
against the C++ oracle on every pattern of tests/remap_patterns.py, which pins the oracle against
an independent restatement; against known answers; and the coverage conditions of the patterns
(what tests/test_gpu_remap_adversarial.py asserts before it trusts a device result), so they run
where there is no GPU. CPU only.
"""
import numpy as np
import pytest

import remap_patterns as rp
from oracle import remap_definition as rd

NAMES = sorted(rp.PATTERNS)


# ---- what the patterns reach --------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pattern_reaches_its_branch(name):
    src, mx, my, _ = rp.built(name)
    rp.pre(name)(src, mx, my)


def test_window_sweep_coverage():
    fast, d6, fail = rp.sweep_coverage()
    print("fast groups per off_0 & 3:", fast, "; fast with largest d = 6:", d6, "; failing clause:", fail)
    assert min(fast) >= 20, fast
    assert d6 >= 10
    for clause in (rd.D_BIG, rd.D_NEG, rd.WINDOW):
        assert fail.get(clause, 0) >= 10, (clause, fail)


def test_right_edge_overhangs():
    """Over the right-edge widths, groups with every sample inside end their window at sw exactly
    (fast) and 1, 2 and 3 columns past it."""
    seen = set()
    for sw in rp.EDGE_WIDTHS:
        src, mx, my, _ = rp.built(f"right-edge-sw{sw}")
        seen |= {(g.verdict, g.over) for row in rp._groups(src, mx, my) for g in row if g.over is not None}
    assert {(rd.FAST, 0), (rd.WINDOW, 1), (rd.WINDOW, 2), (rd.WINDOW, 3)} <= seen, seen


def test_undistort_break_classes():
    """The 4-coefficient set: the icdist < 0 break at iteration 0 for some points, at an iteration
    >= 1 for others, never for the rest; the other sets never break on these points."""
    pts = rp.undistort_points()
    _, brk = rd.undistort_points_def(pts, rp.UNDIST_K, np.array(rp.UNDIST_DIST[4], np.float32), trace=True)
    assert (brk == 0).sum() >= 10 and (brk >= 1).sum() >= 10 and (brk == -1).sum() >= 10, np.unique(brk, return_counts=True)
    assert sorted(rp.UNDIST_DIST) == [0, 4, 5, 8, 12] and all(len(d) == n for n, d in rp.UNDIST_DIST.items())
    assert all(v != 0 for v in rp.UNDIST_DIST[12][8:])
    p = pts.tolist()
    assert p[0] == [float(np.float32(rp.UNDIST_K[2])), float(np.float32(rp.UNDIST_K[3]))] and [0.0, 0.0] in p
    assert np.isnan(pts).any() and np.isinf(pts).any() and (np.abs(pts[np.isfinite(pts)]) == 1e6).any()


# ---- against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_definition_matches_oracle(name, oracle_lib):
    src, mx, my, _ = rp.built(name)
    for k in range(3):
        img = rp.variant(src, k)
        want, got = rp.expected(name, k), oracle_lib.remap_linear(img, mx, my)
        bad = np.argwhere(want != got)
        assert bad.size == 0, (f"{name} image {k}: {len(bad)} px differ, first (y, x) {bad[:4].tolist()}: definition "
                               f"{[int(want[y, x]) for y, x in bad[:4]]} vs oracle {[int(got[y, x]) for y, x in bad[:4]]}")


@pytest.mark.parametrize("ndist", sorted(rp.UNDIST_DIST))
def test_undistort_definition_matches_oracle(ndist, oracle_lib):
    pts, dist = rp.undistort_points(), np.array(rp.UNDIST_DIST[ndist], np.float32)
    want = rd.undistort_points_def(pts, rp.UNDIST_K, dist)
    got = oracle_lib.undistort_points(pts, rp.UNDIST_K, dist)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


def test_nan_map_entry_is_outside(oracle_lib):
    """A NaN map entry converts to INT_MIN (the x86-64 cvtss2si result), not to 0: the pixel is 0
    although source row 0 and column 0 are 255."""
    src = np.full((8, 8), 255, np.uint8)
    nan = float("nan")
    mx = np.array([[nan, 2.5, nan, 3.0]], np.float32)
    my = np.array([[2.5, nan, nan, 3.0]], np.float32)
    assert rd.sat_int(nan) == rd.INT_MIN
    assert rd.remap_linear_def(src, mx, my).tolist() == [[0, 0, 0, 255]]
    assert oracle_lib.remap_linear(src, mx, my).tolist() == [[0, 0, 0, 255]]


# ---- known answers ------------------------------------------------------------------------------
def test_identity_shift_and_half_pixel():
    img = rp.source(1, 50, 40)
    v, u = np.mgrid[0:40, 0:50].astype(np.float32)
    assert np.array_equal(rd.remap_linear_def(img, u, v), img)
    out = rd.remap_linear_def(img, u + 3, v - 2)
    assert np.array_equal(out[2:, :47], img[:38, 3:])
    assert (out[:1] == 0).all() and (out[:, 49:] == 0).all()   # wholly outside: 0
    # fx = fy = 0 one column or row outside: the only inside weight is 0
    assert (out[1] == 0).all() and (out[:, 47:49] == 0).all()
    half = rd.remap_linear_def(img, u + 0.5, v)
    a = img.astype(np.int64)
    assert np.array_equal(half[:, :-1], (a[:, :-1] * 16384 + a[:, 1:] * 16384 + 16384) >> 15)
    assert np.array_equal(half[:, -1], (a[:, -1] * 16384 + 16384) >> 15)


def test_border_ring_closed_form():
    src, mx, my, _ = rp.built("border-ring")
    assert (src == 255).all()
    assert np.array_equal(rp.expected("border-ring"), rp.ring_closed_form(mx, my))


def test_cell_0_0_is_invisible():
    """(32767 S00 + S11 + 2**14) >> 15 == (32768 S00 + 2**14) >> 15 == S00 for every byte pair."""
    s00, s11 = np.mgrid[0:256, 0:256].astype(np.int64)
    table = (32767 * s00 + s11 + 2 ** 14) >> 15
    assert np.array_equal(table, s00) and np.array_equal((32768 * s00 + 2 ** 14) >> 15, s00)
    assert rd.weights(0, 0) == (32768, 0, 0, 0) and all(sum(rd.weights(fx, fy)) == 32768 for fx in range(32) for fy in range(32))


def test_undistort_known_answers():
    """No coefficients: the identity up to the float32 rounding of (u - c) / f * f + c; the
    principal point maps to itself under every set."""
    pts = rp.undistort_points()
    fin = np.isfinite(pts).all(1) & (np.abs(pts) < 1e5).all(1)
    out = rd.undistort_points_def(pts, rp.UNDIST_K, np.zeros(0, np.float32))
    assert np.abs(out[fin].astype(np.float64) - pts[fin]).max() <= 2.0 ** -14   # an ulp of 772 is 2**-14
    for dist in rp.UNDIST_DIST.values():
        o = rd.undistort_points_def(pts[:1], rp.UNDIST_K, np.array(dist, np.float32))
        assert o.tolist() == pts[:1].tolist()
