"""The plain definition of the rectification stage: cv::remap(src, dst, map1, map2, INTER_LINEAR)
for 8UC1 images with CV_32FC1 map pairs and BORDER_CONSTANT 0, cv::undistortPoints for CV_32FC2
points, and the fast-path rule of k_remap as its comment states it. Pure Python and numpy: no
ctypes, no GPU, one output pixel or one point at a time. tests/test_remap_definition.py holds it
against the C++ oracle (oracle/orb_oracle_remap.cpp); tests/test_gpu_remap_adversarial.py holds
the HIP kernels against it.

remap, per output pixel, in Python integers
-------------------------------------------
  X  = saturate_cast<int>(float32(mapx) * float32(32))      (the product formed in float32;
       a multiplication by 32 is exact, so only overflow to +-inf can change it)
  sx = clamp(X >> 5, -32768, 32767), fx = X & 31            (>> floors; the same for y)
  w  = ((32-fy)(32-fx), (32-fy)fx, fy(32-fx), fy fx) * 32
  D  = (w0 S00 + w1 S01 + w2 S10 + w3 S11 + 2**14) >> 15    (a sample outside the source is 0)

saturate_cast<int>(float) is cvRound(float): round half to even. The reference runs OpenCV 4.2 on
x86-64, where cvRound(float) is the SSE2 cvtss2si; its result for NaN and for every value outside
[-2**31, 2**31) is INT_MIN ("integer indefinite"). sx is then -32768, the footprint lies outside
the source, and the pixel is 0. This comes from reading, not from running OpenCV, which is not
available here. The definition follows that rule: NaN and every out-of-range product, +-inf
included, give INT_MIN. A saturating conversion that gives INT_MAX for the positive ones (as the
HIP kernel and the C++ oracle do) puts sx at 32767, which is outside every source narrower than
32768 columns, so the pixel is 0 either way; the definition refuses wider sources.

The (0, 0) table cell. OpenCV's BilinearTab_i holds shorts, so the 32768 of fx = fy = 0 saturates
to 32767 and initInterTab2D adds the deficit to the (1, 1) weight: the cell is (32767, 0, 0, 1).
That can never change an output byte:
  (32767 S00 + S11 + 2**14) >> 15 = (32768 S00 + (S11 - S00) + 2**14) >> 15
                                  = S00 + ((S11 - S00 + 2**14) >> 15)
and |S11 - S00| <= 255 < 2**14 keeps S11 - S00 + 2**14 inside [16129, 16639], a subset of
[0, 2**15), so the second term is 0 and D = S00 = (32768 S00 + 2**14) >> 15. This covers samples
outside the source too (they read 0, which is a byte value). The definition therefore uses
(32768, 0, 0, 0) for that cell; tests/test_remap_definition.py proves the equality over all
256 x 256 (S00, S11) pairs.

undistortPoints follows the expression order written out in undistort_point (orbfe_remap.hip),
one IEEE double operation at a time on np.float64 scalars (which never contract), and rounds once
to float32.
"""
from collections import namedtuple

import numpy as np

INT_MIN = -2 ** 31
F32_32 = np.float32(32)


def round_half_even(v: float) -> int:
    """Python's round() on a float is exact and rounds halves to even."""
    return int(round(v))


def sat_int(m) -> int:
    """saturate_cast<int>(float32(m) * 32) under the x86-64 rule (see the module docstring)."""
    with np.errstate(all="ignore"):
        p = np.float32(m) * F32_32   # float32 product
    p = float(p)
    if p != p or not (-2147483648.0 <= p < 2147483648.0):
        return INT_MIN
    return round_half_even(p)


def fixed_point(m):
    """(s, f): the int16-clamped integer part and the 5-bit fraction of one map entry."""
    X = sat_int(m)
    return min(max(X >> 5, -32768), 32767), X & 31


def weights(fx: int, fy: int):
    if fx == 0 and fy == 0:
        return 32768, 0, 0, 0   # the table's (32767, 0, 0, 1): equivalent, see the module docstring
    return (32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32


def remap_linear_def(src, mapx, mapy):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    sh, sw = src.shape
    assert sw <= 32767 and sh <= 32767
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    assert mapx.shape == mapy.shape and mapx.ndim == 2
    dh, dw = mapx.shape
    S = [[int(v) for v in row] for row in src]

    def at(y, x):
        return S[y][x] if 0 <= x < sw and 0 <= y < sh else 0

    out = np.zeros((dh, dw), np.uint8)
    for y in range(dh):
        for x in range(dw):
            sx, fx = fixed_point(mapx[y, x])
            sy, fy = fixed_point(mapy[y, x])
            w0, w1, w2, w3 = weights(fx, fy)
            d = (w0 * at(sy, sx) + w1 * at(sy, sx + 1) + w2 * at(sy + 1, sx) + w3 * at(sy + 1, sx + 1) + 2 ** 14) >> 15
            assert 0 <= d <= 255
            out[y, x] = d
    return out


# ---- cv::undistortPoints ------------------------------------------------------------------------
def undistort_points_def(pts, K4, dist, trace=False):
    """pts float32 [n, 2], K4 = (fx, fy, cx, cy) and dist (0 to 12 coefficients) as float32, widened
    to double. Returns float32 [n, 2]; with trace also the iteration of each point's icdist < 0
    break (-1: none)."""
    f64 = np.float64
    p = np.asarray(pts, np.float32).reshape(-1, 2)
    fx, fy, cx, cy = (f64(np.float32(v)) for v in K4)
    d = [np.float32(v) for v in np.asarray(dist, np.float32).reshape(-1)]
    assert len(d) <= 12
    k = [f64(d[i]) if i < len(d) else f64(0) for i in range(12)]
    one, two, zero = f64(1), f64(2), f64(0)
    out = np.zeros_like(p)
    brk = np.full(len(p), -1, np.int64)
    with np.errstate(all="ignore"):
        ifx, ify = one / fx, one / fy
        for i in range(len(p)):
            x, y = f64(p[i, 0]), f64(p[i, 1])
            u, v = x, y
            x = (x - cx) * ifx
            y = (y - cy) * ify
            ux = (one * x + zero * y) + zero * one
            uy = (zero * x + one * y) + zero * one
            uz = (zero * x + zero * y) + one * one
            inv = one / uz if uz != 0 else one
            x0 = x = inv * ux
            y0 = y = inv * uy
            for j in range(5):
                r2 = x * x + y * y
                icdist = (one + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (one + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
                if icdist < 0:
                    x = (u - cx) * ifx
                    y = (v - cy) * ify
                    brk[i] = j
                    break
                dx = two * k[2] * x * y + k[3] * (r2 + two * x * x) + k[8] * r2 + k[9] * r2 * r2
                dy = k[2] * (r2 + two * y * y) + two * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
                x = (x0 - dx) * icdist
                y = (y0 - dy) * icdist
            xx = fx * x + zero * y + cx
            yy = zero * x + fy * y + cy
            ww = one / (zero * x + zero * y + one)
            out[i, 0] = np.float32(xx * ww)
            out[i, 1] = np.float32(yy * ww)
    return (out, brk) if trace else out


# ---- the fast-path rule of k_remap --------------------------------------------------------------
FAST, PARTIAL, OUTSIDE, D_NEG, D_BIG, WINDOW, UNALIGNED = (
    "fast", "partial group", "a sample outside", "d < 0", "d > 6", "window past sw", "unaligned source")

# verdict: FAST or the first clause that fails. phase = off_0 & 3, dmax = the largest d of the four
# pixels, over = base column + 8 - sw; these three are None where a sample is outside or the group
# is partial (there is no offset then).
Group = namedtuple("Group", "verdict phase dmax over")


def classify_groups(sw, sh, sstride, mapx, mapy, src_aligned):
    """For every group of four adjacent output pixels (rows of (dw + 3) // 4 groups), the rule of
    k_remap's comment: the group is whole, every sample of its four footprints is inside the
    source, and with off = sy * sstride + sx and base = off_0 & ~3 every pixel has d = off - base
    in [0, 6] and the 8-byte window from base ends inside the row's sw columns; the sources'
    rows are 4-byte aligned (src_aligned: every base pointer is; the rule adds sstride % 4 == 0)
    and hold 16 bytes or more. Used to prove what a pattern reaches, never to predict a byte."""
    mapx, mapy = np.asarray(mapx, np.float32), np.asarray(mapy, np.float32)
    dh, dw = mapx.shape
    aligned = bool(src_aligned) and sstride % 4 == 0 and sstride * (sh - 1) + sw >= 16
    rows = []
    for y in range(dh):
        row = []
        for x0 in range(0, dw, 4):
            if x0 + 4 > dw:
                row.append(Group(PARTIAL, None, None, None))
                continue
            px = [(fixed_point(mapx[y, x0 + q])[0], fixed_point(mapy[y, x0 + q])[0]) for q in range(4)]
            if not all(0 <= sx and sx + 1 < sw and 0 <= sy and sy + 1 < sh for sx, sy in px):
                row.append(Group(OUTSIDE, None, None, None))
                continue
            off = [sy * sstride + sx for sx, sy in px]
            base = off[0] & ~3
            d = [o - base for o in off]
            over = base - px[0][1] * sstride + 8 - sw
            if min(d) < 0:
                verdict = D_NEG
            elif max(d) > 6:
                verdict = D_BIG
            elif over > 0:
                verdict = WINDOW
            elif not aligned:
                verdict = UNALIGNED
            else:
                verdict = FAST
            row.append(Group(verdict, off[0] & 3, max(d), over))
        rows.append(row)
    return rows
