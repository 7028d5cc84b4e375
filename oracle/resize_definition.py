"""cv::resize(src, dst, dsize, 0, 0, INTER_LINEAR) for CV_8UC1 and ORBextractor::ComputePyramid's
level chain, restated in plain Python from OpenCV 4.2's semantics — TEST INFRASTRUCTURE ONLY.

Independent of oracle/orb_oracle.cpp: the tables are numpy float32 / float64 expressions with one
rounded operation per step, the sums are int64, and the SIMD vertical pass is modelled by its
rounding formula alone.

Semantics (imgproc/resize.cpp, resizeGeneric_ / HResizeLinear / VResizeLinear for uchar):

  scale_x = 1 / (dw / sw) in double (the reciprocal of the rounded quotient, not sw / dw);
  per output column dx: fx = float((dx + 0.5) * scale_x - 0.5), the product and difference in double,
    sx = cvFloor(fx), fx -= sx in float; sx < 0 gives (0, fx = 0); sx + 1 >= sw lowers xmax to dx,
    and sx >= sw - 1 gives (sw - 1, fx = 0);
  the 11-bit coefficients a0 = saturate_cast<short>((1.f - fx) * 2048), a1 = saturate_cast<short>(fx *
    2048): float products, round half to even, saturate to int16 (a0 + a1 is 2048 or 2049);
  rows the same with scale_y, except that nothing is clamped in the table: fy keeps its value and the
    two source rows sy, sy + 1 are clipped to [0, sh - 1] when they are read;
  horizontal pass (exact, int): H = S[sx] a0 + S[sx + 1] a1 for dx < xmax, S[sx] * 2048 from xmax on;
  vertical pass: the vector loop covers the columns below simd_end with
    (((H0 >> 4) b0 >> 16) + ((H1 >> 4) b1 >> 16) + 2) >> 2, the scalar loop the rest with
    (H0 b0 + H1 b1 + 2^21) >> 22, both saturated to a byte;
  simd_end for a vector of `lanes` bytes: whole vectors while x <= w - lanes, then half vectors
    (lanes / 2 int16 results) while x < w - lanes / 2, strictly; lanes = 0 is a build without the
    vector loop;
  dsize equal to the source size copies.

ComputePyramid (ORBextractor.cc): mvScaleFactor[i] = mvScaleFactor[i - 1] * scaleFactor in float,
mvInvScaleFactor = 1.0f / it, level size (cvRound(float(w) * inv), cvRound(float(h) * inv)), level l
resized from level l - 1.
"""
from __future__ import annotations

import numpy as np

COEF_BITS = 11
ONE = 1 << COEF_BITS
LANES = (0, 8, 16, 32, 64)


def _sat_s16(v):
    """saturate_cast<short>(float): round half to even, saturate."""
    return np.clip(np.rint(v.astype(np.float32)).astype(np.int64), -32768, 32767)


def _axis(dn, sn):
    """(float position, floor, float fraction) of every output index of an axis resized sn -> dn."""
    scale = 1.0 / (np.float64(dn) / np.float64(sn))
    d = np.arange(dn, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    frac = (f - s.astype(np.float32)).astype(np.float32)
    return s, frac


def simd_end(w, lanes):
    """First column the scalar vertical loop handles."""
    assert lanes in LANES
    x = 0
    if lanes > 0:
        while x <= w - lanes:
            x += lanes
        while x < w - lanes // 2:
            x += lanes // 2
    return x


def tables(sw, sh, dw, dh, lanes=16):
    """The per-level tables: dict of sx, a0, a1 (per column), xmax, sy0, sy1, b0, b1 (per row),
    simd_end; int64 arrays and Python ints."""
    sx, fx = _axis(dw, sw)
    fx = fx.copy()
    xmax = dw
    for dx in range(dw):
        if sx[dx] < 0:
            fx[dx], sx[dx] = 0, 0
        if sx[dx] + 1 >= sw:
            xmax = min(xmax, dx)
            if sx[dx] >= sw - 1:
                fx[dx], sx[dx] = 0, sw - 1
    one = np.float32(1.0)
    a0 = _sat_s16((one - fx) * np.float32(ONE))
    a1 = _sat_s16(fx * np.float32(ONE))
    sy, fy = _axis(dh, sh)
    b0 = _sat_s16((one - fy) * np.float32(ONE))
    b1 = _sat_s16(fy * np.float32(ONE))
    return dict(sx=sx, a0=a0, a1=a1, xmax=int(xmax), sy0=np.clip(sy, 0, sh - 1), sy1=np.clip(sy + 1, 0, sh - 1),
                b0=b0, b1=b1, simd_end=simd_end(dw, lanes), sw=sw, sh=sh, dw=dw, dh=dh)


def horizontal(src, t):
    """H[sy, dx] for every source row: exact int64."""
    S = src.astype(np.int64)
    sx = t["sx"]
    right = np.minimum(sx + 1, t["sw"] - 1)
    H = S[:, sx] * t["a0"] + S[:, right] * t["a1"]
    H[:, t["xmax"]:] = S[:, sx[t["xmax"]:]] * ONE
    return H


def round_vector(H0, H1, b0, b1):
    return np.clip(((((H0 >> 4) * b0) >> 16) + (((H1 >> 4) * b1) >> 16) + 2) >> 2, 0, 255)


def round_scalar(H0, H1, b0, b1):
    return np.clip((H0 * b0 + H1 * b1 + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255)


def resize_with(src, t):
    """The resize of `src` under the tables t."""
    H = horizontal(src, t)
    H0, H1 = H[t["sy0"]], H[t["sy1"]]
    b0, b1 = t["b0"][:, None], t["b1"][:, None]
    out = round_scalar(H0, H1, b0, b1)
    e = t["simd_end"]
    out[:, :e] = round_vector(H0[:, :e], H1[:, :e], b0, b1)
    return out.astype(np.uint8)


def resize(src, dw, dh, lanes=16):
    src = np.ascontiguousarray(src, np.uint8)
    sh, sw = src.shape
    if (dw, dh) == (sw, sh):
        return src.copy()
    return resize_with(src, tables(sw, sh, dw, dh, lanes))


def level_sizes(w, h, scale, nlevels):
    """ORBextractor's level sizes: float chain of scale factors, float inverse, cvRound."""
    s, out = np.float32(1.0), []
    for l in range(nlevels):
        if l:
            s = np.float32(s * np.float32(scale))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def pyramid_tables(w, h, scale, nlevels, lanes=16):
    """tables() of every level >= 1 (index 0 is None), equal-size levels included."""
    sizes = level_sizes(w, h, scale, nlevels)
    return [None] + [tables(*sizes[l - 1], *sizes[l], lanes) for l in range(1, nlevels)]


def pyramid(img, scale, nlevels, lanes=16):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = [img.copy()]
    for dw, dh in level_sizes(w, h, scale, nlevels)[1:]:
        out.append(resize(out[-1], dw, dh, lanes))
    return out
