"""Orientation, blur and rBRIEF of one keypoint written from their descriptions, in plain numpy:
TEST INFRASTRUCTURE ONLY.

An independent second reference for what k_describe computes per key of one pyramid level
(ORBextractor.cc:76-103 IC_Angle, cv::fastAtan2, GaussianBlur 7x7 sigma 2 BORDER_REFLECT_101 of the
whole level, ORBextractor.cc:107-146 computeOrbDescriptor). When the HIP kernel and the C++ oracle
disagree on an angle or a descriptor bit, this module says which side is wrong; its trace says which
edge of the arithmetic a key reaches, so that a planted case can prove on the CPU that it reaches
the branch it is named for; its switches each compute a plausible wrong answer, so that a case can
prove that a kernel with that mistake would fail it. It touches no GPU and none of the oracle's C++.

Algorithm. The intensity centroid of the key (x, y) is taken over a disc of radius 15: row v of the
disc spans the columns -umax[|v|] .. umax[|v|], m10 = sum u I, m01 = sum v I, in exact integers. The
angle is fastAtan2((float)m01, (float)m10) in degrees: with ax = |x|, ay = |y| the octant polynomial
(((p7 c^2 + p5) c^2 + p3) c^2 + p1) c of c = min / (max + eps), taken as is when ax >= ay and
subtracted from 90 otherwise, then reflected to 180 - a when x < 0 and to 360 - a when y < 0; every
step a float32 operation of its own. The level is blurred by the separable 7-tap kernel in fixed
point: a row pass of integer sums, a column pass, + 2^15 >> 16, clamped to 255. With a = cosf(angle
pi / 180), b = sinf(..) from the host libm, pattern point (px, py) is read from the blurred level at
row y + round(px b + py a), column x + round(px a - py b), the two products and their sum or
difference each rounded to float32, the rounding to an integer half to even. Bit k of byte i is
t0 < t1 of pattern pair 8 i + k.

float32 scalars are np.float32; the 512 sample coordinates of a key are float32 arrays, whose
elementwise products and sums numpy rounds one operation at a time like the scalars.
"""
from __future__ import annotations

import ctypes
import ctypes.util
import os
import re
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
HALF_PATCH = 15
BORDERS = {"reflect-101": "reflect", "reflect": "symmetric", "replicate": "edge"}
ROUNDINGS = ("half-even", "half-away", "floor-plus-half")
TAPS = {0: (18, 34, 48, 56, 48, 34, 18), 1: (18, 34, 49, 55, 49, 34, 18)}
# what the kernel stages: a 43 x 43 patch from (x - 21, y - 21), as 48-byte rows from the 4-aligned
# column below it plus one dword (orbfe_kernels.hip, desc_slot)
PATCH_R, PATCH_N, STAGE_BYTES = 21, 43, 52

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.restype = ctypes.c_float
    _f.argtypes = [ctypes.c_float]


def cosf(x):
    return F32(_libm.cosf(float(x)))


def sinf(x):
    return F32(_libm.sinf(float(x)))


def umax_table():
    """The disc's half-widths as the extractor's constructor derives them (ORBextractor.cc:452-471)."""
    umax = [0] * (HALF_PATCH + 2)
    vmax = int(np.floor(HALF_PATCH * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(HALF_PATCH * np.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(HALF_PATCH * HALF_PATCH - v * v))))
    v0 = 0
    for v in range(HALF_PATCH, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:HALF_PATCH + 1]


def load_pattern(path=None):
    """The 256 pattern pairs as (512, 2) integers (x, y), read from the header the engine compiles."""
    path = path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam3_ros_amd", "csrc",
                                "brief_pattern.h")
    text = open(path).read()
    body = text[text.index("ORBFE_BRIEF_PATTERN_INIT {") + len("ORBFE_BRIEF_PATTERN_INIT {"):]
    vals = [int(v) for v in re.findall(r"-?\d+", body[: body.index("}")])]
    assert len(vals) == 1024
    return np.asarray(vals, np.int32).reshape(512, 2)


# ---- fastAtan2 ----------------------------------------------------------------------------------
DEG = F32(180 / np.pi)
P1, P3 = F32(0.9997878412794807) * DEG, F32(-0.3258083974640975) * DEG
P5, P7 = F32(0.1555786518463281) * DEG, F32(-0.04432655554792128) * DEG
EPS = F32(2.220446049250313e-16)


def _mad(a, b, c):
    return a * b + c          # two float32 roundings


def _fma(a, b, c):
    # one rounding: the product of two float32 is exact in float64 (the sum then rounds twice, to 53
    # and to 24 bits, which differs from a true fma only on a 53-bit tie; this switch is a wrong answer
    # to tell apart, not a reference)
    return F32(np.float64(a) * np.float64(b) + np.float64(c))


def fast_atan2(y, x, fma=False):
    """(angle, branch, tie, reflections) of float32 scalars y, x."""
    y, x = F32(y), F32(x)
    mad = _fma if fma else _mad
    ax, ay = np.abs(x), np.abs(y)

    def poly(c):
        c2 = c * c
        return mad(mad(mad(P7, c2, P5), c2, P3), c2, P1) * c

    if ax >= ay:
        branch, a = "ax>=ay", poly(ay / (ax + EPS))
    else:
        branch, a = "ax<ay", F32(90) - poly(ax / (ay + EPS))
    refl = []
    if x < 0:
        a = F32(180) - a
        refl.append("180-a")
    if y < 0:
        a = F32(360) - a
        refl.append("360-a")
    return F32(a), branch, bool(ax == ay), tuple(refl)


def fast_atan2_array(y, x):
    """The same arithmetic on float32 arrays (one rounded numpy operation per step)."""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    c = np.where(first, ay, ax) / (np.where(first, ax, ay) + EPS)
    c2 = c * c
    p = (((P7 * c2 + P5) * c2 + P3) * c2 + P1) * c
    a = np.where(first, p, F32(90) - p)
    a = np.where(x < 0, F32(180) - a, a)
    a = np.where(y < 0, F32(360) - a, a)
    return a.astype(F32)


# ---- rBRIEF sample coordinates ------------------------------------------------------------------
FACTOR_PI = F32(np.pi / 180.0)


def round_sums(s, rounding="half-even"):
    s = np.asarray(s, F32)
    if rounding == "half-even":
        return np.rint(s).astype(np.int32)
    if rounding == "half-away":
        d = s.astype(np.float64)
        return np.where(d >= 0, np.floor(d + 0.5), np.ceil(d - 0.5)).astype(np.int32)
    assert rounding == "floor-plus-half"
    return np.floor(s + F32(0.5)).astype(np.int32)


def sample_sums(angle, pattern):
    """(row sums, column sums) of every pattern point for a float32 angle in degrees: unrounded float32."""
    ang = F32(angle) * FACTOR_PI
    a, b = cosf(ang), sinf(ang)
    px, py = pattern[:, 0].astype(F32), pattern[:, 1].astype(F32)
    rows = px * b + py * a        # float32 arrays: product, product, sum, each rounded
    cols = px * a - py * b
    return rows, cols


def is_half(s):
    s = np.asarray(s, np.float64)
    return (s - np.floor(s)) == 0.5


# ---- staging class of the kernel, from the geometry alone -----------------------------------------
def staging(x, y, w, h, pitch=None, base_aligned=True):
    """('interior', sh) or ('gather', reason) as desc_slot's interior test decides it."""
    px0, py0 = x - PATCH_R, y - PATCH_R
    gx0 = px0 & ~3
    if px0 < 0:
        return "gather", "left"
    if py0 < 0:
        return "gather", "top"
    if py0 + PATCH_N > h:
        return "gather", "bottom"
    if gx0 + STAGE_BYTES > w:
        return "gather", "right-by-gx0"
    if (w if pitch is None else pitch) % 4 or not base_aligned:
        return "gather", "unaligned"
    return "interior", px0 - gx0


@dataclass
class Switches:
    border: str = "reflect-101"
    rounding: str = "half-even"
    mask: int = 0              # columns added to (+1) or taken from (-1) every row of the disc, each side
    le: bool = False           # t0 <= t1
    clamp: bool = True         # False: value & 0xFF
    fma: bool = False          # contracted fastAtan2 polynomial
    window: int = 18           # largest offset read: 17 is a blurred window one row and column too small


@dataclass
class Trace:
    m10: int = 0
    m01: int = 0
    branch: str = ""
    tie: bool = False                    # ax == ay
    reflections: tuple = ()
    angle: float = 0.0
    row_sums: np.ndarray = None          # (512,) float32, unrounded
    col_sums: np.ndarray = None
    rows: np.ndarray = None              # (512,) rounded offsets
    cols: np.ndarray = None
    half_rows: np.ndarray = None         # (512,) bool: the sum is an exact half-integer
    half_cols: np.ndarray = None
    max_offset: int = 0
    outside: dict = field(default_factory=dict)   # side -> samples with a blur tap outside the level
    n_outside: int = 0
    ties: int = 0                        # of the 256 comparisons
    over_255: bool = False               # a sampled column-pass value above 255 before the clamp
    pre_clamp_max: int = 0
    staging: tuple = ()

    @property
    def n_half(self):
        return int(self.half_rows.sum() + self.half_cols.sum())


class Level:
    """One pyramid level and everything described on it."""

    def __init__(self, img, variant=0, umax=None, pattern=None, pitch=None, base_aligned=True):
        self.img = np.ascontiguousarray(img, np.uint8)
        self.h, self.w = self.img.shape
        self.variant = variant
        self.umax = list(umax) if umax is not None else umax_table()
        self.pattern = pattern if pattern is not None else load_pattern()
        self.pitch, self.base_aligned = pitch, base_aligned
        self._blur = {}

    def blur_pre_clamp(self, border="reflect-101"):
        """Column-pass values (sum + 2^15) >> 16 of the whole level, before the clamp."""
        if border not in self._blur:
            k = TAPS[self.variant]
            p = np.pad(self.img.astype(np.uint32), 3, mode=BORDERS[border])
            h, w = self.h, self.w
            rowq = sum(np.uint32(k[i]) * p[:, i:i + w] for i in range(7))        # (h + 6, w)
            s = sum(np.uint32(k[j]) * rowq[j:j + h] for j in range(7))            # (h, w)
            self._blur[border] = ((s + np.uint32(32768)) >> np.uint32(16)).astype(np.int32)
        return self._blur[border]

    def blurred(self, border="reflect-101", clamp=True):
        v = self.blur_pre_clamp(border)
        return (np.minimum(v, 255) if clamp else (v & 0xFF)).astype(np.uint8)

    def moments(self, x, y, mask=0):
        a = self.img.astype(np.int64)
        m10 = m01 = 0
        for v in range(-HALF_PATCH, HALF_PATCH + 1):
            d = self.umax[abs(v)] + mask
            for u in range(-d, d + 1):
                m10 += u * int(a[y + v, x + u])
                m01 += v * int(a[y + v, x + u])
        return m10, m01

    def describe(self, x, y, sw=None):
        """(angle bits, 32 descriptor bytes, Trace) of the key on column x, row y."""
        sw = sw or Switches()
        tr = Trace()
        tr.m10, tr.m01 = self.moments(x, y, sw.mask)
        angle, tr.branch, tr.tie, tr.reflections = fast_atan2(F32(tr.m01), F32(tr.m10), sw.fma)
        tr.angle = angle
        tr.row_sums, tr.col_sums = sample_sums(angle, self.pattern)
        tr.rows, tr.cols = round_sums(tr.row_sums, sw.rounding), round_sums(tr.col_sums, sw.rounding)
        tr.rows, tr.cols = np.clip(tr.rows, -sw.window, sw.window), np.clip(tr.cols, -sw.window, sw.window)
        tr.half_rows, tr.half_cols = is_half(tr.row_sums), is_half(tr.col_sums)
        tr.max_offset = int(max(np.abs(tr.rows).max(), np.abs(tr.cols).max()))
        r, c = y + tr.rows, x + tr.cols
        sides = {"left": c - 3 < 0, "right": c + 3 >= self.w, "top": r - 3 < 0, "bottom": r + 3 >= self.h}
        tr.outside = {k: int(v.sum()) for k, v in sides.items()}
        tr.n_outside = int((sides["left"] | sides["right"] | sides["top"] | sides["bottom"]).sum())
        pre = self.blur_pre_clamp(sw.border)[r, c]
        tr.pre_clamp_max = int(pre.max())
        tr.over_255 = bool(tr.pre_clamp_max > 255)
        val = np.minimum(pre, 255) if sw.clamp else (pre & 0xFF)
        t0, t1 = val[0::2], val[1::2]
        tr.ties = int((t0 == t1).sum())
        bits = (t0 <= t1) if sw.le else (t0 < t1)
        desc = np.packbits(bits.astype(np.uint8).reshape(32, 8), axis=1, bitorder="little").reshape(32)
        tr.staging = staging(x, y, self.w, self.h, self.pitch, self.base_aligned)
        return int(np.asarray(angle, F32).view(np.uint32)), desc, tr
