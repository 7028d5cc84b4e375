"""Planted keypoints for k_describe (IC_Angle, 7x7 Gaussian, rBRIEF, patch staging), and the CPU
preconditions that prove each case reaches the edge it is named for. Shared by
tests/test_describe_definition.py (CPU) and tests/test_gpu_describe_adversarial.py (GPU); nothing
here touches a GPU.

The planting kit. The background of every image has a value range of at most minThFAST = 7, so FAST
is silent on it whatever its texture (a corner needs nine ring pixels more than the threshold away
from the centre). A key is one isolated impulse of high contrast. Around it:
  - a 43 x 43 patch of noise that is point-symmetric about the key textures the blurred window and,
    being symmetric, adds nothing to the moments of the 31-px disc;
  - a pixel at disc offset (u, v) raised by d adds (u d, v d) to (m10, m01): `bumps` set the moments,
    and so the angle, exactly.
The impulse itself sits on (0, 0) and adds nothing. reference() asserts from the oracle's raw FAST
keys that the planted impulses are the only keys.

A case is a DCase; pre(case, ref) asserts the case's precondition from the definition's traces
(ref["keys"][i].trace) and, where a wrong-answer switch of oracle/describe_definition.py applies,
that the switch changes the angle or the descriptor of at least one key of the case.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import fast_patterns as fp
from oracle import describe_definition as dd

BG = 100
PATCH_R = dd.PATCH_R
MIN_TH = 7


@dataclass
class DCase(fp.Case):
    variant: int = 0        # blur taps (set_opencv_model)
    pitch: int = 0          # row pitch of the images in the device batch; 0: the width
    planted: tuple = ()     # level-0 (x, y) of the impulses

    def __repr__(self):
        return self.name

    @property
    def batch_pitch(self):
        return self.pitch or self.img.shape[1]


@dataclass
class Key:
    level: int
    x: int
    y: int
    bits: int               # oracle: float32 angle bits
    desc: np.ndarray        # oracle: 32 bytes
    d_bits: int = 0         # definition
    d_desc: np.ndarray = None
    trace: dd.Trace = None
    staging_host: tuple = ()
    staging_batch: tuple = ()


# ---- the kit ------------------------------------------------------------------------------------
def _sym(rng, n, hi):
    p = rng.integers(0, hi + 1, n * n)
    p[n * n // 2 + 1:] = p[:n * n // 2][::-1]
    return p.reshape(n, n)


def sym_patch(seed, amp):
    """43 x 43 integers in [0, amp], point-symmetric about the centre: 5 x 5 blocks of [0, amp - 1] (a
    texture that survives the blur) plus pixel noise of [0, 1]."""
    rng = np.random.default_rng(seed)
    if amp <= 1:
        return _sym(rng, dd.PATCH_N, amp)
    coarse = np.kron(_sym(rng, 9, amp - 1), np.ones((5, 5), np.int64))[1:44, 1:44]
    return coarse + _sym(rng, dd.PATCH_N, 1)


def plant(img, x, y, c=120, seed=None, amp=4, bumps=()):
    """An impulse of contrast c (dark where bright does not fit) on (x, y), a symmetric texture patch
    of amplitude amp around it (seed None: none) and the bumps (u, v, d)."""
    h, w = img.shape
    bg = int(img[y, x])
    if seed is not None:
        p = sym_patch(seed, amp)
        y0, y1, x0, x1 = max(y - PATCH_R, 0), min(y + PATCH_R + 1, h), max(x - PATCH_R, 0), min(x + PATCH_R + 1, w)
        img[y0:y1, x0:x1] = bg + p[y0 - y + PATCH_R:y1 - y + PATCH_R, x0 - x + PATCH_R:x1 - x + PATCH_R]
    for u, v, d in bumps:
        img[y + v, x + u] += d
    img[y, x] = bg + c if bg + c <= 255 else bg - c


def moment_bumps(m10, m01, dmax=3):
    """Bumps on the disc's row 0 and column 0 that add exactly (m10, m01): greedy from the rim inwards."""
    out = []
    for axis, m in ((0, m10), (1, m01)):
        s, r = (1 if m > 0 else -1), abs(m)
        for k in range(dd.HALF_PATCH, 0, -1):
            d = min(dmax, r // k)
            if d:
                out.append((s * k, 0, d) if axis == 0 else (0, s * k, d))
                r -= d * k
        assert r == 0, (m10, m01)
    return out


def image(w, h, keys, bg=BG, texture=None):
    """keys: dicts of plant() arguments. texture: seed of a whole-image noise of range MIN_TH."""
    img = np.full((h, w), bg, np.int32)
    if texture is not None:
        img += np.random.default_rng(texture).integers(0, MIN_TH + 1, (h, w)) * (1 if bg + MIN_TH <= 255 else -1)
    for k in keys:
        plant(img, **k)
    assert img.min() >= 0 and img.max() <= 255
    out = img.astype(np.uint8)
    quiet = out.copy()
    for k in keys:
        quiet[k["y"], k["x"]] = quiet[k["y"], k["x"] - 1]
    # the background without the impulses stays within minThFAST around every pixel's ring
    assert int(quiet.max()) - int(quiet.min()) <= MIN_TH, "background range exceeds minThFAST"
    return out


def dcase(name, img, keys, pre, variant=0, pitch=0, nlevels=1, nfeat=300):
    return DCase(name=name, img=img, ini=20, min=MIN_TH, nlevels=nlevels, scale=1.2, nfeat=nfeat, pre=pre, variant=variant,
                 pitch=pitch, planted=tuple((k["x"], k["y"]) for k in keys))


# ---- what a switch would change -----------------------------------------------------------------
def switch_changes(ref, **sw):
    """Keys of the case whose angle or descriptor differ under the wrong-answer switch."""
    s = dd.Switches(**sw)
    out = []
    for k in ref["keys"]:
        bits, desc, _ = ref["levels"][k.level].describe(k.x, k.y, s)
        if bits != k.d_bits or not np.array_equal(desc, k.d_desc):
            out.append(k)
    return out


def need_switch(case, ref, **sw):
    assert switch_changes(ref, **sw), f"{case.name}: the switch {sw} changes no key of the case"


def key_at(ref, x, y, level=0):
    got = [k for k in ref["keys"] if (k.level, k.x, k.y) == (level, x, y)]
    assert len(got) == 1, f"no key on level {level} ({x}, {y})"
    return got[0]


# ---- edges of the level: the gather path and the blur's border mode ---------------------------------
# fastAtan2 of equal moments is 44.99 degrees: angle 45 takes pattern point (-13, -13) to row offset
# -18, 315 to column offset -18, 225 to row +18, 135 to column +18; those samples' taps leave a level
# whose edge is 19 or 20 px away
def _diag(sx, sy, n=30):
    return moment_bumps(sx * n, sy * n)


def _pre_edge(side, inner):
    def pre(case, ref):
        for k in ref["keys"]:
            if (k.x, k.y) in inner:
                assert k.staging_host[0] == "interior" and k.trace.n_outside == 0, (case.name, k.x, k.y, k.trace.outside)
            else:
                assert k.staging_host[0] == "gather" and k.staging_batch[0] == "gather"
                for s in side:
                    assert k.trace.outside[s] >= 1, f"{case.name}: key ({k.x}, {k.y}) reads no tap outside on the {s}"
        for border in ("reflect", "replicate"):
            need_switch(case, ref, border=border)
    return pre


EDGE_W, EDGE_H = 104, 136        # three keys 44 rows / two keys 44 columns apart


def edge_cases(seeds=(6, 13, 14, 14, 6)):      # texture seeds found on the CPU: the border switches change a bit
    w, h = EDGE_W, EDGE_H
    left = [dict(x=x, y=24 + 44 * i, seed=seeds[0] + 100 * i, bumps=_diag(1, -1)) for i, x in enumerate((19, 20, 21))]
    top = [dict(x=30 + 44 * i, y=y, seed=seeds[1] + 100 * i, bumps=_diag(1, 1)) for i, y in enumerate((19, 20))]
    hb = 104
    bottom = [dict(x=24 + 44 * i, y=y, seed=seeds[2] + 100 * i, bumps=_diag(-1, -1))
              for i, y in enumerate((hb - 22, hb - 21, hb - 20))]
    corner = [dict(x=19, y=19, seed=seeds[3], bumps=_diag(1, 1))]
    right = [dict(x=w - 20 - i, y=24 + 44 * i, seed=seeds[4] + 100 * i, bumps=_diag(-1, 1)) for i in range(2)]
    return [dcase("edge-left", image(w, h, left), left, _pre_edge(("left",), {(21, 24 + 88)})),
            dcase("edge-top", image(h, w, top), top, _pre_edge(("top",), set())),
            dcase("edge-bottom", image(h, hb, bottom), bottom, _pre_edge(("bottom",), {(24, hb - 22)})),
            dcase("edge-corner", image(w, w, corner), corner, _pre_edge(("left", "top"), set())),
            dcase("edge-right-taps", image(w, w, right), right, _pre_edge(("right",), set()))]


# ---- the right edge: where interior turns into gather, for every width residue ---------------------
def _pre_edge_right(case, ref):
    h, w = case.img.shape
    assert sorted(k.x for k in ref["keys"]) == list(range(w - 33, w - 19))
    flip = [k.x for k in ref["keys"] if k.staging_batch[0] == "gather"]
    for k in ref["keys"]:
        gx0 = (k.x - PATCH_R) & ~3
        assert (k.staging_batch == ("gather", "right-by-gx0")) == (gx0 + dd.STAGE_BYTES > w), (case.name, k.x)
        assert k.staging_batch[0] == "interior" or k.staging_batch[1] == "right-by-gx0"
        # a tight pitch that is no multiple of 4 leaves the host call no interior slot on level 0
        assert (k.staging_host == k.staging_batch) if w % 4 == 0 else (k.staging_host[0] == "gather")
    # both sides of the flip are present, and it falls on one column
    assert flip and len(flip) < 14 and sorted(flip) == list(range(min(flip), w - 19)), (case.name, flip)


def edge_right_cases():
    out = []
    for r in range(4):
        w, h = 100 + r, 19 + 14 * 8 + 21
        keys = [dict(x=w - 33 + i, y=22 + 8 * ((5 * i) % 14)) for i in range(14)]
        out.append(dcase(f"edge-right-w{r}", image(w, h, keys, texture=40 + r), keys, _pre_edge_right, pitch=(w + 3) & ~3))
    return out


# ---- interior realignment -----------------------------------------------------------------------
def _pre_align(sh):
    def pre(case, ref):
        for k in ref["keys"]:
            assert k.staging_host == k.staging_batch == ("interior", sh), (case.name, k.x, k.staging_host)
        # the patch's last column (offset +18 plus three taps), first and last rows are read
        assert any((k.trace.cols == 18).any() for k in ref["keys"]), f"{case.name}: no sample on column offset +18"
        assert any((k.trace.rows == -18).any() for k in ref["keys"]) and any((k.trace.rows == 18).any() for k in ref["keys"])
        assert all(k.trace.ties < 200 for k in ref["keys"])
        # and they matter: a wrong value on patch column 42, row 0 or row 42 alone flips a bit of some key
        lv = ref["levels"][0]
        for name, dx, dy in (("column 42", PATCH_R, None), ("row 0", None, -PATCH_R), ("row 42", None, PATCH_R)):
            hit = False
            for k in ref["keys"]:
                img = lv.img.copy()
                if dx is not None:
                    img[k.y - PATCH_R:k.y + PATCH_R + 1, k.x + dx] = 255
                else:
                    img[k.y + dy, k.x - PATCH_R:k.x + PATCH_R + 1] = 255
                bits, desc, _ = dd.Level(img, case.variant, lv.umax, lv.pattern).describe(k.x, k.y)
                assert bits == k.d_bits            # outside the disc: the angle stays
                hit |= not np.array_equal(desc, k.d_desc)
            assert hit, f"{case.name}: patch {name} changes no descriptor bit"
    return pre


ALIGN_SEEDS = (300, 310, 320, 331)   # texture seeds: found on the CPU where a case's first choice left a patch edge without a bit


def align_cases(seeds=ALIGN_SEEDS):
    out = []
    for sh in range(4):
        x0 = 24 + ((sh + 21 - 24) % 4)          # (x - 21) & 3 == sh
        keys = [dict(x=x0 + 44 * (i % 2), y=30 + 44 * (i // 2), seed=seeds[sh] + i, bumps=_diag(sx, sy))
                for i, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1)))]
        assert all((k["x"] - 21) & 3 == sh for k in keys)
        out.append(dcase(f"align-sh{sh}", image(120, 120, keys), keys, _pre_align(sh)))
    return out


# ---- fastAtan2 branches -------------------------------------------------------------------------
def _grid(moments, w=140, h=140):
    """One key per (m10, m01) on a 44-px lattice of flat background."""
    keys = []
    for i, (m10, m01) in enumerate(moments):
        keys.append(dict(x=24 + 44 * (i % 3), y=24 + 44 * (i // 3), bumps=moment_bumps(m10, m01)))
    assert len(keys) <= 9
    return image(w, h, keys), keys


def _pre_moments(moments, check):
    def pre(case, ref):
        for (x, y), (m10, m01) in zip(case.planted, moments):
            k = key_at(ref, x, y)
            assert (k.trace.m10, k.trace.m01) == (m10, m01), (case.name, x, y, k.trace.m10, k.trace.m01)
            check(case, k, m10, m01)
    return pre


def _f32(bits_of):
    return int(np.float32(bits_of).view(np.uint32))


def angle_cases():
    out = []
    axes = [(15, 0), (0, 15), (-15, 0), (0, -15), (0, 0)]
    want = dict(zip(axes, (0.0, 90.0, 180.0, 270.0, 0.0)))

    def chk_axes(case, k, m10, m01):
        assert k.d_bits == k.bits == _f32(want[(m10, m01)]), (case.name, m10, m01, k.trace.angle)
        assert k.trace.branch == ("ax>=ay" if abs(m10) >= abs(m01) else "ax<ay")
    img, keys = _grid(axes)
    out.append(dcase("angle-axes", img, keys, _pre_moments(axes, chk_axes)))

    diag = [(7, 7), (-7, 7), (-7, -7), (7, -7), (300, 300), (-300, -300)]

    def chk_diag(case, k, m10, m01):
        assert k.trace.tie and k.trace.branch == "ax>=ay"
        assert k.trace.reflections == (("180-a",) if m10 < 0 else ()) + (("360-a",) if m01 < 0 else ())
    img, keys = _grid(diag)
    out.append(dcase("angle-diagonal-tie", img, keys, _pre_moments(diag, chk_diag)))

    edge = [(sx * a, sy * b) for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)) for a, b in ((3, 2), (2, 3))]

    def chk_edge(case, k, m10, m01):
        assert abs(abs(m10) - abs(m01)) == 1 and not k.trace.tie
        assert k.trace.branch == ("ax>=ay" if abs(m10) > abs(m01) else "ax<ay")
    img, keys = _grid(edge)
    out.append(dcase("angle-branch-edge", img, keys, _pre_moments(edge, chk_edge)))

    # every disc pixel right of the centre column raised by the whole sub-threshold range: the largest
    # m10 the kit plants; m01 = -1 from one pixel
    um = dd.umax_table()
    half = [(u, v, MIN_TH - 1) for v in range(-15, 16) for u in range(1, um[abs(v)] + 1)]
    m10_max = sum(u * d for u, _, d in half)
    wrap = [dict(x=40, y=40, bumps=half + [(0, -1, 1)]), dict(x=100, y=40, bumps=half + [(0, 1, 1)])]

    def pre_wrap(case, ref):
        k, k2 = key_at(ref, 40, 40), key_at(ref, 100, 40)
        assert (k.trace.m10, k.trace.m01) == (m10_max, -1) and (k2.trace.m10, k2.trace.m01) == (m10_max, 1)
        a = np.float32(k.trace.angle)
        assert k.trace.reflections == ("360-a",) and np.float32(359.99) < a < np.float32(360), a
        assert k.d_bits == k.bits
        # the radians fed to cosf / sinf are the largest any key of the kit produces
        assert np.float32(a) * dd.FACTOR_PI > np.float32(6.2831)
    out.append(dcase("angle-near-wrap", image(140, 80, wrap), wrap, pre_wrap))
    return out


# ---- the last row and column of the blurred window decide a bit ---------------------------------------
# A frame of two pixels at patch offsets 20 and 21 (outside the disc), d above or below a flat field:
# the blurred value on offset 18 sees both frame pixels (taps 18 + 34 of 256: one grey level at
# d = 5), on offset 17 one (a third of a level: none). A sample on offset 18 against a partner on the
# flat field gives a bit that only the outermost blurred row or column decides.
def offset18_cases():
    out = []
    for name, d in (("raised", 5), ("lowered", -5)):
        keys = []
        for i, (sx, sy) in enumerate(((1, 1), (-1, 1), (-1, -1), (1, -1))):
            frame = [(u, v, d) for u in range(-PATCH_R, PATCH_R + 1) for v in range(-PATCH_R, PATCH_R + 1)
                     if max(abs(u), abs(v)) >= PATCH_R - 1]
            keys.append(dict(x=24 + 44 * (i % 2), y=24 + 44 * (i // 2), bumps=frame + moment_bumps(30 * sx, 30 * sy, 2)))

        def pre(case, ref):
            lv = ref["levels"][0]
            by_row = by_col = 0
            for k in ref["keys"]:
                assert k.trace.max_offset == 18
                desc17 = lv.describe(k.x, k.y, dd.Switches(window=17))[1]
                flipped = np.unpackbits(desc17 ^ k.d_desc, bitorder="little")          # pair index
                for pair in np.nonzero(flipped)[0]:
                    r, c = np.abs(k.trace.rows[2 * pair:2 * pair + 2]), np.abs(k.trace.cols[2 * pair:2 * pair + 2])
                    assert max(r.max(), c.max()) == 18
                    by_row += int(r.max() == 18)
                    by_col += int(c.max() == 18)
            assert by_row and by_col, f"{case.name}: bits decided by the outermost row {by_row}, column {by_col}"
        out.append(dcase(f"offset-18-{name}", image(112, 112, keys, bg=BG + (0 if d > 0 else 5)), keys, pre))
    return out


# ---- the disc's rim -----------------------------------------------------------------------------
def disc_rim_cases():
    um = dd.umax_table()
    rows = (0, 3, -7, 11, -15, 15)

    def rim(sign_in, sign_out):
        b = []
        for i, v in enumerate(rows):
            s, t = (1 if i % 2 == 0 else -1), (1 if i % 3 == 0 else -1)
            b.append((s * sign_in * um[abs(v)], v, 3))            # last column inside
            b.append((t * sign_out * (um[abs(v)] + 1), v, 2))     # first column outside
        # row 0 on both sides: u = -15 inside, u = -16 outside
        return b + [(-sign_in * um[0], 0, 1), (-sign_out * (um[0] + 1), 0, 1)]
    keys = [dict(x=30, y=30, bumps=rim(1, 1)), dict(x=90, y=30, bumps=rim(1, -1)), dict(x=30, y=90, bumps=rim(-1, 1))]

    def pre(case, ref):
        flat = _f32(0.0)
        for k in ref["keys"]:
            assert k.d_bits == k.bits != flat
            m10, m01 = k.trace.m10, k.trace.m01
            lv = ref["levels"][0]
            assert lv.moments(k.x, k.y, 1) != (m10, m01) and lv.moments(k.x, k.y, -1) != (m10, m01)
        assert len(switch_changes(ref, mask=1)) == len(ref["keys"]) and len(switch_changes(ref, mask=-1)) == len(ref["keys"])
    return [dcase("disc-rim", image(120, 120, keys), keys, pre)]


# ---- the clamp: taps that sum to 257 on a saturated field -----------------------------------------
def _sat_keys():
    return [dict(x=24 + 44 * (i % 2), y=24 + 44 * (i // 2), c=200 + 10 * i) for i in range(4)]


def saturated_cases():
    keys = _sat_keys()
    white, black = image(112, 112, keys, bg=255), image(112, 112, keys, bg=0)

    def pre_v1(case, ref):
        assert all(k.trace.pre_clamp_max == 257 and k.trace.over_255 for k in ref["keys"])
        need_switch(case, ref, clamp=False)

    def pre_v0(case, ref):
        assert all(k.trace.pre_clamp_max == 255 and not k.trace.over_255 for k in ref["keys"])
        assert not switch_changes(ref, clamp=False)

    def pre_black(case, ref):
        assert all(not k.trace.over_255 and k.trace.ties > 150 for k in ref["keys"])
    return [dcase("saturated-variant1", white, keys, pre_v1, variant=1), dcase("saturated-variant0", white, keys, pre_v0),
            dcase("black-variant1", black, keys, pre_black, variant=1)]


# ---- ties of the comparison ---------------------------------------------------------------------
def tie_cases():
    flat = [dict(x=30, y=30), dict(x=80, y=60, c=60)]
    two = [dict(x=30, y=30, seed=501, amp=1), dict(x=80, y=60, seed=502, amp=1)]

    def pre_flat(case, ref):
        assert all(k.trace.ties >= 200 and (k.trace.m10, k.trace.m01) == (0, 0) for k in ref["keys"])
        assert len(switch_changes(ref, le=True)) == len(ref["keys"])

    def pre_two(case, ref):
        lv = ref["levels"][0]
        assert set(np.unique(case.img)) <= {BG, BG + 1, BG + 120}
        b = lv.blurred()
        far = b[10:20, 50:70]        # away from the impulses: blurred two-valued noise
        assert int(far.max()) - int(far.min()) <= 1
        assert all(30 <= k.trace.ties < 256 for k in ref["keys"])
        need_switch(case, ref, le=True)
    return [dcase("compare-ties", image(112, 92, flat), flat, pre_flat),
            dcase("compare-ties-two-valued", image(112, 92, two), two, pre_two)]


# ---- exact half-integer sample sums ---------------------------------------------------------------
# (m10, m01) found on the CPU by sweeping [-360, 360]^2 (tests/test_describe_definition.py::test_window_bound
# finds the smaller ones again): fastAtan2 of the pair gives an angle whose libm cosf / sinf put a sample sum px b + py a or
# px a - py b on an exact half-integer
ROUND_HALF_MOMENTS = ((49, 3), (-3, 49), (-49, 3), (-129, 28), (-229, 51), (12, -314), (-12, -314), (194, -9), (50, -193))


def round_half_cases(seeds=None):
    if not ROUND_HALF_MOMENTS:
        return []
    seeds = seeds or ROUND_HALF_SEEDS
    keys = [dict(x=24 + 44 * (i % 3), y=24 + 44 * (i // 3), seed=s, bumps=moment_bumps(m10, m01))
            for i, ((m10, m01), s) in enumerate(zip(ROUND_HALF_MOMENTS, seeds))]

    def pre(case, ref):
        for (x, y), (m10, m01) in zip(case.planted, ROUND_HALF_MOMENTS):
            k = key_at(ref, x, y)
            assert (k.trace.m10, k.trace.m01) == (m10, m01) and k.trace.n_half >= 1, (case.name, m10, m01)
        need_switch(case, ref, rounding="half-away")
        need_switch(case, ref, rounding="floor-plus-half")
    return [dcase("round-half", image(140, 140, keys), keys, pre)]


ROUND_HALF_SEEDS = tuple(4000 + i for i in range(9))   # texture seeds found on the CPU: both rounding switches change a bit


# ---- the slot walk of a wave ------------------------------------------------------------------------
# orbfe_engine.hip, build_geom: L.out_cap = max(budget + 3, 4 n_ini); L.out_off = the sum of the
# capacities below ("L.out_off = out_off; out_off += L.out_cap"). Key i of level l, in octree order,
# is flat slot out_off[l] + i. orbfe_kernels.hip, k_describe<KPW>: a wave takes the KPW = 4 slots from
# flat0 = 4 * (wave index) ("flat0 = ((lb % gridDim.x) * DP_WPB + wave) * KPW"), finds each slot's
# level by walking out_off upwards and treats slots past the level's n as invalid (desc_slot).
KPW = 4
WAVE_SEED, WAVE_NFEAT = 1, 2000      # found on the CPU: the seed and budget at which the precondition holds


def slot_groups(case, ref):
    """Per group of KPW flat slots: the (level, Key) of its valid slots, in slot order."""
    from oracle import octree_definition as od
    h, w = case.img.shape
    budget, off, flat = ref["budget"], 0, {}
    keys = iter(ref["keys"])
    for l, (lw, lh) in enumerate(fp.level_sizes(w, h, case.nlevels, case.scale)):
        n_ini = od.root_geometry(lw - 2 * fp.B, lh - 2 * fp.B)[0]
        for i in range(len(ref["oct"][l])):
            flat[off + i] = next(keys)
            assert flat[off + i].level == l
        assert len(ref["oct"][l]) <= max(budget[l] + 3, 4 * n_ini)
        off += max(budget[l] + 3, 4 * n_ini)
    groups = {}
    for f, k in flat.items():
        groups.setdefault(f // KPW, []).append((f, k))
    return [groups[g] for g in sorted(groups)], off


def sides_of(k, w, h):
    px0, py0 = k.x - PATCH_R, k.y - PATCH_R
    return {s for s, hit in (("left", px0 < 0), ("top", py0 < 0), ("bottom", py0 + dd.PATCH_N > h),
                             ("right", (px0 & ~3) + dd.STAGE_BYTES > w)) if hit}


def pre_wave_mix(case, ref):
    groups, total = slot_groups(case, ref)
    trans, straddle = set(), 0
    for g in groups:
        for (f0, a), (f1, b) in zip(g, g[1:]):
            if f1 == f0 + 1:       # consecutive slots of one wave: b's patch is prefetched while a is described
                trans.add((a.staging_batch[0], b.staging_batch[0]))
        straddle += len({k.level for _, k in g}) > 1
    assert trans == {(p, q) for p in ("interior", "gather") for q in ("interior", "gather")}, sorted(trans)
    assert straddle >= 1, f"{case.name}: no group of {KPW} slots holds valid slots of two levels"
    assert len(groups[-1]) in (1, 2, 3), f"{case.name}: the last group holds {len(groups[-1])} valid slots"
    for l, lv in enumerate(ref["levels"]):
        ks = [k for k in ref["keys"] if k.level == l]
        sides = set().union(*[sides_of(k, lv.w, lv.h) for k in ks])
        assert sides == {"left", "top", "bottom", "right"}, f"{case.name}: level {l} has gather keys on {sorted(sides)} only"
        shs = {k.staging_batch[1] for k in ks if k.staging_batch[0] == "interior"}
        assert shs == {0, 1, 2, 3}, f"{case.name}: level {l} has interior shifts {sorted(shs)} only"


def wave_cases(seed=WAVE_SEED, nfeat=WAVE_NFEAT):
    # 320 x 264: the smallest 8-level geometry the cell grid accepts (level 7 is 89 x 74)
    return [dcase("wave-mix", fp.noise_image(seed, 320, 264), (), pre_wave_mix, nlevels=8, nfeat=nfeat)]


# ---- a level without keys between two with keys -----------------------------------------------------
# iniThFAST = minThFAST = 20 (octree_patterns' k-0-on-level-1). An impulse of contrast 21 or 22 is a key
# on level 0 only: the bilinear taps of level 1 keep at most 0.9 x 0.9 of it. A 2 x 2 block is no key
# on level 0 (its four pixels tie and strict suppression removes them all); on phases found on the
# CPU level 1 spreads it below the threshold again, and level 2 gathers it into one pixel above it.
EMPTY_IMPULSES = ((30, 30, 21), (100, 40, 22), (40, 75, 22), (110, 80, 21))
EMPTY_BLOCKS = ((66, 52, 27),)
EMPTY_W, EMPTY_H = 140, 112     # level 2 is 97 x 78, above the 73 px the cell grid accepts


def pre_empty_level(case, ref):
    n = [len(ref["oct"][l]) for l in range(3)]
    raw = [int(ref["cells"][l][0].sum()) for l in range(3)]
    assert raw[1] == 0 and n[1] == 0 and n[0] == len(EMPTY_IMPULSES) and n[2] >= 1, (case.name, raw, n)
    assert sorted((k.x, k.y) for k in ref["keys"] if k.level == 0) == sorted((x, y) for x, y, _ in EMPTY_IMPULSES)
    # the level-2 slots lie past level 1's empty range of the slot walk
    groups, _ = slot_groups(case, ref)
    assert {k.level for g in groups for _, k in g} == {0, 2}


def empty_level_cases(blocks=EMPTY_BLOCKS):
    img = np.zeros((EMPTY_H, EMPTY_W), np.uint8)
    for x, y, c in EMPTY_IMPULSES:
        img[y, x] = c
    for x, y, c in blocks:
        img[y:y + 2, x:x + 2] = c
    return [DCase(name="empty-level-between", img=img, ini=20, min=20, nlevels=3, scale=1.2, nfeat=300, pre=pre_empty_level)]


def all_cases():
    return (edge_cases() + edge_right_cases() + align_cases() + angle_cases() + offset18_cases() + disc_rim_cases() +
            saturated_cases() + tie_cases() + round_half_cases() + wave_cases() + empty_level_cases())


# ---- references ---------------------------------------------------------------------------------
_REFS = {}


def oracle_keys(ref, nlevels):
    """Key records of the oracle's output in output order (no lapping area: the levels in octree order)."""
    keys, i = [], 0
    for l in range(nlevels):
        o = ref["oct"][l]
        for x, y in zip(o["x"].astype(int).tolist(), o["y"].astype(int).tolist()):
            kp = ref["kp"][i]
            assert int(kp["octave"]) == l
            keys.append(Key(l, x, y, int(np.float32(kp["angle"]).view(np.uint32)), ref["desc"][i].copy()))
            i += 1
    assert i == len(ref["kp"])
    return keys


def reference(case, oracle_lib):
    """Oracle outputs and intermediates of a case (test_gpu_fast_adversarial.build_ref, under the case's
    blur taps) plus, per key in output order, the definition's result and trace and the staging class of
    the host call and of the device batch. Computed once per case, never modified."""
    if case.name not in _REFS:
        from test_gpu_fast_adversarial import build_ref
        ref = build_ref(oracle_lib, case.img, case.nfeat, case.scale, case.nlevels, case.ini, case.min)
        ora = oracle_lib.OracleExtractor(case.nfeat, case.scale, case.nlevels, case.ini, case.min, blur_variant=case.variant)
        umax = ora.level_info()["umax"].tolist()
        ref["budget"] = [int(v) for v in ora.level_info()["per_level"]]
        if case.variant:
            ref["mono"], ref["kp"], ref["desc"] = ora(case.img)
        ora.close()
        if case.planted:
            raw = ref["cells"][0][1]
            got = sorted((x + fp.B, y + fp.B) for lst in raw for x, y, _ in lst)
            assert got == sorted(case.planted), f"{case.name}: FAST keys {got} differ from the planted {sorted(case.planted)}"
        w = case.img.shape[1]
        ref["levels"] = [dd.Level(ref["pyr"][l], case.variant, umax) for l in range(case.nlevels)]
        ref["keys"] = oracle_keys(ref, case.nlevels)
        for k in ref["keys"]:
            lv = ref["levels"][k.level]
            k.d_bits, k.d_desc, k.trace = lv.describe(k.x, k.y)
            # level 0 is read in place with the caller's pitch; the pyramid's levels are 16-aligned
            ph, pb = (w, case.batch_pitch) if k.level == 0 else (16, 16)
            k.staging_host = dd.staging(k.x, k.y, lv.w, lv.h, ph)
            k.staging_batch = dd.staging(k.x, k.y, lv.w, lv.h, pb)
        _REFS[case.name] = ref
    return _REFS[case.name]
