"""Seeded adversarial images for the FAST cell loop, and the CPU preconditions that prove each one
reaches the branch it is meant for. Shared by tests/test_fast_definition.py (CPU) and
tests/test_gpu_fast_adversarial.py (GPU); nothing here touches a GPU or the C++ oracle.

A case is a Case(name, img, ini_th, min_th, nlevels, scale, nfeatures, pre); pre(case) asserts the
case's precondition from oracle/fast_definition.py alone, on level 0 (the input image).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np

from oracle import fast_definition as fd

B = fd.BORDER
D0 = B + 3            # first detection row / column of a level
TH_PAIRS = [(20, 7), (7, 7), (40, 0), (255, 254)]


@dataclass
class Case:
    name: str
    img: np.ndarray
    ini: int = 20
    min: int = 7
    nlevels: int = 1
    scale: float = 1.2
    nfeat: int = 300
    pre: Callable | None = None

    def __repr__(self):
        return self.name


# ---- per-cell reference facts -------------------------------------------------------------------
def cell_facts(img, ini, mn):
    """Per cell of level 0: (rect, keys at ini alone, keys at min alone, emitted keys), ROI coords."""
    h, w = img.shape
    n_cols, n_rows, w_cell, h_cell = fd.grid(w, h)
    out = []
    for i in range(n_rows):
        for j in range(n_cols):
            # a skipped cell: an empty rectangle, no keys
            r0, r1, c0, c1 = fd.cell_rect(w, h, i, j) or (B + i * h_cell, B + i * h_cell, B + j * w_cell, B + j * w_cell)
            roi = img[r0:r1, c0:c1]
            ki, km = fd.fast9(roi, ini), fd.fast9(roi, mn)
            out.append(((r0, r1, c0, c1), ki, km, ki or km))
    return out


def cell_of(x, y, w, h):
    """Cell index of level pixel (x, y) of the detection area."""
    n_cols, _, w_cell, h_cell = fd.grid(w, h)
    return ((y - D0) // h_cell) * n_cols + (x - D0) // w_cell


# ---- threshold edges: isolated impulses on a flat background ------------------------------------
# An isolated impulse of contrast c has M = c exactly (its whole ring is background), so it is a
# corner at threshold t iff c > t, with score c - 1.
CLASS_MID, CLASS_STRONG, CLASS_WEAK, CLASS_MIX = range(4)


def impulse_contrasts(ini, mn):
    return [c for c in (mn, mn + 1, ini, ini + 1) if 0 < c <= 255]


def impulse_image(seed, w, h, ini, mn, classes=(CLASS_MID, CLASS_STRONG, CLASS_WEAK, CLASS_MIX), off=(0, 0)):
    """Impulses on a lattice of pitch 7 (offset `off` from the first detection pixel). Cell k draws
    its contrasts by class classes[k % 4]: MID only min < c <= ini, STRONG one c = ini + 1 among
    weaker ones, WEAK only contrasts that cannot be emitted, MIX any. Bright on background 0 where
    c > 127 is needed, else bright or dark at random around 128."""
    rng = np.random.default_rng(seed)
    cs = impulse_contrasts(ini, mn)
    # contrast 1 is a corner at threshold 0 with score 0, which strict suppression never keeps
    sets = {CLASS_MID: [c for c in cs if mn < c <= ini], CLASS_WEAK: [c for c in cs if c <= mn or c == 1],
            CLASS_STRONG: [c for c in cs if c <= ini], CLASS_MIX: cs}
    big = max(cs) > 127
    bg = 0 if big else 128
    img = np.full((h, w), bg, np.uint8)
    seen_strong = set()
    for y in range(D0 + off[1], h - D0, 7):
        for x in range(D0 + off[0], w - D0, 7):
            k = cell_of(x, y, w, h)
            cls = classes[k % 4]
            pool = sets[cls]
            if cls == CLASS_STRONG and k not in seen_strong and ini + 1 in cs:
                c = ini + 1            # exactly one strong impulse, the first lattice point of the cell
                seen_strong.add(k)
            elif not pool or rng.random() < 0.25:
                continue
            else:
                c = int(rng.choice(pool))
            sign = 1 if big or rng.random() < 0.5 else -1
            img[y, x] = bg + sign * c
    return img


def pre_impulses(case, want=("fallback", "dropped", "empty")):
    """fallback: a cell whose only corners have min < M <= ini and that emits them; dropped: a cell
    with a corner above ini whose weaker corners (present at min) are not emitted; empty: a cell
    that holds impulses, all with M <= min (or score 0), and emits nothing."""
    img = case.img
    seen = set()
    for (r0, r1, c0, c1), ki, km, em in cell_facts(img, case.ini, case.min):
        roi = img[r0 + 3:r1 - 3, c0 + 3:c1 - 3]
        has_impulse = bool((roi != img[0, 0]).any())
        if not ki and km and em == km:
            assert all(case.min <= s < case.ini for _, _, s in km)
            seen.add("fallback")
        if ki and len(km) > len(ki) and em == ki:
            seen.add("dropped")
        if has_impulse and not em:
            seen.add("empty")
    assert set(want) <= seen, f"{case.name}: wanted {want}, reference shows {sorted(seen)}"


# what each pair can show at all. ini == min: the second attempt repeats the first, so no cell can
# fall back or drop weaker corners, whatever the contrasts. ini == 255: no contrast exceeds 255, so
# no corner lies above ini
IMPULSE_WANT = {(20, 7): ("fallback", "dropped", "empty"), (7, 7): ("empty",),
                (40, 0): ("fallback", "dropped", "empty"), (255, 254): ("fallback", "empty")}


def threshold_cases():
    out = []
    for ini, mn in TH_PAIRS:
        for off in ((0, 0), (6, 6)):   # first and last detection column / row of the 35-px cells
            img = impulse_image(1000 + ini + off[0], 137, 102, ini, mn, off=off)
            want = IMPULSE_WANT[(ini, mn)]
            out.append(Case(f"impulses-{ini}-{mn}-off{off[0]}", img, ini, mn, 2, 1.2, 300,
                            lambda c, want=want: pre_impulses(c, want)))
    return out


# ---- threshold edges behind the candidate test ---------------------------------------------------
# A centre whose 9-arc has contrast `strong` except one pixel of contrast `weak` at an odd ring
# position: M = weak, while every even opposite pair still has a member of contrast `strong`, so
# the pixel is a candidate at any threshold below `strong` and only the exact M > th decides.
def arc_structure(img, x, y, sign, strong, weak, start=0):
    v = int(img[y, x])
    for n in range(9):
        k = (start + n) % 16
        dx, dy = fd.RING[k]
        img[y + dy, x + dx] = v - sign * (weak if n == 3 else strong)


def arc_image(w=137, h=102, ini=20, mn=7):
    """Top row of cells: arcs with M = ini and M = ini + 1. Bottom row: nothing above ini, arcs with
    M = min and M = min + 1 (the fallback decides them)."""
    n_cols, n_rows, w_cell, h_cell = fd.grid(w, h)
    img = np.full((h, w), 100, np.uint8)
    k = 0
    for i in range(n_rows):
        th, strong = (ini, ini + 10) if i == 0 else (mn, min(mn + 3, ini))
        for j in range(n_cols):
            for oy in (8, 20):
                for ox in (8, 20):
                    arc_structure(img, D0 + j * w_cell + ox, D0 + i * h_cell + oy, 1 if k % 2 else -1, strong,
                                  th + (k // 2) % 2, start=2 * (k % 8))
                    k += 1
    return img


def pre_arcs(case):
    img = case.img
    h, w = img.shape
    m = fd.arc_max(img[B:h - B, B:w - B])          # M over the detection area
    facts = cell_facts(img, case.ini, case.min)
    n_cols, _, w_cell, h_cell = fd.grid(w, h)
    for th, fallback in ((case.ini, False), (case.min, True)):
        bright, dark = pretest_masks(img, th)
        cand = bright | dark
        for edge in (th, th + 1):                  # a candidate with M == th (no corner) and M == th + 1 (corner)
            ys, xs = np.nonzero(cand & (m == edge))
            cells = {cell_of(D0 + x, D0 + y, w, h) for x, y in zip(xs, ys)}
            cells = {c for c in cells if bool(facts[c][1]) != fallback}   # decided by the attempt at th
            assert cells, f"{case.name}: no candidate with M == {edge} decided at threshold {th}"


def arc_cases():
    return [Case("threshold-arcs", arc_image(), 20, 7, 2, pre=pre_arcs)]


# ---- saturation ---------------------------------------------------------------------------------
def saturation_image(seed, w, h, invert):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w), np.uint8)
    ys, xs = np.mgrid[D0:h - D0:5, D0:w - D0:5]
    keep = rng.random(ys.shape) < 0.6
    img[ys[keep], xs[keep]] = 255
    return (255 - img) if invert else img


def pre_saturation(case):
    _, lists = fd.cell_keys(case.img, case.ini, case.min)
    scores = [s for l in lists for _, _, s in l]
    assert scores and max(scores) == 254, f"{case.name}: maximum score {max(scores, default=None)}"


def saturation_cases():
    return [Case(f"saturation-{'dark' if inv else 'bright'}", saturation_image(7 + inv, 137, 102, inv), 20, 7, 2,
                 pre=pre_saturation) for inv in (0, 1)]


# ---- NMS ties -----------------------------------------------------------------------------------
# Adjacent impulses are not on each other's rings, so each keeps M = its own contrast: equal
# neighbours tie and strict suppression removes them all; across a cell boundary each member is
# outside the other cell's detection rectangle, scores 0 there, and survives in its own cell.
NMS_SHAPES = {"h2": [(0, 0, 50), (1, 0, 50)], "v2": [(0, 0, 50), (0, 1, 50)], "d2": [(0, 0, 50), (1, 1, 50)],
              "a2": [(1, 0, 50), (0, 1, 50)], "q4": [(0, 0, 50), (1, 0, 50), (0, 1, 50), (1, 1, 50)],
              "h2u": [(0, 0, 50), (1, 0, 55)], "v2u": [(0, 0, 60), (0, 1, 50)], "d2u": [(0, 0, 50), (1, 1, 51)],
              "one": [(0, 0, 50)]}


def nms_image(w=137, h=102, sign=1):
    n_cols, n_rows, w_cell, h_cell = fd.grid(w, h)
    img = np.full((h, w), 100, np.uint8)

    def put(x, y, shape):
        for dx, dy, c in NMS_SHAPES[shape]:
            img[y + dy, x + dx] = 100 + sign * c

    names = list(NMS_SHAPES)
    k = 0
    for i in range(n_rows):
        for j in range(n_cols):
            for oy in (5, 14, 23):           # in-cell structures, 9 apart, clear of the boundaries
                for ox in (5, 14, 23):
                    put(D0 + j * w_cell + ox, D0 + i * h_cell + oy, names[k % len(names)])
                    k += 1
    for j in range(1, n_cols):               # pairs across a vertical cell boundary
        bx = D0 + j * w_cell
        put(bx - 1, D0 + 9, "h2")
        put(bx - 1, D0 + 18, "d2")
        if n_rows > 1:
            put(bx - 1, D0 + h_cell + 9, "a2")
    for i in range(1, n_rows):               # pairs across a horizontal cell boundary
        by = D0 + i * h_cell
        put(D0 + 9, by - 1, "v2")
        put(D0 + 18, by - 1, "d2")
        for j in range(1, n_cols):           # a 2 x 2 block on a four-cell junction
            if j % 2:
                put(D0 + j * w_cell - 1, by - 1, "q4")
    return img


def pre_nms(case):
    img = case.img
    h, w = img.shape
    facts = cell_facts(img, case.ini, case.min)
    # (a) an adjacent pair of survivors that sit in different cells
    surv = {}
    for k, ((r0, _, c0, _), _, _, em) in enumerate(facts):
        for x, y, _ in em:
            surv[(c0 + x, r0 + y)] = k
    straddle = sum(1 for (x, y), k in surv.items() for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1))
                   if surv.get((x + dx, y + dy), k) != k)
    assert straddle >= 3, f"{case.name}: {straddle} straddling survivor pairs"
    # (b) an in-cell pair of adjacent corners of equal score, neither of which survives
    dead = 0
    for (r0, r1, c0, c1), ki, _, em in facts:
        assert ki and em == ki
        s, corner = fd.score_map(img[r0:r1, c0:c1], case.ini)
        alive = {(x, y) for x, y, _ in em}
        ys, xs = np.nonzero(corner)
        for x, y in zip(xs, ys):
            for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1)):
                x2, y2 = x + dx, y + dy
                if 0 <= x2 < s.shape[1] and y2 < s.shape[0] and corner[y2, x2] and s[y2, x2] == s[y, x]:
                    assert (x, y) not in alive and (x2, y2) not in alive
                    dead += 1
    assert dead >= 4, f"{case.name}: {dead} suppressed equal pairs"
    # (c) unequal neighbours: some corner is suppressed by a strictly better neighbour while that one lives
    ncorner = sum(int(fd.score_map(img[r0:r1, c0:c1], case.ini)[1].sum()) for (r0, r1, c0, c1), *_ in facts)
    assert 0 < len(surv) < ncorner


def nms_cases():
    return [Case(f"nms-ties-{'bright' if s > 0 else 'dark'}", nms_image(sign=s), 20, 7, 2, pre=pre_nms) for s in (1, -1)]


# ---- both signs ---------------------------------------------------------------------------------
def checkerboard(w, h, period, flip=0.0, seed=0):
    yy, xx = np.mgrid[0:h, 0:w]
    img = ((((xx // period) + (yy // period)) & 1) * 255).astype(np.uint8)
    if flip:
        rng = np.random.default_rng(seed)
        img = np.where(rng.random(img.shape) < flip, 255 - img, img).astype(np.uint8)
    return img


def polarities(img, ini, mn):
    """(#bright, #dark) keys: the keypoint against the mean of its ring."""
    h, w = img.shape
    _, lists = fd.cell_keys(img, ini, mn)
    a = img.astype(np.int32)
    nb = nd = 0
    for l in lists:
        for x, y, _ in l:
            ring = np.mean([a[B + y + dy, B + x + dx] for dx, dy in fd.RING])
            if a[B + y, B + x] > ring:
                nb += 1
            else:
                nd += 1
    return nb, nd


def pre_both_signs(case):
    nb, nd = polarities(case.img, case.ini, case.min)
    assert nb > 0 and nd > 0, f"{case.name}: {nb} bright, {nd} dark keys"


def pretest_masks(img, th):
    """(bright possible, dark possible) over the detection area: every opposite ring pair (k, k + 8),
    k = 0, 2, 4, 6, has a member > v + th (resp. < v - th). Each 9-arc holds one pixel of every such
    pair, so this is necessary for a corner; it is not sufficient, and it can hold while M == th."""
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[D0:h - D0, D0:w - D0]
    bright, dark = np.ones(v.shape, bool), np.ones(v.shape, bool)
    for k in (0, 2, 4, 6):
        (ax, ay), (bx, by) = fd.RING[k], fd.RING[k + 8]
        p = a[D0 + ay:h - D0 + ay, D0 + ax:w - D0 + ax]
        q = a[D0 + by:h - D0 + by, D0 + bx:w - D0 + bx]
        bright &= np.maximum(p, q) > v + th
        dark &= np.minimum(p, q) < v - th
    return bright, dark


def both_sign_pretest(img, th):
    """Number of pixels of the detection area that are candidates of both signs at once."""
    bright, dark = pretest_masks(img, th)
    return int((bright & dark).sum())


def pre_pure_checkerboard(case):
    # a regular board never has 9 contiguous ring pixels of one colour: all candidates, no corner
    counts, _ = fd.cell_keys(case.img, case.ini, case.min)
    assert counts.sum() == 0


def pre_three_level(case):
    pre_both_signs(case)
    assert both_sign_pretest(case.img, case.ini) > 0 and both_sign_pretest(case.img, case.min) > 0


def both_sign_cases():
    rng = np.random.default_rng(21)
    out = [Case("binary-random", (rng.integers(0, 2, (102, 137)) * 255).astype(np.uint8), 20, 7, 2, pre=pre_both_signs)]
    for p in (1, 2, 3):
        out.append(Case(f"checkerboard-{p}", checkerboard(137, 102, p), 20, 7, 2, pre=pre_pure_checkerboard))
        out.append(Case(f"checkerboard-{p}-flipped", checkerboard(137, 102, p, 0.12, 30 + p), 20, 7, 2,
                        pre=pre_both_signs))
    # a mid-grey centre between black and white ring pixels: the only way to pass the pretest for both signs
    out.append(Case("three-level-random", rng.choice(np.array([0, 128, 255], np.uint8), (102, 137)), 20, 7, 2,
                    pre=pre_three_level))
    return out


# ---- dense --------------------------------------------------------------------------------------
def noise_image(seed, w, h, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w), dtype=np.uint8)


def pre_dense(case):
    counts, _ = fd.cell_keys(case.img, case.ini, case.min)
    assert counts.max() > 64, f"{case.name}: fullest cell has {counts.max()} keys"


def pre_low_amplitude(case):
    facts = cell_facts(case.img, case.ini, case.min)
    nonempty = [f for f in facts if f[3]]
    fell = [f for f in nonempty if not f[1]]
    assert nonempty and 2 * len(fell) > len(nonempty), f"{case.name}: {len(fell)} of {len(nonempty)} cells fell back"


def dense_cases():
    return [Case("dense-noise", noise_image(3, 160, 128), 20, 7, 3, nfeat=500, pre=pre_dense),
            Case("low-amplitude-noise", noise_image(4, 160, 128, 100, 130), 20, 7, 3, nfeat=500, pre=pre_low_amplitude)]


# ---- flat ---------------------------------------------------------------------------------------
def pre_flat(case):
    counts, _ = fd.cell_keys(case.img, case.ini, case.min)
    assert counts.sum() == 0


def flat_cases():
    return [Case(f"flat-{v}", np.full((102, 137), v, np.uint8), 20, 7, 2, pre=pre_flat) for v in (0, 255)]


def content_cases():
    return threshold_cases() + arc_cases() + saturation_cases() + nms_cases() + both_sign_cases() + dense_cases() + flat_cases()


# ---- geometry list ------------------------------------------------------------------------------
# (w, h, nlevels): chosen with geometry_facts below (tests/test_fast_definition.py asserts the coverage)
GEOMETRIES = [(73, 73, 1), (101, 101, 1), (102, 102, 1), (175, 80, 1), (100, 160, 1), (172, 75, 1), (131, 97, 2),
              (139, 103, 1)]


def level_sizes(w, h, nlevels, scale=1.2):
    """Level sizes as the extractor derives them: float32 scale chain, inverse, round half to even."""
    s, out = np.float32(1.0), []
    for l in range(nlevels):
        if l:
            s = np.float32(np.float64(s) * np.float64(np.float32(scale)))
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def geometry_facts(w, h):
    """Grid arithmetic of one level: per cell the detection width dw / height dh, the staged rows,
    the LDS row stride in bytes 16 ceil((ceil(dw / 4) + 2) / 4), the rows one prefetch covers and the
    realignment (c0 - 1) & 3."""
    n_cols, n_rows, w_cell, h_cell = fd.grid(w, h)
    cells = []
    for i in range(n_rows):
        for j in range(n_cols):
            r0, r1, c0, c1 = fd.cell_rect(w, h, i, j)
            dw, rows = c1 - c0 - 6, r1 - r0
            nd = -(-dw // 4) + 2
            chunks_per_row = (nd + 4) // 4
            cells.append(dict(dw=dw, dh=rows - 6, rows=rows, stride=16 * (-(-nd // 4)), prefetch_rows=4 * (64 // chunks_per_row),
                              realign=(c0 - 1) & 3))
    return dict(n_cols=n_cols, n_rows=n_rows, w_cell=w_cell, h_cell=h_cell, cells=cells)


def geometry_cases():
    out = []
    for k, (w, h, nl) in enumerate(GEOMETRIES):
        out.append(Case(f"geom-{w}x{h}-noise", noise_image(50 + k, w, h), 20, 7, nl, nfeat=200))
        out.append(Case(f"geom-{w}x{h}-impulses",
                        impulse_image(70 + k, w, h, 20, 7, classes=(CLASS_MIX, CLASS_MID, CLASS_STRONG, CLASS_WEAK),
                                      off=(k % 7, (3 * k) % 7)), 20, 7, nl, nfeat=200))
    return out


# ---- other pyramids -----------------------------------------------------------------------------
PYRAMIDS = [(251, 249, 1.5, 4), (151, 150, 2.0, 2), (213, 211, 1.1, 12)]   # top level 74-75 px


def mixed_image(seed, w, h):
    """Smooth shading with noise patches and impulses: keys on every level of a pyramid."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = (96 + 48 * np.sin(xx / 9.0) * np.cos(yy / 11.0)).astype(np.int32)
    for _ in range(6):
        x, y = int(rng.integers(0, w - 24)), int(rng.integers(0, h - 24))
        img[y:y + 24, x:x + 24] = rng.integers(0, 256, (24, 24))
    for _ in range(12):
        x, y = int(rng.integers(8, w - 16)), int(rng.integers(8, h - 16))
        img[y:y + 6, x:x + 6] = int(rng.integers(0, 2)) * 255
    ys, xs = rng.integers(0, h, 60), rng.integers(0, w, 60)
    img[ys, xs] = rng.integers(0, 256, 60)
    return np.clip(img, 0, 255).astype(np.uint8)


def pyramid_cases():
    return [Case(f"pyramid-{s}-{nl}", mixed_image(90 + nl, w, h), 20, 7, nl, s, 500) for w, h, s, nl in PYRAMIDS]
