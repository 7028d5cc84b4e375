"""FAST-9/16 written from its definition, in numpy — TEST INFRASTRUCTURE ONLY.

An independent second reference for the detector: when the HIP kernel and the C++ oracle disagree
on a FAST key, this module says which side is wrong. It shares no code with either.

Definition. The ring of a pixel p is the 16 pixels of the Bresenham circle of radius 3 around it.
p (value v) is a corner at threshold t iff 9 contiguous ring pixels are all > v + t (bright arc)
or all < v - t (dark arc). With the contrast of a ring pixel r taken as r - v for a bright arc and
v - r for a dark one, let M be the maximum, over the 16 arcs and both signs, of the arc's minimum
contrast: p is a corner iff M > t, and its score is M - 1 (the largest threshold at which it is
still a corner). Corners are sought in rows and columns 3 .. n - 4 of the region; every other
pixel scores 0. Non-maximum suppression is strict over the 3 x 3 neighbourhood: a corner is kept
iff its score is greater than all eight neighbours' scores. Output is in row-major order, as
cv::FAST(roi, keypoints, t, true) gives it.
"""
from __future__ import annotations

import numpy as np

# ring in circular order, (dx, dy)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
        (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))

BORDER = 16   # EDGE_THRESHOLD - 3: the cell grid's margin in a pyramid level
CELL = 35     # nominal cell size W of the grid


def arc_max(roi) -> np.ndarray:
    """M of every pixel of rows / columns 3 .. n - 4, as an int array of shape (h - 6, w - 6)."""
    a = np.asarray(roi).astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    # contrast of ring pixel k for a bright arc; the dark one is its negative
    d = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in RING])
    best = np.full(v.shape, -256, np.int32)
    for sign in (1, -1):
        c = np.concatenate([sign * d, sign * d[:8]])       # arcs wrap round the ring
        m = c[0:16].copy()
        for k in range(1, 9):
            np.minimum(m, c[k:k + 16], out=m)              # m[s] = min of arc s .. s + 8
        np.maximum(best, m.max(axis=0), out=best)
    return best


def score_map(roi, th: int) -> tuple[np.ndarray, np.ndarray]:
    """(score, corner) of every pixel of the region before suppression: inside the 3-pixel frame a
    pixel with M > th is a corner of score M - 1; every other pixel is no corner and scores 0."""
    roi = np.asarray(roi)
    h, w = roi.shape
    s, c = np.zeros((h, w), np.int32), np.zeros((h, w), bool)
    if h >= 7 and w >= 7:
        m = arc_max(roi)
        c[3:h - 3, 3:w - 3] = m > th
        s[3:h - 3, 3:w - 3] = np.where(m > th, m - 1, 0)
    return s, c


def fast9(roi, th: int) -> list[tuple[int, int, int]]:
    """[(x, y, score)] in row-major order: cv::FAST(roi, th, nonmaxSuppression=true)."""
    roi = np.asarray(roi)
    h, w = roi.shape
    s, corner = score_map(roi, th)
    p = np.pad(s, 1)
    nb = np.zeros_like(s)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dx, dy) != (1, 1):
                np.maximum(nb, p[dy:dy + h, dx:dx + w], out=nb)
    ys, xs = np.nonzero(corner & (s > nb))
    return [(int(x), int(y), int(s[y, x])) for x, y in zip(xs, ys)]


def grid(w: int, h: int) -> tuple[int, int, int, int]:
    """(n_cols, n_rows, w_cell, h_cell) of a level of w x h pixels."""
    width, height = w - 2 * BORDER, h - 2 * BORDER
    n_cols, n_rows = width // CELL, height // CELL
    return n_cols, n_rows, -(-width // n_cols), -(-height // n_rows)


def cell_rect(w: int, h: int, i: int, j: int):
    """Region (r0, r1, c0, c1) that FAST sees for cell (row i, column j), or None when skipped: the
    cell's detection rectangle plus 3 pixels on each side, clipped at the far border."""
    _, _, w_cell, h_cell = grid(w, h)
    max_x, max_y = w - BORDER, h - BORDER
    r0, c0 = BORDER + i * h_cell, BORDER + j * w_cell
    if r0 >= max_y - 3 or c0 >= max_x - 6:
        return None
    return r0, min(r0 + h_cell + 6, max_y), c0, min(c0 + w_cell + 6, max_x)


def cell_keys(level_img, ini_th: int, min_th: int):
    """The per-cell detection of one pyramid level: FAST at ini_th in every cell's region, again
    at min_th where that found nothing. Returns (counts[n_rows * n_cols], per-cell lists of
    (x_rel, y_rel, score)), cells in row-major order, coordinates relative to the level's border."""
    img = np.asarray(level_img)
    h, w = img.shape
    n_cols, n_rows, w_cell, h_cell = grid(w, h)
    counts, lists = [], []
    for i in range(n_rows):
        for j in range(n_cols):
            rect = cell_rect(w, h, i, j)
            keys = []
            if rect is not None:
                r0, r1, c0, c1 = rect
                roi = img[r0:r1, c0:c1]
                keys = fast9(roi, ini_th) or fast9(roi, min_th)
            lists.append([(x + j * w_cell, y + i * h_cell, s) for x, y, s in keys])
            counts.append(len(keys))
    return np.asarray(counts, np.int32), lists


def bin_keys(xs, ys, scores, w: int, h: int):
    """Bin a level's keys (coordinates relative to the border, cell-major order as the extractor
    emits them) into the grid: a key of cell (i, j) lies in columns [j w_cell + 3, (j + 1) w_cell + 3)
    and rows [i h_cell + 3, (i + 1) h_cell + 3). Returns (counts, per-cell lists) like cell_keys."""
    n_cols, n_rows, w_cell, h_cell = grid(w, h)
    lists = [[] for _ in range(n_cols * n_rows)]
    for x, y, s in zip(xs, ys, scores):
        x, y = int(x), int(y)
        lists[((y - 3) // h_cell) * n_cols + (x - 3) // w_cell].append((x, y, int(s)))
    return np.asarray([len(v) for v in lists], np.int32), lists
