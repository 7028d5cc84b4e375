"""SearchForInitialization by definition: the reference's sequential loop restated in plain Python with
np.float32 scalars, one source line per rule, written from the reference text. Test infrastructure only
(as the other *_definition modules): slow, sequential, and the trace says which rule decided every query.

  SearchForInitialization                    ORBmatcher.cc:648-763   -> py_search_for_init
  Frame::GetFeaturesInArea                   Frame.cc:657-723        -> features_in_area
  Frame::AssignFeaturesToGrid / PosInGrid    Frame.cc:385-416, 725-735 -> sbp_definition.PyGrid (the cells)
  rotation bin, ComputeThreeMaxima                                   -> sbp_definition.py_rot_bin, three_maxima_inds

Frames are MatchFrame-like: keys (x, y, octave, angle), desc uint8 [n, 32], bounds (mnMinX, mnMaxX, mnMinY,
mnMaxY). prev is vbPrevMatched as float32 [n1, 2]; it is not modified, the updated copy is returned.

py_search_for_init returns (nmatches, vnMatches12 int32 [n1], vbPrevMatched float32 [n1, 2], trace):
  trace["q"][i1]     for every query that reached GetFeaturesInArea (octave <= 0):
                     {"area": None | "min-x" | "max-x" | "min-y" | "max-y" (the early return taken),
                      "cells": (c0, c1, r0, r1) | None,
                      "cands": [[i2, rule, dist], ...] in enumeration order (ix outer, iy inner, cell order),
                      "bd", "bd2", "best", "outcome", "stole", "bin"}
  rule               "level" / "box" (GetFeaturesInArea, in the order it tests them; dist None), "blocked"
                     (vMatchedDistance[i2] <= dist, before bestDist / bestDist2 are touched), "lost", "best"
  outcome            "none" (no candidate reached the comparison), "distance", "ratio", "selected";
                     after the loop a selected query reads "stolen", "dropped bin" or "kept"
  stole              the query whose match this selection cleared, or -1
  trace["bins"]      the 30 rotHist sizes (every selection, stolen ones included) and trace["kept_bins"]
                     the three maxima (checkOri), else None
double=True evaluates the ratio test with mfNNratio as the double the caller wrote (the member is a float)
and a double product, and the 0.1f of ComputeThreeMaxima as a double: what a careless restatement
computes. The tests use it to prove that a planted case tells the two apart.
"""
import math

import numpy as np

from oracle.sbp_definition import GRID_COLS, GRID_ROWS, HISTO_LENGTH, PyGrid, _ham, py_rot_bin, three_maxima_inds

f32 = np.float32
TH_LOW = 50            # ORBmatcher.cc:34
INT_MAX = 2 ** 31 - 1


def ratio_passes(bd, bd2, nnratio, double=False):
    """bestDist < (float)bestDist2 * mfNNratio (ORBmatcher.cc:704): float product, strict."""
    if double:
        return bd < float(bd2) * float(nnratio)
    return bool(f32(bd) < f32(f32(bd2) * f32(nnratio)))


def features_in_area(grid, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea (Frame.cc:657-723) over PyGrid's cells -> (early return taken | None,
    (c0, c1, r0, r1) | None, [[idx, None | "level" | "box"], ...])."""
    F = grid.F
    x, y, r = f32(x), f32(y), f32(r)                                       # const float& r <- int windowSize
    mnx, mny = f32(F.bounds[0]), f32(F.bounds[2])
    c0 = max(0, math.floor(f32(f32(f32(x - mnx) - r) * grid.invw)))        # :665
    if c0 >= GRID_COLS:                                                    # :666
        return "min-x", None, []
    c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(x - mnx) + r) * grid.invw)))   # :671
    if c1 < 0:                                                             # :672
        return "max-x", None, []
    r0 = max(0, math.floor(f32(f32(f32(y - mny) - r) * grid.invh)))        # :677
    if r0 >= GRID_ROWS:                                                    # :678
        return "min-y", None, []
    r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(y - mny) + r) * grid.invh)))   # :683
    if r1 < 0:                                                             # :684
        return "max-y", None, []
    check_levels = min_level > 0 or max_level >= 0                         # :689
    out = []
    for ix in range(c0, c1 + 1):                                           # :691
        for iy in range(r0, r1 + 1):                                       # :693
            for i in grid.cells.get((ix, iy), []):                         # :699
                k = F.keys[i]
                if check_levels and (k["octave"] < min_level or (max_level >= 0 and k["octave"] > max_level)):
                    out.append([i, "level"])                               # :704-711
                elif abs(f32(k["x"] - x)) < r and abs(f32(k["y"] - y)) < r:   # :713-716, strict
                    out.append([i, None])
                else:
                    out.append([i, "box"])
    return None, (c0, c1, r0, r1), out


def py_search_for_init(F1, F2, prev, window, nnratio, check_ori, double=False):
    """ORBmatcher.cc:648-763."""
    n1, n2 = len(F1.keys), len(F2.keys)
    grid = PyGrid(F2)
    prev = np.array(prev, np.float32).reshape(n1, 2)
    nmatches = 0                                                           # :650
    m12 = np.full(n1, -1, np.int32)                                        # :651
    rot_hist = [[] for _ in range(HISTO_LENGTH)]                           # :653
    matched_dist = [INT_MAX] * n2                                          # :658
    m21 = [-1] * n2                                                        # :659
    tr = {"q": {}, "bins": None, "kept_bins": None}
    for i1 in range(n1):                                                   # :661
        level1 = int(F1.keys[i1]["octave"])                                # :664
        if level1 > 0:                                                     # :665
            continue
        early, cells, walk = features_in_area(grid, prev[i1, 0], prev[i1, 1], window, level1, level1)   # :668
        rec = {"area": early, "cells": cells, "cands": [], "bd": INT_MAX, "bd2": INT_MAX, "best": -1,
               "outcome": "none", "stole": -1, "bin": None}
        tr["q"][i1] = rec
        bd, bd2, best = INT_MAX, INT_MAX, -1                               # :675-677
        for i2, rule in walk:
            if rule is not None:
                rec["cands"].append([i2, rule, None])
                continue
            d = _ham(F1.desc[i1], F2.desc[i2])                             # :685
            if matched_dist[i2] <= d:                                      # :687
                rec["cands"].append([i2, "blocked", d])
                continue
            rec["cands"].append([i2, "lost", d])
            if d < bd:                                                     # :690
                bd2, bd, best = bd, d, i2
            elif d < bd2:                                                  # :696
                bd2 = d
        for c in rec["cands"]:
            if c[0] == best and c[1] == "lost":
                c[1] = "best"
        rec.update(bd=bd, bd2=bd2, best=best)
        if best < 0:
            continue
        rec["outcome"] = "distance"
        if bd <= TH_LOW:                                                   # :702
            rec["outcome"] = "ratio"
            if ratio_passes(bd, bd2, nnratio, double):                     # :704
                if m21[best] >= 0:                                         # :706
                    rec["stole"] = m21[best]
                    m12[m21[best]] = -1
                    nmatches -= 1
                m12[i1] = best                                             # :711
                m21[best] = i1
                matched_dist[best] = bd
                nmatches += 1
                rec["outcome"] = "selected"
                if check_ori:                                              # :716-726
                    rec["bin"] = py_rot_bin(F1.keys[i1]["angle"], F2.keys[best]["angle"])
                    rot_hist[rec["bin"]].append(i1)
    if check_ori:                                                          # :732-755
        tr["bins"] = [len(h) for h in rot_hist]
        ind = three_maxima_inds(tr["bins"], double)
        tr["kept_bins"] = set(ind) - {-1}
        for i in range(HISTO_LENGTH):
            if i in ind:
                continue
            for idx1 in rot_hist[i]:
                if m12[idx1] >= 0:                                         # :747
                    m12[idx1] = -1
                    nmatches -= 1
                    tr["q"][idx1]["outcome"] = "dropped bin"
    for i1, rec in tr["q"].items():
        if rec["outcome"] == "selected":
            rec["outcome"] = "kept" if m12[i1] >= 0 else "stolen"
    for i1 in range(n1):                                                   # :758-760
        if m12[i1] >= 0:
            prev[i1, 0] = F2.keys[m12[i1]]["x"]
            prev[i1, 1] = F2.keys[m12[i1]]["y"]
    return nmatches, m12, prev, tr
