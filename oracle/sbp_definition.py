"""SearchByProjection by definition: the reference's three single-camera forms restated in plain
Python with np.float32 scalars, one source line per rule, so that every comparison is evaluated in
the precision the reference evaluates it in. Test infrastructure only (as the other *_definition
modules): slow, sequential, and with tracing on it says which rule removed which candidate.

  Frame::AssignFeaturesToGrid / PosInGrid   Frame.cc:385-416, 725-735   -> PyGrid
  Frame::GetFeaturesInArea                  Frame.cc:657-723            -> PyGrid.walk / PyGrid.area
  SearchByProjection (local map)            ORBmatcher.cc:43-213        -> py_sbp_local
  RadiusByViewingCos                        ORBmatcher.cc:215-221
  SearchByProjection (last frame)           ORBmatcher.cc:1676-1887     -> py_sbp_lastframe
  SearchByProjection (keyframe)             ORBmatcher.cc:1889-2010     -> py_sbp_kf
  ComputeThreeMaxima                        ORBmatcher.cc:2012-2053     -> py_three_maxima
  rotation bin                              ORBmatcher.cc:1784-1789, 1973-1978 -> py_rot_bin

The last-frame and keyframe forms take projected point records (PROJ_POINT records: u, v, invzc,
octave, angle, valid, observations, id, desc) as the C-ABI does; the projection is not restated here.

Trace (trace=True): the functions return (nmatches, trace) with
  trace["q"][i]   for every query that reached GetFeaturesInArea: {"R": radius, "cands": [[idx, rule],
                  ...] in the reference's enumeration order (cell column, cell row, insertion order),
                  "best": idx, "bd": bestDist, "bd2": bestDist2 (local map), "bl" / "bl2", "outcome"}
  rule            "level" / "box" (GetFeaturesInArea, in the order it tests them), "blocked", "uR",
                  "lost" (compared and not the best), "best"
  outcome         of the best candidate: "distance", "ratio", "kept" or "dropped bin"; "none" when no
                  candidate reached the comparison
  trace["bins"]   the 30 bin counts and trace["kept_bins"] the kept bins (checkOri), else None
The `double` switches evaluate one rule the way a careless restatement would (the float constant
promoted to double); the tests use them to prove that a planted case tells the two apart.
"""
import math

import numpy as np

f32 = np.float32
TH_HIGH, HISTO_LENGTH = 100, 30   # ORBmatcher.cc:33-35
MP_IN_VIEW, MP_BAD = 1, 2
GRID_COLS, GRID_ROWS = 64, 48     # Frame.h:38-39


def _ham(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def round_half_away(v):
    return math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5)


class PyGrid:
    """Frame::AssignFeaturesToGrid + GetFeaturesInArea (Frame.cc:385-416, 657-723)."""

    def __init__(self, F):
        self.F = F
        self.invw = f32(GRID_COLS) / f32(f32(F.bounds[1]) - f32(F.bounds[0]))
        self.invh = f32(GRID_ROWS) / f32(f32(F.bounds[3]) - f32(F.bounds[2]))
        self.cells = {}
        self.cell_of = {}
        for i, k in enumerate(F.keys):
            px = int(round_half_away(f32(f32(k["x"] - f32(F.bounds[0])) * self.invw)))
            py = int(round_half_away(f32(f32(k["y"] - f32(F.bounds[2])) * self.invh)))
            if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:   # PosInGrid (Frame.cc:725-735)
                self.cells.setdefault((px, py), []).append(i)
                self.cell_of[i] = (px, py)

    def cell_range(self, x, y, r):
        """(c0, c1, r0, r1) of the window, or None where the reference returns empty (Frame.cc:666-690)."""
        F, x, y, r = self.F, f32(x), f32(y), f32(r)
        mnx, mny = f32(F.bounds[0]), f32(F.bounds[2])
        c0 = max(0, math.floor(f32(f32(f32(x - mnx) - r) * self.invw)))
        if c0 >= GRID_COLS:
            return None
        c1 = min(GRID_COLS - 1, math.ceil(f32(f32(f32(x - mnx) + r) * self.invw)))
        if c1 < 0:
            return None
        r0 = max(0, math.floor(f32(f32(f32(y - mny) - r) * self.invh)))
        if r0 >= GRID_ROWS:
            return None
        r1 = min(GRID_ROWS - 1, math.ceil(f32(f32(f32(y - mny) + r) * self.invh)))
        if r1 < 0:
            return None
        return c0, c1, r0, r1

    def walk(self, x, y, r, minL, maxL):
        """Every keypoint of the window's cells in the reference's order with the rule that removes it
        ("level", "box") or None (Frame.cc:692-720: the level is tested before the box)."""
        F, x, y, r = self.F, f32(x), f32(y), f32(r)
        rng = self.cell_range(x, y, r)
        if rng is None:
            return []
        c0, c1, r0, r1 = rng
        check = minL > 0 or maxL >= 0
        out = []
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for i in self.cells.get((ix, iy), []):
                    k = F.keys[i]
                    if check and (k["octave"] < minL or (maxL >= 0 and k["octave"] > maxL)):
                        out.append([i, "level"])
                    elif abs(f32(k["x"] - x)) < r and abs(f32(k["y"] - y)) < r:
                        out.append([i, None])
                    else:
                        out.append([i, "box"])
        return out

    def area(self, x, y, r, minL, maxL):
        return [i for i, rule in self.walk(x, y, r, minL, maxL) if rule is None]


def py_rot_bin(a1, a2, double=False):
    """ORBmatcher.cc:1784-1789: float rot, float factor = 1.0f / HISTO_LENGTH, round() of the float
    product. double=True: rot / 30 in double (what the rule is not)."""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    if double:
        b = int(round_half_away(float(rot) / 30.0))
    else:
        b = int(round_half_away(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH)))))
    return 0 if b == HISTO_LENGTH else b


def three_maxima_inds(hist, double=False):
    """ComputeThreeMaxima (ORBmatcher.cc:2012-2053) -> (ind1, ind2, ind3). double=True: 0.1f promoted
    to double (what the rule is not)."""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, c in enumerate(hist):
        if c > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, c, i2, i1, i
        elif c > max2:
            max3, max2, i3, i2 = max2, c, i2, i
        elif c > max3:
            max3, i3 = c, i
    lim = float(f32(0.1)) * max1 if double else f32(f32(0.1) * f32(max1))
    if max2 < lim:
        i2 = i3 = -1
    elif max3 < lim:
        i3 = -1
    return i1, i2, i3


def py_three_maxima(hist, double=False):
    return set(three_maxima_inds(hist, double))


def ratio_rejects(bd, bd2, nnratio, double=False):
    """bestDist > mfNNratio * bestDist2 (ORBmatcher.cc:127): float * int in float. double=True: the
    float ratio promoted to double."""
    if double:
        return bd > float(f32(nnratio)) * bd2
    return f32(bd) > f32(f32(nnratio) * f32(bd2))


def py_ur(u, mbf, invzc, fused=False):
    """uv(0) - mbf * invzc (ORBmatcher.cc:1753), product and difference each rounded to float;
    fused=True: one rounding (a contracted multiply-subtract, what the rule is not)."""
    if fused:
        return f32(float(f32(u)) - float(f32(mbf)) * float(f32(invzc)))
    return f32(f32(u) - f32(f32(mbf) * f32(invzc)))


def _commit(hist, mvp, n, tq, trace):
    """ORBmatcher.cc:1864-1884 / 1988-2007: every entry of a dropped bin clears its slot and counts."""
    keep = py_three_maxima([len(h) for h in hist])
    for b, h in enumerate(hist):
        if b in keep:
            continue
        for slot, qi in h:
            mvp[slot] = -1
            n -= 1
            if trace:
                tq[qi]["outcome"] = "dropped bin"
    return n, keep


def py_sbp_local(F, mvp, obs, mps, th, nnratio, trace=False):
    """ORBmatcher.cc:43-213 (single camera). mvp is updated in place."""
    g = PyGrid(F)
    obs = obs.copy()
    n = 0
    tq = {}
    for qi, mp in enumerate(mps):
        if not (mp["flags"] & MP_IN_VIEW) or (mp["flags"] & MP_BAD):   # :58-71
            continue
        lvl = int(mp["scale_level"])
        r = f32(2.5) if float(mp["view_cos"]) > 0.998 else f32(4.0)    # :215-221, compared as double
        if th != 1.0:
            r = f32(r * f32(th))                                        # :80-81
        R = f32(r * F.scale_factors[lvl])
        bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
        cands = g.walk(mp["proj_x"], mp["proj_y"], R, lvl - 1, lvl)    # :83-85
        for c in cands:
            idx = c[0]
            if c[1] is not None:
                continue
            if mvp[idx] >= 0 and obs[idx] > 0:                          # :99-101
                c[1] = "blocked"
                continue
            if F.uright is not None and F.uright[idx] > 0 and \
                    abs(f32(f32(mp["proj_xr"]) - F.uright[idx])) > R:   # :103-108
                c[1] = "uR"
                continue
            c[1] = "lost"
            d = _ham(mp["desc"], F.desc[idx])
            if d < bd:                                                  # :114-131, strict: the first of equals stays
                bd2, bd, bl2, bl, bi = bd, d, bl, int(F.keys[idx]["octave"]), idx
            elif d < bd2:
                bl2, bd2 = int(F.keys[idx]["octave"]), d
        for c in cands:
            if c[0] == bi and c[1] == "lost":
                c[1] = "best"
        outcome = "none" if bi < 0 else "distance"
        if bd <= TH_HIGH:                                               # :134
            if bl == bl2 and ratio_rejects(bd, bd2, nnratio):          # :136-137
                outcome = "ratio"
            else:
                outcome = "kept"
                mvp[bi] = mp["id"]
                obs[bi] = mp["observations"]
                n += 1
        if trace:
            tq[qi] = {"R": R, "cands": cands, "best": bi, "bd": bd, "bd2": bd2, "bl": bl, "bl2": bl2,
                      "outcome": outcome}
    if trace:
        return n, {"q": tq, "bins": None, "kept_bins": None}
    return n


def _py_sbp_proj(F, mvp, obs, pts, th, level_range, blocked, max_dist, check_ori, lastframe, trace):
    g = PyGrid(F)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    tq = {}
    for qi, p in enumerate(pts):
        if not p["valid"]:
            continue
        if lastframe:
            if p["invzc"] < 0:                                          # :1710-1711
                continue
            if p["u"] < f32(F.bounds[0]) or p["u"] > f32(F.bounds[1]):  # :1715-1718
                continue
            if p["v"] < f32(F.bounds[2]) or p["v"] > f32(F.bounds[3]):
                continue
        octv = int(p["octave"])
        R = f32(f32(th) * F.scale_factors[octv])                        # :1724 / :1937
        minL, maxL = level_range(octv)
        cands = g.walk(p["u"], p["v"], R, minL, maxL)
        bd, bi = 256, -1
        for c in cands:
            idx = c[0]
            if c[1] is not None:
                continue
            if blocked(idx):
                c[1] = "blocked"
                continue
            if lastframe and F.uright is not None and F.uright[idx] > 0:   # :1751-1757
                ur = py_ur(p["u"], F.mbf, p["invzc"])
                if abs(f32(ur - F.uright[idx])) > R:
                    c[1] = "uR"
                    continue
            c[1] = "lost"
            d = _ham(p["desc"], F.desc[idx])
            if d < bd:                                                  # :1763-1767 / :1959-1963
                bd, bi = d, idx
        for c in cands:
            if c[0] == bi and c[1] == "lost":
                c[1] = "best"
        outcome = "none" if bi < 0 else "distance"
        if bd <= max_dist:                                              # :1770 / :1966
            outcome = "kept"
            mvp[bi] = p["id"]
            if obs is not None:
                obs[bi] = p["observations"]
            n += 1
            if check_ori:                                               # :1775-1792 / :1971-1981
                hist[py_rot_bin(p["angle"], F.keys[bi]["angle"])].append((bi, qi))
        if trace:
            tq[qi] = {"R": R, "cands": cands, "best": bi, "bd": bd, "outcome": outcome}
    bins = keep = None
    if check_ori:
        bins = [len(h) for h in hist]
        n, keep = _commit(hist, mvp, n, tq, trace)
    if trace:
        return n, {"q": tq, "bins": bins, "kept_bins": keep}
    return n


def py_sbp_lastframe(F, mvp, obs, pts, th, bForward, bBackward, check_ori, trace=False):
    """ORBmatcher.cc:1676-1887 (single camera), from the projected records. mvp is updated in place.
    A slot held by a point with Observations() == 0 is free; the writer's Observations() then decide
    (the reference reads them through the slot's new MapPoint)."""
    obs = obs.copy()

    def level_range(o):                                                 # :1728-1733
        if bForward:
            return o, -1
        if bBackward:
            return 0, o
        return o - 1, o + 1
    return _py_sbp_proj(F, mvp, obs, pts, th, level_range, lambda i: mvp[i] >= 0 and obs[i] > 0, TH_HIGH,
                        check_ori, True, trace)


def py_sbp_kf(F, mvp, pts, th, ORBdist, check_ori, trace=False):
    """ORBmatcher.cc:1889-2010, from the projected records. Any held slot blocks (:1952-1953)."""
    return _py_sbp_proj(F, mvp, None, pts, th, lambda o: (o - 1, o + 1), lambda i: mvp[i] >= 0, int(ORBdist),
                        check_ori, False, trace)
