"""SearchByProjection by definition: the reference's three single-camera forms and its two two-camera
forms (Frame.Nleft != -1) restated in plain
Python with np.float32 scalars, one source line per rule, so that every comparison is evaluated in
the precision the reference evaluates it in. Test infrastructure only (as the other *_definition
modules): slow, sequential, and with tracing on it says which rule removed which candidate.

  Frame::AssignFeaturesToGrid / PosInGrid   Frame.cc:385-416, 725-735   -> PyGrid
  Frame::GetFeaturesInArea                  Frame.cc:657-723            -> PyGrid.walk / PyGrid.area
  SearchByProjection (local map)            ORBmatcher.cc:43-213        -> py_sbp_local, py_sbp_local_two
  RadiusByViewingCos                        ORBmatcher.cc:215-221
  SearchByProjection (last frame)           ORBmatcher.cc:1676-1887     -> py_sbp_lastframe, py_sbp_lastframe_two
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
promoted to double); the tests use them to prove that a planted case tells the two apart. The
two-camera functions take `variant=` to the same end: one named wrong reading of the reference each.
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

    def __init__(self, F, side=None):
        """side: None every row (Nleft == -1); 0 the left rows [0, nleft) (mGrid); 1 the right rows
        [nleft, n) (mGridRight, GetFeaturesInArea(..., bRight = true)). Rows keep the global numbering
        (right row = nleft + the reference's right index) (Frame.cc:399-413)."""
        self.F = F
        i0 = F.nleft if side == 1 else 0
        i1 = F.nleft if side == 0 else len(F.keys)
        self.invw = f32(GRID_COLS) / f32(f32(F.bounds[1]) - f32(F.bounds[0]))
        self.invh = f32(GRID_ROWS) / f32(f32(F.bounds[3]) - f32(F.bounds[2]))
        self.cells = {}
        self.cell_of = {}
        for i in range(i0, i1):
            k = F.keys[i]
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


# ------------------------------------------------------------------ two cameras (Frame.Nleft != -1)
MP_IN_VIEW_R = 8
LOCAL_TWO_VARIANTS = ("partner-guarded", "first-writer", "own-partner-unseen", "ratio-searches-right",
                      "far-left-stops", "right-radius-th", "right-ratio-cross-level", "count-slots",
                      "level-r-minus1-searched")
LOCAL_TWO_EXTRA = ("no-partners", "no-sequence", "one-grid", "right-cos-float", "right-ratio-double")
LASTFRAME_TWO_VARIANTS = ("empty-left-searches-right", "blocked-left-is-empty", "right-bounds", "right-sees-later",
                          "stereo-gate", "right-left-grid", "hist-left-only")
LASTFRAME_TWO_EXTRA = ("no-sequence", "gates-left-only")


def _best2(F, desc, cands, taken):
    """The candidate loop of :84-120 / :164-190 over a PyGrid.walk list (rules filled in) ->
    (bestDist, bestLevel, bestDist2, bestLevel2, bestIdx)."""
    bd, bl, bd2, bl2, bi = 256, -1, 256, -1, -1
    for c in cands:
        idx = c[0]
        if c[1] is not None:
            continue
        if taken(idx):                                                  # :88-90 / :168-170
            c[1] = "blocked"
            continue
        c[1] = "lost"
        d = _ham(desc, F.desc[idx])
        if d < bd:                                                      # strict: the first of equals stays
            bd2, bd, bl2, bl, bi = bd, d, bl, int(F.keys[idx]["octave"]), idx
        elif d < bd2:
            bl2, bd2 = int(F.keys[idx]["octave"]), d
    for c in cands:
        if c[0] == bi and c[1] == "lost":
            c[1] = "best"
    return bd, bl, bd2, bl2, bi


def py_sbp_local_two(F, mvp, obs, mps, th, nnratio, bFar=False, thFar=50.0, trace=False, variant=None):
    """ORBmatcher.cc:43-213 with Nleft != -1, literal; rows in the global numbering (left [0, nleft), right
    [nleft, n)). mvp is updated in place. Point q writes up to four slots, in this order: the left best
    (:129), its mvLeftToRightMatch partner (:131-135, no test of the slot), the right best's
    mvRightToLeftMatch partner (:198-202, no test either), the right best (:205); every write counts.

    Trace: trace["q"][qi] = {"gate": None or why the point was skipped ("not in view", "far", "bad"),
    "L" / "R": None where that camera's search did not run, else {"R", "cands", "best", "bd", "bd2", "bl",
    "bl2", "outcome"} as py_sbp_local's (outcome "empty": the window returned nothing), "R_skip": why the
    right search did not run ("left ratio", "not in view R", "level -1"), "writes": [[b, slot, holder
    before the write, its observations], ...] with b the position 0..3 in the order above}.

    variant: one deliberately wrong reading (LOCAL_TWO_VARIANTS), None = the reference's.
      partner-guarded           a partner write is skipped when its slot is blocked
      first-writer              a slot keeps its first writer of this call (later writes are lost)
      own-partner-unseen        the right search tests the own l2r partner's slot as it was before that write
      ratio-searches-right      a failed left ratio test does not `continue` (:125-126)
      far-left-stops            an empty left window or a left bestDist > TH_HIGH skips the right search
      right-radius-th           the right radius is scaled by th as the left one is (:68-69 against :147)
      right-ratio-cross-level   the right ratio test ignores bestLevel == bestLevel2 (:195)
      count-slots               the return value counts distinct slots written, not writes
      level-r-minus1-searched   mnTrackScaleLevelR == -1 is searched, at the left level (:146)
    and, for the cases whose rule none of these reaches (LOCAL_TWO_EXTRA):
      no-partners               no partner is written
      no-sequence               only the holders before the search block (no point sees another's write)
      one-grid                  both searches walk one grid of every row
      right-cos-float           mTrackViewCosR > 0.998 compared in float
      right-ratio-double        the right ratio test with mfNNratio promoted to double"""
    assert variant is None or variant in LOCAL_TWO_VARIANTS + LOCAL_TWO_EXTRA, variant
    nl = F.nleft
    gl, gr = PyGrid(F, 0), PyGrid(F, 1)                                 # mGrid / mGridRight
    if variant == "one-grid":
        gl = gr = PyGrid(F)
    held0 = (mvp >= 0) & (obs > 0)
    obs = obs.copy()
    n = 0
    tq = {}
    written = set()

    def taken(idx):
        if variant == "no-sequence":
            return bool(held0[idx])
        return mvp[idx] >= 0 and obs[idx] > 0

    def put(t, b, slot, mp):
        t["writes"].append([b, int(slot), int(mvp[slot]), int(obs[slot])])
        if variant == "first-writer" and slot in written:
            return
        written.add(int(slot))
        mvp[slot], obs[slot] = mp["id"], mp["observations"]

    for qi, mp in enumerate(mps):
        inv, invr = bool(mp["flags"] & MP_IN_VIEW), bool(mp["flags"] & MP_IN_VIEW_R)
        t = {"gate": None, "L": None, "R": None, "R_skip": None, "writes": []}
        if trace:
            tq[qi] = t
        if not inv and not invr:                                        # :52-53
            t["gate"] = "not in view"
            continue
        if bFar and f32(mp["depth"]) > f32(thFar):                      # :55-56
            t["gate"] = "far"
            continue
        if mp["flags"] & MP_BAD:                                        # :58-59
            t["gate"] = "bad"
            continue
        own = None
        if inv:                                                         # :61-142
            lvl = int(mp["scale_level"])
            r = f32(2.5) if float(mp["view_cos"]) > 0.998 else f32(4.0)   # :215-221, compared as double
            if th != 1.0:
                r = f32(r * f32(th))                                    # :68-69
            R = f32(r * F.scale_factors[lvl])
            cands = gl.walk(mp["proj_x"], mp["proj_y"], R, lvl - 1, lvl)   # :71-72, the left grid
            s = t["L"] = {"R": R, "cands": cands, "best": -1, "bd": 256, "bd2": 256, "bl": -1, "bl2": -1,
                          "outcome": "empty"}
            if any(c[1] is None for c in cands):                        # :74 !vIndices.empty()
                bd, bl, bd2, bl2, bi = _best2(F, mp["desc"], cands, taken)
                s.update(best=bi, bd=bd, bd2=bd2, bl=bl, bl2=bl2, outcome="none" if bi < 0 else "distance")
                if bd <= TH_HIGH:                                       # :123
                    if bl == bl2 and ratio_rejects(bd, bd2, nnratio):  # :125-126: the next point
                        s["outcome"] = "ratio"
                        if variant != "ratio-searches-right":
                            t["R_skip"] = "left ratio"
                            continue
                    else:
                        s["outcome"] = "kept"
                        put(t, 0, bi, mp)                               # :129
                        n += 1
                        p = int(F.l2r[bi]) if bi < nl else -1
                        if p != -1 and variant != "no-partners":        # :131-135
                            if not (variant == "partner-guarded" and taken(p + nl)):
                                own = (p + nl, int(mvp[p + nl]), int(obs[p + nl]))
                                put(t, 1, p + nl, mp)
                                n += 1
                elif variant == "far-left-stops":
                    continue
            elif variant == "far-left-stops":
                continue
        if not invr:                                                    # :144
            t["R_skip"] = "not in view R"
            continue
        lvl = int(mp["scale_level_r"])
        if lvl == -1:                                                   # :146
            if variant != "level-r-minus1-searched":
                t["R_skip"] = "level -1"
                continue
            lvl = int(mp["scale_level"])
        r = f32(2.5) if float(mp["view_cos_r"]) > 0.998 else f32(4.0)   # :147, never scaled by th
        if variant == "right-cos-float":
            r = f32(2.5) if f32(mp["view_cos_r"]) > f32(0.998) else f32(4.0)
        if variant == "right-radius-th" and th != 1.0:
            r = f32(r * f32(th))
        R = f32(r * F.scale_factors[lvl])
        cands = gr.walk(mp["proj_xr"], mp["proj_yr"], R, lvl - 1, lvl)  # :149-150, bRight
        s = t["R"] = {"R": R, "cands": cands, "best": -1, "bd": 256, "bd2": 256, "bl": -1, "bl2": -1,
                      "outcome": "empty"}
        if not any(c[1] is None for c in cands):                        # :152-153
            continue

        def taken_r(idx):
            if variant == "own-partner-unseen" and own is not None and idx == own[0]:
                return own[1] >= 0 and own[2] > 0
            return taken(idx)
        bd, bl, bd2, bl2, bi = _best2(F, mp["desc"], cands, taken_r)
        s.update(best=bi, bd=bd, bd2=bd2, bl=bl, bl2=bl2, outcome="none" if bi < 0 else "distance")
        if bd <= TH_HIGH:                                               # :193
            if (bl == bl2 or variant == "right-ratio-cross-level") and \
                    ratio_rejects(bd, bd2, nnratio, double=variant == "right-ratio-double"):   # :195-196
                s["outcome"] = "ratio"
                continue
            s["outcome"] = "kept"
            p = int(F.r2l[bi - nl]) if bi >= nl else -1
            if p != -1 and variant != "no-partners":                    # :198-202
                if not (variant == "partner-guarded" and taken(p)):
                    put(t, 2, p, mp)
                    n += 1
            put(t, 3, bi, mp)                                           # :205
            n += 1
    if variant == "count-slots":
        n = len(written)
    if trace:
        return n, {"q": tq, "bins": None, "kept_bins": None}
    return n


def py_sbp_lastframe_two(F, mvp, obs, pts, right_uv, th, bForward, bBackward, check_ori, trace=False, variant=None,
                         _later=None):
    """ORBmatcher.cc:1695-1884 with CurrentFrame.Nleft != -1, from the projected records and right_uv [n, 2],
    the points projected into the right camera (:1795-1796). mvp is updated in place. Point q has two
    entries: 2q the left best (:1772), 2q + 1 the right best (:1838); the right search runs whenever the
    left window returned anything (:1735-1736), whatever became of the left best, and its projection is
    tested against nothing but the window.

    Trace: trace["q"][qi] = {"gate": None or "invalid" / "invzc" / "bounds", "L": the left search as
    py_sbp_lastframe's, "R": the right search or None, "R_skip": why it did not run}; trace["bins"] /
    trace["kept_bins"] as the single-camera form's, over both cameras' matches.

    variant (LASTFRAME_TWO_VARIANTS):
      empty-left-searches-right   an empty left window does not `continue`
      blocked-left-is-empty       a left window holding only blocked candidates counts as empty
      right-bounds                the right projection is tested against the image bounds as the left is
      right-sees-later            the right search sees the reference's writes of every later entry too
      stereo-gate                 the mvuRight test runs although Nleft != -1 (:1751)
      right-left-grid             the right search walks the left grid
      hist-left-only              right matches are not entered in the rotation histogram
    and (LASTFRAME_TWO_EXTRA):
      no-sequence                 only the holders before the search block
      gates-left-only             a point failing :1698-1718 skips its left search only"""
    assert variant is None or variant in LASTFRAME_TWO_VARIANTS + LASTFRAME_TWO_EXTRA, variant
    if variant == "right-sees-later" and _later is None:
        m0, log = mvp.copy(), []
        py_sbp_lastframe_two(F, m0, obs, pts, right_uv, th, bForward, bBackward, False, _later=log)
        _later = {}
        for e, slot, o in log:                                          # the last write of every slot
            _later[slot] = (e, o)
    gl, gr = PyGrid(F, 0), PyGrid(F, 1)
    held0 = (mvp >= 0) & (obs > 0)
    obs = obs.copy()
    hist = [[] for _ in range(HISTO_LENGTH)]
    n = 0
    tq = {}

    def level_range(o):                                                 # :1728-1733 / :1806-1811
        if bForward:
            return o, -1
        if bBackward:
            return 0, o
        return o - 1, o + 1

    def taken(idx):
        if variant == "no-sequence":
            return bool(held0[idx])
        return mvp[idx] >= 0 and obs[idx] > 0

    def search(p, g, x, y, R, tk, gate):
        minL, maxL = level_range(int(p["octave"]))
        cands = g.walk(x, y, R, minL, maxL)
        s = {"R": R, "cands": cands, "best": -1, "bd": 256, "outcome": "empty"}
        if not any(c[1] is None for c in cands):
            return s
        bd, bi = 256, -1
        for c in cands:
            idx = c[0]
            if c[1] is not None:
                continue
            if tk(idx):                                                 # :1747-1749 / :1821-1823
                c[1] = "blocked"
                continue
            if gate and F.uright is not None and F.uright[idx] > 0:     # :1751-1757, Nleft == -1 only
                if abs(f32(py_ur(p["u"], F.mbf, p["invzc"]) - F.uright[idx])) > R:
                    c[1] = "uR"
                    continue
            c[1] = "lost"
            d = _ham(p["desc"], F.desc[idx])
            if d < bd:                                                  # :1763-1767 / :1829-1833
                bd, bi = d, idx
        for c in cands:
            if c[0] == bi and c[1] == "lost":
                c[1] = "best"
        s.update(best=bi, bd=bd, outcome="none" if bi < 0 else "distance")
        return s

    def keep(s, p, qi, e, vote):
        nonlocal n
        if s["bd"] > TH_HIGH:                                           # :1770 / :1836
            return
        s["outcome"] = "kept"
        bi = s["best"]
        mvp[bi], obs[bi] = p["id"], p["observations"]
        if isinstance(_later, list):
            _later.append((e, int(bi), int(p["observations"])))
        n += 1
        if check_ori and vote:                                          # :1775-1792 / :1840-1856
            hist[py_rot_bin(p["angle"], F.keys[bi]["angle"])].append((bi, (qi, "R" if e & 1 else "L")))

    for qi, p in enumerate(pts):
        t = {"gate": None, "L": None, "R": None, "R_skip": None}
        if trace:
            tq[qi] = t
        if not p["valid"]:                                              # :1698-1700
            t["gate"] = "invalid"
        elif p["invzc"] < 0:                                            # :1710-1711
            t["gate"] = "invzc"
        elif p["u"] < f32(F.bounds[0]) or p["u"] > f32(F.bounds[1]) or \
                p["v"] < f32(F.bounds[2]) or p["v"] > f32(F.bounds[3]):   # :1715-1718
            t["gate"] = "bounds"
        if t["gate"] is not None and variant != "gates-left-only":
            continue
        R = f32(f32(th) * F.scale_factors[int(p["octave"])])           # :1724 / :1802
        if t["gate"] is None:
            s = t["L"] = search(p, gl, p["u"], p["v"], R, taken, variant == "stereo-gate")
            empty = s["outcome"] == "empty" or (variant == "blocked-left-is-empty" and s["outcome"] == "none")
            if empty and variant != "empty-left-searches-right":        # :1735-1736: the next point
                t["R_skip"] = "left window empty"
                continue
            if s["outcome"] != "empty":
                keep(s, p, qi, 2 * qi, True)
        ur, vr = f32(right_uv[qi][0]), f32(right_uv[qi][1])            # :1795-1796
        if variant == "right-bounds" and (ur < f32(F.bounds[0]) or ur > f32(F.bounds[1]) or
                                          vr < f32(F.bounds[2]) or vr > f32(F.bounds[3])):
            t["R_skip"] = "bounds"
            continue
        tk = taken
        if variant == "right-sees-later":
            def tk(idx, e=2 * qi + 1):
                w = _later.get(int(idx))
                return w[1] > 0 if w is not None and w[0] > e else taken(idx)
        s = t["R"] = search(p, gl if variant == "right-left-grid" else gr, ur, vr, R, tk, False)
        if s["outcome"] != "empty":
            keep(s, p, qi, 2 * qi + 1, variant != "hist-left-only")
    bins = kept = None
    if check_ori:                                                       # :1864-1884
        bins = [len(h) for h in hist]
        kept = py_three_maxima(bins)
        for b, h in enumerate(hist):
            if b in kept:
                continue
            for slot, (qi, side) in h:
                mvp[slot] = -1
                n -= 1
                if trace:
                    tq[qi][side]["outcome"] = "dropped bin"
    if trace:
        return n, {"q": tq, "bins": bins, "kept_bins": kept}
    return n
