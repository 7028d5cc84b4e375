"""ComputeStereoMatches written from its description, in plain numpy: TEST INFRASTRUCTURE ONLY.

An independent second reference for the rectified stereo stage (Frame.cc:811-981): when the HIP
kernels (k_stereo, k_stereo_cut) and the C++ oracle disagree on a uRight or depth value, this module
says which side is wrong, and its trace says which branch every left keypoint took, so that a
planted case can prove on the CPU that it reaches the branch it is named for. It touches no GPU and
no C++.

Algorithm. Every right keypoint is entered into the rows floor(y - r) .. ceil(y + r) of a row table,
r = 2 scale[octave]. A left keypoint on row (int)vL takes that row's entries, in right-index order,
as candidates; a candidate passes when its octave is within one of the left key's and its column uR
lies in [uL - maxD, uL], maxD = bf / mb, mb = bf / fx. Among the passing
candidates the smallest descriptor distance below 100 wins, the first one among equals. A winner
below 75 goes on to the window search on the unblurred pyramid level of the left key: with
(u, v, uR0) the key's column, row and the winner's column, each multiplied by the level's inverse
scale and rounded half away from zero, the search is rejected when uR0 + 11 >= level width (or
uR0 < 0); else the 11 x 11 window at (u, v) of the left level is compared by the sum of absolute
differences with the windows at (uR0 + inc, v), inc = -5 .. 5, of the right level. The first
strictly smallest sum wins; a winner at either end is rejected. A parabola through the winner and
its neighbours gives deltaR = (d1 - d3) / (2 (d1 + d3 - 2 d2)), rejected outside [-1, 1];
bestuR = scale (uR0 + inc + deltaR), disparity = uL - bestuR, accepted in [0, maxD) with a
disparity of zero clamped to 0.01. Over the accepted matches of the frame, the median is the
(n / 2)-th smallest winning sum and every match whose sum is not below 1.5f * 1.4f * median is cut.
The count returned is the number accepted before the cut; no accepted match returns 0.

Every value the reference holds in a `float` is an np.float32 here; std::round is half away from
zero; (int) truncates.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
TH_HIGH, TH_LOW = 100, 50
TH_ORB = (TH_HIGH + TH_LOW) // 2
W_HALF = 5   # w: half the window
L_HALF = 5   # L: half the search range

OUTCOMES = ("no-candidates", "no-filtered", "dist>=75", "window-out", "inc-at-end", "delta-out", "disparity-out",
            "clamped", "accepted", "cut")


@dataclass
class KeyTrace:
    row: int
    ncand: int = 0          # entries of the row table at (int)vL
    nfiltered: int = 0      # of those, inside the octave and uR bounds
    best_dist: int = TH_HIGH
    best_idx: int = -1      # right index of the winner (-1: none below 100)
    nties: int = 0          # passing candidates whose distance equals best_dist
    window: tuple | None = None   # (level, first row, first left column, first right column) of the windows read
    sads: list | None = None
    bestinc: int | None = None
    delta: np.float32 | None = None
    sad: int | None = None        # the winning sum of an accepted match
    match: str | None = None      # "accepted" / "clamped" before the cut
    outcome: str = "no-candidates"


@dataclass
class FrameTrace:
    keys: list = field(default_factory=list)
    n: int = 0
    median: np.float32 | None = None
    th_dist: np.float32 | None = None


def round_half_away(x):
    """std::round of a float."""
    x = F32(x)
    return F32(np.copysign(np.floor(np.abs(np.float64(x)) + 0.5), np.float64(x)))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def band(y, octave, scale):
    """Rows floor(y - r) .. ceil(y + r) of a right keypoint."""
    r = F32(2.0) * F32(scale[octave])
    return int(np.floor(F32(y) - r)), int(np.ceil(F32(y) + r))


def search_bounds(bf, fx):
    """(minU offset maxD, mb) as floats."""
    mb = F32(bf) / F32(fx)
    return F32(bf) / mb, mb


def sad_window(lv_l, lv_r, r0, c0l, c0r):
    a = lv_l[r0:r0 + 2 * W_HALF + 1, c0l:c0l + 2 * W_HALF + 1].astype(np.int64)
    b = lv_r[r0:r0 + 2 * W_HALF + 1, c0r:c0r + 2 * W_HALF + 1].astype(np.int64)
    assert a.shape == (11, 11) and b.shape == (11, 11), "window outside the level"
    return int(np.abs(a - b).sum())


def stereo_match(pyr_l, pyr_r, scale, inv_scale, kl, dl, kr, dr, bf, fx, tie_last=False):
    """-> (uRight float32[N], depth float32[N], count, FrameTrace). kl / kr: records with fields x, y,
    octave; dl / dr: uint8 [n, 32]. tie_last = True keeps the LAST of equal best distances: a deliberately
    wrong variant, for cases that must prove their answer depends on the tie rule."""
    n_l, n_r = len(kl), len(kr)
    u_right = np.full(n_l, -1.0, F32)
    depth = np.full(n_l, -1.0, F32)
    tr = FrameTrace()
    n_rows = pyr_l[0].shape[0]
    rows = [[] for _ in range(n_rows)]
    for i_r in range(n_r):
        lo, hi = band(kr["y"][i_r], int(kr["octave"][i_r]), scale)
        for yi in range(lo, hi + 1):
            if 0 <= yi < n_rows:   # the reference does not guard; keys the extractor emits stay inside
                rows[yi].append(i_r)
    max_d, _ = search_bounds(bf, fx)
    min_d = F32(0)
    accepted = []
    for i_l in range(n_l):
        u_l, v_l, level = F32(kl["x"][i_l]), F32(kl["y"][i_l]), int(kl["octave"][i_l])
        kt = KeyTrace(row=int(v_l))
        tr.keys.append(kt)
        cand = rows[int(v_l)]
        kt.ncand = len(cand)
        if not cand:
            continue
        min_u, max_u = F32(u_l - max_d), F32(u_l - min_d)
        kt.outcome = "no-filtered"
        if max_u < 0:
            continue
        for i_r in cand:
            o = int(kr["octave"][i_r])
            if o < level - 1 or o > level + 1:
                continue
            u_r = F32(kr["x"][i_r])
            if u_r >= min_u and u_r <= max_u:
                kt.nfiltered += 1
                d = hamming(dl[i_l], dr[i_r])
                if d < kt.best_dist or (tie_last and d == kt.best_dist and d < TH_HIGH):
                    kt.best_dist, kt.best_idx = d, i_r
        if kt.nfiltered == 0:
            continue
        kt.nties = sum(1 for i_r in cand if kt.best_idx >= 0 and abs(int(kr["octave"][i_r]) - level) <= 1
                       and min_u <= F32(kr["x"][i_r]) <= max_u and hamming(dl[i_l], dr[i_r]) == kt.best_dist)
        kt.outcome = "dist>=75"
        if not kt.best_dist < TH_ORB:
            continue
        u_r0 = F32(kr["x"][kt.best_idx])
        sf = F32(inv_scale[level])
        su_l, sv_l, su_r0 = round_half_away(u_l * sf), round_half_away(v_l * sf), round_half_away(u_r0 * sf)
        lv_l, lv_r = pyr_l[level], pyr_r[level]
        iniu = su_r0 + F32(L_HALF) - F32(W_HALF)
        endu = su_r0 + F32(L_HALF) + F32(W_HALF) + F32(1)
        kt.outcome = "window-out"
        if iniu < 0 or endu >= lv_r.shape[1]:
            continue
        r0, c0l = int(sv_l - F32(W_HALF)), int(su_l - F32(W_HALF))
        c0r = int(su_r0 - F32(L_HALF) - F32(W_HALF))
        kt.window = (level, r0, c0l, c0r)
        best_d, best_inc, dists = 2 ** 31 - 1, 0, []
        for inc in range(-L_HALF, L_HALF + 1):
            dist = F32(sad_window(lv_l, lv_r, r0, c0l, int(su_r0 + F32(inc) - F32(W_HALF))))
            if dist < F32(best_d):
                best_d, best_inc = int(dist), inc
            dists.append(dist)
        kt.sads, kt.bestinc = [int(d) for d in dists], best_inc
        kt.outcome = "inc-at-end"
        if best_inc == -L_HALF or best_inc == L_HALF:
            continue
        d1, d2, d3 = dists[L_HALF + best_inc - 1], dists[L_HALF + best_inc], dists[L_HALF + best_inc + 1]
        delta = F32(F32(d1 - d3) / F32(F32(2.0) * F32(F32(d1 + d3) - F32(F32(2.0) * d2))))
        kt.delta = delta
        kt.outcome = "delta-out"
        if delta < -1 or delta > 1:
            continue
        best_ur = F32(F32(scale[level]) * F32(F32(su_r0 + F32(best_inc)) + delta))
        disparity = F32(u_l - best_ur)
        kt.outcome = "disparity-out"
        if disparity >= min_d and disparity < max_d:
            kt.outcome = kt.match = "accepted"
            if disparity <= 0:
                disparity = F32(0.01)
                best_ur = F32(np.float64(u_l) - 0.01)
                kt.outcome = kt.match = "clamped"
            depth[i_l] = F32(bf) / disparity
            u_right[i_l] = best_ur
            kt.sad = best_d
            accepted.append((best_d, i_l))
    tr.n = len(accepted)
    if not accepted:
        return u_right, depth, 0, tr
    accepted.sort()
    tr.median = F32(accepted[len(accepted) // 2][0])
    tr.th_dist = F32(F32(F32(1.5) * F32(1.4)) * tr.median)
    for d, i_l in reversed(accepted):
        if F32(d) < tr.th_dist:
            break
        u_right[i_l] = depth[i_l] = F32(-1)
        tr.keys[i_l].outcome = "cut"
    return u_right, depth, len(accepted), tr
