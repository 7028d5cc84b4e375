"""The back-end ORBmatcher searches by definition: the reference's loops restated in plain Python with
np.float32 scalars, one source line per rule, every comparison in the precision the reference's C++
evaluates it in. Test infrastructure only (as the other *_definition modules): slow and sequential;
with trace=True it says which rule removed which point and which candidate.

  KeyFrame::GetFeaturesInArea / IsInImage     KeyFrame.cc:707-756 (left grid)     -> kf_area / kf_in_image
  MapPoint::PredictScale(dist, KeyFrame*)     MapPoint.cc:514-529                 -> predict_scale
  Sophus SE3f / Sim3f point action            (Eigen's evaluation order)          -> pose_apply
  Fuse(pKF, vpMapPoints, th)                  ORBmatcher.cc:1148-1338             -> py_fuse(sim3=False)
  Fuse(pKF, Scw, vpPoints, th, vpReplace)     ORBmatcher.cc:1340-1455             -> py_fuse(sim3=True)
  SearchByProjection(pKF, Scw, ...)           ORBmatcher.cc:427-532               -> py_sbp_sim3
  ... the vpPointsKFs overload                ORBmatcher.cc:534-646               -> py_sbp_sim3(point_kfs=)
  SearchBySim3                                ORBmatcher.cc:1457-1674             -> py_search_by_sim3
  SearchForTriangulation                      ORBmatcher.cc:907-1146              -> py_search_for_triangulation
  Pinhole::epipolarConstrain                  Pinhole.cpp:107-125                 -> epipolar_pinhole

The rotation bin, ComputeThreeMaxima and the Hamming distance are oracle/sbp_definition.py's.

Trace. The projection searches return per point i trace["p"][i] = {"rule": the rule that removed the
point before the search ("null", "bad", "skip", "found", "depth", "image", "distance", "view") or None,
"pc", "u", "v", "ur", "dist", "level", "R", "cands": [[idx, rule], ...] in the reference's enumeration
order (cell column, cell row, insertion order) with rule in "box", "blocked", "level", "chi2-stereo",
"chi2-mono", "lost", "best", "bd": bestDist, "best": bestIdx, "outcome": "none" / "threshold" /
"kept"}. SearchBySim3 returns the two directions' traces and the agreement; SearchForTriangulation
per KF1 keypoint of a shared node {"rule": "has-mappoint-1" / "only-stereo" / None, "cands": [[idx2,
rule]] with rule in "has-mappoint-2", "only-stereo", "threshold", "worse", "epipole", "epiline",
"den-zero", "replaced", "best"} and the histogram.

`variant` is a set of names; each evaluates one rule the way a careless restatement would, and the
planted cases (tests/backend_patterns.py) prove that they can tell:
  "chi2-float"    the 7.8 / 5.99 gates compared in float
  "epiline-float" 3.84 * sigma2 as a float product
  "proj-div" / "proj-invz-f" / "proj-invz-d"   the projection expression forced
  "log-double"    PredictScale's logf evaluated in double and rounded
  "log-all-double" ceil(log(ratio) / logsf) taken wholly in double (the float ratio and logsf promoted)
  "tie-other"     <= for < in the projection searches (last wins), >= for > in triangulation (first wins)
  "sum-order"     (a + b) + c for Eigen's a + (b + c)
  "pose-order"    the other association of the pose action's sum, and of the Sim3 scale
  "dist-double"   0.8f / 1.2f applied in double
  "ratio-double"  TH_LOW * ratioHamming in double
  "one-pass"      SearchByProjection(Sim3) as one parallel round: every query sees only the keypoints held
                  on entry, the slots are then written in query order
"""
import ctypes
import math

import numpy as np

from oracle.sbp_definition import HISTO_LENGTH, PyGrid, _ham, py_rot_bin, three_maxima_inds

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50   # ORBmatcher.cc:33-34
MP_BAD, MP_SKIP = 2, 4
SE3, SIM3 = 0, 1
INT_MAX = 2 ** 31 - 1
PRJ_DIV, PRJ_INVZ_F, PRJ_INVZ_D = "proj-div", "proj-invz-f", "proj-invz-d"

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    """The C library's logf, as the reference's log(float) resolves to."""
    return f32(_libm.logf(float(f32(x))))


def sum3(a, b, c, variant=()):
    """Eigen 3.3's fixed-size 3-term reduction (norm, dot, a product's coefficient): a + (b + c)."""
    if "sum-order" in variant:
        return f32(f32(a + b) + c)
    return f32(a + f32(b + c))


def _cross(a, b):
    return [f32(f32(a[1] * b[2]) - f32(a[2] * b[1])), f32(f32(a[2] * b[0]) - f32(a[0] * b[2])),
            f32(f32(a[0] * b[1]) - f32(a[1] * b[0]))]


def pose_apply(P, p, variant=()):
    """Sophus' point action q * p * q^-1 (* scale) + t in Eigen's evaluation order: uv = 2 (v x p);
    SE3: ((p + w uv) + v x uv) + t; Sim3 (RxSO3, scale |q|^2 reduced as one packet (x^2 + z^2) + (y^2 +
    w^2)): (s p + (w uv + v x uv)) + t."""
    q = [f32(v) for v in P.q]
    t = [f32(v) for v in P.t]
    p = [f32(v) for v in p]
    v, w = q[:3], q[3]
    uv = _cross(v, p)
    uv = [f32(a + a) for a in uv]
    c = _cross(v, uv)
    other = "pose-order" in variant
    if P.kind == SIM3:
        if other:
            sc = f32(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2])) + f32(w * w))
            return [f32(f32(f32(f32(sc * p[k]) + f32(w * uv[k])) + c[k]) + t[k]) for k in range(3)]
        sc = f32(f32(f32(v[0] * v[0]) + f32(v[2] * v[2])) + f32(f32(v[1] * v[1]) + f32(w * w)))
        return [f32(f32(f32(sc * p[k]) + f32(f32(w * uv[k]) + c[k])) + t[k]) for k in range(3)]
    if other:
        return [f32(f32(p[k] + f32(f32(w * uv[k]) + c[k])) + t[k]) for k in range(3)]
    return [f32(f32(f32(p[k] + f32(w * uv[k])) + c[k]) + t[k]) for k in range(3)]


def project(expr, fx, fy, cx, cy, pc):
    """The three projection expressions of the back end -> (u, v, invz)."""
    x, y, z = pc
    with np.errstate(all="ignore"):
        if expr == PRJ_DIV:       # Pinhole::project (Pinhole.cpp:43-49); invz = 1 / z in float (Fuse :1206)
            invz = f32(f32(1.0) / z)
            return f32(f32(f32(fx * x) / z) + cx), f32(f32(f32(fy * y) / z) + cy), invz
        if expr == PRJ_INVZ_F:    # :571-576: const float invz = 1 / p3Dc(2)
            invz = f32(f32(1.0) / z)
        else:                     # :1514-1519 / :1594-1599: const float invz = 1.0 / p3Dc(2), a double quotient
            invz = f32(1.0 / float(z)) if z != 0 else f32(math.copysign(math.inf, float(z)))
        return f32(f32(fx * f32(x * invz)) + cx), f32(f32(fy * f32(y * invz)) + cy), invz


def kf_in_image(F, u, v):
    """KeyFrame::IsInImage (KeyFrame.cc:753-756): >= min and < max; NaN fails."""
    return bool(u >= f32(F.bounds[0]) and u < f32(F.bounds[1]) and v >= f32(F.bounds[2]) and v < f32(F.bounds[3]))


def raw_scale(max_dist, dist, logsf, variant=()):
    """ceil(log(mfMaxDistance / currentDist) / mfLogScaleFactor) before the clamps (MapPoint.cc:516-522):
    the ratio in float, the C library's float log."""
    with np.errstate(all="ignore"):
        ratio = f32(f32(max_dist) / f32(dist))
        if "log-all-double" in variant:
            return math.ceil(math.log(float(ratio)) / float(f32(logsf)))
        lg = f32(math.log(float(ratio))) if "log-double" in variant else logf(ratio)
        return math.ceil(f32(lg / f32(logsf)))


def predict_scale(max_dist, dist, logsf, nlevels, variant=()):
    """MapPoint::PredictScale (MapPoint.cc:514-529): raw_scale clamped to [0, nlevels - 1]."""
    n = raw_scale(max_dist, dist, logsf, variant)
    if n < 0:
        n = 0
    elif n >= nlevels:
        n = nlevels - 1
    return n


def kf_area(grid, u, v, r):
    """KeyFrame::GetFeaturesInArea (KeyFrame.cc:707-751), left grid: Frame's cell range and |d| < r box
    without a level test -> [[idx, "box" or None], ...] in enumeration order."""
    return grid.walk(u, v, r, -1, -1)


def _geometry(F, cam, mp, T, S, expr, dist_cam, view, logsf, skip_flags, found, variant):
    """Everything of one point before GetFeaturesInArea -> the trace record (rule None: it goes on)."""
    t = {"rule": None, "level": -1}
    if mp["id"] < 0:
        t["rule"] = "null"
        return t
    if mp["flags"] & MP_BAD & skip_flags:                                  # pMP->isBad()
        t["rule"] = "bad"
        return t
    if mp["flags"] & MP_SKIP & skip_flags:                                 # pMP->IsInKeyFrame(pKF) (:1177)
        t["rule"] = "skip"
        return t
    if found is not None and int(mp["id"]) in found:                      # spAlreadyFound (:451) / vbAlreadyMatched
        t["rule"] = "found"
        return t
    P = [f32(v) for v in mp["pos"]]
    pc = pose_apply(T, P, variant)
    if S is not None:
        pc = pose_apply(S, pc, variant)
    t["pc"] = pc
    if pc[2] < 0.0:                                                        # :461, :1200, :1375, :1509
        t["rule"] = "depth"
        return t
    for name in (PRJ_DIV, PRJ_INVZ_F, PRJ_INVZ_D):
        if name in variant:
            expr = name
    u, v, invz = project(expr, f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy), pc)
    t["u"], t["v"] = u, v
    if not kf_in_image(F, u, v):                                          # :468
        t["rule"] = "image"
        return t
    with np.errstate(all="ignore"):
        t["ur"] = f32(u - f32(f32(F.mbf) * invz))                           # :1214
    if "dist-double" in variant:
        maxd, mind = float(f32(1.2)) * float(mp["max_dist"]), float(f32(0.8)) * float(mp["min_dist"])
    else:
        maxd, mind = f32(f32(1.2) * mp["max_dist"]), f32(f32(0.8) * mp["min_dist"])   # MapPoint.cc:504-512
    if dist_cam:
        PO = None
        dist = f32(np.sqrt(sum3(f32(pc[0] * pc[0]), f32(pc[1] * pc[1]), f32(pc[2] * pc[2]), variant)))   # :1525
    else:
        PO = [f32(P[k] - f32(cam.Ow[k])) for k in range(3)]
        dist = f32(np.sqrt(sum3(f32(PO[0] * PO[0]), f32(PO[1] * PO[1]), f32(PO[2] * PO[2]), variant)))   # :475
    t["dist"] = dist
    if float(dist) < float(mind) or float(dist) > float(maxd):            # :477 (both sides floats in the reference)
        t["rule"] = "distance"
        return t
    if view:
        n = [f32(x) for x in mp["normal"]]
        dotn = sum3(f32(PO[0] * n[0]), f32(PO[1] * n[1]), f32(PO[2] * n[2]), variant)
        t["dotn"] = dotn
        if float(dotn) < 0.5 * float(dist):                               # :483, float < double
            t["rule"] = "view"
            return t
    t["level"] = predict_scale(mp["max_dist"], dist, logsf, len(F.scale_factors), variant)   # :486
    return t


def _search(F, grid, t, mp, th, init_best, variant, blocked=None, inv_sigma2=None):
    """GetFeaturesInArea and the best-descriptor loop of one point; fills t."""
    lvl = t["level"]
    R = f32(f32(th) * F.scale_factors[lvl])                                # :489
    cands = kf_area(grid, t["u"], t["v"], R)
    bd, bi = init_best, -1
    for c in cands:
        idx = c[0]
        if c[1] is not None:
            continue
        if blocked is not None and blocked(idx):                          # :504
            c[1] = "blocked"
            continue
        o = int(F.keys[idx]["octave"])
        if o < lvl - 1 or o > lvl:                                        # :509
            c[1] = "level"
            continue
        if inv_sigma2 is not None:                                        # Fuse(pKF, vpMapPoints) only (:1270-1303)
            k = F.keys[idx]
            ex, ey = f32(t["u"] - k["x"]), f32(t["v"] - k["y"])
            if F.uright is not None and F.uright[idx] >= 0:
                er = f32(t["ur"] - F.uright[idx])
                e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                prod = f32(e2 * f32(inv_sigma2[o]))
                if (prod > f32(7.8)) if "chi2-float" in variant else (float(prod) > 7.8):
                    c[1] = "chi2-stereo"
                    continue
            else:
                e2 = f32(f32(ex * ex) + f32(ey * ey))
                prod = f32(e2 * f32(inv_sigma2[o]))
                if (prod > f32(5.99)) if "chi2-float" in variant else (float(prod) > 5.99):
                    c[1] = "chi2-mono"
                    continue
        c[1] = "lost"
        d = _ham(mp["desc"], F.desc[idx])
        if (d <= bd) if "tie-other" in variant else (d < bd):             # :516, strict
            bd, bi = d, idx
    for c in cands:
        if c[0] == bi and c[1] == "lost":
            c[1] = "best"
    t.update(R=R, cands=cands, bd=bd, best=bi)
    return bd, bi


def py_fuse(F, cam, inv_sigma2, pts, th, sim3, variant=(), trace=False):
    """The search half of both Fuse overloads -> (nFused, best_idx, best_dist[, trace]). best_dist is
    reported for every point that compared a candidate, -1 otherwise."""
    grid = PyGrid(F)
    n = len(pts)
    best_idx, best_dist = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    nf, tp = 0, {}
    for i, mp in enumerate(pts):
        t = _geometry(F, cam, mp, cam.Tcw, None, PRJ_DIV, False, True, cam.log_scale_factor, MP_BAD | MP_SKIP, None,
                      variant)
        tp[i] = t
        if t["rule"] is not None:
            continue
        bd, bi = _search(F, grid, t, mp, th, INT_MAX if sim3 else 256, variant,     # :1258 / :1415
                         inv_sigma2=None if sim3 else inv_sigma2)
        t["outcome"] = "none" if bi < 0 else "threshold"
        if bi >= 0:
            best_dist[i] = bd
        if bd <= TH_LOW:                                                  # :1312 / :1437
            best_idx[i] = bi
            nf += 1
            t["outcome"] = "kept"
    return (nf, best_idx, best_dist, {"p": tp}) if trace else (nf, best_idx, best_dist)


def py_sbp_sim3(F, cam, pts, matched, th, ratio, point_kfs=None, matched_kf=None, variant=(), trace=False):
    """SearchByProjection(pKF, Scw, vpPoints, [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratioHamming):
    sequential; matched (and matched_kf) are updated in place."""
    grid = PyGrid(F)
    found = {int(m) for m in matched if m >= 0}                            # :440-441
    held0 = matched >= 0
    lim = float(TH_LOW) * float(f32(ratio)) if "ratio-double" in variant else f32(f32(TH_LOW) * f32(ratio))
    expr = PRJ_INVZ_F if point_kfs is not None else PRJ_DIV               # :571-576 / :465
    parallel = "one-pass" in variant
    n, tp, writes = 0, {}, []
    for i, mp in enumerate(pts):
        t = _geometry(F, cam, mp, cam.Tcw, None, expr, False, True, cam.log_scale_factor, MP_BAD, found, variant)
        tp[i] = t
        if t["rule"] is not None:
            continue
        blocked = (lambda idx: bool(held0[idx])) if parallel else (lambda idx: matched[idx] >= 0)
        bd, bi = _search(F, grid, t, mp, th, 256, variant, blocked=blocked)   # :499
        t["outcome"] = "none" if bi < 0 else "threshold"
        if (float(bd) <= lim) if "ratio-double" in variant else (f32(bd) <= lim):   # :523, int * float
            t["outcome"] = "kept"
            if parallel:
                writes.append((i, bi))
                continue
            matched[bi] = mp["id"]
            if point_kfs is not None and matched_kf is not None:
                matched_kf[bi] = point_kfs[i]
            n += 1
    for i, bi in writes:
        matched[bi] = pts[i]["id"]
        if point_kfs is not None and matched_kf is not None:
            matched_kf[bi] = point_kfs[i]
        n += 1
    return (n, {"p": tp}) if trace else n


def _sim3_side(B, ptsA, already, TAw, SBA, cam1, logsfB, th, variant):
    grid = PyGrid(B)
    vn = np.full(len(ptsA), -1, np.int64)
    tp = {}
    for i, mp in enumerate(ptsA):
        if mp["id"] >= 0 and already[i]:                                  # :1491 / :1571
            tp[i] = {"rule": "found", "level": -1}
            continue
        t = _geometry(B, cam1, mp, TAw, SBA, PRJ_INVZ_D, True, False, logsfB, MP_BAD, None, variant)
        tp[i] = t
        if t["rule"] is not None:
            continue
        bd, bi = _search(B, grid, t, mp, th, INT_MAX, variant)            # :1547 / :1627
        t["outcome"] = "none" if bi < 0 else "threshold"
        if bd <= TH_HIGH:                                                 # :1569 / :1649
            vn[i] = bi
            t["outcome"] = "kept"
    return vn, tp


def py_search_by_sim3(K1, K2, pts1, pts2, cam1, cam2, S12, S21, th, matches12, matched_idx2=None, variant=(),
                      trace=False):
    """SearchBySim3: matches12 (handles) updated in place -> nFound."""
    N1, N2 = K1.N, K2.N
    a1, a2 = np.zeros(N1, bool), np.zeros(N2, bool)
    for i in range(N1):                                                   # :1473-1485
        if matches12[i] >= 0:
            a1[i] = True
            j = -1 if matched_idx2 is None else int(matched_idx2[i])
            if 0 <= j < N2:
                a2[j] = True
    vn1, t1 = _sim3_side(K2, pts1, a1, cam1.Tcw, S21, cam1, cam2.log_scale_factor, th, variant)
    vn2, t2 = _sim3_side(K1, pts2, a2, cam2.Tcw, S12, cam1, cam1.log_scale_factor, th, variant)
    nf, agree = 0, {}
    for i1 in range(N1):                                                  # :1655-1671
        j = int(vn1[i1])
        if j >= 0:
            agree[i1] = (j, int(vn2[j]))
            if vn2[j] == i1:
                matches12[i1] = pts2[j]["id"]
                nf += 1
    return (nf, {"side1": {"p": t1}, "side2": {"p": t2}, "vn1": vn1, "vn2": vn2, "agree": agree}) if trace else nf


def epipolar_pinhole(kp1, kp2, F12, unc, variant=()):
    """Pinhole::epipolarConstrain (Pinhole.cpp:107-125) on a precomputed F12 -> "den-zero", "epiline" or
    None. The line and the distance in float, dsqr < 3.84 * unc with the double literal."""
    F12 = [f32(x) for x in np.asarray(F12).reshape(9)]
    x1, y1, x2, y2 = f32(kp1["x"]), f32(kp1["y"]), f32(kp2["x"]), f32(kp2["y"])
    a = f32(f32(f32(x1 * F12[0]) + f32(y1 * F12[3])) + F12[6])
    b = f32(f32(f32(x1 * F12[1]) + f32(y1 * F12[4])) + F12[7])
    c = f32(f32(f32(x1 * F12[2]) + f32(y1 * F12[5])) + F12[8])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return "den-zero"
    dsqr = f32(f32(num * num) / den)
    if "epiline-float" in variant:
        ok = dsqr < f32(f32(3.84) * f32(unc))
    else:
        ok = float(dsqr) < 3.84 * float(f32(unc))
    return None if ok else "epiline"


def py_search_for_triangulation(K1, mp1, fv1, K2, mp2, fv2, F12, ep, sigma2_2, only_stereo, coarse, check_ori,
                                epi=None, variant=(), trace=False):
    """SearchForTriangulation (a second camera only as far as bStereo and the epipole test read it). fv1 / fv2: {node id: [keypoint indices]}.
    epi(idx1, idx2) -> bool replaces the pinhole test (the caller-supplied form). -> (n, matches12)."""
    m12 = np.full(K1.N, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    n, tq = 0, {}
    ep = [f32(ep[0]), f32(ep[1])]
    # a keyframe with a second camera (NLeft != -1): no stereo keypoints; KF1's switches the epipole test off
    two1, two2 = getattr(K1, "nleft", None) is not None, getattr(K2, "nleft", None) is not None
    for node in sorted(set(fv1) & set(fv2)):                              # :947-1107, the shared nodes
        for i1 in fv1[node]:
            t = tq[i1] = {"rule": None, "cands": [], "best": -1, "bd": TH_LOW}
            if mp1[i1] >= 0:                                              # :967-971
                t["rule"] = "has-mappoint-1"
                continue
            st1 = not two1 and K1.uright is not None and K1.uright[i1] >= 0   # :973 (!pKF1->mpCamera2 && ...)
            if only_stereo and not st1:                                   # :975-977
                t["rule"] = "only-stereo"
                continue
            k1 = K1.keys[i1]
            bd, bi = TH_LOW, -1                                           # :994
            for i2 in fv2[node]:
                c = [i2, None]
                t["cands"].append(c)
                if mp2[i2] >= 0:                                          # :1004 (vbMatched2 is never set)
                    c[1] = "has-mappoint-2"
                    continue
                st2 = not two2 and K2.uright is not None and K2.uright[i2] >= 0
                if only_stereo and not st2:                               # :1010-1012
                    c[1] = "only-stereo"
                    continue
                d = _ham(K1.desc[i1], K2.desc[i2])
                if d > TH_LOW:                                            # :1018
                    c[1] = "threshold"
                    continue
                if (d >= bd) if "tie-other" in variant else (d > bd):   # :1018: an equal one goes on
                    c[1] = "worse"
                    continue
                k2 = K2.keys[i2]
                if not st1 and not st2 and not two1:                      # :1025-1033 (&& !pKF1->mpCamera2)
                    dx, dy = f32(ep[0] - k2["x"]), f32(ep[1] - k2["y"])
                    if f32(f32(dx * dx) + f32(dy * dy)) < f32(f32(100) * K2.scale_factors[int(k2["octave"])]):
                        c[1] = "epipole"
                        continue
                if not coarse:                                            # :1036-1074
                    if epi is not None:
                        r = None if epi(int(i1), int(i2)) else "epiline"
                    else:
                        r = epipolar_pinhole(k1, k2, F12, sigma2_2[int(k2["octave"])], variant)
                    if r is not None:
                        c[1] = r
                        continue
                for o in t["cands"]:
                    if o[1] == "best":
                        o[1] = "replaced"
                c[1] = "best"
                bd, bi = d, i2
            t["best"], t["bd"] = bi, bd
            if bi >= 0:                                                   # :1077-1098
                m12[i1] = bi
                n += 1
                if check_ori:
                    hist[py_rot_bin(k1["angle"], K2.keys[bi]["angle"])].append(i1)
    bins = keep = None
    if check_ori:                                                         # :1114-1131
        bins = [len(h) for h in hist]
        keep = set(three_maxima_inds(bins))
        for b, h in enumerate(hist):
            if b not in keep:
                for i1 in h:
                    m12[i1] = -1
                    n -= 1
                    tq[i1]["dropped"] = True
    return (n, m12, {"q": tq, "bins": bins, "kept_bins": keep}) if trace else (n, m12)
