"""The projection of SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) restated in
numpy float32 scalars (ORBmatcher.cc:1904-1939, MapPoint::PredictScale MapPoint.cc:531-546), the
definition orbfe_search_by_projection_kf_batch's device projection is checked against, and the
scenes the CPU and GPU tests of that call share.

Per point: x3Dc = Tcw * x3Dw (the Sophus SE3 point action in Eigen's order, as
oracle/orb_oracle_match.cpp:575-586 states it), uv = mpCamera->project(x3Dc) (Pinhole.cpp:43-49,
KannalaBrandt8.cpp:67-82), the image bounds, dist3D = |x3Dw - Ow| with Eigen's 3-term sum
a + (b + c), the gates 0.8f * mfMinDistance / 1.2f * mfMaxDistance, PredictScale with the C library's
logf. Every operation is one IEEE float32 operation (numpy float32 scalars never contract); logf,
atan2f, cosf and sinf are libm's. There is no z > 0 test (the reference has none); a non-finite uv is
rejected (the one narrowing of the device call). The expected search result of a candidate is
OracleMatcher.sbp_kf on the records this returns.
"""
import ctypes

import numpy as np

from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import (MAP_POINT_3D_DTYPE, PROJ_POINT_DTYPE, CameraModel, KFCamera, MatchFrame,
                                       Pose)

f32 = np.float32
_libm = ctypes.CDLL("libm.so.6")
for _n, _k in (("logf", 1), ("cosf", 1), ("sinf", 1), ("atan2f", 2)):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float] * _k


def _m(name, *a):
    return f32(getattr(_libm, name)(*[float(v) for v in a]))


# why a point is not searched
OK, NONFINITE, LEFT, RIGHT, ABOVE, BELOW, NEAR, FAR = range(8)


def sum3(a, b, c):
    return f32(a + f32(b + c))


def pose_apply(q, t, p):
    """Sophus::SE3f * point (oracle/orb_oracle_match.cpp:575-586, the ORBFE_SE3 branch)."""
    vx, vy, vz, w = (f32(v) for v in q)
    p = [f32(v) for v in p]
    uv = [f32(f32(vy * p[2]) - f32(vz * p[1])), f32(f32(vz * p[0]) - f32(vx * p[2])), f32(f32(vx * p[1]) - f32(vy * p[0]))]
    uv = [f32(v + v) for v in uv]
    c = [f32(f32(vy * uv[2]) - f32(vz * uv[1])), f32(f32(vz * uv[0]) - f32(vx * uv[2])), f32(f32(vx * uv[1]) - f32(vy * uv[0]))]
    return [f32(f32(f32(p[k] + f32(w * uv[k])) + c[k]) + f32(t[k])) for k in range(3)]


def cam_project(kind, prm, x, y, z):
    fx, fy, cx, cy = (f32(v) for v in prm[:4])
    if kind == CameraModel.KANNALA_BRANDT8:
        k = [f32(v) for v in prm[4:8]]
        x2y2 = f32(f32(x * x) + f32(y * y))
        theta = _m("atan2f", np.sqrt(x2y2), z)
        psi = _m("atan2f", y, x)
        t2 = f32(theta * theta)
        t3 = f32(theta * t2)
        t5 = f32(t3 * t2)
        t7 = f32(t5 * t2)
        t9 = f32(t7 * t2)
        r = f32(f32(f32(f32(theta + f32(k[0] * t3)) + f32(k[1] * t5)) + f32(k[2] * t7)) + f32(k[3] * t9))
        return (f32(f32(f32(fx * r) * _m("cosf", psi)) + cx), f32(f32(f32(fy * r) * _m("sinf", psi)) + cy))
    return f32(f32(f32(fx * x) / z) + cx), f32(f32(f32(fy * y) / z) + cy)


def project(F, cam: KFCamera, points, kf_idx, kf_angles, model=None):
    """The records of one candidate. Returns (PROJ_POINT records, reason [n], clamp [n], x3Dc [n, 3]):
    valid / u / v / octave = predicted level / angle = kf_angles[kf_idx] / id / desc; reason = OK or
    why the point is not searched; clamp = -1 / +1 where PredictScale clamped at level 0 / nlevels - 1."""
    n = len(points)
    rec = np.zeros(n, PROJ_POINT_DTYPE)
    reason = np.zeros(n, np.int32)
    clamp = np.zeros(n, np.int32)
    xc = np.zeros((n, 3), np.float32)
    q, t = [f32(v) for v in cam.Tcw.q], [f32(v) for v in cam.Tcw.t]
    Ow = [f32(v) for v in cam.Ow]
    if model is None:
        kind, prm = CameraModel.PINHOLE, [cam.fx, cam.fy, cam.cx, cam.cy]
    else:
        kind, prm = model.type, list(model.params)
    minx, maxx, miny, maxy = (f32(b) for b in F.bounds)
    logsf, nlev = f32(cam.log_scale_factor), len(F.scale_factors)
    rec["id"] = points["id"]
    rec["desc"] = points["desc"]
    rec["angle"] = np.asarray(kf_angles, np.float32)[np.asarray(kf_idx)]
    with np.errstate(all="ignore"):
        for i in range(n):
            P = [f32(v) for v in points["pos"][i]]
            c = pose_apply(q, t, P)
            xc[i] = c
            u, v = cam_project(kind, prm, *c)
            if not (np.isfinite(u) and np.isfinite(v)):
                reason[i] = NONFINITE
                continue
            rec["u"][i], rec["v"][i] = u, v
            if u < minx or u > maxx:
                reason[i] = LEFT if u < minx else RIGHT
                continue
            if v < miny or v > maxy:
                reason[i] = ABOVE if v < miny else BELOW
                continue
            PO = [f32(P[k] - Ow[k]) for k in range(3)]
            dist = np.sqrt(sum3(f32(PO[0] * PO[0]), f32(PO[1] * PO[1]), f32(PO[2] * PO[2])))
            mx, mn = f32(points["max_dist"][i]), f32(points["min_dist"][i])
            if dist < f32(f32(0.8) * mn) or dist > f32(f32(1.2) * mx):
                reason[i] = NEAR if dist < f32(f32(0.8) * mn) else FAR
                continue
            ns = int(np.ceil(f32(_m("logf", f32(mx / dist)) / logsf)))
            if ns < 0:
                ns, clamp[i] = 0, -1
            elif ns >= nlev:
                ns, clamp[i] = nlev - 1, 1
            rec["octave"][i] = ns
            rec["valid"][i] = 1
    return rec, reason, clamp, xc


# ---------------------------------------------------------------------------------------------------
# scenes: candidates whose points are perturbed keypoints of the current frame, un-projected at random
# depths through the candidate's inverse pose
FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
W, H, NLEV = 752, 480, 8


def frame(rng, n, w=W, h=H):
    return sm.synth_frame(rng, n, w, h, NLEV, stereo=False)


def camera(R, t):
    """KFCamera of x_c = R x_w + t with Ow as the caller's Sophus would give it (here: in double)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    pose = Pose.se3(R, t)
    return KFCamera.make(pose, FX, FY, CX, CY, 1.2, Ow=-(pose.rotation().T @ np.array(pose.t[:], np.float64)))


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * K @ K


class Candidate:
    """points / kf_idx / the keyframe (its angles are what the resident handle keeps) / cam / row."""

    def __init__(self, KF, cam, points, kf_idx, row, model=None):
        self.KF, self.cam, self.points, self.kf_idx, self.row, self.model = KF, cam, points, kf_idx, row, model

    def records(self, F):
        return project(F, self.cam, self.points, self.kf_idx, self.KF.keys["angle"], self.model)

    def expected(self, om, F, th, ORBdist, check_ori, row=None, records=None):
        """(nmatches, row) of the oracle's single search on the definition's records."""
        rec = self.records(F)[0] if records is None else records
        out = (self.row if row is None else row).copy()
        n = om.OracleMatcher(0.9, check_ori).sbp_kf(F, out, np.ascontiguousarray(rec), th, ORBdist)
        return n, out


def unproject(cam, u, v, depth, model=None):
    """World points on the rays of pixels (u, v) at `depth` along the optical axis for cam's pose."""
    if model is not None and model.type == CameraModel.KANNALA_BRANDT8:
        prm = [float(x) for x in model.params]
        rays = sm.kb8_unproject(u, v, *prm[:4], prm[4:8])
        c = rays * (depth / np.maximum(np.abs(rays[:, 2]), 1e-3))[:, None]
    else:
        c = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones(len(u))], 1) * depth[:, None]
    R, t = cam.Tcw.rotation(), np.array(cam.Tcw.t[:], np.float64)
    return ((c - t[None, :]) @ R).astype(np.float32)   # R^T (c - t)


def candidate(rng, F, cam, n_pts, kf_n=None, rot=15.0, ang_sd=3.0, prefill=0.1, model=None, level_jitter=True,
              src=None):
    """n_pts points copying keypoints of F (position +- 1 px, 5 % of the descriptor bits flipped, KF
    angle = keypoint angle + rot), distance limits that put the predicted level at the keypoint's
    octave (+- 1 for a third of them), in ascending slots of a keyframe of kf_n keypoints."""
    kf_n = max(n_pts, 1) + 40 if kf_n is None else kf_n
    if src is None:
        src = rng.choice(F.N, n_pts, replace=n_pts > F.N)
    u = F.keys["x"][src].astype(np.float64) + rng.normal(0, 1.0, n_pts)
    v = F.keys["y"][src].astype(np.float64) + rng.normal(0, 1.0, n_pts)
    p = np.zeros(n_pts, MAP_POINT_3D_DTYPE)
    p["pos"] = unproject(cam, u, v, rng.uniform(2.0, 10.0, n_pts), model)
    dist = np.linalg.norm(p["pos"].astype(np.float64) - np.array(cam.Ow[:], np.float64)[None, :], axis=1)
    lvl = F.keys["octave"][src].astype(np.float64)
    if level_jitter:
        lvl = np.clip(lvl + rng.choice([-1, 0, 0, 1], n_pts), 0, NLEV - 1)
    p["max_dist"] = (dist * 1.2 ** (lvl - 0.5)).astype(np.float32)
    p["min_dist"] = (p["max_dist"] / 1.2 ** (NLEV - 1)).astype(np.float32)
    p["desc"] = sm.flip_bits(rng, F.desc[src], 0.05) if n_pts else np.zeros((0, 32), np.uint8)
    p["id"] = 1000 + np.arange(n_pts)
    p["normal"] = rng.normal(size=(n_pts, 3))          # ignored by the call
    p["flags"], p["observations"] = 7, 3               # ignored by the call
    kf_idx = np.sort(rng.choice(kf_n, n_pts, replace=False)).astype(np.int32)
    KF = frame(rng, kf_n)
    KF.keys["angle"][kf_idx] = np.mod(F.keys["angle"][src] + rot + rng.normal(0, ang_sd, n_pts), 360.0)
    row = np.where(rng.random(F.N) < prefill, 500000 + np.arange(F.N), -1).astype(np.int32)
    return Candidate(KF, cam, p, kf_idx, row, model)


def plant_rejections(rng, F, cd):
    """Overwrites the first points of cd with one or more of every rejection path and level clamp;
    returns the number of points it planted."""
    p, cam = cd.points, cd.cam
    one = np.ones(1)

    def put(i, u, v, depth):
        p["pos"][i] = unproject(cam, u * one, v * one, depth * one)[0]
        d = float(np.linalg.norm(p["pos"][i].astype(np.float64) - np.array(cam.Ow[:], np.float64)))
        p["max_dist"][i], p["min_dist"][i] = d * 1.2 ** 2.5, d * 1.2 ** 2.5 / 1.2 ** (NLEV - 1)
        return d
    put(0, -6.0, 200.0, 4.0)            # left of the image
    put(1, W + 6.0, 200.0, 4.0)         # right
    put(2, 300.0, -6.0, 4.0)            # above
    put(3, 300.0, H + 6.0, 4.0)         # below
    d = put(4, 300.0, 200.0, 4.0)       # nearer than 0.8 mfMinDistance
    p["min_dist"][4], p["max_dist"][4] = d * 1.5, d * 1.5 * 1.2 ** (NLEV - 1)
    d = put(5, 310.0, 210.0, 4.0)       # farther than 1.2 mfMaxDistance
    p["max_dist"][5], p["min_dist"][5] = d / 1.3, d / 1.3 / 1.2 ** (NLEV - 1)
    for i in (6, 7):                    # behind the camera, the projection inside the image: searched
        k = int(rng.integers(F.N))
        put(i, float(F.keys["x"][k]), float(F.keys["y"][k]), -float(rng.uniform(2.0, 8.0)))
        p["desc"][i] = sm.flip_bits(rng, F.desc[k:k + 1], 0.03)[0]
    d = put(8, 320.0, 220.0, 4.0)       # ratio far above the pyramid: clamped at nlevels - 1
    p["max_dist"][8], p["min_dist"][8] = d * 1.2 ** 8.1, d * 1.2 ** 8.1 / 1.2 ** (NLEV - 1)
    # dist3D a little above mfMaxDistance (inside the 1.2 gate): ceil(logf(ratio) / logsf) = ceil(-0.x) =
    # 0, the lowest level; and at the gate itself, where the float ratio's logarithm can fall below
    # -logsf: PredictScale's nScale < 0 clamp
    d = put(9, 330.0, 230.0, 4.0)
    p["max_dist"][9], p["min_dist"][9] = d / 1.1, d / 1.1 / 1.2 ** (NLEV - 1)
    Ow = [f32(x) for x in cam.Ow]
    for depth in np.arange(4.0, 6.0, 0.05):   # about one depth in three has such a float next to dist / 1.2f
        put(10, 340.0, 240.0, float(depth))
        PO = [f32(f32(p["pos"][10][k]) - Ow[k]) for k in range(3)]
        dist = np.sqrt(sum3(f32(PO[0] * PO[0]), f32(PO[1] * PO[1]), f32(PO[2] * PO[2])))
        for mx in (f32(dist / f32(1.2)), np.nextafter(f32(dist / f32(1.2)), f32(0))):
            inside = not dist > f32(f32(1.2) * mx)
            if inside and int(np.ceil(f32(_m("logf", f32(mx / dist)) / f32(cam.log_scale_factor)))) < 0:
                p["max_dist"][10], p["min_dist"][10] = mx, mx / f32(1.2 ** (NLEV - 1))
                return 11
    raise AssertionError("no distance with a negative predicted scale inside the gate")


POSES = (((0, 0, 1), 0.0, (0.3, -0.2, 0.1)), ((1, 2, 0.5), 8.0, (-0.2, 0.1, 0.3)), ((0.2, 1, 0.1), 25.0, (0.4, 0.1, -0.2)))


def pose(i):
    axis, deg, t = POSES[i % len(POSES)]
    return camera(rotation(axis, deg), t)


def scene_main(seed=4100, n=300, n_pts=150):
    """Three candidates with distinct poses (the third rotated by 25 degrees); candidate 0 carries every
    rejection path. Returns (F, candidates)."""
    rng = np.random.default_rng(seed)
    F = frame(rng, n)
    cands = [candidate(rng, F, pose(i), n_pts, rot=10.0 + 20.0 * i) for i in range(3)]
    plant_rejections(rng, F, cands[0])
    return F, cands


def scene_rows(seed=4200):
    """Two candidates with the same pose, points and keyframe, and different slots held beforehand."""
    rng = np.random.default_rng(seed)
    F = frame(rng, 300)
    a = candidate(rng, F, pose(1), 120, prefill=0.3)
    row = np.where(rng.random(F.N) < 0.3, 700000 + np.arange(F.N), -1).astype(np.int32)
    return F, [a, Candidate(a.KF, a.cam, a.points, a.kf_idx, row)]


def scene_contention(seed=4300, planted=10):
    """`planted` consecutive points of candidate 0 on one window, every descriptor nearest the same
    keypoint k0, with ten more keypoints of k0's octave and near-copies of its descriptor around it: the
    first point in order takes k0, the later ones their next-best. Returns (F, candidates, (first, count))."""
    rng = np.random.default_rng(seed)
    F0 = frame(rng, 300)
    keys, desc = F0.keys.copy(), F0.desc.copy()
    k0 = 17
    keys["x"][k0], keys["y"][k0], keys["octave"][k0] = 400.0, 250.0, 2
    near = np.arange(100, 110)
    keys["x"][near] = 400.0 + rng.uniform(-6, 6, len(near))
    keys["y"][near] = 250.0 + rng.uniform(-6, 6, len(near))
    keys["octave"][near] = 2
    keys["angle"][near] = keys["angle"][k0]
    desc[near] = sm.flip_bits(rng, np.repeat(desc[k0:k0 + 1], len(near), 0), 0.12)
    F = MatchFrame(keys, desc, F0.bounds, F0.scale_factors)
    src = rng.choice(np.setdiff1d(np.arange(F.N), np.append(near, k0)), 140, replace=False)
    first = 40
    src[first:first + planted] = k0
    cd = candidate(rng, F, pose(2), 140, src=src, level_jitter=False, prefill=0.0)
    cd.points["desc"][first:first + planted] = sm.flip_bits(rng, np.repeat(desc[k0:k0 + 1], planted, 0), 0.02)
    return F, [cd, candidate(rng, F, pose(0), 60)], (first, planted)


def reversed_block(cd, first, count):
    """cd with the points [first, first + count) in reverse order (the KF slots stay ascending)."""
    pts = cd.points.copy()
    pts[first:first + count] = cd.points[first:first + count][::-1]
    KF = MatchFrame(cd.KF.keys.copy(), cd.KF.desc, cd.KF.bounds, cd.KF.scale_factors)
    blk = cd.kf_idx[first:first + count]
    KF.keys["angle"][blk] = cd.KF.keys["angle"][blk][::-1]
    return Candidate(KF, cd.cam, pts, cd.kf_idx, cd.row, cd.model)


def scene_rotation(seed=4400):
    """A third of candidate 0's keyframe angles are 120 degrees off and a sixth 240 degrees, each group
    spread over neighbouring bins: more than three bins are filled, so ComputeThreeMaxima drops some."""
    rng = np.random.default_rng(seed)
    F = frame(rng, 300)
    cd = candidate(rng, F, pose(1), 180, ang_sd=9.0)
    j = np.arange(180)
    off = np.where(j % 3 == 1, 120.0, np.where(j % 6 == 2, 240.0, 0.0))
    a = cd.KF.keys["angle"]
    a[cd.kf_idx] = np.mod(a[cd.kf_idx] + off, 360.0).astype(np.float32)
    return F, [cd, candidate(rng, F, pose(0), 100)]


def scene_tiny(seed=4500, C=33):
    """C candidates of 3 to 8 points, every one with its own pose."""
    rng = np.random.default_rng(seed)
    F = frame(rng, 300)
    cands = []
    for c in range(C):
        R, t = sm.synth_pose(rng, 30.0, 0.4)
        cands.append(candidate(rng, F, camera(R, t), int(rng.integers(3, 9)), prefill=0.05))
    return F, cands


def scene_limits(seed=4600):
    """The one-workgroup limits: 2048 keypoints, two candidates of 2048 points."""
    rng = np.random.default_rng(seed)
    F = frame(rng, 2048)
    return F, [candidate(rng, F, pose(i + 1), 2048, kf_n=2100) for i in range(2)]


def scene_kb8(seed=4700):
    """A KannalaBrandt8 current frame (the TUM-VI left camera on a 512 x 512 image)."""
    rng = np.random.default_rng(seed)
    F = frame(rng, 300, 512, 512)
    model = CameraModel.make("kb8", *sm.TUMVI_LEFT[:4], sm.TUMVI_LEFT[4])
    return F, [candidate(rng, F, pose(i), 120, model=model) for i in (2, 1)], model
