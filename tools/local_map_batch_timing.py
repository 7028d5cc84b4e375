"""TrackLocalMap's SearchLocalPoints (isInFrustum + SearchByProjection(F, local map), th 1, stereo, nnratio
0.8) for many camera streams on 1,000-feature synthetic frames, two workloads:
  shared     one local map of 4,000 points, about a third of them in view of every frame; 16 distinct frames
             (poses around one place, keypoints made from what each pose sees of the map), each with its own
             skip list of 50 points
  per_frame  16 distinct frames (synth_match.synth_frame), each with its own map of 1,500 points
             (synth_match.synth_local_map_3d) and its own pose
The distinct frames are planted into device slabs of 512 images (each 32 times); a tenth of the slots hold a
point before the search.

Legs at B = 1 / 32 / 512 frames (wall time of synchronous C-ABI calls through ctypes with arguments built in
advance, host clock; every call returns complete results):
  batch   one orbfe_search_local_points_slabs call on the device slabs
  loop    B calls of orbfe_search_local_points_device on device copies of the same frames, points and slots,
          each after the slot reset a caller has to do (a device-to-device copy, timed)
  cpu     the oracle's search_local_points, B sequential calls on one CPU thread
The legs alternate inside every repetition; parity of batch and loop with the oracle is checked on every row
before any timing. The JSON keeps median, p10, p90 and min of each leg, per-frame times and the kernel time
of the batch (device events, orbfe_matcher_set_timing).

  python tools/local_map_batch_timing.py [--reps 30] [--out profiles/local_map_batch.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from oracle import oracle
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
from orb_slam3_ros_amd.matcher import MP_IN_VIEW, MP_SKIP, Camera, DeviceMatchFrame, LocalMapJob, MatchFrame

NFEAT, TH, NNRATIO, CAP, UNIQUE, BATCHES = 1000, 1.0, 0.8, 1024, 16, (1, 32, 512)
W, H, MBF = 752, 480, 0.110078 * 458.654
SF = sm.scale_factors(8)
BOUNDS = (0.0, float(W), 0.0, float(H))


def stats(ms, frames):
    a = np.asarray(ms)
    med = float(np.median(a))
    return {"median_ms": round(med, 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size),
            "per_frame_us": round(med * 1e3 / frames, 3)}


def geometry():
    return MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), BOUNDS, SF, None, MBF)


def shared_workload(rng):
    """-> frames, cams, point arrays (one object), skip lists"""
    cam0 = sm.synth_camera(rng)
    empty = sm.synth_frame(rng, 0, W, H, 8, True, MBF)
    front = sm.synth_local_map_3d(rng, empty, cam0, 2300)
    D = np.diag([-1.0, 1.0, -1.0])   # the rest of the map lies behind the camera
    back_cam = Camera.make(D @ np.array(cam0.Rcw[:], np.float64).reshape(3, 3), D @ np.array(cam0.tcw[:], np.float64),
                           cam0.fx, cam0.fy, cam0.cx, cam0.cy)
    pts = np.concatenate([front, sm.synth_local_map_3d(rng, empty, back_cam, 1700)])
    pts = np.ascontiguousarray(pts[rng.permutation(len(pts))])
    pts["id"] = np.arange(len(pts)) + 20000
    frames, cams, skips = [], [], []
    for u in range(UNIQUE):
        R = np.array(cam0.Rcw[:], np.float64).reshape(3, 3)
        t = np.array(cam0.tcw[:], np.float64) + rng.normal(0, 0.05, 3)
        cam = Camera.make(R, t, cam0.fx, cam0.fy, cam0.cx, cam0.cy)
        _, tr = oracle.is_in_frustum(geometry(), cam, pts)
        seen = np.nonzero(tr["flags"] & MP_IN_VIEW)[0]
        pick = rng.choice(seen, min(NFEAT, len(seen)), replace=False)
        k = np.zeros(len(pick), KEYPOINT_DTYPE)
        k["x"] = np.clip(tr["proj_x"][pick] + rng.normal(0, 1.0, len(pick)), 0, W - 1).astype(np.float32)
        k["y"] = np.clip(tr["proj_y"][pick] + rng.normal(0, 1.0, len(pick)), 0, H - 1).astype(np.float32)
        k["octave"] = tr["scale_level"][pick]
        k["size"] = (31.0 * SF[k["octave"]]).astype(np.float32)
        k["angle"] = rng.uniform(0, 360, len(pick)).astype(np.float32)
        k["response"], k["class_id"] = 50.0, -1
        ur = np.where(rng.random(len(pick)) < 0.7, tr["proj_xr"][pick] + rng.uniform(-1, 1, len(pick)), -1.0)
        frames.append(MatchFrame(k, sm.flip_bits(rng, pts["desc"][pick], 0.05), BOUNDS, SF, ur.astype(np.float32), MBF))
        cams.append(cam)
        skips.append(rng.choice(len(pts), 50, replace=False).astype(np.int32))
    return frames, cams, [pts] * UNIQUE, skips


def per_frame_workload(rng):
    frames, cams, maps = [], [], []
    for u in range(UNIQUE):
        F = sm.synth_frame(rng, NFEAT, W, H, 8, True, MBF)
        cam = sm.synth_camera(rng)
        frames.append(F)
        cams.append(cam)
        maps.append(sm.synth_local_map_3d(rng, F, cam, 1500))
    return frames, cams, maps, [None] * UNIQUE


def measure(lib, torch, dev, rng, frames, cams, maps, skips, reps, warmup):
    Bmax = max(BATCHES)
    kps = np.zeros((Bmax, CAP, 7), np.int32)
    desc = np.zeros((Bmax, CAP, 32), np.uint8)
    counts = np.zeros((Bmax, 2), np.int32)
    ur = np.zeros((Bmax, CAP), np.float32)
    mvp_in = np.full((Bmax, CAP), -1, np.int32)
    obs_in = np.zeros((Bmax, CAP), np.int32)
    slots = [sm.initial_slots(rng, F.N, 0.1) for F in frames]
    for f in range(Bmax):
        F = frames[f % UNIQUE]
        kps[f, :F.N] = F.keys.view(np.int32).reshape(F.N, 7)
        desc[f, :F.N] = F.desc
        counts[f] = (F.N, 0)
        ur[f, :F.N] = F.uright
        mvp_in[f, :F.N], obs_in[f, :F.N] = slots[f % UNIQUE]
    d_kps, d_desc, d_counts, d_ur = (torch.from_numpy(a).to(dev) for a in (kps, desc, counts, ur))
    stream = torch.cuda.current_stream(dev).cuda_stream
    geom = geometry()
    jobs = [LocalMapJob.make(cams[u], maps[u], TH, skips[u]) for u in range(UNIQUE)]
    arr = (LocalMapJob * Bmax)(*[jobs[f % UNIQUE] for f in range(Bmax)])
    rows = np.zeros((Bmax, CAP), np.int32)
    nm, ntm, nk = (np.zeros(Bmax, np.int32) for _ in range(3))
    # the points as each frame sees them (its skip flags set): what the single call and the oracle take
    flagged = []
    for u in range(UNIQUE):
        p = maps[u].copy()
        if skips[u] is not None:
            p["flags"][skips[u]] |= MP_SKIP
        flagged.append(p)
    dframes = [DeviceMatchFrame(F, dev) for F in frames]
    d_pts = [torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to(dev) for p in flagged]
    d_mvp0 = [torch.from_numpy(s[0].copy()).to(dev) for s in slots]
    d_obs = [torch.from_numpy(s[1].copy()).to(dev) for s in slots]
    d_mvp = [t.clone() for t in d_mvp0]
    torch.cuda.synchronize()
    one = ctypes.c_int32(0)

    def batch(B):
        rc = lib.orbfe_search_local_points_slabs(
            d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), CAP, 0, 1, d_ur.data_ptr(), geom.ref(), None, arr,
            B, mvp_in.ctypes.data, obs_in.ctypes.data, 0, 50.0, NNRATIO, rows.ctypes.data, nm.ctypes.data,
            ntm.ctypes.data, nk.ctypes.data, stream)
        assert rc == _lib.ORBFE_OK, rc

    def single(u):
        d_mvp[u].copy_(d_mvp0[u])
        n = lib.orbfe_search_local_points_device(dframes[u].ref(), ctypes.byref(cams[u]), d_pts[u].data_ptr(),
                                                 len(flagged[u]), d_mvp[u].data_ptr(), d_obs[u].data_ptr(), TH, 0, 50.0,
                                                 NNRATIO, ctypes.byref(one), stream)
        assert n >= 0, n
        return n

    def loop(B):
        return sum(single(f % UNIQUE) for f in range(B))

    def cpu_one(u):
        m, o = slots[u][0].copy(), slots[u][1]
        return oracle.search_local_points(frames[u], cams[u], flagged[u], m, o, TH, False, 50.0, NNRATIO), m

    def cpu(B):
        return sum(cpu_one(f % UNIQUE)[0][0] for f in range(B))

    # parity before timing: every row of the batch, and the single call, equal the oracle
    batch(Bmax)
    matches, in_view = [], []
    for u in range(UNIQUE):
        (n, v), exp = cpu_one(u)
        matches.append(int(n))
        in_view.append(int(v))
        N = frames[u].N
        for f in range(u, Bmax, UNIQUE):
            assert nm[f] == n and ntm[f] == v and nk[f] == N and np.array_equal(rows[f, :N], exp), \
                "the batch differs from the oracle"
            assert (rows[f, N:] == -1).all()
        ng = single(u)
        torch.cuda.synchronize()
        assert ng == n and one.value == v and np.array_equal(d_mvp[u].cpu().numpy(), exp), \
            "the single call differs from the oracle"
    legs = {f"{name}_B{B}": (fn, B) for B in BATCHES for name, fn in (("batch", batch), ("loop", loop), ("cpu", cpu))}
    for _ in range(warmup):
        for fn, B in legs.values():
            fn(B)
    ms = {k: [] for k in legs}
    for _ in range(reps):   # alternating: drift on the shared host hits every leg alike
        for k, (fn, B) in legs.items():
            t0 = time.perf_counter()
            fn(B)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    lib.orbfe_matcher_set_timing(1)
    kern = {B: [] for B in BATCHES}
    for _ in range(30):
        for B in BATCHES:
            batch(B)
            kern[B].append(float(lib.orbfe_matcher_last_ms()))
    lib.orbfe_matcher_set_timing(0)
    res = {"points_per_frame": int(np.mean([len(m) for m in maps])), "in_view_per_frame_mean": round(float(np.mean(in_view)), 1),
           "matches_per_frame_mean": round(float(np.mean(matches)), 1), "parity_on_every_row": True,
           "distinct_point_arrays_uploaded_B512": int(lib.orbfe_matcher_last_local_uploads()),
           "legs": {k: stats(v, legs[k][1]) for k, v in ms.items()},
           "batch_kernel_ms_device_events": {f"B{B}": stats(v, B) for B, v in kern.items()}}
    for B in BATCHES:
        b, lp, c = (res["legs"][f"{k}_B{B}"]["per_frame_us"] for k in ("batch", "loop", "cpu"))
        res[f"per_frame_us_B{B}"] = {"batch": b, "loop_of_single_device_calls": lp, "cpu_one_thread": c,
                                     "loop_over_batch": round(lp / b, 3), "cpu_over_batch": round(c / b, 3)}
    res["batch_is_faster_per_frame_than_the_loop_B32"] = bool(
        res["per_frame_us_B32"]["batch"] < res["per_frame_us_B32"]["loop_of_single_device_calls"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "local_map_batch.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("local_map_batch_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    oracle.build()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    res = {"command": "python tools/local_map_batch_timing.py --reps %d --warmup %d" % (args.reps, args.warmup),
           "workload": {"frame_features": NFEAT, "th": TH, "nnratio": NNRATIO, "stereo": True, "cap": CAP,
                        "distinct_frames": UNIQUE, "held_slots": 0.1},
           "method": "host clock around synchronous C-ABI calls through ctypes with arguments built in advance, legs "
                     "alternating per repetition, parity with the oracle checked on every row first; loop = B single "
                     "device-resident calls, each after resetting its slots; cpu = the oracle on one thread",
           "warmup": args.warmup}
    for name, make in (("shared", shared_workload), ("per_frame", per_frame_workload)):
        res[name] = measure(lib, torch, dev, rng, *make(rng), args.reps, args.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
