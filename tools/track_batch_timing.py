"""TrackWithMotionModel's SearchByProjection(CurrentFrame, LastFrame, th 7, stereo) for many camera
streams: 1,000-feature synthetic stereo frames (synth_match.synth_frame) with 316 last-frame points each,
about 300 of them valid (synth_match.synth_last_points), every frame with its own pose, checkOri on.
64 distinct frames are planted into device slabs of 512 images (each eight times).

Legs at B = 1 / 32 / 512 frames (wall time of synchronous C-ABI calls through ctypes with arguments built
in advance, host clock; every call returns complete results):
  batch   one orbfe_search_by_projection_lastframe_slabs call on the device slabs
  loop    B calls of orbfe_search_by_projection_lastframe_pose on host copies of the same frames, each
          starting from slots reset to -1 (the reset is timed: a caller has to do it)
  cpu     the oracle's sbp_lastframe_pose, B sequential calls on one CPU thread
The legs alternate inside every repetition; parity of batch and loop with the oracle is checked on every
distinct frame before any timing. The JSON keeps median, p10, p90 and min of each leg, per-frame times, the
kernel time of the batch (device events) and the ratios at B = 512.

  python tools/track_batch_timing.py [--reps 100] [--out profiles/track_batch.json]
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
from orb_slam3_ros_amd.matcher import CameraModel, MatchFrame, Pose, TrackJob

NFEAT, NPTS, TH, CAP, UNIQUE, BATCHES = 1000, 316, 7.0, 1024, 64, (1, 32, 512)
W, H, MBF = 752, 480, 0.110078 * 458.654


def stats(ms, frames):
    a = np.asarray(ms)
    med = float(np.median(a))
    return {"median_ms": round(med, 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size),
            "per_frame_us": round(med * 1e3 / frames, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "track_batch.json"))
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30")
    import torch
    if not torch.cuda.is_available():
        sys.exit("track_batch_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    oracle.build()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    cam = CameraModel.make("pinhole", 458.654, 457.296, 367.215, 248.375)
    sf = sm.scale_factors(8)
    bounds = (0.0, float(W), 0.0, float(H))
    geom = MatchFrame(np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), bounds, sf, None, MBF)
    frames, jobs = [], []
    for _ in range(UNIQUE):
        F = sm.synth_frame(rng, NFEAT, W, H, 8, True, MBF)
        R, t = sm.synth_pose(rng)
        frames.append(F)
        jobs.append(TrackJob.make(Pose.se3(R, t), sm.synth_last_points(rng, F, cam, R, t, NPTS), TH))
    valid = [int(j._points["valid"].sum()) for j in jobs]
    Bmax = max(BATCHES)
    kps = np.zeros((Bmax, CAP, 7), np.int32)
    desc = np.zeros((Bmax, CAP, 32), np.uint8)
    counts = np.zeros((Bmax, 2), np.int32)
    ur = np.zeros((Bmax, CAP), np.float32)
    for f in range(Bmax):
        F = frames[f % UNIQUE]
        kps[f, :F.N] = F.keys.view(np.int32).reshape(F.N, 7)
        desc[f, :F.N] = F.desc
        counts[f] = (F.N, 0)
        ur[f, :F.N] = F.uright
    d_kps, d_desc, d_counts, d_ur = (torch.from_numpy(a).to(dev) for a in (kps, desc, counts, ur))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    arr = (TrackJob * Bmax)(*[jobs[f % UNIQUE] for f in range(Bmax)])
    rows = np.zeros((Bmax, CAP), np.int32)
    nm = np.zeros(Bmax, np.int32)
    nk = np.zeros(Bmax, np.int32)
    om = oracle.OracleMatcher(0.9, True)
    mvp1 = np.zeros(NFEAT, np.int32)
    obs1 = np.zeros(NFEAT, np.int32)
    single = [(frames[u].ref(), jobs[u]._points.ctypes.data, len(jobs[u]._points), ctypes.byref(jobs[u].Tcw))
              for u in range(UNIQUE)]
    pmvp, pobs, pcam = mvp1.ctypes.data, obs1.ctypes.data, ctypes.byref(cam)

    def batch(B):
        rc = lib.orbfe_search_by_projection_lastframe_slabs(
            d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), CAP, 0, 1, d_ur.data_ptr(), geom.ref(), pcam,
            arr, B, 1, rows.ctypes.data, nm.ctypes.data, nk.ctypes.data, stream)
        assert rc == _lib.ORBFE_OK, rc

    def loop(B):
        n = 0
        for f in range(B):
            fr, pts, npts, T = single[f % UNIQUE]
            mvp1.fill(-1)
            n += lib.orbfe_search_by_projection_lastframe_pose(fr, pmvp, pobs, pts, npts, T, None, pcam, TH, 0, 0, 1)
        return n

    def cpu(B):
        n = 0
        for f in range(B):
            u = f % UNIQUE
            mvp1.fill(-1)
            n += om.sbp_lastframe_pose(frames[u], mvp1, obs1, jobs[u]._points, jobs[u].Tcw, cam, TH, 0, 0)
        return n

    # parity before timing: the batch and the single call equal the oracle on every distinct frame
    batch(Bmax)
    matches = []
    for u in range(UNIQUE):
        mvp1.fill(-1)
        n = om.sbp_lastframe_pose(frames[u], mvp1, obs1, jobs[u]._points, jobs[u].Tcw, cam, TH, 0, 0)
        exp = mvp1.copy()
        matches.append(int(n))
        for f in range(u, Bmax, UNIQUE):
            assert nm[f] == n and nk[f] == NFEAT and np.array_equal(rows[f, :NFEAT], exp), "the batch differs from the oracle"
            assert (rows[f, NFEAT:] == -1).all()
        fr, pts, npts, T = single[u]
        mvp1.fill(-1)
        ng = lib.orbfe_search_by_projection_lastframe_pose(fr, pmvp, pobs, pts, npts, T, None, pcam, TH, 0, 0, 1)
        assert ng == n and np.array_equal(mvp1, exp), "the single call differs from the oracle"
    legs = {f"{name}_B{B}": (fn, B) for B in BATCHES for name, fn in (("batch", batch), ("loop", loop), ("cpu", cpu))}
    for _ in range(args.warmup):
        for fn, B in legs.values():
            fn(B)
    ms = {k: [] for k in legs}
    for _ in range(args.reps):   # alternating: drift on the shared host hits every leg alike
        for k, (fn, B) in legs.items():
            t0 = time.perf_counter()
            fn(B)
            ms[k].append((time.perf_counter() - t0) * 1e3)
    lib.orbfe_matcher_set_timing(1)
    kern = {B: [] for B in BATCHES}
    for _ in range(50):
        for B in BATCHES:
            batch(B)
            kern[B].append(float(lib.orbfe_matcher_last_ms()))
    lib.orbfe_matcher_set_timing(0)
    res = {"command": "python tools/track_batch_timing.py --reps %d --warmup %d" % (args.reps, args.warmup),
           "workload": {"frame_features": NFEAT, "points_per_frame": NPTS, "valid_points_per_frame_mean":
                        round(float(np.mean(valid)), 1), "th": TH, "stereo": True, "check_ori": True, "cap": CAP,
                        "distinct_frames": UNIQUE, "matches_per_frame_mean": round(float(np.mean(matches)), 1)},
           "method": "host clock around synchronous C-ABI calls through ctypes with arguments built in advance, legs "
                     "alternating per repetition, parity with the oracle checked first; loop = B single calls on host "
                     "copies, cpu = the oracle on one thread",
           "warmup": args.warmup, "legs": {k: stats(v, legs[k][1]) for k, v in ms.items()},
           "batch_kernel_ms_device_events": {f"B{B}": stats(v, B) for B, v in kern.items()}}
    b, lp, c = (res["legs"][f"{k}_B512"]["per_frame_us"] for k in ("batch", "loop", "cpu"))
    res["per_frame_us_B512"] = {"batch": b, "loop_of_single_calls": lp, "cpu_one_thread": c}
    res["loop_over_batch_B512"] = round(lp / b, 3)
    res["cpu_over_batch_B512"] = round(c / b, 3)
    res["batch_is_faster_per_frame_than_the_loop_B512"] = bool(b < lp)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
