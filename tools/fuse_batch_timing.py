#!/usr/bin/env python3
"""Times the Fuse loops of LocalMapping::SearchInNeighbors and LoopClosing::SearchAndFuse and writes
profiles/fuse_batch.json.

Fuse(pKF[c], points): N resident stereo keyframes of 1,000 features, each another view of one scene
(keypoints jittered, descriptors noisy, a tenth replaced), against one shared set of 1,000 map points of that
scene, about half of them valid (a quarter NULL, a quarter bad), sim3 = 0 and th = 3 for 1, 10, 30 and 60
keyframes, and the loop-closing shape (sim3 = 1, th = 4) for 30: the batched call (orbfe_fuse_batch), a loop
of single orbfe_fuse_rig calls on the host copies in the same process, and the oracle's fuse loop on one CPU
thread; also a batch of 1 next to one single call, and the kernel's share of the batched call (device events,
orbfe_matcher_set_timing) in a pass of its own.

Host clock around synchronous calls (each returns with its results on the host); the legs alternate per
repetition, after warm-up calls; median, p10, p90 and minimum are reported. The parity of the timed inputs
(batched rows == single-call rows == oracle rows) is checked first and recorded.

Usage: python tools/fuse_batch_timing.py [--reps 30] [--warmup 5] [--out profiles/fuse_batch.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": len(a)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def fuse_case(args, n_kf, sim3, th):
    from oracle import oracle
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.matcher import FeatureVector, FuseJob, KeyFrameFeatures, ORBmatcher
    oracle.build()
    lib = _lib.load()
    rng = np.random.default_rng(3300 + n_kf + 1000 * sim3)
    KF0, cam, pts = sm.synth_fuse_scene(rng, 1000, 1000, dup=1)
    pts["id"][rng.random(len(pts)) < 0.25] = -1
    pts["flags"][rng.random(len(pts)) < 0.33] |= 2   # ORBFE_MP_BAD
    kfs = [sm.perturbed_frame(rng, KF0, shift=(0.0, 0.0), jitter=0.7, rot=5.0, drop=0.1)[0] for _ in range(n_kf)]
    sg = (KF0.scale_factors * KF0.scale_factors).astype(np.float32)
    inv = (np.float32(1.0) / sg).astype(np.float32)
    hs = [KeyFrameFeatures(K, FeatureVector({}), sg, grid=True) for K in kfs]
    skips = [rng.random(len(pts)) < 0.1 for _ in kfs]
    jobs = [FuseJob.make(h, cam, skip=s) for h, s in zip(hs, skips)]
    flagged = []
    for s in skips:
        p = pts.copy()
        p["flags"][s] |= 4   # ORBFE_MP_SKIP
        flagged.append(p)
    m, om = ORBmatcher(), oracle.OracleMatcher()

    def batch(k=n_kf):
        return m.FuseBatch(jobs[:k], pts, th, sim3)

    def loop(k=n_kf):
        return [m.Fuse(K, cam, p, th, inv, sim3=sim3) for K, p in zip(kfs[:k], flagged[:k])]

    def cpu(k=n_kf):
        return [om.fuse(K, cam, p, th, inv, sim3=sim3) for K, p in zip(kfs[:k], flagged[:k])]
    nf, bi, bd = batch()
    record = list(m.last_fuse_batch())
    rl, rc = loop(), cpu()

    def same(rows):
        return bool(all(nf[c] == rows[c][0] and np.array_equal(bi[c], rows[c][1]) and np.array_equal(bd[c], rows[c][2])
                        for c in range(n_kf)))
    parity = {"batch_equals_single_calls": same(rl), "batch_equals_oracle": same(rc)}
    assert all(parity.values()), parity
    for _ in range(args.warmup):
        batch(), loop(), batch(1), loop(1)
    t = {k: [] for k in ("batch", "loop", "cpu", "batch1", "single1")}
    for _ in range(args.reps):
        t["batch"].append(timed(batch))
        t["loop"].append(timed(loop))
        t["cpu"].append(timed(cpu))
        t["batch1"].append(timed(lambda: batch(1)))
        t["single1"].append(timed(lambda: loop(1)))
    kern = []
    lib.orbfe_matcher_set_timing(1)
    for _ in range(args.reps):
        batch()
        kern.append(float(lib.orbfe_matcher_last_ms()))
    lib.orbfe_matcher_set_timing(0)
    res = {k: stats(v) for k, v in t.items()}
    res["batch_kernel"] = stats(kern)
    res["keyframes"] = n_kf
    res["sim3"] = int(sim3)
    res["th"] = th
    res["points"] = int(len(pts))
    res["points_valid"] = int(((pts["id"] >= 0) & ((pts["flags"] & 2) == 0)).sum())
    res["jobs_empty_workgroups"] = record
    res["fused_per_keyframe"] = [int(x) for x in nf]
    res["parity"] = parity
    res["batch_over_loop"] = round(res["batch"]["median_ms"] / res["loop"]["median_ms"], 4)
    res["batch_over_cpu"] = round(res["batch"]["median_ms"] / res["cpu"]["median_ms"], 4)
    res["batch1_over_single1"] = round(res["batch1"]["median_ms"] / res["single1"]["median_ms"], 4)
    res["kernel_share_of_batch"] = round(res["batch_kernel"]["median_ms"] / res["batch"]["median_ms"], 4)
    res["batch_beats_loop"] = bool(res["batch"]["median_ms"] < res["loop"]["median_ms"])
    for h in hs:
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fuse_batch.json"))
    args = ap.parse_args()
    out = {"method": "host clock around synchronous calls through the Python wrappers, legs alternating per repetition "
                     "after warm-up calls; the kernel time from device events in a pass of its own; parity of the "
                     "timed inputs checked first",
           "warmup": args.warmup,
           "workload": "N resident stereo keyframes of 1,000 features (views of one scene) x 1,000 shared map points, "
                       "about half valid, a tenth skipped per keyframe",
           "fuse": {str(n): fuse_case(args, n, False, 3.0) for n in (1, 10, 30, 60)},
           "fuse_sim3": {"30": fuse_case(args, 30, True, 4.0)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
