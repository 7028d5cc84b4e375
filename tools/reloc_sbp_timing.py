"""Relocalisation refinement (Tracking.cc:3765 / :3779): SearchByProjection(CurrentFrame, pKF, sFound, 10,
100) of one 1000-feature frame against 20 candidate keyframes with 400 map points each, every candidate
with its own pose and its own copy of the frame's slots, checkOri on.

Legs (wall time of the synchronous calls, host clock; every call returns complete results):
  a  one ORBmatcher.SearchByProjectionKeyFrameBatch call (projection on the device, one launch)
  b  20 calls of ORBmatcher.SearchByProjectionKeyFrame on records projected IN ADVANCE (the caller's CPU
     projection is not timed, which favours b)
  c  the oracle's 20 sequential CPU calls, on the same records projected in advance
  d  SearchByProjectionKeyFrameBatch with a batch of 1
The legs alternate inside every repetition, parity of a / b / d with the oracle is checked before any
timing, and the JSON keeps median, p10, p90 and min of each leg, the kernel time of a and of d (device
events) and the ratios a/b and a/c. Every leg starts from a fresh copy of the slots.

  python tools/reloc_sbp_timing.py [--reps 200] [--out profiles/reloc_sbp_batch.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import reloc_sbp_definition as D
from oracle import oracle
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures, ORBmatcher

NKF, NFEAT, NPTS, TH, ORBDIST = 20, 1000, 400, 10.0, 100


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "reloc_sbp_batch.json"))
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    import torch
    if not torch.cuda.is_available():
        sys.exit("reloc_sbp_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    oracle.build()
    lib = _lib.load()
    rng = np.random.default_rng(2026)
    F = D.frame(rng, NFEAT)
    cands = []
    for c in range(NKF):   # every candidate its own pose (PnP gives one per candidate)
        R, t = sm.synth_pose(rng, 25.0, 0.4)
        cands.append(D.candidate(rng, F, D.camera(R, t), NPTS, kf_n=NFEAT))
    handles = [KeyFrameFeatures(c.KF, FeatureVector({})) for c in cands]
    cams = [c.cam for c in cands]
    pts = [c.points for c in cands]
    idx = [c.kf_idx for c in cands]
    rows0 = np.stack([c.row for c in cands])
    recs = [np.ascontiguousarray(c.records(F)[0]) for c in cands]   # projected in advance (legs b, c)
    m = ORBmatcher(0.9, True)
    om = oracle.OracleMatcher(0.9, True)

    def leg_a():
        mvp = rows0.copy()
        return m.SearchByProjectionKeyFrameBatch(F, handles, cams, pts, idx, mvp, TH, ORBDIST), mvp

    def leg_b():
        mvp = rows0.copy()
        return [m.SearchByProjectionKeyFrame(F, mvp[c], recs[c], TH, ORBDIST) for c in range(NKF)], mvp

    def leg_c():
        mvp = rows0.copy()
        return [om.sbp_kf(F, mvp[c], recs[c], TH, ORBDIST) for c in range(NKF)], mvp

    def leg_d():
        mvp = rows0[:1].copy()
        return m.SearchByProjectionKeyFrameBatch(F, handles[:1], cams[:1], pts[:1], idx[:1], mvp, TH, ORBDIST), mvp

    # parity before timing: every leg equals the oracle
    nc, rc = leg_c()
    na, ra = leg_a()
    nb, rb = leg_b()
    nd, rd = leg_d()
    assert list(na) == nc and np.array_equal(ra, rc), "the batch differs from the oracle"
    assert nb == nc and np.array_equal(rb, rc), "the per-candidate calls differ from the oracle"
    assert nd[0] == nc[0] and np.array_equal(rd[0], rc[0]), "the batch of 1 differs from the oracle"
    legs = {"a_batch20": leg_a, "b_percall20": leg_b, "c_cpu20": leg_c, "d_batch1": leg_d}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    ms = {k: [] for k in legs}
    for _ in range(args.reps):   # alternating: drift on the shared host hits every leg alike
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    lib.orbfe_matcher_set_timing(1)
    dev = {"a": [], "d": []}
    for _ in range(50):
        leg_a()
        dev["a"].append(float(lib.orbfe_matcher_last_ms()))
        leg_d()
        dev["d"].append(float(lib.orbfe_matcher_last_ms()))
    lib.orbfe_matcher_set_timing(0)
    res = {"workload": {"candidates": NKF, "points_per_candidate": NPTS, "frame_features": NFEAT, "th": TH,
                        "ORBdist": ORBDIST, "check_ori": True, "matches_per_candidate": [int(n) for n in nc]},
           "method": "host clock around synchronous calls through the Python wrappers, legs alternating per "
                     "repetition, parity with the oracle checked first; b and c read records projected in advance",
           "warmup": args.warmup, "legs": {k: stats(v) for k, v in ms.items()},
           "a_kernel_ms_device_events": stats(dev["a"]), "d_kernel_ms_device_events": stats(dev["d"])}
    a, b, c = (res["legs"][k]["median_ms"] for k in ("a_batch20", "b_percall20", "c_cpu20"))
    res["a_over_b"] = round(a / b, 4)
    res["a_over_c"] = round(a / c, 4)
    res["batch_beats_cpu_20_calls"] = bool(a < c)
    res["batch_beats_20_gpu_calls"] = bool(a < b)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for h in handles:
        h.close()


if __name__ == "__main__":
    main()
