"""Relocalisation candidates loop (Tracking.cc:3680-3701): SearchByBoW of one 1000-feature frame against
20 candidate keyframes of 1000 features, 400 words, nnratio 0.75, checkOri on.

Legs (wall time of the synchronous calls, host clock; every call returns complete results):
  a  one ORBmatcher.SearchByBoWBatch call over 20 resident keyframes (KeyFrameFeatures)
  b  20 calls of ORBmatcher.SearchByBoW (one workgroup and one round trip per candidate)
  c  the oracle's 20 sequential CPU calls
  d  SearchByBoWBatch with a batch of 1
The legs alternate inside every repetition, parity of a / b / d with the oracle is checked before any
timing, and the JSON keeps median, p10, p90 and min of each leg, a's kernel time (device events)
and the ratios a/b and a/c.

  python tools/reloc_timing.py [--reps 200] [--out profiles/reloc_bow_batch.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from oracle import oracle
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures, ORBmatcher

NKF, NFEAT, WORDS, NNRATIO = 20, 1000, 400, 0.75


def fv_of(words):
    d = {}
    for i, wd in enumerate(words.tolist()):
        d.setdefault(int(wd) * 7 + 3, []).append(i)
    return FeatureVector(d)


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "reloc_bow_batch.json"))
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    import torch
    if not torch.cuda.is_available():
        sys.exit("reloc_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    oracle.build()
    lib = _lib.load()
    rng = np.random.default_rng(2025)
    F = sm.synth_frame(rng, NFEAT, stereo=False)
    wf = rng.integers(0, WORDS, F.N)
    ff = fv_of(wf)
    kfs = []
    for c in range(NKF):   # 15 views of F's scene, 5 unrelated frames over the same words
        if c % 4 != 3:
            KF, src = sm.perturbed_frame(rng, F, rot=20.0, flip_p=0.05, drop=0.15)
            wk = rng.integers(0, WORDS, KF.N)
            wk[src >= 0] = wf[src[src >= 0]]
        else:
            KF, wk = sm.synth_frame(rng, NFEAT, stereo=False), rng.integers(0, WORDS, NFEAT)
        mp = np.where(rng.random(KF.N) < 0.25, -1, np.arange(KF.N) + 100).astype(np.int32)
        kfs.append((KF, fv_of(wk), mp))
    handles = [KeyFrameFeatures(KF, fv) for KF, fv, _ in kfs]
    mps = [mp for _, _, mp in kfs]
    m = ORBmatcher(NNRATIO, True)
    om = oracle.OracleMatcher(NNRATIO, True)

    def leg_a():
        return m.SearchByBoWBatch(handles, mps, F, ff)

    def leg_b():
        return [m.SearchByBoW(KF.keys, KF.desc, mp, fv, F, ff) for KF, fv, mp in kfs]

    def leg_c():
        return [om.search_by_bow(KF.keys, KF.desc, mp, fv, F, ff) for KF, fv, mp in kfs]

    def leg_d():
        return m.SearchByBoWBatch(handles[:1], mps[:1], F, ff)

    # parity before timing: every leg equals the oracle
    ref = leg_c()
    na, oa = leg_a()
    nd, od = leg_d()
    rb = leg_b()
    for c, (no, oo) in enumerate(ref):
        assert na[c] == no and np.array_equal(oa[c], oo), f"batch row {c} differs from the oracle"
        assert rb[c][0] == no and np.array_equal(rb[c][1], oo), f"per-call row {c} differs from the oracle"
    assert nd[0] == ref[0][0] and np.array_equal(od[0], ref[0][1])
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
    dev = []
    for _ in range(50):
        leg_a()
        dev.append(float(lib.orbfe_matcher_last_ms()))
    lib.orbfe_matcher_set_timing(0)
    res = {"workload": {"candidates": NKF, "kf_features": NFEAT, "frame_features": NFEAT, "words": WORDS,
                        "nnratio": NNRATIO, "check_ori": True, "matches_per_candidate": [int(n) for n, _ in ref]},
           "method": "host clock around synchronous calls through the Python wrappers, legs alternating per "
                     "repetition, parity with the oracle checked first",
           "warmup": args.warmup, "legs": {k: stats(v) for k, v in ms.items()},
           "a_kernel_ms_device_events": stats(dev)}
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


if __name__ == "__main__":
    main()
