"""Relocalisation candidates (KeyFrameDatabase::DetectRelocalizationCandidates, KeyFrameDatabase.cc:733-845)
at 500, 2,000 and 8,000 keyframes: BowVectors of 1,000 features each on a synth_vocabulary(10, 5)
(100,000 words), the query a perturbed copy of one keyframe's features. No covisibility neighbours.

Legs per database size (wall time of synchronous calls, host clock, alternating inside every repetition):
  gpu   KeyFrameDatabase.DetectRelocalizationCandidates over the HBM-resident database
  cpu   the std::list / std::map restatement (tests/native/kfdb_cpu.cpp), one thread, the BowVector
        built outside the timed call's loop
and once: gpu_fixed, the same GPU call against a database of one keyframe (the per-query fixed cost:
wrapper, upload, launch, host wait). The JSON keeps median, p10, p90 and min of each leg, the GPU
leg's kernel time from device events, its remainder (host wait and upload) and the ratio gpu/cpu.
Parity of the GPU candidates and shared-word list with the CPU twin is checked before any timing.

  python tools/kfdb_timing.py [--reps 200] [--sizes 500,2000,8000] [--out profiles/kfdb_query.json]
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

from kfdb_definition import KF, KeyFrameDatabaseNative
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
from orb_slam3_ros_amd.vocabulary import L1_NORM, TF_IDF, ORBVocabulary, synth_vocabulary

NFEAT, VK, VL = 1000, 10, 5


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="500,2000,8000")
    ap.add_argument("--out", default=os.path.join("profiles", "kfdb_query.json"))
    args = ap.parse_args()
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    sizes = [int(x) for x in args.sizes.split(",")]
    import torch
    if not torch.cuda.is_available():
        sys.exit("kfdb_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    lib = _lib.load()
    rng = np.random.default_rng(2026)
    par, leaf, desc, w = synth_vocabulary(rng, VK, VL)
    voc = ORBVocabulary.from_arrays(VK, VL, L1_NORM, TF_IDF, par, leaf, desc, w)
    # features are vocabulary leaves with a few flipped bits, so that keyframes of one scene share words
    leaves = desc[np.nonzero(leaf)[0]]

    def feats(n):
        f = leaves[rng.integers(0, len(leaves), n)].copy()
        f[np.arange(n), rng.integers(0, 32, n)] ^= (1 << rng.integers(0, 8, n)).astype(np.uint8)
        return f

    nmax = max(sizes)
    bows, target_desc = [], None
    for i in range(nmax):
        d = feats(NFEAT)
        if i == 7:
            target_desc = d
        bows.append(voc.transform(d, 4)[0])
    qd = target_desc.copy()
    qd[:100] = feats(100)   # a tenth of the scene changed
    q = voc.transform(qd, 4)[0]
    one = KeyFrameDatabase(voc.n_words)
    one.add(0, bows[0])
    res = {"workload": {"kf_features": NFEAT, "vocabulary": f"synth_vocabulary({VK}, {VL})", "n_words": voc.n_words,
                        "query_words": int(len(q[0])), "mean_kf_words": round(float(np.mean([len(b[0]) for b in bows])), 1),
                        "neighbours": "none"},
           "method": "host clock around synchronous calls (GPU through the Python wrapper, CPU one native call per "
                     "query on one thread), legs alternating per repetition, parity with the CPU twin checked first",
           "warmup": args.warmup, "sizes": {}}
    fixed = []
    for n in sizes:
        g, c = KeyFrameDatabase(voc.n_words), KeyFrameDatabaseNative(voc.n_words)
        for i in range(n):
            g.add(i, bows[i])
            c.add(KF(i, bows[i]))
        # parity before timing
        gs, cs = g.shared_words(q), c.shared_words(q)
        assert np.array_equal(gs[0], cs[0]) and np.array_equal(gs[1], cs[1]) and np.array_equal(gs[3], cs[3])
        assert gs[2].tobytes() == cs[2].tobytes() and gs[4] == cs[4], "scores differ from the CPU twin"
        cand = g.DetectRelocalizationCandidates(q)
        assert np.array_equal(cand, c.DetectRelocalizationCandidates(q)) and 7 in cand.tolist()
        legs = {"gpu": lambda: g.DetectRelocalizationCandidates(q), "cpu": lambda: c.detect_reps(q, 1),
                "gpu_fixed": lambda: one.DetectRelocalizationCandidates(q)}
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        fixed += ms.pop("gpu_fixed")
        lib.orbfe_matcher_set_timing(1)
        dev = []
        for _ in range(50):
            legs["gpu"]()
            dev.append(float(lib.orbfe_matcher_last_ms()))
        lib.orbfe_matcher_set_timing(0)
        r = {k: stats(v) for k, v in ms.items()}
        r["gpu_kernel_ms_device_events"] = stats(dev)
        r["gpu_host_wait_and_upload_ms"] = round(r["gpu"]["median_ms"] - r["gpu_kernel_ms_device_events"]["median_ms"], 5)
        r["sharing_keyframes"] = int(len(gs[0]))
        r["scored_keyframes"] = int(gs[3].sum())
        r["candidates"] = int(len(cand))
        r["gpu_over_cpu"] = round(r["gpu"]["median_ms"] / r["cpu"]["median_ms"], 4)
        r["gpu_beats_cpu"] = bool(r["gpu"]["median_ms"] < r["cpu"]["median_ms"])
        res["sizes"][str(n)] = r
        g.close()
        c.close()
    res["gpu_fixed_cost_one_keyframe"] = stats(fixed)
    one.close()
    voc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
