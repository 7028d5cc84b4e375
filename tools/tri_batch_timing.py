#!/usr/bin/env python3
"""Times LocalMapping::CreateNewMapPoints' neighbour searches and writes profiles/tri_batch.json.

SearchForTriangulation(KF1, KF2[c]): one current keyframe of 1,000 features against 10 (stereo / RGB-D) and
30 (monocular) resident neighbours of about 1,000 features, 100 FeatureVector nodes (the node level of a
k = 10, L = 6 vocabulary), fine mode (bCoarse false), 40 % of the slots on either side holding a map point,
no rotation check (the matcher of CreateNewMapPoints): the batched call
(orbfe_search_for_triangulation_batch), a loop of single orbfe_search_for_triangulation calls on the host
copies in the same process, and the oracle's search_for_triangulation loop on one CPU thread; also a batch
of 1 next to one single call, and the kernel's share of the batched call (device events,
orbfe_matcher_set_timing) in a pass of its own.

Host clock around synchronous calls (each returns with its results on the host); the legs alternate per
repetition, after warm-up calls; median, p10, p90 and minimum are reported. The parity of the timed
inputs (batched rows == single-call rows == oracle rows) is checked first and recorded.

Usage: python tools/tri_batch_timing.py [--reps 30] [--warmup 5] [--out profiles/tri_batch.json]
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


def tri_case(args, n_nb):
    from oracle import oracle
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.matcher import KeyFrameFeatures, ORBmatcher, TriJob
    oracle.build()
    lib = _lib.load()
    rng = np.random.default_rng(2200 + n_nb)
    K1, fv1, mp1, sg1, nbs = sm.synth_tri_scene(rng, 1000, n_nb, 100, stereo=False, occupied=0.4)
    h1 = KeyFrameFeatures(K1, fv1, sg1)
    hs = [KeyFrameFeatures(b.K, b.fv, b.sigma2) for b in nbs]
    jobs = [TriJob.make(h, b.mp, b.F12, b.ep) for h, b in zip(hs, nbs)]
    m, om = ORBmatcher(0.6, False), oracle.OracleMatcher(0.6, False)

    def batch(k=n_nb):
        return m.SearchForTriangulationBatch(h1, mp1, jobs[:k], False, False)

    def loop(k=n_nb):
        return [m.SearchForTriangulation(K1, mp1, fv1, b.K, b.mp, b.fv, b.F12, b.ep, b.sigma2, False, False)
                for b in nbs[:k]]

    def cpu(k=n_nb):
        return [om.search_for_triangulation(K1, mp1, fv1, b.K, b.mp, b.fv, b.F12, b.ep, b.sigma2, False, False)
                for b in nbs[:k]]
    nb, rb = batch()
    forms = list(m.last_tri_batch())
    rl, rc = loop(), cpu()
    parity = {"batch_equals_single_calls": bool(all(nb[c] == rl[c][0] and np.array_equal(rb[c], rl[c][1])
                                                    for c in range(n_nb))),
              "batch_equals_oracle": bool(all(nb[c] == rc[c][0] and np.array_equal(rb[c], rc[c][1])
                                              for c in range(n_nb)))}
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
    res["neighbours"] = n_nb
    res["features"] = [int(K1.N)] + [int(b.K.N) for b in nbs]
    res["forms_workgroup_empty_fallback"] = forms
    res["matches_per_neighbour"] = [int(x) for x in nb]
    res["parity"] = parity
    res["batch_over_loop"] = round(res["batch"]["median_ms"] / res["loop"]["median_ms"], 4)
    res["batch_over_cpu"] = round(res["batch"]["median_ms"] / res["cpu"]["median_ms"], 4)
    res["batch1_over_single1"] = round(res["batch1"]["median_ms"] / res["single1"]["median_ms"], 4)
    res["kernel_share_of_batch"] = round(res["batch_kernel"]["median_ms"] / res["batch"]["median_ms"], 4)
    res["batch_beats_loop"] = bool(res["batch"]["median_ms"] < res["loop"]["median_ms"])
    for h in [h1] + hs:
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tri_batch.json"))
    args = ap.parse_args()
    out = {"method": "host clock around synchronous calls through the Python wrappers, legs alternating per repetition "
                     "after warm-up calls; the kernel time from device events in a pass of its own; parity of the "
                     "timed inputs checked first",
           "warmup": args.warmup,
           "workload": "1 current keyframe of 1,000 features x N resident neighbours of about 1,000, 100 nodes, fine "
                       "mode, 40 % of the slots occupied, no rotation check",
           "search_for_triangulation": {str(n): tri_case(args, n) for n in (10, 30)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
