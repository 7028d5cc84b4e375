#!/usr/bin/env python3
"""Times the loop-closure place-recognition pair and writes profiles/place_recognition.json.

 * SearchByBoW(KF1, KF2): one query keyframe of 1,000 features against 33 resident candidates of 1,000
   features (3 candidates x 11 covisibles), nnratio 0.9: the batched call
   (orbfe_search_by_bow_kf_batch), a loop of 33 orbfe_search_by_bow_kf2 calls in the same process, and
   the oracle's search_by_bow_kf loop on one CPU thread; also a batch of 1 against one single call.
 * orbfe_kfdb_detect_nbest against databases of 500 / 2,000 / 8,000 keyframes, next to
   orbfe_kfdb_detect_reloc on the same database.

Host clock around synchronous calls (each returns with its results on the host); the legs alternate per
repetition, after warm-up calls; median, p10, p90 and minimum are reported. The parity of the timed
inputs (batched rows == single-call rows == oracle rows) is checked first and recorded.

Usage: python tools/place_recognition_timing.py [--reps 30] [--warmup 5] [--out profiles/place_recognition.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": len(a)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def bow_case(args):
    from oracle import oracle
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.matcher import FeatureVector, KeyFrameFeatures, MatchFrame, ORBmatcher
    oracle.build()
    rng = np.random.default_rng(1509)
    n, words, ncand = 1000, 400, 33

    def fv(w):
        d = {}
        for i, x in enumerate(np.asarray(w).tolist()):
            d.setdefault(int(x) * 7 + 3, []).append(i)
        return FeatureVector(d)

    def mp(k, base):
        return np.where(rng.random(k) < 0.2, -1, np.arange(k) + base).astype(np.int32)
    F = sm.synth_frame(rng, n, stereo=False)
    wf = rng.integers(0, words, n)
    f1, m1 = fv(wf), mp(n, 100)
    h1 = KeyFrameFeatures(F, f1)
    cands = []
    for c in range(ncand):   # a candidate and its covisibles see the query's scene; every third is unrelated
        if c % 3 == 2:
            X = sm.synth_frame(rng, n, stereo=False)
            keys, desc, wk = X.keys, X.desc, rng.integers(0, words, n)
        else:
            KF, src = sm.perturbed_frame(rng, F, rot=20.0, flip_p=0.05, drop=0.15)
            keys, desc = KF.keys, KF.desc
            wk = rng.integers(0, words, n)
            wk[src >= 0] = wf[src[src >= 0]]
        f2 = fv(wk)
        frame = MatchFrame(keys, desc, F.bounds, F.scale_factors)
        cands.append((keys, desc, f2, mp(n, 10000 * (c + 1)), KeyFrameFeatures(frame, f2)))
    m, om = ORBmatcher(0.9, True), oracle.OracleMatcher(0.9, True)
    hs, mps = [c[4] for c in cands], [c[3] for c in cands]

    def batch(k=ncand):
        return m.SearchByBoWKFBatch(h1, m1, hs[:k], mps[:k])

    def loop(k=ncand):
        return [m.SearchByBoWKF(F.keys, F.desc, m1, f1, c[0], c[1], c[3], c[2]) for c in cands[:k]]

    def cpu(k=ncand):
        return [om.search_by_bow_kf(F.keys, F.desc, m1, f1, c[0], c[1], c[3], c[2]) for c in cands[:k]]
    nb, rb = batch()
    rl, rc = loop(), cpu()
    parity = {"batch_equals_single_calls": bool(all(nb[c] == rl[c][0] and np.array_equal(rb[c], rl[c][1])
                                                    for c in range(ncand))),
              "batch_equals_oracle": bool(all(nb[c] == rc[c][0] and np.array_equal(rb[c], rc[c][1])
                                              for c in range(ncand)))}
    for _ in range(args.warmup):
        batch(), loop(), batch(1), loop(1)
    t = {k: [] for k in ("batch33", "loop33", "cpu33", "batch1", "single1")}
    for _ in range(args.reps):
        t["batch33"].append(timed(batch))
        t["loop33"].append(timed(loop))
        t["cpu33"].append(timed(cpu))
        t["batch1"].append(timed(lambda: batch(1)))
        t["single1"].append(timed(lambda: loop(1)))
    res = {k: stats(v) for k, v in t.items()}
    res["matches_per_candidate"] = [int(x) for x in nb]
    res["parity"] = parity
    res["batch33_over_loop33"] = round(res["batch33"]["median_ms"] / res["loop33"]["median_ms"], 4)
    res["batch33_over_cpu33"] = round(res["batch33"]["median_ms"] / res["cpu33"]["median_ms"], 4)
    res["batch1_over_single1"] = round(res["batch1"]["median_ms"] / res["single1"]["median_ms"], 4)
    res["batch_beats_loop"] = bool(res["batch33"]["median_ms"] < res["loop33"]["median_ms"])
    for c in cands:
        c[4].close()
    h1.close()
    return res


def kfdb_case(args, n_kf):
    import kfdb_definition as kd
    from orb_slam3_ros_amd.keyframe_db import KeyFrameDatabase
    rng = np.random.default_rng(n_kf)
    n_words = 100000
    db = KeyFrameDatabase(n_words)
    hot = np.sort(rng.choice(n_words, 3000, replace=False))   # the words of the place the query sees
    bows = []
    for i in range(n_kf):
        ids = np.unique(np.concatenate([rng.choice(hot, 300), rng.choice(n_words, 700)])).astype(np.uint32)
        w = rng.uniform(0.05, 1.0, len(ids))
        bows.append((ids, w / w.sum()))
        db.add(i, bows[-1])
    q = bows[int(rng.integers(0, n_kf))]
    nbrs = {i: [int(x) for x in rng.integers(0, n_kf, 10)] for i in range(n_kf)}
    maps = {i: i % 2 for i in range(n_kf)}
    con = [int(x) for x in rng.integers(0, n_kf, 15)]

    def nbest():
        return db.DetectNBestCandidates(q, con, 0, 3, nbrs, maps)

    def reloc():
        return db.DetectRelocalizationCandidates(q, 0, nbrs, maps)
    for _ in range(args.warmup):
        nbest(), reloc()
    t = {"detect_nbest": [], "detect_reloc": []}
    for _ in range(args.reps):
        t["detect_nbest"].append(timed(nbest))
        t["detect_reloc"].append(timed(reloc))
    loop, merge = nbest()
    res = {k: stats(v) for k, v in t.items()}
    res["n_loop"], res["n_merge"] = len(loop), len(merge)
    db.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_recognition.json"))
    args = ap.parse_args()
    out = {"method": "host clock around synchronous calls through the Python wrappers, legs alternating per repetition "
                     "after warm-up calls; parity of the timed inputs checked first",
           "warmup": args.warmup,
           "search_by_bow_kf": {"workload": "1 query keyframe x 33 resident candidates, 1,000 features each, 400 nodes, "
                                            "nnratio 0.9, checkOri", **bow_case(args)},
           "kfdb": {str(n): kfdb_case(args, n) for n in (500, 2000, 8000)}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
