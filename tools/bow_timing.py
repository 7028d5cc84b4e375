"""Frame::ComputeBoW (TemplatedVocabulary::transform, levelsup 4) per frame, for frames of about 1,000
descriptors on a synth_vocabulary(10, 6) (the ORBvoc shape: k = 10, L = 6, 1,111,111 nodes; ORBvoc itself
is not in the reference snapshot). Features are vocabulary nodes with a few flipped bits.

Legs per batch size (1, 32, 512 images), alternating inside every repetition:
  batch   ORBVocabulary.transform_batch over device-resident descriptors and counts: HIP events around
          the call on the current stream (no host wait inside), per frame = window / images
  loop    the same images one by one through ORBVocabulary.transform (host descriptors, three to four
          host waits per frame): host clock around the synchronous loop, per frame = window / images
  cpu     the oracle's transform on one CPU thread through its ctypes wrapper: host clock, per frame
and once: frame, ORBVocabulary.compute_bow on a device-resident frame (one host wait), host clock.
The loop and cpu legs run over at most --loop-images images of a batch (the per-frame cost does not
depend on how many follow). Parity of batch, loop, frame and cpu is checked before any timing.

  python tools/bow_timing.py [--reps 20] [--sizes 1,32,512] [--out profiles/bow_batch.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

from orb_slam3_ros_amd import synth_match as sm
from orb_slam3_ros_amd.matcher import DeviceMatchFrame
from orb_slam3_ros_amd.vocabulary import L1_NORM, TF_IDF, BowBatch, ORBVocabulary, synth_vocabulary

NFEAT, CAP, VK, VL = 1000, 1200, 10, 6


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="1,32,512")
    ap.add_argument("--loop-images", type=int, default=32)
    ap.add_argument("--out", default=os.path.join("profiles", "bow_batch.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    sizes = [int(x) for x in args.sizes.split(",")]
    import torch
    if not torch.cuda.is_available():
        sys.exit("bow_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    from oracle import oracle
    oracle.build()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(2027)
    par, leaf, desc, w = synth_vocabulary(rng, VK, VL)
    voc = ORBVocabulary.from_arrays(VK, VL, L1_NORM, TF_IDF, par, leaf, desc, w)
    ora = oracle.OracleVocabulary.from_arrays(VK, VL, L1_NORM, TF_IDF, par, leaf, desc, w)

    def feats(n):
        f = desc[rng.integers(1, len(desc), n)].copy()
        flips = rng.integers(0, 256, (n, 12))
        for c in range(12):   # up to 12 flipped bits: near a node, not on it
            f[np.arange(n), flips[:, c] >> 3] ^= (1 << (flips[:, c] & 7)).astype(np.uint8)
        return f

    nmax = max(sizes)
    counts = rng.integers(NFEAT - 100, NFEAT + 101, nmax).astype(np.int32)
    host = np.zeros((nmax, CAP, 32), np.uint8)
    for i in range(nmax):
        host[i, :counts[i]] = feats(int(counts[i]))
    d_desc = torch.from_numpy(host).to(dev)
    d_cnt = torch.from_numpy(np.stack([counts, np.full(nmax, -1, np.int32)], axis=1).copy()).to(dev)
    res = {"workload": {"features_per_frame": f"{NFEAT - 100}..{NFEAT + 100}", "cap": CAP, "levelsup": 4,
                        "vocabulary": f"synth_vocabulary({VK}, {VL})", "n_nodes": voc.n_nodes, "n_words": voc.n_words},
           "method": "batch: HIP events around one transform_batch call, per frame = window / images "
                     "(small batches: 64 // images calls per window); loop, cpu, frame: host clock around synchronous calls "
                     "through the Python wrappers; legs alternate per repetition; "
                     "parity of all four checked first",
           "warmup": args.warmup, "sizes": {}}
    # parity before timing
    F0 = sm.synth_frame(rng, int(counts[0]), stereo=False)
    F0.desc[:] = host[0, :counts[0]]
    DF0 = DeviceMatchFrame(F0, dev)
    chk = voc.transform_batch(d_desc[:2], d_cnt[:2])
    torch.cuda.synchronize()
    for i in range(2):
        (bb, bw), bfv = chk.host(i)
        (sb, sw), sfv = voc.transform(host[i, :counts[i]], 4)
        (ob, ow), (ofid, ofoff, ofidx) = ora.transform(host[i, :counts[i]], 4)
        assert np.array_equal(bb, sb) and bw.tobytes() == sw.tobytes() and np.array_equal(bfv.indices, sfv.indices)
        assert np.array_equal(bb, ob) and bw.tobytes() == ow.tobytes() and np.array_equal(bfv.node_ids, ofid)
    (fb, fw), _ = voc.compute_bow(DF0)
    assert np.array_equal(fb, chk.host(0)[0][0]) and fw.tobytes() == chk.host(0)[0][1].tobytes()
    res["workload"]["mean_words_per_frame"] = round(float(chk.counts[:, 0].float().mean().cpu()), 1)

    frame_ms = []
    for n in sizes:
        dd, dc = d_desc[:n], d_cnt[:n]
        out = BowBatch(n, CAP, dev)
        nl = min(n, args.loop_images)

        inner = max(1, 64 // n)   # small batches: several calls per window, so the window is not one launch

        def batch():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                voc.transform_batch(dd, dc, 4, out=out)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / (n * inner)

        def loop():
            t0 = time.perf_counter()
            for i in range(nl):
                voc.transform(host[i, :counts[i]], 4)
            return (time.perf_counter() - t0) * 1e3 / nl

        def cpu():
            t0 = time.perf_counter()
            for i in range(nl):
                ora.transform(host[i, :counts[i]], 4)
            return (time.perf_counter() - t0) * 1e3 / nl

        def frame():
            t0 = time.perf_counter()
            voc.compute_bow(DF0)
            return (time.perf_counter() - t0) * 1e3

        legs = {"batch": batch, "loop": loop, "cpu": cpu, "frame": frame}
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                ms[k].append(fn())
        frame_ms += ms.pop("frame")
        r = {k + "_per_frame": stats(v) for k, v in ms.items()}
        r["loop_and_cpu_images"] = nl
        r["batch_over_loop"] = round(r["batch_per_frame"]["median_ms"] / r["loop_per_frame"]["median_ms"], 4)
        r["batch_over_cpu"] = round(r["batch_per_frame"]["median_ms"] / r["cpu_per_frame"]["median_ms"], 4)
        r["batch_beats_loop"] = bool(r["batch_per_frame"]["median_ms"] < r["loop_per_frame"]["median_ms"])
        res["sizes"][str(n)] = r
    res["frame_compute_bow_device_view"] = stats(frame_ms)
    voc.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
