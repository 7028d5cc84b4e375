"""SearchByBoW(pKF, F) for (frame, keyframe) jobs over device-resident frames: 16 distinct keyframes of 1,000
features and 16 frames that are their perturbed views, on a synthetic k = 10, L = 6 vocabulary (FeatureVectors
at levelsup 4). The frames are planted into device slabs of 512 images (each 32 times) and their FeatureVectors
are made where they stay, by orbfe_vocabulary_transform_batch.

Shapes: 1, 32 and 512 jobs with one reference keyframe per frame (TrackReferenceKeyFrame), and 32 frames x 5
candidate keyframes (Relocalization's first loop). Legs (wall time of synchronous calls, host clock; every call
returns complete results):
  slabs   one orbfe_search_by_bow_slabs call on the slabs and the BowBatch rows
  route   today's route per job: the frame's count, keypoints and descriptors and its FeatureVector copied to
          the host, then orbfe_search_by_bow with the keyframe's host arrays
  single  orbfe_search_by_bow per job on host copies made in advance (the route without its downloads)
  batch1  orbfe_search_by_bow_batch per job, one candidate per call, the frame a host copy made in advance
  cpu     the oracle's search_by_bow per job on one CPU thread
The legs alternate inside every repetition; every row of the slabs call is compared with the oracle before any
timing. The JSON keeps median, p10, p90 and min of each leg, per-job times, the kernel time of the slabs call
(device events, orbfe_matcher_set_timing), its per-form job counts, and the same call with its LDS request
untouched but every keyframe padded past it (all jobs in the HBM form).

  python tools/bow_slabs_timing.py [--reps 30] [--out profiles/bow_slabs.json]
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
from orb_slam3_ros_amd.matcher import BowJob, CFeatureVector, FeatureVector, KeyFrameFeatures, MatchFrame
from orb_slam3_ros_amd.vocabulary import L1_NORM, TF_IDF, BowBatch, ORBVocabulary, synth_vocabulary

NFEAT, NNRATIO, CAP, UNIQUE, NIMG, CANDS = 1000, 0.7, 1024, 16, 512, 5
SHAPES = (("ref_J1", 1, 1), ("ref_J32", 32, 1), ("ref_J512", 512, 1), ("reloc_32x5", 32, CANDS))
W, H = 752, 480
SF = sm.scale_factors(8)
BOUNDS = (0.0, float(W), 0.0, float(H))


def stats(ms, jobs):
    a = np.asarray(ms)
    med = float(np.median(a))
    return {"median_ms": round(med, 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size),
            "per_job_us": round(med * 1e3 / jobs, 3)}


def pad_keyframe(K, fv, mp, add, rng):
    """K + add features in no node, without map point: inert, but the pack no longer fits a workgroup's LDS."""
    X = sm.synth_frame(rng, add, W, H, 8, False)
    return (MatchFrame(np.concatenate([K.keys, X.keys]), np.concatenate([K.desc, X.desc]), BOUNDS, SF), fv,
            np.concatenate([mp, np.full(add, -1, np.int32)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "bow_slabs.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bow_slabs_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    oracle.build()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(2026)
    par, leaf, vdesc, vw = synth_vocabulary(rng, 10, 6)
    voc = ORBVocabulary.from_arrays(10, 6, L1_NORM, TF_IDF, par, leaf, vdesc, vw)
    leaves = np.nonzero(leaf)[0]

    # the distinct keyframes and frames; a keyframe's FeatureVector by the single-frame transform
    kfs, frames = [], []
    for u in range(UNIQUE):
        K = sm.synth_frame(rng, NFEAT, W, H, 8, False)
        K = MatchFrame(K.keys, sm.flip_bits(rng, vdesc[rng.choice(leaves, NFEAT)], 0.03), BOUNDS, SF)
        F, _ = sm.perturbed_frame(rng, K, rot=20.0, flip_p=0.03, drop=0.15)
        mp = np.where(rng.random(NFEAT) < 0.2, -1, np.arange(NFEAT) + 1000 * (u + 1)).astype(np.int32)
        kfs.append((K, voc.transform(K.desc, 4)[1], mp))
        frames.append(MatchFrame(F.keys, F.desc, BOUNDS, SF))
    kps = np.zeros((NIMG, CAP, 7), np.int32)
    desc = np.zeros((NIMG, CAP, 32), np.uint8)
    counts = np.zeros((NIMG, 2), np.int32)
    for f in range(NIMG):
        F = frames[f % UNIQUE]
        kps[f, :F.N] = F.keys.view(np.int32).reshape(F.N, 7)
        desc[f, :F.N] = F.desc
        counts[f] = (F.N, 0)
    d_kps, d_desc, d_counts = (torch.from_numpy(a).to(dev) for a in (kps, desc, counts))
    bows = voc.transform_batch(d_desc, d_counts, 4, out=BowBatch(NIMG, CAP, dev))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    f_fvs = [bows.host(u)[1] for u in range(UNIQUE)]
    handles = [KeyFrameFeatures(K, fv) for K, fv, _ in kfs]
    big = [pad_keyframe(K, fv, mp, 4096, rng) for K, fv, mp in kfs]
    big_handles = [KeyFrameFeatures(K, fv) for K, fv, _ in big]

    def job_list(nf, nc):
        """(frame, keyframe) per job: the frame's own keyframe first, then its neighbours."""
        return [(f, (f + c) % UNIQUE) for f in range(nf) for c in range(nc)]

    def job_array(pairs, hs, src):
        arr = (BowJob * len(pairs))()
        for j, (f, u) in enumerate(pairs):
            arr[j].frame, arr[j].kf, arr[j].kf_mp = f, hs[u].handle, src[u][2].ctypes.data
        return arr

    rows = np.zeros((NIMG * CANDS, CAP), np.int32)
    nm, nk = np.zeros(NIMG * CANDS, np.int32), np.zeros(NIMG * CANDS, np.int32)
    forms = np.zeros(4, np.int32)

    def slabs(arr, J, nf):
        rc = lib.orbfe_search_by_bow_slabs(d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), CAP, 0, 1, bows.ref(),
                                           arr, J, nf, NNRATIO, 1, rows.ctypes.data, nm.ctypes.data, nk.ctypes.data, stream)
        assert rc == _lib.ORBFE_OK, rc

    out1 = np.zeros(CAP, np.int32)
    nm1 = np.zeros(1, np.int32)

    def single(F, fv, u):
        K, kfv, mp = kfs[u]
        n = lib.orbfe_search_by_bow(K.keys.ctypes.data, K.desc.ctypes.data, mp.ctypes.data, K.N, kfv.ref(), F.ref(),
                                    fv.ref(), out1.ctypes.data, NNRATIO, 1)
        assert n >= 0, n
        return n

    def route(f, u):
        """The frame and its FeatureVector from the device to the host, then the single call."""
        n = int(d_counts[f, 0].cpu())
        kp = d_kps[f, :n].cpu().numpy().view(KEYPOINT_DTYPE).reshape(n)
        d = d_desc[f, :n].cpu().numpy()
        nfv = int(bows.counts[f, 1].cpu())
        fv = object.__new__(FeatureVector)   # the downloaded arrays as they are, no dictionary in between
        fv.node_ids = bows.fv_node_ids[f, :nfv].cpu().numpy().view(np.uint32)
        fv.offsets = bows.fv_offsets[f, :nfv + 1].cpu().numpy()
        fv.indices = bows.fv_indices[f, :max(int(fv.offsets[nfv]), 1)].cpu().numpy().view(np.uint32)
        fv.c = CFeatureVector(nfv, fv.node_ids.ctypes.data, fv.offsets.ctypes.data, fv.indices.ctypes.data)
        return single(MatchFrame(kp, d, BOUNDS, SF), fv, u)

    one_h, one_mp = (ctypes.c_void_p * 1)(), (ctypes.c_void_p * 1)()

    def batch1(f, u):
        one_h[0], one_mp[0] = handles[u].handle, kfs[u][2].ctypes.data
        rc = lib.orbfe_search_by_bow_batch(one_h, one_mp, 1, frames[f % UNIQUE].ref(), f_fvs[f % UNIQUE].ref(),
                                           out1.ctypes.data, nm1.ctypes.data, NNRATIO, 1)
        assert rc == _lib.ORBFE_OK, rc

    om = oracle.OracleMatcher(NNRATIO, True)

    def cpu(f, u):
        K, kfv, mp = kfs[u]
        return om.search_by_bow(K.keys, K.desc, mp, kfv, frames[f % UNIQUE], f_fvs[f % UNIQUE])

    # parity before timing: every row of the largest calls, plain and padded keyframes, equals the oracle
    exp = {(f, u): cpu(f, u) for f in range(UNIQUE) for u in range(UNIQUE) if (u - f) % UNIQUE < CANDS}
    matches = []
    for name, nf, nc in SHAPES[2:]:
        pairs = job_list(nf, nc)
        for hs, src, col in ((handles, kfs, 0), (big_handles, big, 2)):
            slabs(job_array(pairs, hs, src), len(pairs), nf)
            assert lib.orbfe_matcher_last_bow_slabs(forms.ctypes.data) == _lib.ORBFE_OK
            assert forms[col] == len(pairs) and forms.sum() == len(pairs), forms
            for j, (f, u) in enumerate(pairs):
                n, s = exp[(f % UNIQUE, u)]
                N = frames[f % UNIQUE].N
                assert nm[j] == n and nk[j] == N and np.array_equal(rows[j, :N], s) and (rows[j, N:] == -1).all(), \
                    "the slabs call differs from the oracle"
                matches.append(int(n))
    assert route(3, 3) == exp[(3, 3)][0] and single(frames[3], f_fvs[3], 3) == exp[(3, 3)][0]

    res = {"command": "python tools/bow_slabs_timing.py --reps %d --warmup %d" % (args.reps, args.warmup),
           "workload": {"frame_features": NFEAT, "keyframe_features": NFEAT, "vocabulary": "synthetic k=10 L=6",
                        "levelsup": 4, "nnratio": NNRATIO, "check_orientation": True, "cap": CAP,
                        "distinct_frames": UNIQUE, "distinct_keyframes": UNIQUE,
                        "frame_nodes_mean": round(float(np.mean([len(v.node_ids) for v in f_fvs])), 1),
                        "matches_per_job_mean": round(float(np.mean(matches)), 1)},
           "method": "host clock around synchronous calls through ctypes (slabs, single, batch1: arguments built in "
                     "advance; route: torch device-to-host copies of the frame and its FeatureVector, then the single "
                     "call), legs alternating per repetition, every row of the slabs call compared with the oracle "
                     "first; cpu = the oracle on one thread",
           "parity_on_every_row": True, "warmup": args.warmup, "shapes": {}}
    for name, nf, nc in SHAPES:
        pairs = job_list(nf, nc)
        J = len(pairs)
        arr, arr_big = job_array(pairs, handles, kfs), job_array(pairs, big_handles, big)
        legs = {
            "slabs": lambda: slabs(arr, J, nf),
            "route": lambda: [route(f, u) for f, u in pairs],
            "single": lambda: [single(frames[f % UNIQUE], f_fvs[f % UNIQUE], u) for f, u in pairs],
            "batch1": lambda: [batch1(f, u) for f, u in pairs],
            "cpu": lambda: [cpu(f, u) for f, u in pairs],
            "slabs_all_hbm_form": lambda: slabs(arr_big, J, nf),
        }
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
        kern = {"slabs": [], "slabs_all_hbm_form": []}
        counted = {}
        for _ in range(30):
            for k in kern:
                legs[k]()
                kern[k].append(float(lib.orbfe_matcher_last_ms()))
                lib.orbfe_matcher_last_bow_slabs(forms.ctypes.data)
                counted[k] = {"lds_form": int(forms[0]), "empty": int(forms[1]), "hbm_form": int(forms[2]),
                              "refused": int(forms[3])}
        lib.orbfe_matcher_set_timing(0)
        sh = {"jobs": J, "frames": nf, "candidates_per_frame": nc, "legs": {k: stats(v, J) for k, v in ms.items()},
              "kernel_ms_device_events": {k: stats(v, J) for k, v in kern.items()}, "forms": counted}
        per = {k: sh["legs"][k]["per_job_us"] for k in legs}
        sh["per_job_us"] = per
        sh["route_over_slabs"] = round(per["route"] / per["slabs"], 3)
        sh["single_over_slabs"] = round(per["single"] / per["slabs"], 3)
        sh["batch1_over_slabs"] = round(per["batch1"] / per["slabs"], 3)
        sh["cpu_over_slabs"] = round(per["cpu"] / per["slabs"], 3)
        res["shapes"][name] = sh
    for name in ("ref_J32", "ref_J512"):
        per = res["shapes"][name]["per_job_us"]
        res[f"slabs_is_faster_per_job_than_the_loop_of_single_calls_{name}"] = bool(per["slabs"] < per["single"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
