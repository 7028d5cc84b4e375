"""The RGB-D frame call (Frame::Frame(imGray, imDepth, ...), Frame.cc:222-237) at the TUM shape: 640x480,
1000 features, 8 levels, u16 depth with factor 1/5000, TUM1 intrinsics and distortion.

Legs (wall time of the synchronous calls, host clock; every call returns complete results):
  a  orbfe_frame_rgbd (extraction + UndistortKeyPoints + ComputeStereoFromRGBD, raw depth in)
  b  orbfe_extract alone on the same image (the base: a - b is the cost of the feature)
  c  the CPU path: the oracle's extraction, a whole-image numpy conversion (GrabImageRGBD's convertTo),
     the depth look-ups and oracle.undistort_points
  d  the two depth-staging variants of orbfe_frame_rgbd, from a diagnostic build of the library
     (tools/build_variant.sh abknobs -DORBFE_AB_KNOBS=1, given with --variant-lib): d_dma copies the
     depth image to the device on a second stream beside the extraction (the product's path), d_mapped
     has k_rgbd read it in mapped pinned memory in place (ORBFE_RGBD_MAPPED=1 when the handle is created)
The legs alternate inside every repetition and parity of a / d with the oracle is checked before any
timing. The JSON keeps median, p10, p90 and min of each leg, a - b, a / c, the device-event split of
leg a (upload, extraction kernels, RGB-D kernel, result pull) and the host's copy of the depth image
into pinned memory timed alone.

  python tools/rgbd_timing.py [--reps 200] [--out profiles/rgbd_frame.json] [--variant-lib PATH]
  python tools/rgbd_timing.py --table-from profiles/rgbd_frame.json --design DESIGN.md   (no GPU needed)
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

W, H, NFEAT, NLEVELS = 640, 480, 1000, 8
TUM1 = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, dist=[0.262383, -0.953104, -0.005358, 0.002628, 1.163314],
            bf=40.0, factor=1.0 / 5000.0)
BEGIN, END = "<!-- rgbd-timing:begin -->", "<!-- rgbd-timing:end -->"


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5), "min_ms": round(float(a.min()), 5), "n": int(a.size)}


def table(res):
    rows = [("(a) `orbfe_frame_rgbd`", "a_frame_rgbd"), ("(b) `orbfe_extract` alone", "b_extract"),
            ("(c) CPU path (oracle + numpy)", "c_cpu"), ("(d) depth read in mapped pinned memory", "d_mapped"),
            ("(d) depth by DMA beside the extraction", "d_dma")]
    out = ["| leg | median ms | p10 - p90 ms |", "|---|---|---|"]
    for name, key in rows:
        if key in res["legs"]:
            s = res["legs"][key]
            out.append(f"| {name} | {s['median_ms']:.4f} | {s['p10_ms']:.4f} - {s['p90_ms']:.4f} |")
    out.append("")
    out.append(f"(a) - (b) = {res['a_minus_b_ms']:.4f} ms; (a) / (c) = {res['a_over_c']:.4f}. Device events of (a), "
               f"median ms: upload {res['a_device_events_ms']['upload']:.4f}, extraction kernels "
               f"{res['a_device_events_ms']['extract_kernels']:.4f}, `k_rgbd` {res['a_device_events_ms']['k_rgbd']:.4f}, "
               f"result pull {res['a_device_events_ms']['pull']:.4f}; the host's depth copy into pinned memory alone: "
               f"{res['host_depth_copy_ms']['median_ms']:.4f} ms.")
    return "\n".join(out)


def write_table(res, design):
    s = open(design).read()
    if BEGIN not in s or END not in s:
        sys.exit(f"{design}: markers {BEGIN} / {END} not found")
    head, rest = s.split(BEGIN, 1)
    _, tail = rest.split(END, 1)
    with open(design, "w") as f:
        f.write(head + BEGIN + "\n" + table(res) + "\n" + END + tail)


class Handle:
    """One extractor handle of a given build of the library, through the raw C-ABI."""

    def __init__(self, lib):
        from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
        self.lib, self.h = lib, ctypes.c_void_p()
        assert lib.orbfe_extractor_create(NFEAT, 1.2, NLEVELS, 20, 7, ctypes.byref(self.h)) == 0
        self.cap = lib.orbfe_extractor_capacity(self.h, W, H)
        self.kps, self.kun = np.zeros(self.cap, KEYPOINT_DTYPE), np.zeros(self.cap, KEYPOINT_DTYPE)
        self.desc = np.zeros((self.cap, 32), np.uint8)
        self.ur, self.dp = np.zeros(self.cap, np.float32), np.zeros(self.cap, np.float32)
        self.n = ctypes.c_int()

    def frame_rgbd(self, img, raw, p):
        rc = self.lib.orbfe_frame_rgbd(self.h, img.ctypes.data, W, H, W, raw.ctypes.data, 0, 2 * W, p.ref(),
                                       self.kps.ctypes.data, self.kun.ctypes.data, self.desc.ctypes.data, self.cap,
                                       ctypes.byref(self.n), self.ur.ctypes.data, self.dp.ctypes.data)
        assert rc >= 0, rc
        return self.n.value

    def extract(self, img):
        rc = self.lib.orbfe_extract(self.h, img.ctypes.data, W, H, W, 0, 0, self.kps.ctypes.data, self.desc.ctypes.data,
                                    self.cap, ctypes.byref(self.n))
        assert rc >= 0, rc
        return self.n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "rgbd_frame.json"))
    ap.add_argument("--variant-lib", default=None, help="a -DORBFE_AB_KNOBS=1 build of liborbfe.so for the (d) legs")
    ap.add_argument("--table-from", default=None, help="only rewrite the DESIGN table from this JSON")
    ap.add_argument("--design", default=None, help="DESIGN.md, whose rgbd-timing block is rewritten")
    args = ap.parse_args()
    if args.table_from:
        write_table(json.load(open(args.table_from)), args.design or "DESIGN.md")
        return
    if args.reps < 50:
        ap.error("--reps must be at least 50")
    import torch
    if not torch.cuda.is_available():
        sys.exit("rgbd_timing: no HIP device (this is a GPU measurement; there is no fallback)")
    from oracle import oracle
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd.extractor import RGBDParams
    from orb_slam3_ros_amd.synth import _value_noise, synth_image
    oracle.build()
    lib = _lib.load()
    img = synth_image(81, W, H)
    rng = np.random.default_rng(520)
    metres = 0.5 + 4.0 * _value_noise(rng, H, W, 24)
    metres[100:220, 300:460] = 0.0   # a hole without depth
    raw = np.ascontiguousarray(np.rint(metres * 5000.0).astype(np.uint16))   # (the noise comes column-major)
    p = RGBDParams(TUM1["fx"], TUM1["fy"], TUM1["cx"], TUM1["cy"], TUM1["dist"], TUM1["bf"], TUM1["factor"])
    oext = oracle.OracleExtractor(NFEAT, 1.2, NLEVELS, 20, 7)

    def leg_c():
        _, k, d = oext(img)
        conv = raw.astype(np.float32) * np.float32(p.depth_factor)   # GrabImageRGBD: the whole image
        dv = conv[k["y"].astype(np.int32), k["x"].astype(np.int32)]
        u = oracle.undistort_points(np.stack([k["x"], k["y"]], 1), p.K4, p.dist)
        ok = dv > 0
        with np.errstate(divide="ignore"):
            ur = np.where(ok, u[:, 0] - np.float32(p.bf) / dv, np.float32(-1)).astype(np.float32)
        return k, d, u, ur, np.where(ok, dv, np.float32(-1)).astype(np.float32)

    ha, hb = Handle(lib), Handle(lib)
    legs = {"a_frame_rgbd": lambda: ha.frame_rgbd(img, raw, p), "b_extract": lambda: hb.extract(img), "c_cpu": leg_c}
    checked = [("a_frame_rgbd", ha)]
    if args.variant_lib:
        vlib = _lib.load(args.variant_lib)
        os.environ.pop("ORBFE_RGBD_MAPPED", None)
        hd = Handle(vlib)
        os.environ["ORBFE_RGBD_MAPPED"] = "1"   # read when the handle is created (diagnostic builds only)
        hm = Handle(vlib)
        os.environ.pop("ORBFE_RGBD_MAPPED", None)
        legs["d_mapped"] = lambda: hm.frame_rgbd(img, raw, p)
        legs["d_dma"] = lambda: hd.frame_rgbd(img, raw, p)
        checked += [("d_mapped", hm), ("d_dma", hd)]
    # parity before timing: every GPU leg equals the CPU path bit for bit
    k, d, u, ur, dp = leg_c()
    for name, hx in checked:
        n = hx.frame_rgbd(img, raw, p)
        assert n == len(k), f"{name}: {n} keypoints, the oracle has {len(k)}"
        pairs = {"mvKeys": (hx.kps[:n].view(np.uint8).reshape(n, -1), k.view(np.uint8).reshape(n, -1)),
                 "mDescriptors": (hx.desc[:n], d),
                 "mvKeysUn": (np.stack([hx.kun["x"][:n], hx.kun["y"][:n]], 1).view(np.uint32), u.view(np.uint32)),
                 "mvuRight": (hx.ur[:n].view(np.uint32), ur.view(np.uint32)),
                 "mvDepth": (hx.dp[:n].view(np.uint32), dp.view(np.uint32))}
        bad = {w: int((np.asarray(g) != np.asarray(e)).reshape(n, -1).any(1).sum()) for w, (g, e) in pairs.items()}
        assert not any(bad.values()), f"{name}: rows differing from the CPU path: {bad}"
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
    ms = {key: [] for key in legs}
    # alternating: drift on the shared host hits every leg alike. The GPU legs rotate their order every
    # repetition and the CPU leg comes last: the first GPU call after its 14 ms of idle device is slower
    # by several microseconds, and a fixed order would charge that to one leg.
    gpu_legs = [key for key in legs if key != "c_cpu"]
    for r in range(args.reps):
        order = gpu_legs[r % len(gpu_legs):] + gpu_legs[:r % len(gpu_legs)] + ["c_cpu"]
        for key in order:
            t0 = time.perf_counter()
            legs[key]()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    # the device-event split of leg a, and the host's depth copy alone (into a page-locked tensor)
    lib.orbfe_set_stage_timing(ha.h, 1)
    ev = []
    for _ in range(50):
        ha.frame_rgbd(img, raw, p)
        t = np.zeros(5, np.float32)
        lib.orbfe_get_call_timing(ha.h, t.ctypes.data)
        ev.append(t.copy())
    lib.orbfe_set_stage_timing(ha.h, 0)
    ev = np.median(np.stack(ev), 0)
    pinned = torch.empty((H, 2 * W), dtype=torch.uint8).pin_memory().numpy().view(np.uint16)
    cp = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        np.copyto(pinned, raw)
        cp.append((time.perf_counter() - t0) * 1e3)
    res = {"workload": {"width": W, "height": H, "nfeatures": NFEAT, "nlevels": NLEVELS, "depth": "u16",
                        "depth_factor": "1/5000", "camera": "TUM1", "keypoints": int(len(k)),
                        "with_depth": int((dp > 0).sum())},
           "method": "host clock around synchronous C-ABI calls, legs alternating per repetition (GPU legs in rotating "
                     "order, the CPU leg last), parity with the oracle checked first",
           "warmup": args.warmup, "legs": {key: stats(v) for key, v in ms.items()},
           "a_device_events_ms": {"upload": round(float(ev[0]), 5), "extract_kernels": round(float(ev[1]), 5),
                                  "k_rgbd": round(float(ev[3]), 5), "pull": round(float(ev[2]), 5)},
           "host_depth_copy_ms": stats(cp)}
    a, b, c = (res["legs"][key]["median_ms"] for key in ("a_frame_rgbd", "b_extract", "c_cpu"))
    res["a_minus_b_ms"] = round(a - b, 5)
    res["a_over_c"] = round(a / c, 5)
    if args.variant_lib:
        res["d_mapped_minus_dma_ms"] = round(res["legs"]["d_mapped"]["median_ms"] - res["legs"]["d_dma"]["median_ms"], 5)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if args.design:
        write_table(res, args.design)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
