"""GPU: an extractor call's answer does not depend on what earlier calls left in the buffers it reuses.

The parity suites run one call at a time on fresh handles, whose hipMalloc memory is usually zero. Here
the scratch is under the test's control: orbfe_debug_fill_extractor writes one 32-bit word over every
buffer the next call has to define for itself (include/orbfe.h lists them), live handles are resized and
their batches shrunk under a larger capacity, and the cached pointer tables are hit with new contents
behind the same pointers. Every result is bit-exact against OracleExtractor on the same image:
keypoints (all 28 bytes), descriptors, monoIndex, the intermediates read back through orbfe_debug_copy,
and uR / depth / l2r bits where a stereo or RGB-D stage follows.

Fill words are 0 and 1 only: read as a count, an index, a node id, a flag or a float, both stay inside
every array, so a stale read gives a wrong answer and never a wild address. Sizes change only across a
reallocation. Geometries: 272 x 264 and 400 x 300, 8 levels at 1.2, 500 features (every buffer size
differs between the two)."""
import ctypes

import numpy as np
import pytest

from oracle import fast_definition as fd
from orb_slam3_ros_amd.synth import synth_image, synth_stereo
from test_gpu_fast_adversarial import check_outputs, check_stages
from test_gpu_rgbd import check_frame, depth_metres, depth_u16, expected, same_bits, tum1

pytestmark = pytest.mark.gpu

SMALL, LARGE = (272, 264), (400, 300)
NFEAT, NLEVELS = 500, 8
BF, FX = 0.110078 * 458.654, 458.654
WORDS = [0, 1]
SMALL_BATCH = 16   # kSmallBatch (orbfe_engine.hip): the launch shapes change at this many images / frames


# ---- references, computed once per module and never modified --------------------------------------
def _ref_of(ora, img, lap):
    mono, kp, desc = ora(img, lap)
    ref = dict(mono=mono, kp=kp.copy(), desc=desc.copy(), nlevels=NLEVELS, pyr=[], cells=[], oct=[])
    for l in range(NLEVELS):
        lv = ora.pyramid_level(l)
        raw = ora.debug_keys(l, 0)
        ref["pyr"].append(lv)
        ref["cells"].append(fd.bin_keys(raw["x"], raw["y"], raw["response"], lv.shape[1], lv.shape[0]))
        ref["oct"].append(ora.debug_keys(l, 1))
    # check_stages also compares level 0 with the Python definition's cells; that check belongs to the FAST
    # suite and is a no-op here: the oracle's own cells stand in for it
    ref["def0"] = ref["cells"][0]
    return ref


class Refs:
    def __init__(self, oracle):
        self.oracle, self.mono, self.pairs = oracle, {}, {}

    def image(self, seed, size, lap=(0, 0), nfeat=NFEAT):
        """(image, reference) of synth_image(seed, *size)."""
        key = (seed, size, lap, nfeat)
        if key not in self.mono:
            img = synth_image(seed, *size)
            ora = self.oracle.OracleExtractor(nfeat, 1.2, NLEVELS, 20, 7)
            self.mono[key] = (img, _ref_of(ora, img, lap))
            ora.close()
        return self.mono[key]

    def pair(self, seed, size, lap=(0, 0), nfeat=NFEAT):
        """synth_stereo(seed, *size): both images, both references, ComputeStereoMatches' (uR, depth,
        nmatch) and the fisheye stage's (l2r, dist, ngood) at ratio 0.7."""
        key = (seed, size, lap, nfeat)
        if key not in self.pairs:
            left, right = synth_stereo(seed, *size)
            ol = self.oracle.OracleExtractor(nfeat, 1.2, NLEVELS, 20, 7)
            orr = self.oracle.OracleExtractor(nfeat, 1.2, NLEVELS, 20, 7)
            rl, rr = _ref_of(ol, left, lap), _ref_of(orr, right, lap)
            ur, dp, nm = self.oracle.stereo_match(ol, orr, rl["kp"], rl["desc"], rr["kp"], rr["desc"], BF, FX)
            ml, mr = rl["mono"], rr["mono"]
            g, t, d = self.oracle.stereo_knn_ratio(rl["desc"][ml:], rr["desc"][mr:], 0.7)
            l2r, dist = np.full(len(rl["kp"]), -1, np.int32), np.full(len(rl["kp"]), -1, np.int32)
            l2r[ml:][t >= 0] = t[t >= 0] + mr
            dist[ml:][t >= 0] = d[t >= 0]
            ol.close()
            orr.close()
            self.pairs[key] = dict(left=left, right=right, rl=rl, rr=rr, ur=ur.copy(), dp=dp.copy(), nm=nm, l2r=l2r,
                                   dist=dist, ngood=g)
        return self.pairs[key]


@pytest.fixture(scope="module")
def refs(oracle_lib):
    return Refs(oracle_lib)


# ---- the calls -----------------------------------------------------------------------------------
def _new_ext(nfeat=NFEAT):
    from orb_slam3_ros_amd.extractor import ORBextractor
    return ORBextractor(nfeat, 1.2, NLEVELS, 20, 7)


@pytest.fixture
def handles(gpu):
    """A factory of extractor handles that are closed when the test ends, however it ends."""
    made = []

    def new(nfeat=NFEAT):
        made.append(_new_ext(nfeat))
        return made[-1]
    yield new
    for e in made:
        e.close()


def _fill(ext, word):
    n = ctypes.c_int64(-1)
    assert ext._lib.orbfe_debug_fill_extractor(ext.handle, word, ctypes.byref(n)) == 0
    assert n.value > 0 and n.value % 4 == 0
    return n.value


def _read(lib, ptr, nbytes):
    """nbytes of device memory at the 16-byte aligned ptr (whole 16-byte items are copied)."""
    import torch
    n16 = (nbytes + 15) // 16 * 16
    dst = torch.zeros(n16, dtype=torch.uint8, device="cuda")
    assert lib.orbfe_copy_stream(ptr, dst.data_ptr(), n16, None) == 0
    torch.cuda.synchronize()
    return dst.cpu().numpy()[:nbytes]


class DeviceImages:
    """Images of one size in one device tensor, with the pointer array of a batch call."""

    def __init__(self, imgs):
        import torch
        self.t = torch.from_numpy(np.stack(imgs)).cuda()
        self.n, (self.h, self.w) = len(imgs), imgs[0].shape

    def ptrs(self, n=None):
        n = self.n if n is None else n
        return (ctypes.c_void_p * n)(*[self.t[i].data_ptr() for i in range(n)])

    def write(self, imgs):
        """New contents behind the same pointers."""
        import torch
        self.t.copy_(torch.from_numpy(np.stack(imgs)))
        torch.cuda.synchronize()


def _extract_batch(ext, dev, n=None, lap=(0, 0)):
    """orbfe_extract_batch into the handle's own output block; [(monoIndex, keypoints, descriptors)]."""
    import torch
    from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
    n = dev.n if n is None else n
    lib = ext._lib
    assert lib.orbfe_extract_batch(ext.handle, n, dev.ptrs(n), dev.w, dev.h, dev.w, lap[0], lap[1], None) == 0
    torch.cuda.synchronize()
    ext._last_shape = (dev.h, dev.w)
    kp, ds, ct, cap = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int()
    assert lib.orbfe_batch_outputs(ext.handle, ctypes.byref(kp), ctypes.byref(ds), ctypes.byref(ct), ctypes.byref(cap)) == 0
    cap = cap.value
    assert cap == ext.capacity(dev.w, dev.h)
    cnt = _read(lib, ct.value, n * 8).view(np.int32).reshape(n, 2)
    kps = _read(lib, kp.value, n * cap * 28).view(KEYPOINT_DTYPE).reshape(n, cap)
    desc = _read(lib, ds.value, n * cap * 32).reshape(n, cap, 32)
    assert (cnt[:, 0] >= 0).all() and (cnt[:, 0] <= cap).all(), cnt.tolist()
    return [(int(cnt[i, 1]), kps[i, :cnt[i, 0]].copy(), desc[i, :cnt[i, 0]].copy()) for i in range(n)]


def _check_batch(ext, got, want, what, stages=None):
    """Outputs of every image; the intermediates of the images in `stages` (default: first and last)."""
    assert len(got) == len(want)
    for i, ((mono, kp, desc), ref) in enumerate(zip(got, want)):
        check_outputs(mono, kp, desc, ref, f"{what} image {i}")
    for i in sorted(set((0, len(got) - 1) if stages is None else stages)):
        check_stages(ext, i, want[i], f"{what} image {i}")


def _stereo_batch(ext, nframes):
    """orbfe_stereo_match_batch over frames (2f, 2f + 1) of the handle's last batch."""
    import torch
    cap = ext.capacity(*ext._last_shape[::-1])
    ur = torch.full((nframes, cap), -777.0, dtype=torch.float32, device="cuda")
    dp = torch.full((nframes, cap), -555.0, dtype=torch.float32, device="cuda")
    nm = torch.full((nframes,), -9, dtype=torch.int32, device="cuda")
    rc = ext._lib.orbfe_stereo_match_batch(ext.handle, 0, 2, ext.handle, 1, 2, nframes, BF, FX, ur.data_ptr(),
                                           dp.data_ptr(), nm.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return ur.cpu().numpy(), dp.cpu().numpy(), nm.cpu().numpy()


def _check_stereo_rows(got, pairs, what):
    ur, dp, nm = got
    for f, p in enumerate(pairs):
        n = len(p["rl"]["kp"])
        same_bits(ur[f, :n], p["ur"], f"{what} frame {f} uR")
        same_bits(dp[f, :n], p["dp"], f"{what} frame {f} depth")
        assert nm[f] == p["nm"], (what, f, nm[f], p["nm"])


def _check_frame_stereo(el, er, p, what):
    from orb_slam3_ros_amd.extractor import frame_stereo
    (ml, kl, dl), (mr, kr, dr), ur, dp, nm = frame_stereo(el, er, p["left"], p["right"], BF, FX)
    check_outputs(ml, kl, dl, p["rl"], what + " left")
    check_outputs(mr, kr, dr, p["rr"], what + " right")
    same_bits(ur, p["ur"], what + " uR")
    same_bits(dp, p["dp"], what + " depth")
    assert nm == p["nm"] and (ur >= 0).sum() > 0.2 * len(kl), (what, nm, p["nm"])


def _rgbd_inputs(kind, seed, size):
    w, h = size
    if kind == "u16":
        return depth_u16(seed, w, h), tum1(w, h)
    return (depth_metres(seed, w, h) * 5208.0).astype(np.float32), tum1(w, h, factor=1.0 / 5208.0)


def _rgbd_batch(ext, base, step, nframes, dptr, dt, pitch, p):
    import torch
    cap = ext.capacity(*ext._last_shape[::-1])
    kun = torch.full((nframes, cap, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ur = torch.full((nframes, cap), -777.0, dtype=torch.float32, device="cuda")
    dp = torch.full((nframes, cap), -555.0, dtype=torch.float32, device="cuda")
    rc = ext._lib.orbfe_rgbd_stereo_batch(ext.handle, base, step, nframes, dptr, dt, pitch, p.ref(), kun.data_ptr(),
                                          ur.data_ptr(), dp.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return kun.cpu().numpy(), ur.cpu().numpy(), dp.cpu().numpy()


def _check_rgbd_rows(oracle, got, want_refs, raws, p, what):
    from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE
    kun, ur, dp = got
    for f, (ref, raw) in enumerate(zip(want_refs, raws)):
        n = len(ref["kp"])
        ekun, eur, edp = expected(oracle, ref["kp"], raw, p)
        same_bits(kun[f, :n].view(KEYPOINT_DTYPE).reshape(n), ekun, f"{what} frame {f} mvKeysUn")
        same_bits(dp[f, :n], edp, f"{what} frame {f} mvDepth")
        same_bits(ur[f, :n], eur, f"{what} frame {f} mvuRight")
        assert (ur[f, n:] == -777.0).all() and (dp[f, n:] == -555.0).all(), (what, f)


# ---- poisoned scratch, every entry -----------------------------------------------------------------
ENTRIES = ["extract", "batch2", "batch16", "frame_stereo", "frame_fisheye", "frame_rgbd_u16", "frame_rgbd_f32",
           "stereo_batch1", "stereo_batch16", "rgbd_batch"]


def _entry_round(entry, ext, er, refs, oracle, k, size, what):
    """One call of `entry` on images chosen by k, compared; image sets of different k share nothing."""
    from orb_slam3_ros_amd.extractor import depth_type_of, frame_fisheye, frame_rgbd
    if entry == "extract":
        img, ref = refs.image(900 + k, size)
        mono, kp, desc = ext(img, None, (0, 0))
        check_outputs(mono, kp, desc, ref, what)
        check_stages(ext, 0, ref, what)
    elif entry in ("batch2", "batch16"):
        n = 2 if entry == "batch2" else SMALL_BATCH
        got = [refs.image(920 + 40 * k + i, size) for i in range(n)]
        dev = DeviceImages([g[0] for g in got])   # alive while level 0 is read back from it
        _check_batch(ext, _extract_batch(ext, dev), [g[1] for g in got], what)
    elif entry == "frame_stereo":
        p = refs.pair(960 + k, size)
        _check_frame_stereo(ext, er, p, what)
        check_stages(ext, 0, p["rl"], what + " left")
        check_stages(ext, 1, p["rr"], what + " right")
    elif entry == "frame_fisheye":
        lap = (60, 200)
        p = refs.pair(960 + k, size, lap)
        (ml, kl, dl), (mr, kr, dr), l2r, dist, ng = frame_fisheye(ext, er, p["left"], p["right"], lap, 0.7)
        check_outputs(ml, kl, dl, p["rl"], what + " left")
        check_outputs(mr, kr, dr, p["rr"], what + " right")
        np.testing.assert_array_equal(l2r, p["l2r"], err_msg=what)
        np.testing.assert_array_equal(dist, p["dist"], err_msg=what)
        assert ng == p["ngood"] > 10, (what, ng, p["ngood"])
        check_stages(ext, 0, p["rl"], what + " left")
        check_stages(ext, 1, p["rr"], what + " right")
    elif entry in ("frame_rgbd_u16", "frame_rgbd_f32"):
        img, ref = refs.image(900 + k, size)
        raw, p = _rgbd_inputs(entry[-3:], 980 + k, size)
        _, eur, edp = check_frame(oracle, frame_rgbd(ext, img, raw, p), (ref["kp"], ref["desc"]), raw, p, what)
        assert (edp > 0).sum() > 0.2 * len(edp) and (edp == -1).sum() > 0
        check_stages(ext, 0, ref, what)
    elif entry in ("stereo_batch1", "stereo_batch16"):
        nf = 1 if entry == "stereo_batch1" else SMALL_BATCH
        pairs = [refs.pair(1000 + 20 * k + f, size) for f in range(nf)]
        dev = DeviceImages([im for p in pairs for im in (p["left"], p["right"])])
        got = _extract_batch(ext, dev)
        _check_batch(ext, got, [r for p in pairs for r in (p["rl"], p["rr"])], what)
        _check_stereo_rows(_stereo_batch(ext, nf), pairs, what)
    elif entry == "rgbd_batch":
        import torch
        got = [refs.image(920 + 40 * k + i, size) for i in range(3)]
        dev = DeviceImages([g[0] for g in got])
        _check_batch(ext, _extract_batch(ext, dev), [g[1] for g in got], what)
        raws = [_rgbd_inputs("u16", 985 + 3 * k + f, size)[0] for f in range(3)]
        p = tum1(*size)
        dd = torch.from_numpy(np.stack(raws)).cuda()
        dptr = (ctypes.c_void_p * 3)(*[dd[f].data_ptr() for f in range(3)])
        out = _rgbd_batch(ext, 0, 1, 3, dptr, depth_type_of(raws[0]), size[0] * 2, p)
        _check_rgbd_rows(oracle, out, [g[1] for g in got], raws, p, what)
    else:
        raise AssertionError(entry)


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_poisoned_scratch(gpu, oracle_lib, refs, handles, entry, word):
    """Run once to allocate, fill every scratch buffer with `word`, run on different images, compare the
    outputs and the intermediates; then once more after a second fill with the first images."""
    ext, er = handles(), handles()
    _entry_round(entry, ext, er, refs, oracle_lib, 0, SMALL, f"{entry} before the fill")
    for k in (1, 0):
        nbytes = _fill(ext, word)
        print(f"{entry} word {word}: orbfe_debug_fill_extractor filled {nbytes} bytes")
        _entry_round(entry, ext, er, refs, oracle_lib, k, SMALL, f"{entry} after a fill with {word}, images {k}")


def test_fill_is_seen_and_overwritten(gpu, oracle_lib, refs, handles):
    """Non-vacuity: after a fill with 1 the per-cell counts read back as 1 everywhere (the hook reaches the
    buffers the kernels use), and after the next extraction they are the oracle's."""
    ext = handles()
    img, ref = refs.image(900, LARGE)
    ext(img, None, (0, 0))
    assert _fill(ext, 1) > 0
    total = 0
    for l in range(NLEVELS):
        ncell = len(ref["cells"][l][0])
        cnt = np.zeros(ncell, np.int32)
        assert ext._lib.orbfe_debug_copy(ext.handle, 0, 0, l, cnt.ctypes.data, cnt.nbytes) == ncell
        assert (cnt == 1).all(), (l, cnt.tolist())
        total += ncell
    assert total > NLEVELS
    img2, ref2 = refs.image(901, LARGE)
    mono, kp, desc = ext(img2, None, (0, 0))
    check_outputs(mono, kp, desc, ref2, "after the fill")
    check_stages(ext, 0, ref2, "after the fill")
    assert any((ref2["cells"][l][0] != 1).any() for l in range(NLEVELS))


# ---- sizes and batches changing on a live handle -------------------------------------------------
def test_resize_on_a_live_handle(gpu, oracle_lib, refs, handles):
    """272x264 -> 400x300 -> 272x264 (each a reallocation), 400x300 at batch 16, a batch of 2 under that
    capacity, then orbfe_extract and orbfe_frame_rgbd of one image on the same handle (their read-back
    branch for a handle sized for a larger batch); the pyramid getter after the last."""
    from orb_slam3_ros_amd.extractor import frame_rgbd
    ext = handles()
    seeds = iter(range(1100, 1200))

    def one(size, what):
        img, ref = refs.image(next(seeds), size)
        mono, kp, desc = ext(img, None, (0, 0))
        check_outputs(mono, kp, desc, ref, what)
        check_stages(ext, 0, ref, what)

    def batch(n, size, what):
        got = [refs.image(next(seeds), size) for _ in range(n)]
        dev = DeviceImages([g[0] for g in got])   # alive while level 0 is read back from it
        _check_batch(ext, _extract_batch(ext, dev), [g[1] for g in got], what)

    one(SMALL, "first size")
    one(LARGE, "grown")
    one(SMALL, "shrunk")
    batch(SMALL_BATCH, LARGE, "batch of 16")
    batch(2, LARGE, "batch of 2 under a capacity of 16")
    one(LARGE, "orbfe_extract under a capacity of 16")
    img, ref = refs.image(next(seeds), LARGE)
    for kind in ("u16", "f32"):
        raw, p = _rgbd_inputs(kind, 1190, LARGE)
        check_frame(oracle_lib, frame_rgbd(ext, img, raw, p), (ref["kp"], ref["desc"]), raw, p,
                    f"orbfe_frame_rgbd {kind} under a capacity of 16")
    check_stages(ext, 0, ref, "after orbfe_frame_rgbd")
    for l in range(NLEVELS):
        assert np.array_equal(ext.pyramid_level(l), ref["pyr"][l]), f"orbfe_pyramid_level {l}"


@pytest.mark.parametrize("nfeat", [500, 1200])
def test_stereo_pair_resize(gpu, oracle_lib, refs, handles, nfeat):
    """Two handles through orbfe_frame_stereo at 272x264, 400x300 and 272x264 again, with the two-call host
    form (orbfe_extract twice + orbfe_stereo_match) on the same handles at every size: the stereo result
    and SAD-distance buffers regrow with the keypoint capacity, which the feature budget and the size set."""
    from orb_slam3_ros_amd.extractor import compute_stereo_matches
    el, er = handles(nfeat), handles(nfeat)
    caps = []
    for k, size in enumerate((SMALL, LARGE, SMALL)):
        caps.append(el.capacity(*size))
        p = refs.pair(1200 + k, size, nfeat=nfeat)
        _check_frame_stereo(el, er, p, f"frame_stereo {size} nfeatures {nfeat}")
        q = refs.pair(1210 + k, size, nfeat=nfeat)
        ml, kl, dl = el(q["left"], None, (0, 0))
        mr, kr, dr = er(q["right"], None, (0, 0))
        check_outputs(ml, kl, dl, q["rl"], "host left")
        check_outputs(mr, kr, dr, q["rr"], "host right")
        ur, dp, nm = compute_stereo_matches(el, er, BF, FX, len(kl))
        same_bits(ur, q["ur"], f"orbfe_stereo_match {size} uR")
        same_bits(dp, q["dp"], f"orbfe_stereo_match {size} depth")
        assert nm == q["nm"]
    print(f"nfeatures {nfeat}: keypoint capacities {caps}")


# ---- the cached pointer tables ---------------------------------------------------------------------
def test_image_pointer_cache(gpu, oracle_lib, refs, handles):
    """The image-pointer / lapping-area table is uploaded only when it differs from the last call's: the
    same pointers with new pixels, the same pointers with another lapping area, and a batch of 2 that is
    a prefix of the batch of 3 before it all give the new answer."""
    ext = handles()
    a = [refs.image(1300 + i, SMALL) for i in range(3)]
    b = [refs.image(1310 + i, SMALL) for i in range(3)]
    dev = DeviceImages([g[0] for g in a])
    _check_batch(ext, _extract_batch(ext, dev), [g[1] for g in a], "first contents", stages=(0, 1, 2))
    dev.write([g[0] for g in b])
    _check_batch(ext, _extract_batch(ext, dev), [g[1] for g in b], "new contents, same pointers", stages=(0, 1, 2))
    lap = (60, 200)
    c = [refs.image(1310 + i, SMALL, lap) for i in range(3)]
    assert any(x[1]["mono"] != len(x[1]["kp"]) for x in c)
    _check_batch(ext, _extract_batch(ext, dev, lap=lap), [g[1] for g in c], "new lapping area, same pointers")
    _check_batch(ext, _extract_batch(ext, dev, n=2, lap=lap), [g[1] for g in c[:2]], "a prefix of the same pointers")
    _check_batch(ext, _extract_batch(ext, dev, n=3), [g[1] for g in b], "back to three images")


def test_depth_pointer_cache(gpu, oracle_lib, refs, handles):
    """orbfe_rgbd_stereo_batch caches its depth pointer table in the same way: new depth values behind the
    same pointers, then fewer frames from the same pointers."""
    import torch
    from orb_slam3_ros_amd.extractor import depth_type_of
    ext = handles()
    got = [refs.image(1320 + i, SMALL) for i in range(3)]
    want = [g[1] for g in got]
    dev = DeviceImages([g[0] for g in got])
    _check_batch(ext, _extract_batch(ext, dev), want, "extraction")
    p = tum1(*SMALL)
    raws = [depth_u16(1330 + f, *SMALL) for f in range(3)]
    dd = torch.from_numpy(np.stack(raws)).cuda()
    dptr = (ctypes.c_void_p * 3)(*[dd[f].data_ptr() for f in range(3)])
    dt, pitch = depth_type_of(raws[0]), SMALL[0] * 2
    _check_rgbd_rows(oracle_lib, _rgbd_batch(ext, 0, 1, 3, dptr, dt, pitch, p), want, raws, p, "first depth")
    raws2 = [depth_u16(1340 + f, *SMALL) for f in range(3)]
    dd.copy_(torch.from_numpy(np.stack(raws2)))
    torch.cuda.synchronize()
    _check_rgbd_rows(oracle_lib, _rgbd_batch(ext, 0, 1, 3, dptr, dt, pitch, p), want, raws2, p, "new depth, same pointers")
    _check_rgbd_rows(oracle_lib, _rgbd_batch(ext, 0, 1, 2, dptr, dt, pitch, p), want[:2], raws2[:2], p, "two frames")
    _check_rgbd_rows(oracle_lib, _rgbd_batch(ext, 0, 1, 1, dptr, dt, pitch, p), want[:1], raws2[:1], p, "one frame")
    _check_rgbd_rows(oracle_lib, _rgbd_batch(ext, 0, 1, 3, dptr, dt, pitch, p), want, raws2, p, "three frames again")
