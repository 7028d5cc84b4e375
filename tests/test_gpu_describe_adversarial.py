"""GPU parity of k_describe (IC_Angle, 7x7 Gaussian, rBRIEF, patch staging) on planted keypoints,
bit-exact against the CPU oracle, for both instantiations of the kernel: the host call (fewer than
16 images, one slot per wave) and a device batch of 16 images through orbfe_extract_batch (four
slots per wave, the next slot's patch prefetched).

For every image: the stages and outputs test_gpu_fast_adversarial.py checks, then key by key the
angle bits and the descriptor row, so that a failure names the case, the key's (level, x, y) and the
staging class the kernel picks for it. The cases (tests/describe_patterns.py) each come with a CPU
precondition, asserted from the trace of oracle/describe_definition.py before anything runs on the
GPU, that the keys reach the edge the case is named for and that a kernel with the matching mistake
(another border mode, rounding, disc mask, comparison, a missing clamp) would fail the case:

  edge-left / -top / -bottom / -corner / -right-taps   keys 19 and 20 px from an edge: the reflect-101
                             gather, blur taps outside the level; x = 21 and y = h - 22 interior
  edge-right-w0 .. w3        a key on every column w - 33 .. w - 20 for every w mod 4: interior turns into
                             gather where gx0 + 52 > w (batch: pitch padded to 4; a tight pitch that is
                             no multiple of 4 leaves the host call the gather everywhere)
  align-sh0 .. sh3           interior keys of every byte shift; samples on offsets -18 and +18
  angle-axes, -diagonal-tie, -branch-edge, -near-wrap   fastAtan2: zero moments, ax == ay, one unit either
                             side of it in every quadrant, m01 = -1 against the largest m10
  disc-rim                   pixels on umax[v] and umax[v] + 1 of several rows, v = 0 and +-15 included
  saturated-variant1 / -variant0, black-variant1   255 * 257: the column pass reaches 257 and the clamp
  compare-ties, -two-valued  t0 == t1 gives bit 0
  round-half                 sample sums on exact half-integers: round half to even
  offset-18-raised / -lowered   a bit that only the outermost blurred row or column of the 37 x 37 window decides
  wave-mix                   320 x 264, 8 levels of noise: every interior / gather transition between
                             consecutive slots of a wave, a wave across a level boundary, a short last
                             wave, gather keys on four sides and every shift on every level
  empty-level-between        levels 0 and 2 with keys, level 1 without
"""
import ctypes

import numpy as np
import pytest

import describe_patterns as dp
from test_gpu_fast_adversarial import build_ref, check_outputs, check_stages

pytestmark = pytest.mark.gpu

CASES = dp.all_cases()
BATCH = 16
SENTINEL = 0x5A


def check_keys(kp, desc, ref, what, batch):
    """Angle bits and descriptor row of every key against the oracle's, named by level, position and
    staging class."""
    assert len(kp) == len(ref["keys"]), f"{what}: {len(kp)} keypoints vs {len(ref['keys'])}"
    ang = np.ascontiguousarray(kp["angle"]).view(np.uint32)
    for i, k in enumerate(ref["keys"]):
        where = f"{what} key {i} level {k.level} ({k.x}, {k.y}) {k.staging_batch if batch else k.staging_host}"
        assert int(ang[i]) == k.bits, f"{where}: angle bits gpu {int(ang[i]):#x} vs oracle {k.bits:#x} (m10 {k.trace.m10}, m01 {k.trace.m01})"
        bad = np.nonzero(desc[i] != k.desc)[0]
        assert bad.size == 0, f"{where}: descriptor bytes {bad.tolist()} differ, gpu {desc[i][bad].tolist()} vs {k.desc[bad].tolist()}"


@pytest.fixture(scope="module")
def refs(oracle_lib):
    """Oracle reference, definition trace and asserted precondition of every case, once for the module."""
    out = {}
    for c in CASES:
        ref = dp.reference(c, oracle_lib)
        c.pre(c, ref)   # CPU: the keys reach their edge, the switches would change them
        out[c.name] = ref
    return out


def make_extractor(c):
    from orb_slam3_ros_amd.extractor import ORBextractor
    ext = ORBextractor(c.nfeat, c.scale, c.nlevels, c.ini, c.min)
    if c.variant:
        ext.set_opencv_model(blur_variant=c.variant)
    return ext


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_call(case, gpu, refs):
    """One image through the host API: k_describe<1>."""
    ref = refs[case.name]
    ext = make_extractor(case)
    try:
        mono, kp, desc = ext(case.img, None, (0, 0))
        check_stages(ext, 0, ref, case.name)
        check_outputs(mono, kp, desc, ref, case.name)
        check_keys(kp, desc, ref, case.name, batch=False)
    finally:
        ext.close()


# ---- device batches: cases of equal size, parameters and blur taps share one batch of 16 ------------
def _group_key(c):
    return (c.img.shape, c.nfeat, c.nlevels, c.variant, c.batch_pitch)


GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_group_key(_c), []).append(_c)
GROUP_LIST = list(GROUPS.values())


def _filler_ref(oracle_lib, img, c0):
    ref = build_ref(oracle_lib, img, c0.nfeat, c0.scale, c0.nlevels, c0.ini, c0.min)
    if c0.variant:
        ora = oracle_lib.OracleExtractor(c0.nfeat, c0.scale, c0.nlevels, c0.ini, c0.min, blur_variant=c0.variant)
        ref["mono"], ref["kp"], ref["desc"] = ora(img)
        ora.close()
    return ref


def _fillers(cases, count, seed):
    """Distinct images of the group's size to fill the batch: flips of the cases' images (planted keys
    on the opposite edges) and noise."""
    import fast_patterns as fp
    h, w = cases[0].img.shape
    out = []
    for k in range(count):
        src = cases[k % len(cases)].img
        kind = (k // len(cases)) % 4
        img = [src[:, ::-1], src[::-1], src[::-1, ::-1], None][kind]
        out.append(np.ascontiguousarray(img) if img is not None else fp.noise_image(seed + k, w, h))
    return out


@pytest.mark.parametrize("group", GROUP_LIST, ids=lambda g: "+".join(c.name for c in g))
def test_device_batch(group, gpu, refs, oracle_lib):
    """16 images through orbfe_extract_batch: k_describe<4>. The group's cases and fillers of the same
    size sit in seeded shuffled slots of a pitched device buffer; outputs are sentinel-filled; every
    image of the batch is compared."""
    import torch
    c0 = group[0]
    h, w = c0.img.shape
    pitch = c0.batch_pitch
    seed = 9000 + len(c0.name) + w
    imgs = [c.img for c in group]
    ref = [refs[c.name] for c in group]
    for f in _fillers(group, max(BATCH - len(group), 0), seed):
        imgs.append(f)
        ref.append(_filler_ref(oracle_lib, f, c0))
    order = np.random.default_rng(seed).permutation(len(imgs))
    n = len(order)
    assert n >= BATCH
    flat = np.full(n * h * pitch + 256, SENTINEL, np.uint8)      # padding bytes and a tail of foreign bytes
    host = flat[:n * h * pitch].reshape(n, h, pitch)
    for i, u in enumerate(order):
        host[i, :, :w] = imgs[u]
    dev = torch.from_numpy(flat).cuda()
    ext = make_extractor(c0)
    try:
        cap = ext.capacity(w, h)
        kps = torch.full((n, cap, 7), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        desc = torch.full((n, cap, 32), SENTINEL, dtype=torch.uint8, device=gpu)
        cnt = torch.full((n, 2), -1, dtype=torch.int32, device=gpu)
        assert ext._lib.orbfe_set_batch_outputs(ext.handle, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), n) == 0
        ptrs = (ctypes.c_void_p * n)(*[dev.data_ptr() + i * h * pitch for i in range(n)])
        rc = ext._lib.orbfe_extract_batch(ext.handle, n, ptrs, w, h, pitch, 0, 0, None)
        assert rc == 0, f"orbfe_extract_batch refused {n} images of {w}x{h}, pitch {pitch}: {rc}"
        torch.cuda.synchronize()
        cnt_h, kps_h, desc_h = cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
        from oracle.oracle import KEYPOINT_DTYPE
        for i, u in enumerate(order):
            what = f"slot {i} ({group[u].name if u < len(group) else 'filler %d' % (u - len(group))}) of {n}:"
            nk = int(cnt_h[i, 0])
            assert nk == len(ref[u]["kp"]) <= cap, f"{what} {nk} keypoints vs {len(ref[u]['kp'])}"
            check_stages(ext, i, ref[u], what)
            check_outputs(int(cnt_h[i, 1]), kps_h[i, :nk], desc_h[i, :nk], ref[u], what)
            if u < len(group):
                rec = np.ascontiguousarray(kps_h[i, :nk]).view(KEYPOINT_DTYPE).reshape(-1)
                check_keys(rec, desc_h[i, :nk], ref[u], what, batch=True)
    finally:
        ext.close()
    del dev
