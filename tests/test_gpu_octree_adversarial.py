"""GPU parity of DistributeOctTree (k_octree) on adversarial key sets, bit-exact against the CPU
oracle, for both instantiations of the kernel: the host call (fewer than 16 images, k_octree<1024>)
and a device batch of 16 images through orbfe_extract_batch (k_octree<256>).

For every image and level: the octree keys including the score byte, in list order; the four
level-info words (nodes, lapping, non-lapping, keys), the lapping split computed in numpy from the
oracle's keys; then the stages and outputs test_gpu_fast_adversarial.py checks (pyramid, per-cell
FAST lists, monoIndex, keypoints, descriptors). The cases (tests/octree_patterns.py) each come with
a CPU precondition, asserted from the trace of oracle/octree_definition.py before anything runs on
the GPU, that the key set reaches the branch it is named for (NT = the instance's thread count):

  p1-generic-256 / -1024     phase-1 step with n > NT that divides nodes (and the fused one before it);
                             all keys returned; the stall on a list of single-key nodes
  p2-generic-n-256 / -1024   phase-2 step with n > NT, m <= NT after a fused one whose walk runs to
                             t = m without reaching N; the break falls inside a (size, UL.x) tie group
  p2-generic-m-256 / -1024   phase-2 step with m > NT
  keys-global-host           K > 8192: the host instance keeps keys in the global lists, scanned roots
  keys-registers-full        K just below 8192: every register slot group in use
  k-1, k-below-n, k-equals-n, k-0-on-level-1   K = 1, K < N (all returned), K = N, an empty level
  stall-cluster              n == prevN with n < N: a cluster that stays in one child
  break-at-0, break-in-tie, p1-reach-n   the walk breaks at its first node; inside a tie group (the
                             answer depends on std::sort's tie order); n >= N after a phase-1 round
  score-tie-cells, score-tie-binary-noise   equal maximal scores in a node, also across FAST cells:
                             the first in key order wins
  n-ini-1 / -2 / -4, last-root-only, root-boundary-fractional   root columns; leading roots empty;
                             keys on (int)(hX (i + 1)) and its neighbours with a fractional hX
  over-budget                4 nIni > N: more keys than the budget, count and capacity still agree
  lap-exact-*, lap-all, lap-none   lap0 / lap1 equal to a key's scaled x on levels 0 and 1, one-scan
                             and two-scan rank pass
"""
import ctypes

import numpy as np
import pytest

import octree_patterns as op
from test_gpu_extractor import _unpack
from test_gpu_fast_adversarial import build_ref, check_outputs, check_stages, gpu_octree

pytestmark = pytest.mark.gpu

CASES = op.all_cases()
BATCH = op.SMALL_BATCH


def level_info(ext, image, level):
    info = np.zeros(4, np.int32)
    assert ext._lib.orbfe_debug_copy(ext.handle, 3, image, level, info.ctypes.data, 16) == 4
    return info.tolist()


def check_octree(ext, image, ref, nlevels, lap, scale, what):
    """Octree keys (x, y, score) in order and the level-info words of image `image` of the last call."""
    for l in range(nlevels):
        o = ref["oct"][l]
        want = list(zip(o["x"].astype(int).tolist(), o["y"].astype(int).tolist(), o["response"].astype(int).tolist()))
        gx, gy, gs = _unpack(gpu_octree(ext, image, l))
        got = list(zip(gx.tolist(), gy.tolist(), gs.tolist()))
        assert len(got) == len(want), f"{what} level {l}: {len(got)} octree keys vs oracle {len(want)}"
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not bad, f"{what} level {l}: {len(bad)} octree keys (x, y, score) differ, first at {bad[0]}: " \
                        f"gpu {got[bad[0]]} vs oracle {want[bad[0]]}"
        nlap, nmono = op.lap_split([(x - op.B, y, s) for x, y, s in want], l, lap, scale)
        winfo = [len(want), nlap, nmono, int(ref["cells"][l][0].sum())]
        assert level_info(ext, image, l) == winfo, f"{what} level {l}: level info {level_info(ext, image, l)} vs {winfo}"


def root_columns(case):
    """nIni of every level, from the definition's root geometry."""
    import fast_patterns as fp
    from oracle import octree_definition as od
    h, w = case.img.shape
    return [od.root_geometry(lw - 2 * op.B, lh - 2 * op.B)[0] for lw, lh in fp.level_sizes(w, h, case.nlevels, case.scale)]


@pytest.fixture(scope="module")
def refs(oracle_lib):
    """Oracle reference, definition trace and asserted precondition of every case, once for the module."""
    out = {}
    for c in CASES:
        ref = op.reference(c, oracle_lib)
        c.pre(c, ref["levels"])   # CPU: the key set reaches its branch
        out[c.name] = ref
    return out


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_call(case, gpu, refs):
    """One image through the host API: k_octree<1024>."""
    from orb_slam3_ros_amd.extractor import ORBextractor
    ref = refs[case.name]
    ext = ORBextractor(case.nfeat, case.scale, case.nlevels, case.ini, case.min)
    try:
        h, w = case.img.shape
        cap = ext.capacity(w, h)
        n_ini = root_columns(case)
        assert cap == sum(max(b + 3, 4 * k) for b, k in zip(ref["budget"], n_ini))
        mono, kp, desc = ext(case.img, None, case.lap)
        assert len(kp) == len(ref["kp"]) <= cap
        check_octree(ext, 0, ref, case.nlevels, case.lap, case.scale, case.name)
        check_stages(ext, 0, ref, case.name)
        check_outputs(mono, kp, desc, ref, case.name)
    finally:
        ext.close()


# ---- device batches: cases of equal size and parameters share one batch of 16 ----------------------
def _group_key(c):
    return (c.img.shape, c.nfeat, c.nlevels, c.ini, c.min, c.lap)


GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_group_key(_c), []).append(_c)
GROUP_LIST = list(GROUPS.values())


def _fillers(cases, count, seed):
    """Distinct images of the group's size to fill the batch: flips of the cases' images (the same kind
    of key set elsewhere) and noise."""
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
    """16 images through orbfe_extract_batch: k_octree<256>. The group's cases and fillers of the same
    size sit in seeded shuffled slots; every image of the batch is compared."""
    import torch
    from orb_slam3_ros_amd.extractor import ORBextractor
    c0 = group[0]
    h, w = c0.img.shape
    seed = 7000 + len(c0.name) + w
    imgs = [c.img for c in group]
    ref = [refs[c.name] for c in group]
    for f in _fillers(group, max(BATCH - len(group), 0), seed):
        imgs.append(f)
        ref.append(build_ref(oracle_lib, f, c0.nfeat, c0.scale, c0.nlevels, c0.ini, c0.min, c0.lap))
    order = np.random.default_rng(seed).permutation(len(imgs))
    n = len(order)
    assert n >= BATCH
    host = np.stack([imgs[u] for u in order])
    dev = torch.from_numpy(host).cuda()
    ext = ORBextractor(c0.nfeat, c0.scale, c0.nlevels, c0.ini, c0.min)
    try:
        cap = ext.capacity(w, h)
        kps = torch.zeros((n, cap, 7), dtype=torch.int32, device=gpu)
        desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=gpu)
        cnt = torch.zeros((n, 2), dtype=torch.int32, device=gpu)
        assert ext._lib.orbfe_set_batch_outputs(ext.handle, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), n) == 0
        ptrs = (ctypes.c_void_p * n)(*[dev.data_ptr() + i * h * w for i in range(n)])
        rc = ext._lib.orbfe_extract_batch(ext.handle, n, ptrs, w, h, w, c0.lap[0], c0.lap[1], None)
        assert rc == 0, f"orbfe_extract_batch refused {n} images of {w}x{h}: {rc}"
        torch.cuda.synchronize()
        cnt_h, kps_h, desc_h = cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
        for i, u in enumerate(order):
            what = f"slot {i} ({group[u].name if u < len(group) else 'filler %d' % (u - len(group))}) of {n}:"
            assert int(cnt_h[i, 0]) == len(ref[u]["kp"]) <= cap, f"{what} {int(cnt_h[i, 0])} keypoints vs {len(ref[u]['kp'])}"
            check_octree(ext, i, ref[u], c0.nlevels, c0.lap, c0.scale, what)
            check_stages(ext, i, ref[u], what)
            check_outputs(int(cnt_h[i, 1]), kps_h[i, :cnt_h[i, 0]], desc_h[i, :cnt_h[i, 0]], ref[u], what)
    finally:
        ext.close()
    del dev
