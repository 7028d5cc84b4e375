"""GPU parity of k_describe's border staging, bit-exact against the CPU oracle.

A keypoint whose 43x43 patch leaves its level, or ends within 12 columns of the level's right edge, is
a border slot. On a dword-aligned level (base and pitch multiples of 4) the kernel stages it from the
same prefetched 16-byte loads as an interior slot: rows reflect in the load address, the 48-byte window
is clamped into the row, and the columns outside the level are mirrored in LDS. Other levels keep the
byte loop. The images here are 272x264 and 268x264 with 8 levels, the smallest the extractor accepts
(it refuses a geometry with a level under 73 px either way): the top level is 76x74 or 75x74, where
most patches are border patches. Block texture gives corners on every level, and bright squares are
planted at every distance 16..22 px from each edge and in the four corners of level 0.

Every case first takes a census of the oracle's keypoints with the kernel's own predicates (restated in
`slot_class`) and fails unless slots of every class are present: reflection on the left only, right
only, top only, bottom only, on two sides (a corner), and the right-edge window clamp without
reflection. Then keypoint records (angle bits included) and descriptors are compared with the oracle's.

A patch that reflects on the left and the right at once needs a level at most 42 px wide. No such slot
exists: the FAST cell grid has width / 35 columns and height / 35 rows over the level less a 16 px
border, so a level narrower or lower than 67 px has no cell and no key in the oracle (and the
extractor refuses such a geometry). The census asserts that no smaller level holds a key, so the class
is known to be unreachable and not silently missing; `slot_class` still names it.

  test_batch[aligned16]     16 images 272x264, pitch 272: k_describe<4>, every level 16-aligned
  test_batch[w4-tight]      268x264 (a multiple of 4, not of 16), pitch 268
  test_batch[w4-padded]     268x264, level-0 pitch 300
  test_batch[byte-path]     272x264, level-0 pitch 275: level 0 keeps the byte loop, levels 1..7 do not
  test_exact_size_guard     level 0 an exact-size tensor (pitch == width), the border frame its last
                            image, a guard tensor allocated after it: outputs equal the oracle's for two
                            guard fills and the guard is unchanged
  test_host_call            one image through the host call: k_describe<1>
"""
import ctypes

import numpy as np
import pytest

from test_gpu_fast_adversarial import check_outputs

pytestmark = pytest.mark.gpu

H = 264
NFEAT, SCALE, NLEVELS, INI, MIN = 1000, 1.2, 8, 20, 7
BATCH = 16
SENTINEL = 0x5A
R, N, WIN = 21, 43, 48     # patch radius, patch size, staged window (bytes per patch row)
SEED = 3                   # chosen on the CPU: every class below is present at both widths
CLASSES = ("left", "right", "top", "bottom", "corner", "clamp")
MIN_KEY_LEVEL = 67         # 2 * 16 border + one 35 px cell: smaller levels have no FAST cell


def border_image(seed, w, h=H):
    """Grey blocks of 5 px (corners that survive every level) and bright 3x3 squares whose centre is
    16..22 px from each edge, along all four edges and in the four corners."""
    rng = np.random.default_rng(seed)
    blk = rng.integers(40, 200, size=((h + 4) // 5, (w + 4) // 5))
    img = np.kron(blk, np.ones((5, 5), np.int64))[:h, :w].astype(np.uint8)

    def square(x, y):
        img[y - 1:y + 2, x - 1:x + 2] = 255

    for i, d in enumerate(range(16, 23)):
        t = 30 + 11 * i                       # position along the edge
        for x, y in ((d, t), (w - 1 - d, t), (t, d), (t, h - 1 - d)):
            square(x, y)
        e = 16 + (i * 3) % 7                  # distance from the other edge of a corner
        for x, y in ((d, e), (w - 1 - d, e), (d, h - 1 - e), (w - 1 - d, h - 1 - e)):
            square(x, y)
    return img


def slot_class(x, y, w, h, pitch, aligned):
    """The staging class k_describe picks for a key at (x, y) of a w x h level (desc_slot, restated):
    'interior', 'byte', or the name of the border class."""
    px0, py0 = x - R, y - R
    gx0 = px0 & ~3
    if not aligned:
        return "byte"
    if px0 >= 0 and py0 >= 0 and py0 + N <= h and gx0 + WIN + 4 <= w:
        return "interior"
    if pitch < WIN:
        return "byte"
    ws = min(max(gx0, 0), pitch - WIN)
    s = px0 - ws
    nl, cr = max(-px0, 0), min(w - px0, N)
    if not (py0 > -h and py0 + N < 2 * h and nl <= 8 and N - cr <= 8 and 2 * nl < cr and 2 * cr - N - 1 >= nl
            and nl + s >= 0 and cr + s <= WIN):
        return "byte"
    left, right, top, bottom = px0 < 0, px0 + N > w, py0 < 0, py0 + N > h
    if left and right:
        return "left+right"
    if (left or right) and (top or bottom):
        return "corner"
    for name, on in (("left", left), ("right", right), ("top", top), ("bottom", bottom)):
        if on:
            return name
    return "clamp"


def census(ref, pitch0):
    """Slots per staging class over the levels of one reference."""
    out = {}
    for l, (keys, lv) in enumerate(zip(ref["oct"], ref["pyr"])):
        h, w = lv.shape
        pitch = pitch0 if l == 0 else (w + 15) // 16 * 16
        assert len(keys) == 0 or min(w, h) >= MIN_KEY_LEVEL, f"level {l} ({w}x{h}) has keys: left+right slots may exist"
        for k in keys:
            c = slot_class(int(k["x"]), int(k["y"]), w, h, pitch, pitch % 4 == 0)
            out[c] = out.get(c, 0) + 1
            out[(l, c)] = out.get((l, c), 0) + 1
    return out


_REFS = {}


def reference(oracle_lib, w, kind):
    """Oracle outputs of image `kind` (0: the planted image, 1..3: its flips) of width w; computed once."""
    if (w, kind) not in _REFS:
        base = border_image(SEED, w)
        img = np.ascontiguousarray([base, base[:, ::-1], base[::-1], base[::-1, ::-1]][kind])
        ora = oracle_lib.OracleExtractor(NFEAT, SCALE, NLEVELS, INI, MIN)
        mono, kp, desc = ora(img)
        ref = dict(img=img, mono=mono, kp=kp, desc=desc, pyr=[], oct=[])
        for l in range(NLEVELS):
            ref["pyr"].append(ora.pyramid_level(l))
            ref["oct"].append(ora.debug_keys(l, 1))
        ora.close()
        _REFS[(w, kind)] = ref
    return _REFS[(w, kind)]


def require_classes(refs, pitch0, want=CLASSES):
    """The condition of every case: the oracle's keypoints of the batch's images hold every class."""
    tot = {}
    for ref in refs:
        for k, v in census(ref, pitch0).items():
            tot[k] = tot.get(k, 0) + v
    missing = [c for c in want if tot.get(c, 0) == 0]
    per_class = {k: v for k, v in tot.items() if isinstance(k, str)}
    assert not missing, f"no {missing} slot among the oracle's keypoints: {per_class}"
    return tot


def run_batch(gpu, refs, order, w, pitch, dev=None):
    """orbfe_extract_batch over images refs[order[i]] in a pitched device buffer (or in `dev`, a byte
    tensor of exactly len(order) * H * pitch); every image compared with its reference."""
    import torch
    from orb_slam3_ros_amd.extractor import ORBextractor
    n = len(order)
    assert n >= BATCH
    host = np.full((n, H, pitch), SENTINEL, np.uint8)
    for i, u in enumerate(order):
        host[i, :, :w] = refs[u]["img"]
    if dev is None:
        dev = torch.from_numpy(host.reshape(-1)).cuda()
    else:
        assert dev.numel() == host.size
        dev.copy_(torch.from_numpy(host.reshape(-1)))
    ext = ORBextractor(NFEAT, SCALE, NLEVELS, INI, MIN)
    try:
        cap = ext.capacity(w, H)
        kps = torch.full((n, cap, 7), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        desc = torch.full((n, cap, 32), SENTINEL, dtype=torch.uint8, device=gpu)
        cnt = torch.full((n, 2), -1, dtype=torch.int32, device=gpu)
        assert ext._lib.orbfe_set_batch_outputs(ext.handle, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), n) == 0
        ptrs = (ctypes.c_void_p * n)(*[dev.data_ptr() + i * H * pitch for i in range(n)])
        rc = ext._lib.orbfe_extract_batch(ext.handle, n, ptrs, w, H, pitch, 0, 0, None)
        assert rc == 0, f"orbfe_extract_batch refused {n} images of {w}x{H}, pitch {pitch}: {rc}"
        torch.cuda.synchronize()
        cnt_h, kps_h, desc_h = cnt.cpu().numpy(), kps.cpu().numpy(), desc.cpu().numpy()
    finally:
        ext.close()
    for i, u in enumerate(order):
        what = f"image {i} (kind {u}) of {n}, {w}x{H} pitch {pitch}:"
        nk = int(cnt_h[i, 0])
        assert nk == len(refs[u]["kp"]) <= cap, f"{what} {nk} keypoints vs {len(refs[u]['kp'])}"
        check_outputs(int(cnt_h[i, 1]), kps_h[i, :nk], desc_h[i, :nk], refs[u], what)
    return cnt_h, kps_h, desc_h


BATCH_CASES = {
    "aligned16": (272, 272, CLASSES),
    "w4-tight": (268, 268, CLASSES),
    "w4-padded": (268, 300, CLASSES),
    # level 0 all byte loop; levels 1..7 (16-aligned pitches) still hold every class
    "byte-path": (272, 275, CLASSES + ("byte",)),
}


@pytest.mark.parametrize("name", list(BATCH_CASES), ids=str)
def test_batch(name, gpu, oracle_lib):
    w, pitch, want = BATCH_CASES[name]
    refs = [reference(oracle_lib, w, k) for k in range(4)]
    tot = require_classes(refs, pitch, want)
    if name == "byte-path":
        assert tot.get((0, "byte"), 0) == sum(v for (k, v) in tot.items() if isinstance(k, tuple) and k[0] == 0)
    order = np.random.default_rng(700 + pitch).permutation(np.arange(BATCH) % 4)
    run_batch(gpu, refs, order, w, pitch)


def test_exact_size_guard(gpu, oracle_lib):
    """Level 0 is a tensor of exactly 16 * 264 * 272 bytes, pitch == width, and the planted image and
    its vertical flip (border keys on the last rows) are the last two images; a guard tensor is
    allocated right after. No read may pass the last row of the last image: the outputs equal the
    oracle's whatever the guard holds, and the guard keeps its fill."""
    import torch
    w = 272
    refs = [reference(oracle_lib, w, k) for k in range(4)]
    tot = require_classes(refs, w)
    assert tot.get("bottom", 0) > 0 and tot.get((0, "bottom"), 0) > 0, "no bottom-edge slot on level 0"
    order = np.array([k % 4 for k in range(BATCH - 2)] + [0, 2])
    dev = torch.empty(BATCH * H * w, dtype=torch.uint8, device=gpu)
    guard = torch.empty(1 << 16, dtype=torch.uint8, device=gpu)
    outs = []
    for fill in (0x00, 0xFF):
        guard.fill_(fill)
        outs.append(run_batch(gpu, refs, order, w, w, dev=dev))
        assert bool((guard == fill).all()), f"guard bytes changed (fill {fill:#x})"
    for a, b in zip(*outs):
        assert np.array_equal(a, b), "outputs depend on the bytes behind level 0"


def test_host_call(gpu, oracle_lib):
    """One image through the host API: k_describe<1>, one slot per wave, tight pitch 268."""
    from orb_slam3_ros_amd.extractor import ORBextractor
    w = 268
    ref = reference(oracle_lib, w, 0)
    require_classes([ref], w)
    ext = ORBextractor(NFEAT, SCALE, NLEVELS, INI, MIN)
    try:
        mono, kp, desc = ext(ref["img"], None, (0, 0))
        check_outputs(mono, kp, desc, ref, "host call")
    finally:
        ext.close()
