"""GPU parity of the rectification kernels (k_remap, k_undistort) on the planted inputs of
tests/remap_patterns.py, bit-exact against the plain definition of oracle/remap_definition.py
(held against the C++ oracle on the same inputs by tests/test_remap_definition.py, so a difference
here is the device's). No tolerances.

Every remap pattern first asserts on the CPU (classify_groups: the kernel's fast-path rule as its
comment states it) that it reaches what it is named for, then runs in five forms:

  a  the host convenience call remap_linear (tight rows)
  b  the host C call with a pitched source (pitch up4(sw) + 4) and a pitched destination (dw + 3)
  c  a device batch of 3, source pitch up4(sw) and 4-byte aligned bases: the fast path where the
     rule holds; the flat source buffer ends at the last row's width
  d  a device batch of 9, source pitch not a multiple of 4: the guarded byte path throughout
  e  a device batch of 3, aligned pitch, every base one byte off: guarded too

Batches hold distinct images. Destinations are views into buffers prefilled with 0xA5; every byte
outside the image rows and columns must still be 0xA5 afterwards.
"""
import ctypes

import numpy as np
import pytest

import remap_patterns as rp
from oracle import remap_definition as rd

pytestmark = pytest.mark.gpu

NAMES = sorted(rp.PATTERNS)
FILL = 0xA5


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} px differ from the definition, first (y, x) {bad[:6].tolist()}: "
                           f"gpu {[int(got[y, x]) for y, x in bad[:6]]} vs {[int(want[y, x]) for y, x in bad[:6]]}")


def _odd_pitch(sw):
    return sw + 1 if (sw + 1) % 4 else sw + 3


def host_call(src, mx, my, spitch, dpitch, doff=0):
    """orbfe_remap_linear with a strided source and destination (host memory)."""
    from orb_slam3_ros_amd import _lib
    lib = _lib.load()
    sh, sw = src.shape
    dh, dw = mx.shape
    sbuf = np.full(spitch * (sh - 1) + sw, 0x5A, np.uint8)
    np.lib.stride_tricks.as_strided(sbuf, (sh, sw), (spitch, 1))[:] = src
    dbuf = np.full(doff + dpitch * dh + 5, FILL, np.uint8)
    mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
    _lib.check(lib.orbfe_remap_linear(sbuf.ctypes.data, sw, sh, spitch, mx.ctypes.data, my.ctypes.data, dw, dh,
                                      dbuf.ctypes.data + doff, dpitch), "remap_linear")
    view = np.lib.stride_tricks.as_strided(dbuf[doff:], (dh, dw), (dpitch, 1))
    out = view.copy()
    view[:] = FILL
    assert (dbuf == FILL).all(), "the host call wrote outside the image rows and columns"
    return out


def device_batch(imgs, mx, my, spitch, soff, dpitch, doff, bump=None, through_lib=False):
    """remap_linear_batch over as_strided views of flat device buffers: image i of the source at
    soff + i * up4(spitch * sh) (+ 1 for image `bump`), of the destination at doff + i * dpitch * dh.
    The source buffer ends with the last image's last row (width, not pitch). Returns the outputs;
    asserts that every destination byte outside the images is still 0xA5."""
    import torch
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd.rectify import remap_linear_batch
    n, (sh, sw), (dh, dw) = len(imgs), imgs[0].shape, mx.shape
    simg, dimg = rp.up4(spitch * sh) + (4 if bump is not None else 0), dpitch * dh
    sflat = torch.full((soff + (n - 1) * simg + (1 if bump == n - 1 else 0) + spitch * (sh - 1) + sw,), 0x5A,
                       dtype=torch.uint8, device="cuda")
    dflat = torch.full((doff + n * dimg + 7,), FILL, dtype=torch.uint8, device="cuda")
    soffs = [soff + i * simg + (1 if i == bump else 0) for i in range(n)]
    for i, im in enumerate(imgs):
        sflat.as_strided((sh, sw), (spitch, 1), soffs[i]).copy_(torch.from_numpy(np.array(im)).cuda())
    dmx, dmy = torch.from_numpy(np.array(mx)).cuda(), torch.from_numpy(np.array(my)).cuda()
    before = sflat.clone()
    if through_lib or bump is not None:   # a hand-made pointer table
        ps = (ctypes.c_void_p * n)(*[sflat.data_ptr() + o for o in soffs])
        pd = (ctypes.c_void_p * n)(*[dflat.data_ptr() + doff + i * dimg for i in range(n)])
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(_lib.load().orbfe_remap_linear_batch(ps, sw, sh, spitch, dmx.data_ptr(), dmy.data_ptr(), dw, dh, pd,
                                                        dpitch, n, stream), "remap_linear_batch")
    else:
        remap_linear_batch(sflat.as_strided((n, sh, sw), (simg, spitch, 1), soff), dmx, dmy,
                           dflat.as_strided((n, dh, dw), (dimg, dpitch, 1), doff))
    torch.cuda.synchronize()
    assert torch.equal(sflat, before), "the call changed its source"
    flat = dflat.cpu().numpy()
    outs = []
    for i in range(n):
        view = np.lib.stride_tricks.as_strided(flat[doff + i * dimg:], (dh, dw), (dpitch, 1))
        outs.append(view.copy())
        view[:] = FILL
    assert (flat == FILL).all(), f"{int((flat != FILL).sum())} bytes outside the image rows and columns were written"
    return outs


def _check_batch(name, n, what, **kw):
    src, mx, my, _ = rp.built(name)
    outs = device_batch([rp.variant(src, i % 3) for i in range(n)], mx, my, **kw)
    for i in range(n):
        _same(outs[i], rp.expected(name, i % 3), f"{name} {what} image {i} of {n}")


@pytest.mark.parametrize("name", NAMES)
def test_remap_pattern(name, gpu):
    from orb_slam3_ros_amd.rectify import remap_linear
    src, mx, my, _ = rp.built(name)
    rp.pre(name)(src, mx, my)   # CPU: the inputs reach what the pattern is named for
    sh, sw = src.shape
    dw = mx.shape[1]
    want = rp.expected(name)
    _same(remap_linear(src, mx, my), want, f"{name} form a")
    _same(host_call(src, mx, my, rp.up4(sw) + 4, dw + 3), want, f"{name} form b")
    _check_batch(name, 3, "form c", spitch=rp.up4(sw), soff=0, dpitch=dw, doff=0)
    _check_batch(name, 9, "form d", spitch=_odd_pitch(sw), soff=0, dpitch=dw, doff=0)
    _check_batch(name, 3, "form e", spitch=rp.up4(sw), soff=1, dpitch=dw, doff=0)


def test_window_sweep_coverage():
    """Conditions on the inputs alone (also held, without a GPU, by tests/test_remap_definition.py)."""
    fast, d6, fail = rp.sweep_coverage()
    assert min(fast) >= 20 and d6 >= 10, (fast, d6)
    for clause in (rd.D_BIG, rd.D_NEG, rd.WINDOW):
        assert fail.get(clause, 0) >= 10, (clause, fail)


@pytest.mark.parametrize("dw", rp.LAYOUT_WIDTHS)
def test_destination_layouts(dw, gpu):
    """Every base offset 0-3 and the pitches dw, dw + 1 and dw + 3 of the destination: the dword
    store, the byte stores of a misaligned or partial group, and nothing written outside."""
    name = f"layout-dw{dw}"
    src, mx, my, _ = rp.built(name)
    rp.pre(name)(src, mx, my)
    for doff in range(4):
        for dpitch in (dw, dw + 1, dw + 3):
            what = f"destination offset {doff} pitch {dpitch}"
            _check_batch(name, 2, what, spitch=20, soff=0, dpitch=dpitch, doff=doff)
            _same(host_call(src, mx, my, 20, dpitch, doff), rp.expected(name), f"{name} host {what}")


@pytest.mark.parametrize("n", rp.LAYOUT_BATCHES)
def test_batch_sizes(n, gpu):
    """n around the 8 images one block serves: whole and partial image groups, aligned (fast) and not."""
    for name in ("layout-dw8", "layout-dw9"):
        _check_batch(name, n, f"n = {n} aligned", spitch=20, soff=0, dpitch=mx_pitch(name), doff=0)
        _check_batch(name, n, f"n = {n} odd pitch", spitch=21, soff=0, dpitch=mx_pitch(name) + 1, doff=1)


def mx_pitch(name):
    return rp.built(name)[1].shape[1]


@pytest.mark.parametrize("name", ["layout-dw8", "sweep-s1.0-p2", "right-edge-sw12"])
def test_one_misaligned_pointer_of_nine(name, gpu):
    """A hand-made pointer table in which only image 5 of 9 is off by one byte: the whole launch takes
    the guarded path (on the CPU: the same groups are fast when every pointer is aligned)."""
    src, mx, my, _ = rp.built(name)
    sh, sw = src.shape
    assert any(g.verdict == rd.FAST for row in rd.classify_groups(sw, sh, rp.up4(sw), mx, my, True) for g in row)
    assert not any(g.verdict == rd.FAST for row in rd.classify_groups(sw, sh, rp.up4(sw), mx, my, False) for g in row)
    _check_batch(name, 9, "image 5 misaligned", spitch=rp.up4(sw), soff=0, dpitch=mx.shape[1], doff=0, bump=5)
    _check_batch(name, 9, "pointer table, all aligned", spitch=rp.up4(sw), soff=0, dpitch=mx.shape[1], doff=0, through_lib=True)


# ---- undistort ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def undistort_expected():
    pts = rp.undistort_points()
    return {nd: rd.undistort_points_def(pts, rp.UNDIST_K, np.array(d, np.float32)) for nd, d in rp.UNDIST_DIST.items()}


@pytest.mark.parametrize("n", rp.UNDIST_COUNTS)
@pytest.mark.parametrize("ndist", sorted(rp.UNDIST_DIST))
def test_undistort_points(ndist, n, gpu, undistort_expected):
    from orb_slam3_ros_amd.rectify import undistort_points
    pts = rp.undistort_points()
    if ndist == 4:   # CPU: the icdist < 0 break at iteration 0, later, and never
        _, brk = rd.undistort_points_def(pts, rp.UNDIST_K, np.array(rp.UNDIST_DIST[4], np.float32), trace=True)
        assert (brk == 0).any() and (brk >= 1).any() and (brk == -1).any()
    got = undistort_points(pts[:n], rp.UNDIST_K, np.array(rp.UNDIST_DIST[ndist], np.float32))
    want = undistort_expected[ndist][:n]
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(1)).ravel()
    print(f"ndist {ndist} n {n}: {len(bad)} points differ", [(int(i), pts[i].tolist(), got[i].view(np.uint32).tolist(),
                                                              want[i].view(np.uint32).tolist()) for i in bad[:8]])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
