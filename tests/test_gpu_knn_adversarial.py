"""GPU parity of the kNN + ratio stage of ComputeStereoFishEyeMatches on the planted cases of
tests/knn_patterns.py (each proved on the CPU to reach what it names, tests/test_knn_definition.py): every
case through every kernel form, every slot of train / l2r, every slot of dist and the count equal to the C++
oracle's on the same bytes.

  matcher.stereo_knn_ratio                      k_knn2, one call per case
  orbfe_stereo_knn_slabs, 1 and 15 frames       k_knn2_batch<16>
  orbfe_stereo_knn_slabs, 16 and 17 frames      k_knn2_batch<4>
  StereoFrontEnd(stereo="fisheye")              orbfe_stereo_knn_batch over an extractor handle, stride 2

The frames of one launch are different cases at different (monoL, monoR), laid into two slabs of different
sizes or into one interleaved slab, so a wrong frame stride shows another case's answer; the images around
them and the rows around [mono, n) are poison. Outputs are larger than needed and full of a sentinel. Which
kernel ran is asserted from the driver's host record (orbfe_matcher_last_knn_form), so a moved
`nframes < 16` rule fails here instead of testing one kernel twice.

Out of scope: TriangulateMatches and the parallax check after the ratio test, the extractor's lapping split.
"""
import ctypes

import numpy as np
import pytest

import knn_patterns as P
from oracle import knn_definition as kd
from orb_slam3_ros_amd import _lib
from orb_slam3_ros_amd.matcher import stereo_knn_ratio

pytestmark = pytest.mark.gpu

SENT = -777
GROUPS = sorted({c.group for c in P.all_cases()})


@pytest.fixture(scope="module")
def lib(gpu):
    return _lib.load()


def _knn_form(lib):
    w = (ctypes.c_int32 * 2)()
    assert lib.orbfe_matcher_last_knn_form(w) == _lib.ORBFE_OK
    return tuple(w)


@pytest.mark.parametrize("group", GROUPS)
def test_knn2(gpu, oracle_lib, group):
    for c in (c for c in P.all_cases() if c.group == group):
        n_o, t_o, d_o = oracle_lib.stereo_knn_ratio(c.L, c.R, c.ratio)
        n, t, d = stereo_knn_ratio(c.L, c.R, c.ratio)
        assert (t < len(c.R)).all(), c.name   # never a row of the LDS chunk's zero-filled tail
        np.testing.assert_array_equal(t, t_o, err_msg=c.name)
        np.testing.assert_array_equal(d, d_o, err_msg=c.name)
        assert n == n_o == int((t >= 0).sum()), c.name


class Slabs:
    """One launch's inputs on the device and its sentinel-filled outputs, two frames and a few words longer
    than the launch writes."""

    def __init__(self, gpu, cl, dl, cr, dr, adr, cap, nframes, same):
        import torch
        self.t, self.cap, self.n, self.adr = torch, cap, nframes, adr
        self.cl, self.dl = torch.from_numpy(cl).to(gpu), torch.from_numpy(dl).to(gpu)
        self.cr, self.dr = (self.cl, self.dl) if same else (torch.from_numpy(cr).to(gpu), torch.from_numpy(dr).to(gpu))
        self.l2r = torch.full(((nframes + 2) * cap + 7,), SENT, dtype=torch.int32, device=gpu)
        self.dist = torch.full(((nframes + 2) * cap + 7,), SENT, dtype=torch.int32, device=gpu)
        self.ngood = torch.full((nframes + 3,), SENT, dtype=torch.int32, device=gpu)

    def run(self, lib, ratio, cap=None):
        lb, ls, rb, rs = self.adr
        rc = lib.orbfe_stereo_knn_slabs(self.cl.data_ptr(), self.dl.data_ptr(), lb, ls, self.cr.data_ptr(),
                                        self.dr.data_ptr(), rb, rs, self.cap if cap is None else cap, self.n,
                                        float(ratio), self.l2r.data_ptr(), self.dist.data_ptr(),
                                        self.ngood.data_ptr(), self.t.cuda.current_stream().cuda_stream)
        self.t.cuda.synchronize()
        return rc

    def host(self):
        return self.l2r.cpu().numpy(), self.dist.cpu().numpy(), self.ngood.cpu().numpy()


def _check_outputs(s, wants, what):
    """wants[f] = (l2r [cap], dist [cap], ngood) of frame f."""
    l2r, dist, ngood = s.host()
    n, cap = s.n, s.cap
    for f, (w_l2r, w_dist, w_n) in enumerate(wants):
        np.testing.assert_array_equal(l2r[f * cap:(f + 1) * cap], w_l2r, err_msg=f"{what}: l2r of frame {f}")
        np.testing.assert_array_equal(dist[f * cap:(f + 1) * cap], w_dist, err_msg=f"{what}: dist of frame {f}")
        assert ngood[f] == w_n == int((l2r[f * cap:(f + 1) * cap] >= 0).sum()), (what, f, ngood[f], w_n)
    assert (l2r[n * cap:] == SENT).all() and (dist[n * cap:] == SENT).all() and (ngood[n:] == SENT).all(), what
    return ngood[:n].copy()


def _launch(lib, gpu, oracle_lib, frames, addressing, twice):
    n, cap, ratio = len(frames), frames[0].cap, frames[0].case.ratio
    cl, dl, cr, dr, adr = P.pack(frames, addressing)
    s = Slabs(gpu, cl, dl, cr, dr, adr, cap, n, addressing == "interleaved")
    what = f"{n} frames from {frames[0].name}, {addressing}"
    wants = [fr.expected(oracle_lib) for fr in frames]
    for _ in range(2 if twice else 1):   # the count is zeroed by the call, not accumulated
        assert s.run(lib, ratio) == _lib.ORBFE_OK, what
        assert _knn_form(lib) == (16 if n < 16 else 4, cap * 32), (what, _knn_form(lib))
        _check_outputs(s, wants, what)


@pytest.mark.parametrize("nframes", [1, 15, 16, 17])
def test_slabs_every_case(lib, gpu, oracle_lib, nframes):
    """k_knn2_batch<16> (1, 15 frames) and k_knn2_batch<4> (16, 17 frames): every frame of
    knn_patterns.all_frames(), a launch at a time."""
    i = 0
    for (cap, ratio), frames in sorted(P.launch_groups().items()):
        for chunk in P.launches(frames, nframes):
            _launch(lib, gpu, oracle_lib, chunk, P.ADDRESSINGS[i % 2], twice=i % 3 == 0)
            i += 1


@pytest.mark.parametrize("nframes", [15, 16])
def test_one_left_several_rights(lib, gpu, oracle_lib, nframes):
    """(lbase, lstep, rbase, rstep) = (3, 0, 0, 1): one left image against nframes right images, each the
    case's train rows rotated by f and placed at monoR = f."""
    c = P.case("merge-nt17-a")
    cap, monoL, nl, nt = 512, 65, len(c.L), len(c.R)
    left = P.Frame(c, monoL, 0, cap).built()
    spare = P._poison(cap, c.L)   # the other left images and the rows around the train rows: the queries
    cl = np.tile(np.array([cap, 0], np.int32), (5, 1))
    dl = np.tile(spare, (5, 1, 1))
    cl[3], dl[3] = left[0], left[1]
    cr = np.zeros((nframes, 2), np.int32)
    dr = np.tile(spare, (nframes, 1, 1))
    for f in range(nframes):
        cr[f] = (f + nt, f)
        dr[f, f:f + nt] = np.roll(c.R, f, axis=0)
    s = Slabs(gpu, cl, dl, cr, dr, (3, 0, 0, 1), cap, nframes, False)
    assert s.run(lib, c.ratio) == _lib.ORBFE_OK
    assert _knn_form(lib) == (16 if nframes < 16 else 4, cap * 32)
    wants = [P.oracle_frame(oracle_lib, cl[3], dl[3], cr[f], dr[f], cap, c.ratio) for f in range(nframes)]
    t0, _, n0, _ = P.run_definition(c)
    for f, w in enumerate(wants):   # the planted answer, moved with the rows
        np.testing.assert_array_equal(w[0][monoL:monoL + nl], np.where(t0 >= 0, (t0 + f) % nt + f, -1))
        assert w[2] == n0 > 0
    _check_outputs(s, wants, f"one left, {nframes} rights")


@pytest.mark.parametrize("nframes", [15, 16])
@pytest.mark.parametrize("cap", [2112, 4096])
def test_lds_above_64k(lib, gpu, oracle_lib, cap, nframes):
    """cap * 32 bytes of dynamic LDS above 64 KB (66 KB and 128 KB, the latter with 12 KB of static LDS in
    k_knn2_batch<16>), on both W. Measured on the MI355X: HIP accepts both launches as they are, without the
    hipFuncAttributeMaxDynamicSharedMemorySize opt-in, and the results are the oracle's."""
    frames = P.frames_by_cap()[cap]
    assert cap * 32 > 64 * 1024 and all(f.case.ratio == P.RATIO for f in frames)
    for i, chunk in enumerate(P.launches(frames, nframes)):
        _launch(lib, gpu, oracle_lib, chunk, P.ADDRESSINGS[(i + 1) % 2], twice=False)
        assert _knn_form(lib)[1] == cap * 32


def test_cap_4097_refused(lib, gpu):
    """A cap whose train rows cannot fit the LDS: ORBFE_E_ARG, nothing written, the count untouched."""
    fr = P.Frame(P.case(P.GEOMETRY_BASE), 1, 3, 4096)
    cl, dl, cr, dr, adr = P.pack([fr, fr], "separate")
    s = Slabs(gpu, cl, dl, cr, dr, adr, 4096, 2, False)
    assert s.run(lib, 0.7, cap=4097) == _lib.ORBFE_E_ARG
    l2r, dist, ngood = s.host()
    assert (l2r == SENT).all() and (dist == SENT).all() and (ngood == SENT).all()


def test_handle_entry(lib, gpu):
    """orbfe_stereo_knn_batch: the StereoSide filled from an extractor handle (left = even, right = odd image
    of one handle) after a real extract_batch, against the definition applied to the slabs it produced."""
    import torch
    from orb_slam3_ros_amd.frontend import StereoFrontEnd
    from orb_slam3_ros_amd.synth import synth_stereo
    F = 3
    host = np.stack([im for i in range(F) for im in synth_stereo(800 + i, 512, 512)])
    fe = StereoFrontEnd(F, 512, 512, nfeatures=1000, device=gpu, lap_left=(0, 400), lap_right=(100, 511),
                        stereo="fisheye")
    fe.l2r.fill_(SENT)
    fe.l2r_dist.fill_(SENT)
    fe.nmatch.fill_(SENT)
    fe.run(torch.from_numpy(host).to(gpu))
    torch.cuda.synchronize()
    assert _knn_form(lib) == (16, fe.cap * 32)
    counts, desc = fe.counts.cpu().numpy(), fe.desc.cpu().numpy()
    l2r, dist, nmatch = fe.l2r.cpu().numpy(), fe.l2r_dist.cpu().numpy(), fe.nmatch.cpu().numpy()
    for f in range(F):
        w_l2r, w_dist, w_n = kd.knn_frame(counts[2 * f], desc[2 * f], counts[2 * f + 1], desc[2 * f + 1], fe.cap, 0.7)
        assert counts[2 * f, 0] > counts[2 * f, 1] > 0 and counts[2 * f + 1, 0] > counts[2 * f + 1, 1] + 2
        np.testing.assert_array_equal(l2r[f], w_l2r, err_msg=f"frame {f}")
        np.testing.assert_array_equal(dist[f], w_dist, err_msg=f"frame {f}")
        assert nmatch[f] == w_n > 0
    fe.close()
