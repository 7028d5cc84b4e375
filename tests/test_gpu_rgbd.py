"""GPU parity of the RGB-D frame path (orbfe_frame_rgbd, orbfe_rgbd_stereo_batch, the device view after
an RGB-D frame), bitwise against the oracle plus numpy:

  * OracleExtractor gives mvKeys and mDescriptors, oracle.undistort_points gives mvKeysUn;
  * the depth look-up is raw[int(y), int(x)] at the DISTORTED keypoint (truncation), the conversion
    np.float32(raw) * np.float32(factor) (u16 always; f32 only when |factor - 1| > 1e-5 in float32),
    and uR = np.float32(xu) - np.float32(bf) / d in float32, -1 where not d > 0.

Every comparison is on uint32 / uint8 views.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NLEVELS, NFEAT = 133, 107, 3, 300   # the shape of test_gpu_input_layout.py
BF = 40.0
TUM1 = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3, dist=[0.262383, -0.953104, -0.005358, 0.002628, 1.163314])


def tum1(w, h, dist=None, bf=BF, factor=1.0 / 5000.0):
    """TUM1 intrinsics with the principal point scaled into a w x h image."""
    from orb_slam3_ros_amd.extractor import RGBDParams
    return RGBDParams(TUM1["fx"], TUM1["fy"], TUM1["cx"] * w / 640.0, TUM1["cy"] * h / 480.0,
                      TUM1["dist"] if dist is None else dist, bf, factor)


def depth_metres(seed, w, h):
    """A seeded smooth depth field in [0.5, 4.5) m with rectangular holes of 0 over about a quarter of it."""
    from orb_slam3_ros_amd.synth import _value_noise
    rng = np.random.default_rng(seed)
    d = 0.5 + 4.0 * _value_noise(rng, h, w, 24)
    for _ in range(4):
        rw, rh = int(rng.integers(w // 6, w // 3)), int(rng.integers(h // 6, h // 3))
        x, y = int(rng.integers(0, w - rw)), int(rng.integers(0, h - rh))
        d[y:y + rh, x:x + rw] = 0.0
    return np.ascontiguousarray(d)   # (the value noise comes column-major)


def depth_u16(seed, w, h):
    return np.rint(depth_metres(seed, w, h) * 5000.0).astype(np.uint16)


def expected(oracle, kps, raw, p):
    """(mvKeysUn, mvuRight, mvDepth) of keypoints `kps` over the raw depth image `raw`."""
    ix, iy = kps["x"].astype(np.int32), kps["y"].astype(np.int32)   # astype truncates, as (int)
    assert (ix >= 0).all() and (ix < raw.shape[1]).all() and (iy >= 0).all() and (iy < raw.shape[0]).all()
    v = raw[iy, ix]
    f = np.float32(p.depth_factor)
    if raw.dtype == np.uint16:
        d = v.astype(np.float32) * f
    elif abs(f - np.float32(1.0)) > np.float32(1e-5):
        d = v * f
    else:
        d = v.copy()
    assert d.dtype == np.float32
    kun = kps.copy()
    if len(p.dist) and p.dist[0] != 0:
        u = oracle.undistort_points(np.stack([kps["x"], kps["y"]], 1), p.K4, p.dist)
        kun["x"], kun["y"] = u[:, 0], u[:, 1]
    ok = d > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ur = np.where(ok, kun["x"] - np.float32(p.bf) / d, np.float32(-1)).astype(np.float32)
    dp = np.where(ok, d, np.float32(-1)).astype(np.float32)
    return kun, ur, dp


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    if len(a) == 0:
        return
    bad = np.nonzero(a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1))[0]
    assert bad.size == 0, f"{what}: rows {np.unique(bad)[:8]} differ, e.g. {a[bad[0]]} vs {b[bad[0]]}"


def check_frame(oracle, got, ref, raw, p, what):
    kps, kun, desc, ur, dp = got
    okps, odesc = ref
    ekun, eur, edp = expected(oracle, okps, raw, p)
    same_bits(kps, okps, what + " mvKeys")
    assert np.array_equal(desc, odesc), what + " mDescriptors"
    same_bits(kun, ekun, what + " mvKeysUn")
    same_bits(dp, edp, what + " mvDepth")
    same_bits(ur, eur, what + " mvuRight")
    return ekun, eur, edp


@pytest.fixture(scope="module")
def small(oracle_lib):
    """Five small images (one flat: no keypoints) with their oracle keypoints / descriptors, once."""
    from orb_slam3_ros_amd.synth import synth_image
    imgs = [synth_image(seed, W, H) for seed in (71, 72, 73, 75)]
    imgs.insert(2, np.full((H, W), 90, np.uint8))
    o = oracle_lib.OracleExtractor(NFEAT, 1.2, NLEVELS, 20, 7)
    refs = []
    for im in imgs:
        _, k, d = o(im)
        refs.append((k.copy(), d.copy()))
    assert len(refs[2][0]) == 0 and all(len(refs[i][0]) > 100 for i in (0, 1, 3, 4))
    return imgs, refs


def _strided(a, extra, fill):
    """`a` as a view with `extra` foreign elements after every row."""
    big = np.full((a.shape[0], a.shape[1] + extra), fill, a.dtype)
    big[:, :a.shape[1]] = a
    v = big[:, :a.shape[1]]
    assert not v.flags["C_CONTIGUOUS"]
    return v


def test_small_u16(gpu, oracle_lib, small):
    """u16 depth, factor 1/5000, TUM1 distortion; then the same frame with a depth stride larger than
    the row and a non-contiguous gray image."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    imgs, refs = small
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    p = tum1(W, H)
    for k in (0, 1):
        raw = depth_u16(500 + k, W, H)
        _, eur, edp = expected(oracle_lib, refs[k][0], raw, p)
        n = len(eur)
        assert (edp > 0).sum() >= 0.3 * n and (edp == -1).sum() >= 0.05 * n and ((eur == -1) == (edp == -1)).all()
        check_frame(oracle_lib, frame_rgbd(ext, imgs[k], raw, p), refs[k], raw, p, f"image {k} tight")
        got = frame_rgbd(ext, _strided(imgs[k], 19, 0xEE), _strided(raw, 7, 0xFFFF), p)
        check_frame(oracle_lib, got, refs[k], raw, p, f"image {k} strided")
    ext.close()


@pytest.mark.parametrize("factor", [1.0 / 5208.0, 1.0])
def test_small_f32_special_values(gpu, oracle_lib, small, factor):
    """f32 depth with NaN, -1 and +inf under known keypoints: NaN and negative give -1 / -1, +inf
    gives depth inf and uR = the undistorted x."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    imgs, refs = small
    okps = refs[3][0]
    raw = depth_metres(510, W, H).astype(np.float32)
    if factor != 1.0:
        raw = raw * np.float32(5208.0)
    special = {3: np.float32("nan"), 11: np.float32(-1.0), 23: np.float32("inf")}
    px = {i: (int(okps["y"][i]), int(okps["x"][i])) for i in special}
    assert len(set(px.values())) == 3
    for i, v in special.items():
        raw[px[i]] = v
    p = tum1(W, H, factor=factor)
    ekun, eur, edp = expected(oracle_lib, okps, raw, p)
    n = len(eur)
    assert (edp > 0).sum() >= 0.3 * n and (edp == -1).sum() >= 0.05 * n
    assert eur[3] == -1 and edp[3] == -1 and eur[11] == -1 and edp[11] == -1
    assert np.isposinf(edp[23]) and eur[23] == ekun["x"][23]
    hit = raw[okps["y"].astype(np.int32), okps["x"].astype(np.int32)]
    assert np.isnan(hit).sum() >= 1 and (hit < 0).sum() >= 1 and np.isposinf(hit).sum() >= 1
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    check_frame(oracle_lib, frame_rgbd(ext, imgs[3], raw, p), refs[3], raw, p, f"f32 factor {factor}")
    check_frame(oracle_lib, frame_rgbd(ext, imgs[3], _strided(raw, 3, np.float32(7.0)), p), refs[3], raw, p,
                f"f32 factor {factor} strided")
    ext.close()


def test_tum_shape(gpu, oracle_lib):
    """One 640 x 480, 8-level, 1000-feature frame with the TUM1 camera."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    from orb_slam3_ros_amd.synth import synth_image
    img, raw = synth_image(81, 640, 480), depth_u16(520, 640, 480)
    _, ok, od = oracle_lib.OracleExtractor(1000, 1.2, 8, 20, 7)(img)
    assert len(ok) > 900
    ext = ORBextractor(1000, 1.2, 8, 20, 7)
    p = tum1(640, 480)
    ekun, eur, edp = check_frame(oracle_lib, frame_rgbd(ext, img, raw, p), (ok, od), raw, p, "TUM frame")
    assert (edp > 0).sum() >= 0.3 * len(ok) and (ekun["x"] != ok["x"]).mean() > 0.9
    ext.close()


def test_k1_zero_copies_keypoints(gpu, oracle_lib, small):
    """dist[0] == 0 with the other coefficients non-zero: mvKeysUn = mvKeys bytewise (Frame.cc:749-753)
    and uR uses the raw x."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    imgs, refs = small
    raw = depth_u16(530, W, H)
    p = tum1(W, H, dist=[0.0] + TUM1["dist"][1:])
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    kps, kun, desc, ur, dp = got = frame_rgbd(ext, imgs[0], raw, p)
    check_frame(oracle_lib, got, refs[0], raw, p, "k1 = 0")
    same_bits(kun, kps, "mvKeysUn vs mvKeys")
    ok = dp > 0
    assert ok.sum() > 20
    same_bits(ur[ok], (kps["x"][ok] - np.float32(BF) / dp[ok]).astype(np.float32), "uR from the raw x")
    ext.close()


def test_factor_rule(gpu, oracle_lib, small):
    """f32 depth: factor 1 + 5e-6 leaves the depth bits untouched, 1 + 2e-5 multiplies."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    imgs, refs = small
    raw = (depth_metres(540, W, H) * 1.2345).astype(np.float32)
    okps = refs[1][0]
    hit = raw[okps["y"].astype(np.int32), okps["x"].astype(np.int32)]
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    for factor, multiplies in ((1.0 + 5e-6, False), (1.0 + 2e-5, True)):
        p = tum1(W, H, factor=factor)
        assert np.float32(p.depth_factor) != np.float32(1.0)
        got = frame_rgbd(ext, imgs[1], raw, p)
        check_frame(oracle_lib, got, refs[1], raw, p, f"factor {factor}")
        dp, pos = got[4], hit > 0
        assert pos.sum() > 20
        if multiplies:
            same_bits(dp[pos], hit[pos] * np.float32(factor), "scaled depth")
            assert (dp[pos] != hit[pos]).any()
        else:
            same_bits(dp[pos], hit[pos], "untouched depth")
    ext.close()


def test_truncation_identifies_the_pixel(gpu, oracle_lib, small):
    """raw[y, x] = 1 + x + W y (f32, factor 1): mvDepth names the pixel that was read, which is
    (int(x), int(y)) for the fractional coordinates of levels > 0, never a rounded neighbour."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    imgs, refs = small
    raw = (1 + np.arange(W, dtype=np.float32)[None, :] + np.float32(W) * np.arange(H, dtype=np.float32)[:, None])
    p = tum1(W, H, factor=1.0)
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    kps, _, _, _, dp = got = frame_rgbd(ext, imgs[4], raw, p)
    check_frame(oracle_lib, got, refs[4], raw, p, "pixel-index depth")
    up = kps["octave"] > 0
    fx, fy = kps["x"] - np.floor(kps["x"]), kps["y"] - np.floor(kps["y"])
    assert (up & (fx > 0.5)).sum() > 5 and (up & (fy > 0.5)).sum() > 5   # rounding would read a neighbour
    pix = dp.astype(np.int64) - 1
    assert np.array_equal(pix % W, np.floor(kps["x"]).astype(np.int64))
    assert np.array_equal(pix // W, np.floor(kps["y"]).astype(np.int64))
    ext.close()


UR_SENTINEL, DP_SENTINEL, KEY_SENTINEL = -777.0, -555.0, 0x5A5A5A5A


@pytest.mark.parametrize("nimg,base,step,nframes", [(1, 0, 1, 1), (2, 0, 1, 2), (5, 0, 1, 5), (5, 1, 2, 2)])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_batch(gpu, oracle_lib, small, nimg, base, step, nframes, kind):
    """orbfe_extract_batch, then orbfe_rgbd_stereo_batch over frames base + f * step with a pitched
    depth image each: every frame equals the per-frame expectation (the flat image's frame has no
    keypoints), slots past a count keep the sentinel, and a NULL d_keys_un changes nothing else."""
    import torch
    from orb_slam3_ros_amd.extractor import KEYPOINT_DTYPE, ORBextractor
    imgs, refs = small
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    lib, cap = ext._lib, ext.capacity(W, H)
    dev_imgs = torch.from_numpy(np.stack(imgs[:nimg])).to(gpu)
    arr = (ctypes.c_void_p * nimg)(*[dev_imgs[i].data_ptr() for i in range(nimg)])
    assert lib.orbfe_extract_batch(ext.handle, nimg, arr, W, H, W, 0, 0, None) == 0
    if kind == "u16":
        raws = [depth_u16(600 + f, W, H) for f in range(nframes)]
        p, dt, tdt = tum1(W, H), 0, torch.uint16
    else:
        raws = [(depth_metres(600 + f, W, H) * 5208.0).astype(np.float32) for f in range(nframes)]
        p, dt, tdt = tum1(W, H, factor=1.0 / 5208.0), 1, torch.float32
    pad = 5
    host_depth = np.full((nframes, H, W + pad), 9, raws[0].dtype)   # foreign values after every row
    host_depth[:, :, :W] = np.stack(raws)
    dev_depth = torch.from_numpy(host_depth).to(gpu)
    assert dev_depth.dtype == tdt
    dptr = (ctypes.c_void_p * nframes)(*[dev_depth[f].data_ptr() for f in range(nframes)])
    pitch = (W + pad) * dev_depth.element_size()
    outs = []
    for with_keys in (True, False):
        kun = torch.full((nframes, cap, 7), KEY_SENTINEL, dtype=torch.int32, device=gpu)
        ur = torch.full((nframes, cap), UR_SENTINEL, dtype=torch.float32, device=gpu)
        dp = torch.full((nframes, cap), DP_SENTINEL, dtype=torch.float32, device=gpu)
        rc = lib.orbfe_rgbd_stereo_batch(ext.handle, base, step, nframes, dptr, dt, pitch, p.ref(),
                                         kun.data_ptr() if with_keys else None, ur.data_ptr(), dp.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((kun.cpu().numpy(), ur.cpu().numpy(), dp.cpu().numpy()))
    (kun, ur, dp), (kun2, ur2, dp2) = outs
    assert (kun2 == KEY_SENTINEL).all()
    assert np.array_equal(ur.view(np.uint32), ur2.view(np.uint32)) and np.array_equal(dp.view(np.uint32), dp2.view(np.uint32))
    for f in range(nframes):
        okps = refs[base + f * step][0]
        n = len(okps)
        ekun, eur, edp = expected(oracle_lib, okps, raws[f], p)
        what = f"frame {f} (image {base + f * step}, {n} keypoints)"
        same_bits(kun[f, :n].view(KEYPOINT_DTYPE).reshape(n), ekun, what + " mvKeysUn")
        same_bits(dp[f, :n], edp, what + " mvDepth")
        same_bits(ur[f, :n], eur, what + " mvuRight")
        assert (kun[f, n:] == KEY_SENTINEL).all() and (ur[f, n:] == UR_SENTINEL).all() and (dp[f, n:] == DP_SENTINEL).all()
    if nimg == 5:
        assert len(refs[2][0]) == 0   # the flat image is among the frames checked (base 0) or skipped over (base 1)
    # refused before any launch: a pitch smaller than one row, frames past the batch
    ur = torch.full((nframes, cap), UR_SENTINEL, dtype=torch.float32, device=gpu)
    esz = dev_depth.element_size()
    assert lib.orbfe_rgbd_stereo_batch(ext.handle, base, step, nframes, dptr, dt, W * esz - 1, p.ref(), None,
                                       ur.data_ptr(), ur.data_ptr(), None) == -2
    assert lib.orbfe_rgbd_stereo_batch(ext.handle, nimg, 1, 1, dptr, dt, pitch, p.ref(), None, ur.data_ptr(),
                                       ur.data_ptr(), None) == -2
    torch.cuda.synchronize()
    assert (ur.cpu().numpy() == UR_SENTINEL).all()
    ext.close()


def test_batched_front_end(gpu, oracle_lib, small):
    """RGBDFrontEnd (extract_batch + rgbd_stereo_batch on the current torch stream) over three frames."""
    import torch
    from orb_slam3_ros_amd.frontend import RGBDFrontEnd
    imgs, refs = small
    p = tum1(W, H)
    fe = RGBDFrontEnd(3, W, H, p, nfeatures=NFEAT, nlevels=NLEVELS)
    raws = [depth_u16(700 + f, W, H) for f in range(3)]
    fe.run(torch.from_numpy(np.stack(imgs[:3])).to(gpu), torch.from_numpy(np.stack(raws)).to(gpu))
    torch.cuda.synchronize()
    for f in range(3):
        check_frame(oracle_lib, fe.host_frame(f), refs[f], raws[f], p, f"front-end frame {f}")
    fe.close()


def test_device_view(gpu, oracle_lib):
    """After frame_rgbd the handle's device view holds mvKeysUn / mDescriptors / mvuRight:
    SearchByProjection(F, local map) gives the same slots and counts through it as through the host
    MatchFrame built from kps_un and uright; it is refused once the handle extracts again; a stereo
    frame's view on another handle is unaffected throughout."""
    from orb_slam3_ros_amd import _lib
    from orb_slam3_ros_amd import synth_match as sm
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd, frame_stereo
    from orb_slam3_ros_amd.matcher import MatchFrame, ORBmatcher, current_frame_view
    from orb_slam3_ros_amd.synth import synth_image, synth_stereo
    lib = _lib.load()
    m = ORBmatcher(0.8)
    # a stereo frame on its own pair of handles, and its view's answer before anything else happens
    sbf, sfx = 0.110078 * 458.654, 458.654
    sl, sr = ORBextractor(1000, 1.2, 8, 20, 7), ORBextractor(1000, 1.2, 8, 20, 7)
    left, right = synth_stereo(5, 640, 480)
    (_, kl, dl), _, sur, _, _ = frame_stereo(sl, sr, left, right, sbf, sfx)
    sid = lib.orbfe_extractor_frame_id(sl.handle)
    SF = MatchFrame(kl, dl, (0.0, 640.0, 0.0, 480.0), np.asarray(sl.GetScaleFactors(), np.float32), sur, sbf)
    rng = np.random.default_rng(8)
    smps = sm.synth_local_map(rng, SF, 1500)
    smvp0, sobs = sm.initial_slots(rng, SF.N)

    def stereo_view_answer():
        V = current_frame_view(SF, sl, sid)
        assert V is not None and V.N == SF.N
        a = smvp0.copy()
        return m.SearchByProjectionLocalMap(V, a, sobs, smps, 3.0), a
    s_before = stereo_view_answer()
    b = smvp0.copy()
    assert s_before[0] == m.SearchByProjectionLocalMap(SF, b, sobs, smps, 3.0) and np.array_equal(s_before[1], b)

    ext = ORBextractor(1000, 1.2, 8, 20, 7)
    img, raw = synth_image(83, 640, 480), depth_u16(550, 640, 480)
    p = tum1(640, 480)
    assert current_frame_view(SF, ext, lib.orbfe_extractor_frame_id(ext.handle)) is None   # no frame yet
    kps, kun, desc, ur, dp = frame_rgbd(ext, img, raw, p)
    fid = lib.orbfe_extractor_frame_id(ext.handle)
    assert (kun["x"] != kps["x"]).mean() > 0.9 and (ur >= 0).sum() > 0.3 * len(kps)
    bounds = (float(np.floor(kun["x"].min())) - 1, float(np.ceil(kun["x"].max())) + 1,
              float(np.floor(kun["y"].min())) - 1, float(np.ceil(kun["y"].max())) + 1)
    F = MatchFrame(kun, desc, bounds, np.asarray(ext.GetScaleFactors(), np.float32), ur, BF)
    V = current_frame_view(F, ext, fid)
    assert V is not None and V.N == F.N == len(kps)
    mps = sm.synth_local_map(rng, F, 1500)
    mvp0, obs = sm.initial_slots(rng, F.N)
    for th in (1.0, 3.0):
        a, b = mvp0.copy(), mvp0.copy()
        na, nb = m.SearchByProjectionLocalMap(V, a, obs, mps, th), m.SearchByProjectionLocalMap(F, b, obs, mps, th)
        assert na == nb and na > 0
        np.testing.assert_array_equal(a, b)
    # the host frame of the DISTORTED keypoints answers differently: the view really holds mvKeysUn
    Fd = MatchFrame(kps, desc, bounds, np.asarray(ext.GetScaleFactors(), np.float32), ur, BF)
    c = mvp0.copy()
    m.SearchByProjectionLocalMap(Fd, c, obs, mps, 1.0)
    a = mvp0.copy()
    m.SearchByProjectionLocalMap(V, a, obs, mps, 1.0)
    assert not np.array_equal(a, c)
    s_mid = stereo_view_answer()
    assert s_mid[0] == s_before[0] and np.array_equal(s_mid[1], s_before[1])
    ext(img, None, (0, 0))   # the handle extracts again: the view is stale
    assert current_frame_view(F, ext, fid) is None
    assert current_frame_view(F, ext, lib.orbfe_extractor_frame_id(ext.handle)) is None   # a plain extract has no view
    s_after = stereo_view_answer()
    assert s_after[0] == s_before[0] and np.array_equal(s_after[1], s_before[1])
    for e in (ext, sl, sr):
        e.close()


def test_handle_reuse(gpu, oracle_lib, small):
    """frame_rgbd, a plain extract, then frame_rgbd at another size, on one handle."""
    from orb_slam3_ros_amd.extractor import ORBextractor, frame_rgbd
    from orb_slam3_ros_amd.synth import synth_image
    imgs, refs = small
    ext = ORBextractor(NFEAT, 1.2, NLEVELS, 20, 7)
    p, raw = tum1(W, H), depth_u16(560, W, H)
    check_frame(oracle_lib, frame_rgbd(ext, imgs[0], raw, p), refs[0], raw, p, "first frame")
    _, k, d = ext(imgs[1], None, (0, 0))
    same_bits(k, refs[1][0], "plain extract")
    assert np.array_equal(d, refs[1][1])
    w2, h2 = 201, 150
    img2 = synth_image(91, w2, h2)
    _, ok, od = oracle_lib.OracleExtractor(NFEAT, 1.2, NLEVELS, 20, 7)(img2)
    p2 = tum1(w2, h2, factor=1.0)
    raw2 = depth_metres(561, w2, h2).astype(np.float32)
    check_frame(oracle_lib, frame_rgbd(ext, img2, raw2, p2), (ok, od), raw2, p2, "frame at another size")
    check_frame(oracle_lib, frame_rgbd(ext, imgs[0], raw, p), refs[0], raw, p, "back at the first size")
    ext.close()
