"""Batched device front-end: extract(L) + extract(R) + the stereo matcher for many stereo frames
per launch sequence (the multi-frame / multi-camera path of BASELINE config 2-4).

Frame f of a batch is images (2f, 2f+1) of one interleaved [2F, H, W] u8 device tensor: this is
the batched form of Frame::Frame(stereo) (Frame.cc:101-197), which runs ORBextractor::operator()
on the left and right image on two threads (Frame.cc:122-125) and then ComputeStereoMatches
(Frame.cc:141, :811-981). Outputs are device tensors in the reference's order (mvKeys,
mDescriptors, mvuRight, mvDepth per frame, padded to `cap`).

stereo="fisheye" is the KannalaBrandt8 constructor (Frame.cc:1007-1075): each side is extracted
with its camera's vLappingArea (Frame.cc:1059-1060) and ComputeStereoFishEyeMatches' descriptor
stage (knnMatch k=2 over the lapping rows + Lowe's 0.7, Frame.cc:1126-1151) runs batched on the
device; `l2r` holds the mvLeftToRightMatch candidates the host-side TriangulateMatches filters.

torch is used only for device memory and streams; all compute is in liborbfe.so.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .extractor import KEYPOINT_DTYPE


def _compute_bow(fe, voc, levelsup, stream):
    """ORBVocabulary.transform_batch over a front end's bound batch outputs (desc, counts)."""
    from .vocabulary import BowBatch
    bows = getattr(fe, "_bows", None)
    if bows is None or (bows.nimg, bows.cap) != (int(fe.desc.shape[0]), fe.cap):
        bows = fe._bows = BowBatch(int(fe.desc.shape[0]), fe.cap, fe.device)
    return voc.transform_batch(fe.desc, fe.counts, levelsup, out=bows, stream=stream)


def _track_reference_keyframe(fe, kps, step, jobs, bows, nnratio, check_ori, stream):
    """ORBmatcher.SearchByBoWSlabs over a front end's slabs (frame f = image f * step) and BowBatch."""
    from .matcher import ORBmatcher
    if bows is None:
        bows = getattr(fe, "_bows", None)
    if bows is None:
        raise _lib.OrbfeError("track_reference_keyframe needs the BowBatch of compute_bow(): none was computed")
    return ORBmatcher(nnratio, check_ori).SearchByBoWSlabs(kps, fe.desc, fe.counts, fe.cap, 0, step, bows, jobs, fe.F,
                                                           stream=stream)


class _SlabRow:
    """orbfe_frame view (device = 1) of one image's slab row: what orbfe_keyframe_create reads of it."""

    def __init__(self, kps_row, desc_row, n):
        from .matcher import CFrame
        self.c = CFrame(n, kps_row.data_ptr(), desc_row.data_ptr(), None, 0.0, 0.0, 0.0, 0.0, 0, None, 0.0, 0, 0, None,
                        None, 1)

    def ref(self):
        return ctypes.byref(self.c)


def _keyframe(fe, kps, img, bows):
    """KeyFrameFeatures of slab image img, copied device to device; only the count and the FeatureVector of
    the image come to the host (which waits for the caller's current torch stream)."""
    from .matcher import KeyFrameFeatures
    n = int(fe.counts[img, 0].cpu())
    if not 0 <= n <= fe.cap:
        raise _lib.OrbfeError(f"image {img} of the batch has a count outside [0, cap]")
    if (bows.nimg, bows.cap) != (int(fe.desc.shape[0]), fe.cap):
        raise ValueError("bows does not hold this front end's images")
    fv = bows.host_feature_vector(img)
    with fe.torch.cuda.device(fe.device):
        return KeyFrameFeatures(_SlabRow(kps[img], fe.desc[img], n), fv)


class StereoFrontEnd:
    """`pipelines` > 1 splits the frames into that many sub-batches, each with its own engine handle
    and HIP stream, so the kernels of different sub-batches overlap on the GPU (the latency-bound
    octree / stereo stages of one sub-batch run beside the streaming stages of another)."""

    def __init__(self, frames: int, width: int, height: int, nfeatures: int = 1000, scale_factor: float = 1.2,
                 nlevels: int = 8, ini_th: int = 20, min_th: int = 7, bf: float = 0.110078 * 458.654,
                 fx: float = 458.654, device=None, pipelines: int = 1, lap_left=(0, 0), lap_right=(0, 0),
                 stereo: str = "rectified", knn_ratio: float = 0.7):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.F, self.W, self.H = int(frames), int(width), int(height)
        self.bf, self.fx = float(bf), float(fx)
        if stereo not in ("rectified", "fisheye", "none"):
            raise ValueError(f"stereo must be 'rectified', 'fisheye' or 'none', not {stereo!r}")
        self.stereo, self.knn_ratio = stereo, float(knn_ratio)
        self.lap_left = (int(lap_left[0]), int(lap_left[1]))
        self.lap_right = (int(lap_right[0]), int(lap_right[1]))
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        P = max(1, min(int(pipelines), self.F))
        bounds = [self.F * i // P for i in range(P + 1)]
        self.parts = [(bounds[i], bounds[i + 1]) for i in range(P) if bounds[i + 1] > bounds[i]]
        self.handles, self.streams = [], []
        for _ in self.parts:
            h = ctypes.c_void_p()
            _lib.check(self.lib.orbfe_extractor_create(nfeatures, scale_factor, nlevels, ini_th, min_th,
                                                       ctypes.byref(h)), "create")
            self.handles.append(h)
            # an explicit stream per pipeline: the library's NULL-stream default is its own
            # non-blocking stream, which torch's default stream would not be ordered against
            self.streams.append(torch.cuda.Stream(self.device))
        self.h = self.handles[0]
        self.cap = _lib.check(self.lib.orbfe_extractor_capacity(self.h, self.W, self.H), "capacity")
        for h in self.handles[1:]:
            self.lib.orbfe_extractor_capacity(h, self.W, self.H)
        n = 2 * self.F
        t = torch
        self.kps = t.zeros((n, self.cap, 7), dtype=t.int32, device=self.device)        # cv::KeyPoint records
        self.desc = t.zeros((n, self.cap, 32), dtype=t.uint8, device=self.device)
        self.counts = t.zeros((n, 2), dtype=t.int32, device=self.device)
        self.uright = t.zeros((self.F, self.cap), dtype=t.float32, device=self.device)
        self.depth = t.zeros((self.F, self.cap), dtype=t.float32, device=self.device)
        self.nmatch = t.zeros((self.F,), dtype=t.int32, device=self.device)
        if stereo == "fisheye":   # mvLeftToRightMatch candidates + their distances
            self.l2r = t.full((self.F, self.cap), -1, dtype=t.int32, device=self.device)
            self.l2r_dist = t.full((self.F, self.cap), -1, dtype=t.int32, device=self.device)
        self.bind_outputs(self.counts, self.kps, self.desc)
        self._ptrs = None
        self._ptr_key = None
        self._stage_on = False
        self._stereo_ev = []

    def bind_outputs(self, counts, kps, desc):
        """Direct the batch outputs (counts [2F,2] i32, keypoints [2F,cap,7] i32, descriptors
        [2F,cap,32] u8, contiguous device tensors) into caller-owned buffers, e.g. the views of a
        distributed.SlabExchange slab; takes effect from the next run()."""
        n, t = 2 * self.F, self.torch
        assert counts.shape == (n, 2) and counts.dtype == t.int32 and counts.is_contiguous()
        assert kps.shape == (n, self.cap, 7) and kps.dtype == t.int32 and kps.is_contiguous()
        assert desc.shape == (n, self.cap, 32) and desc.dtype == t.uint8 and desc.is_contiguous()
        self.counts, self.kps, self.desc = counts, kps, desc
        for h, (a, b) in zip(self.handles, self.parts):
            _lib.check(self.lib.orbfe_set_batch_outputs(h, kps[2 * a].data_ptr(), desc[2 * a].data_ptr(),
                                                        counts[2 * a].data_ptr(), 2 * (b - a)),
                       "set_batch_outputs")

    def _pointer_arrays(self, images):
        key = (images.data_ptr(), tuple(images.shape), tuple(images.stride()))
        if key != self._ptr_key:
            base, st = images.data_ptr(), images.stride(0)
            self._ptrs = [(ctypes.c_void_p * (2 * (b - a)))(*[base + i * st for i in range(2 * a, 2 * b)])
                          for a, b in self.parts]
            self._ptr_key = key
        return self._ptrs

    def run(self, images, stream=None):
        """images: [2F, H, W] uint8 CUDA tensor, contiguous rows (left = even, right = odd).
        stream=None: the work runs on the front end's own torch streams, ordered after and before
        the caller's current stream; otherwise everything is enqueued on `stream` (a hipStream_t)."""
        torch = self.torch
        assert images.dtype == torch.uint8 and images.dim() == 3 and images.is_cuda
        n = images.shape[0]
        assert n == 2 * self.F and images.shape[1] == self.H and images.shape[2] == self.W
        assert images.stride(2) == 1 and images.stride(1) >= self.W
        main = torch.cuda.current_stream(self.device)
        ptrs = self._pointer_arrays(images)
        if stream is None:   # ordered after / before the caller's current torch stream
            ev0 = torch.cuda.Event()
            ev0.record(main)
        for i, (h, st, p, (a, b)) in enumerate(zip(self.handles, self.streams, ptrs, self.parts)):
            if stream is None:
                st.wait_event(ev0)
                s = st.cuda_stream
            else:
                s = stream
            if self.lap_left == self.lap_right:
                _lib.check(self.lib.orbfe_extract_batch(h, 2 * (b - a), p, self.W, self.H, images.stride(1),
                                                        self.lap_left[0], self.lap_left[1], s), "extract_batch")
            else:
                _lib.check(self.lib.orbfe_extract_batch_laps(h, 2 * (b - a), p, self.W, self.H, images.stride(1),
                                                             self._laps(b - a).ctypes.data, s), "extract_batch_laps")
            if self.stereo == "none":
                continue
            timed = self._stage_on and i == 0 and stream is None
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
            if self.stereo == "fisheye":
                _lib.check(self.lib.orbfe_stereo_knn_batch(h, 0, 2, h, 1, 2, b - a, self.knn_ratio,
                                                           self.l2r[a].data_ptr(), self.l2r_dist[a].data_ptr(),
                                                           self.nmatch[a:].data_ptr(), s), "stereo_knn_batch")
            else:
                _lib.check(self.lib.orbfe_stereo_match_batch(h, 0, 2, h, 1, 2, b - a, self.bf, self.fx,
                                                             self.uright[a].data_ptr(), self.depth[a].data_ptr(),
                                                             self.nmatch[a:].data_ptr(), s), "stereo_match_batch")
            if timed:
                e1.record(st)
                self._stereo_ev.append((e0, e1))
        if stream is None:
            for st in self.streams:
                main.wait_stream(st)

    def _laps(self, nframes):
        key = ("laps", nframes)
        if getattr(self, "_lap_key", None) != key:
            self._lap_arr = np.array([*self.lap_left, *self.lap_right] * nframes, np.int32)
            self._lap_key = key
        return self._lap_arr

    def set_opencv_model(self, resize_simd_lanes: int = 16, blur_variant: int = 0):
        """orbfe_extractor_set_opencv_model on every pipeline handle (see ORBextractor.set_opencv_model);
        the handles rebuild their buffers, so the outputs are re-bound."""
        for h in self.handles:
            _lib.check(self.lib.orbfe_extractor_set_opencv_model(h, int(resize_simd_lanes), int(blur_variant)),
                       "set_opencv_model")
            self.lib.orbfe_extractor_capacity(h, self.W, self.H)
        self.bind_outputs(self.counts, self.kps, self.desc)

    def set_stage_timing(self, on: bool):
        for h in self.handles:
            self.lib.orbfe_set_stage_timing(h, 1 if on else 0)
        self._stage_on = bool(on)
        self._stereo_ev = []

    def stage_timing(self):
        """Mean per-batch stage times of the first pipeline (its own stream); "stereo" =
        ComputeStereoMatches (k_stereo + k_stereo_cut), HIP events on the launch stream."""
        ms = np.zeros(_lib.ORBFE_NUM_STAGES, np.float32)
        n = self.lib.orbfe_get_stage_timing(self.handles[0], ms.ctypes.data)
        for h in self.handles[1:]:
            self.lib.orbfe_get_stage_timing(h, np.zeros(_lib.ORBFE_NUM_STAGES, np.float32).ctypes.data)
        out = dict(zip(_lib.STAGE_NAMES, ms.tolist()))
        if self._stereo_ev:
            self.torch.cuda.synchronize(self.device)
            out["stereo"] = float(np.mean([a.elapsed_time(b) for a, b in self._stereo_ev]))
        return out, n

    def host_image(self, i: int):
        """(monoIndex, keypoints (structured), descriptors) of batch image i, copied to the host."""
        n, mono = (int(v) for v in self.counts[i].cpu().numpy())
        kp = self.kps[i, :n].cpu().numpy().view(KEYPOINT_DTYPE).reshape(n)
        return mono, kp, self.desc[i, :n].cpu().numpy()

    def compute_bow(self, voc, levelsup: int = 4, stream=None):
        """Frame::ComputeBoW for all 2F images of the last run(), enqueued on the caller's current
        torch stream (which run() ordered after its own) or on `stream` (a hipStream_t: the one run()
        was given). No host wait. -> vocabulary.BowBatch, allocated once and filled again by later calls."""
        return _compute_bow(self, voc, levelsup, stream)

    def track_motion_model(self, jobs, geom, cam, stream=None, check_ori: bool = True):
        """TrackWithMotionModel's SearchByProjection(CurrentFrame, LastFrame, th, bMono) for all F frames
        of the last run() in one launch, on the left-image slabs (image 2f) and the uright rows of the
        stereo match where run() left them: nothing is copied to the host first. jobs: F matcher.TrackJob
        (pose, last-frame points, th, bForward / bBackward; no points = frame skipped); geom: a MatchFrame
        with the frames' bounds, mbf and scale factors; cam: matcher.CameraModel. stream: the hipStream_t
        run() was given (None: the caller's current torch stream, which run() ordered after its own).
        -> (nmatches [F], n_keys [F], mvp [F, cap]) numpy int32, see ORBmatcher.SearchByProjectionLastFrameBatch."""
        from .matcher import ORBmatcher
        if self.stereo == "fisheye":
            raise _lib.OrbfeError("track_motion_model searches single-camera frames (stereo 'rectified' or 'none')")
        if len(jobs) != self.F:
            raise ValueError(f"one job per frame: {self.F}")
        return ORBmatcher(0.9, check_ori).SearchByProjectionLastFrameBatch(
            self.kps, self.desc, self.counts, self.cap, 0, 2, self.uright if self.stereo == "rectified" else None,
            geom, cam, jobs, stream=stream)

    def track_local_map(self, jobs, geom, mvp, mvp_obs, bFarPoints: bool = False, thFarPoints: float = 50.0,
                        model=None, nnratio: float = 0.8, stream=None):
        """TrackLocalMap's SearchLocalPoints (isInFrustum over each frame's local map points, then
        SearchByProjection(F, mvpLocalMapPoints, th, bFarPoints, thFarPoints)) for all F frames of the last
        run() in one launch, on the slabs track_motion_model reads. jobs: F matcher.LocalMapJob (pose, local
        map points, th, skip indices); mvp / mvp_obs: int32 [F, cap] host arrays, the frames' mvpMapPoints
        after pose optimisation and their Observations(). geom, stream: as track_motion_model.
        -> (nmatches [F], n_to_match [F], n_keys [F], mvp_out [F, cap]), see ORBmatcher.SearchLocalPointsBatch."""
        from .matcher import ORBmatcher
        if self.stereo == "fisheye":
            raise _lib.OrbfeError("track_local_map searches single-camera frames (stereo 'rectified' or 'none')")
        if len(jobs) != self.F:
            raise ValueError(f"one job per frame: {self.F}")
        return ORBmatcher(nnratio).SearchLocalPointsBatch(
            self.kps, self.desc, self.counts, self.cap, 0, 2, self.uright if self.stereo == "rectified" else None,
            geom, jobs, mvp, mvp_obs, bFarPoints, thFarPoints, model=model, stream=stream)

    def track_reference_keyframe(self, jobs, bows=None, nnratio: float = 0.7, check_ori: bool = True, stream=None):
        """TrackReferenceKeyFrame's SearchByBoW(mpReferenceKF, mCurrentFrame, ..) (one job per frame) or
        Relocalization's candidates loop (several jobs per frame) for the frames of the last run() in one
        launch, on the left-image slabs (image 2f) and the FeatureVector rows of compute_bow(): nothing of a
        frame is copied to the host. jobs: a list of (frame, KeyFrameFeatures or None, kf_map_points); bows:
        the BowBatch of compute_bow() (None: the last one). stream: as track_motion_model.
        -> (nmatches [J], n_keys [J], vpMapPointMatches [J, cap]), see ORBmatcher.SearchByBoWSlabs."""
        if self.stereo == "fisheye":
            raise _lib.OrbfeError("track_reference_keyframe searches single-camera frames (stereo 'rectified' or 'none')")
        return _track_reference_keyframe(self, self.kps, 2, jobs, bows, nnratio, check_ori, stream)

    def keyframe(self, f: int, bows):
        """Frame f of the last run() as a matcher.KeyFrameFeatures (the next frames' reference keyframe): its
        left keypoints' angles and descriptors go from the slabs into the keyframe's pack device to device;
        only its count and its FeatureVector (bows: the BowBatch of compute_bow()) are downloaded."""
        return _keyframe(self, self.kps, 2 * int(f), bows)

    def host_frame(self, f: int):
        """(kps_left structured, desc_left, uright, depth) of frame f, copied to the host."""
        _, kp, d = self.host_image(2 * f)
        n = len(kp)
        return kp, d, self.uright[f, :n].cpu().numpy(), self.depth[f, :n].cpu().numpy()

    def close(self):
        for h in self.handles:
            if h:
                self.lib.orbfe_extractor_destroy(h)
        self.handles = []
        self.h = None


class RGBDFrontEnd:
    """Batched device RGB-D front end: orbfe_extract_batch over F gray images, then
    orbfe_rgbd_stereo_batch over their F depth images (the batched form of Frame::Frame(imGray,
    imDepth, ...), Frame.cc:222-237). Outputs are device tensors padded to `cap`: kps / desc / counts as
    StereoFrontEnd's, keys_un (mvKeysUn records), uright and depth (mvuRight, mvDepth; slots at or past
    an image's count keep their previous contents)."""

    def __init__(self, frames: int, width: int, height: int, params, nfeatures: int = 1000, scale_factor: float = 1.2,
                 nlevels: int = 8, ini_th: int = 20, min_th: int = 7, device=None):
        import torch
        self.torch, self.lib, self.params = torch, _lib.load(), params
        self.F, self.W, self.H = int(frames), int(width), int(height)
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        h = ctypes.c_void_p()
        _lib.check(self.lib.orbfe_extractor_create(nfeatures, scale_factor, nlevels, ini_th, min_th, ctypes.byref(h)),
                   "create")
        self.h = h
        self.cap = _lib.check(self.lib.orbfe_extractor_capacity(h, self.W, self.H), "capacity")
        t, n = torch, self.F
        self.kps = t.zeros((n, self.cap, 7), dtype=t.int32, device=self.device)
        self.desc = t.zeros((n, self.cap, 32), dtype=t.uint8, device=self.device)
        self.counts = t.zeros((n, 2), dtype=t.int32, device=self.device)
        self.keys_un = t.zeros((n, self.cap, 7), dtype=t.int32, device=self.device)
        self.uright = t.zeros((n, self.cap), dtype=t.float32, device=self.device)
        self.depth = t.zeros((n, self.cap), dtype=t.float32, device=self.device)
        _lib.check(self.lib.orbfe_set_batch_outputs(h, self.kps.data_ptr(), self.desc.data_ptr(),
                                                    self.counts.data_ptr(), n), "set_batch_outputs")

    def run(self, images, depths):
        """images: [F, H, W] uint8, depths: [F, H, W] uint16 or float32 (raw depth), device tensors with
        contiguous pixels in a row. Runs on the caller's current torch stream. Returns (uright, depth,
        keys_un)."""
        torch = self.torch
        assert images.dtype == torch.uint8 and images.is_cuda and tuple(images.shape) == (self.F, self.H, self.W)
        assert depths.is_cuda and tuple(depths.shape) == (self.F, self.H, self.W)
        assert images.stride(2) == 1 and depths.stride(2) == 1, (images.stride(), depths.stride())
        if depths.dtype == torch.float32:
            dt = _lib.ORBFE_DEPTH_F32
        elif depths.dtype in (torch.uint16, torch.int16):   # int16: a reinterpreted CV_16U buffer
            dt = _lib.ORBFE_DEPTH_U16
        else:
            raise _lib.OrbfeError("the depth tensor is uint16 (CV_16UC1) or float32 (CV_32FC1)")
        s = torch.cuda.current_stream(self.device).cuda_stream
        ip = (ctypes.c_void_p * self.F)(*[images[i].data_ptr() for i in range(self.F)])
        dptr = (ctypes.c_void_p * self.F)(*[depths[i].data_ptr() for i in range(self.F)])
        _lib.check(self.lib.orbfe_extract_batch(self.h, self.F, ip, self.W, self.H, images.stride(1), 0, 0, s),
                   "extract_batch")
        _lib.check(self.lib.orbfe_rgbd_stereo_batch(self.h, 0, 1, self.F, dptr, dt,
                                                    depths.stride(1) * depths.element_size(), self.params.ref(),
                                                    self.keys_un.data_ptr(), self.uright.data_ptr(),
                                                    self.depth.data_ptr(), s), "rgbd_stereo_batch")
        return self.uright, self.depth, self.keys_un

    def compute_bow(self, voc, levelsup: int = 4, stream=None):
        """Frame::ComputeBoW for all F images of the last run(), on the caller's current torch stream
        (run()'s) or on `stream`. No host wait. -> vocabulary.BowBatch, allocated once and reused."""
        return _compute_bow(self, voc, levelsup, stream)

    def track_local_map(self, jobs, geom, mvp, mvp_obs, bFarPoints: bool = False, thFarPoints: float = 50.0,
                        nnratio: float = 0.8, stream=None):
        """StereoFrontEnd.track_local_map for the F RGB-D frames of the last run(): the search reads the
        undistorted keypoints (keys_un = mvKeysUn) and the mvuRight rows made from depth. Runs after the
        caller's current torch stream (run()'s) or `stream`.
        -> (nmatches [F], n_to_match [F], n_keys [F], mvp_out [F, cap])."""
        from .matcher import ORBmatcher
        if len(jobs) != self.F:
            raise ValueError(f"one job per frame: {self.F}")
        return ORBmatcher(nnratio).SearchLocalPointsBatch(
            self.keys_un, self.desc, self.counts, self.cap, 0, 1, self.uright, geom, jobs, mvp, mvp_obs, bFarPoints,
            thFarPoints, stream=stream)

    def track_reference_keyframe(self, jobs, bows=None, nnratio: float = 0.7, check_ori: bool = True, stream=None):
        """StereoFrontEnd.track_reference_keyframe for the F RGB-D frames of the last run() (image f, the
        undistorted keypoints). Runs after the caller's current torch stream (run()'s) or `stream`.
        -> (nmatches [J], n_keys [J], vpMapPointMatches [J, cap])."""
        return _track_reference_keyframe(self, self.keys_un, 1, jobs, bows, nnratio, check_ori, stream)

    def keyframe(self, f: int, bows):
        """StereoFrontEnd.keyframe for RGB-D frame f (mvKeysUn and mDescriptors of image f)."""
        return _keyframe(self, self.keys_un, int(f), bows)

    def host_frame(self, f: int):
        """(mvKeys, mvKeysUn, mDescriptors, mvuRight, mvDepth) of frame f, copied to the host."""
        n = int(self.counts[f, 0].cpu())
        kp = self.kps[f, :n].cpu().numpy().view(KEYPOINT_DTYPE).reshape(n)
        ku = self.keys_un[f, :n].cpu().numpy().view(KEYPOINT_DTYPE).reshape(n)
        return kp, ku, self.desc[f, :n].cpu().numpy(), self.uright[f, :n].cpu().numpy(), self.depth[f, :n].cpu().numpy()

    def close(self):
        if self.h:
            self.lib.orbfe_extractor_destroy(self.h)
            self.h = None
