// The RGB-D Frame constructor (Frame.cc:200-286) after ExtractORB: UndistortKeyPoints (:747-780) and
// ComputeStereoFromRGBD (:984-1005), with Tracking::GrabImageRGBD's depth conversion
// (imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor), Tracking.cc:1576-1577) applied only to the
// depth values the keypoints read. Included by orbfe_engine.hip after orbfe_remap.hip: it uses the
// extractor handle and undistort_point().
#pragma once

struct RgbdArgs {
    UndistArgs u;
    int undist;            // DistCoef(0) != 0: UndistortKeyPoints runs (else mvKeysUn = mvKeys, Frame.cc:749-753)
    int scale;             // the depth value is multiplied by `factor`
    float bf, factor;
    int width, height;     // the depth image (= the gray image's size)
    int pitch;             // depth row pitch in bytes
    int cap, base, step;   // keypoint slots per image; frame f is image base + f * step of the batch
};

// One thread per keypoint slot of nframes x cap; a slot at or past its image's count is not written.
// depth_tab[f] is frame f's depth image; a NULL table means one frame whose image is depth_one (the
// host call's staged copy).
// One wave per block: a frame's ~1000 keypoints spread over 16 CUs, and the double-precision
// fixed-point iteration of a point is the longest chain of the launch.
template <typename T>
__global__ __launch_bounds__(64) void k_rgbd(const OrbKeyPoint* __restrict__ kps, const int* __restrict__ counts,
                                             const void* const* __restrict__ depth_tab, const void* depth_one,
                                             RgbdArgs a, OrbKeyPoint* keys_un, float* uright, float* depth_out) {
    const int i = blockIdx.x * 64 + threadIdx.x, f = blockIdx.y;
    if (i >= a.cap) return;
    const int img = a.base + f * a.step;
    if (i >= counts[2 * img]) return;
    OrbKeyPoint kp = kps[(size_t)img * a.cap + i];
    // depth at the DISTORTED keypoint, imDepth.at<float>(v, u) with the float -> int truncation of
    // C++ (Frame.cc:994-998); the extractor's keypoints lie inside the image, any other reads as 0
    const int px = (int)kp.x, py = (int)kp.y;
    float d = 0.f;
    if (px >= 0 && px < a.width && py >= 0 && py < a.height) {
        const uint8_t* base = (const uint8_t*)(depth_tab ? depth_tab[f] : depth_one);
        T raw;
        __builtin_memcpy(&raw, base + (size_t)py * a.pitch + (size_t)px * sizeof(T), sizeof(T));
        d = (float)raw;
        if (a.scale) d = d * a.factor;   // convertTo: saturate_cast<float>(x * alpha + 0)
    }
    if (a.undist) undistort_point(a.u, kp.x, kp.y, kp.x, kp.y);
    const size_t o = (size_t)f * a.cap + i;
    if (keys_un) keys_un[o] = kp;
    if (d > 0) {   // NaN and negative depths fail; +inf gives uR = kpU.pt.x
        depth_out[o] = d;
        uright[o] = kp.x - a.bf / d;
    } else {
        depth_out[o] = -1.f;
        uright[o] = -1.f;
    }
}

// The checks of both entry points that need no handle state, and the kernel's arguments.
static int rgbd_args(const orbfe_rgbd_params* p, int depth_type, RgbdArgs& a) {
    if (!p || (depth_type != ORBFE_DEPTH_U16 && depth_type != ORBFE_DEPTH_F32)) return ORBFE_E_ARG;
    if (p->ndist != 0 && p->ndist != 4 && p->ndist != 5 && p->ndist != 8 && p->ndist != 12) return ORBFE_E_ARG;
    const float K4[4] = {p->fx, p->fy, p->cx, p->cy};
    a.u = undist_args(K4, p->dist, p->ndist);
    a.undist = p->ndist > 0 && p->dist[0] != 0.f;
    // CV_16U is always converted; CV_32F only when the factor differs from 1 (Tracking.cc:1576)
    a.scale = depth_type == ORBFE_DEPTH_U16 || fabsf(p->depth_factor - 1.0f) > 1e-5f;
    a.bf = p->bf;
    a.factor = p->depth_factor;
    return ORBFE_OK;
}

static void rgbd_launch(int depth_type, int nframes, hipStream_t s, const OrbKeyPoint* kps, const int* counts,
                        const void* const* depth_tab, const void* depth_one, const RgbdArgs& a, OrbKeyPoint* keys_un,
                        float* uright, float* depth_out) {
    const dim3 grid((a.cap + 63) / 64, nframes);
    if (depth_type == ORBFE_DEPTH_U16)
        hipLaunchKernelGGL(k_rgbd<uint16_t>, grid, dim3(64), 0, s, kps, counts, depth_tab, depth_one, a, keys_un, uright,
                           depth_out);
    else
        hipLaunchKernelGGL(k_rgbd<float>, grid, dim3(64), 0, s, kps, counts, depth_tab, depth_one, a, keys_un, uright,
                           depth_out);
}

extern "C" {

int orbfe_rgbd_stereo_batch(orbfe_extractor* h, int base, int step, int nframes, const void* const* d_depth,
                            int depth_type, int depth_pitch_bytes, const orbfe_rgbd_params* p,
                            orbfe_keypoint* d_keys_un, float* d_uright, float* d_depth_out, void* stream) {
    RgbdArgs a;
    if (!h || nframes < 0) return ORBFE_E_ARG;
    int rc = rgbd_args(p, depth_type, a);
    if (rc) return rc;
    if (nframes == 0) return ORBFE_OK;
    if (!d_depth || !d_uright || !d_depth_out) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = depth_type == ORBFE_DEPTH_U16 ? 2 : 4;
    if (!h->cap_b || !h->last_kps || base < 0 || step < 0 || base + (nframes - 1) * step >= h->last_nimg ||
        depth_pitch_bytes < 0 || (size_t)depth_pitch_bytes < (size_t)h->W * esz)
        return ORBFE_E_ARG;
    for (int f = 0; f < nframes; f++)
        if (!d_depth[f]) return ORBFE_E_ARG;
    hipStream_t s = pick_stream(h, stream);
    // the depth pointer table goes up as the image pointer table of a batch does (run_batch): only
    // when it differs from the last call's, synchronously with respect to the caller's array
    if (h->rg_ptrs_cap < nframes) {
        if (h->d_rg_ptrs) HIPCHK(hipFree(h->d_rg_ptrs));
        h->d_rg_ptrs = nullptr;
        h->rg_ptrs_cap = 0;
        h->last_rg_ptrs.clear();
        HIPCHK(hipMalloc(&h->d_rg_ptrs, (size_t)nframes * sizeof(void*)));
        h->rg_ptrs_cap = nframes;
    }
    if ((int)h->last_rg_ptrs.size() != nframes || !std::equal(d_depth, d_depth + nframes, h->last_rg_ptrs.begin())) {
        h->last_rg_ptrs.assign(d_depth, d_depth + nframes);
        HIPCHK(hipMemcpyAsync(h->d_rg_ptrs, h->last_rg_ptrs.data(), (size_t)nframes * sizeof(void*),
                              hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    a.width = h->W;
    a.height = h->H;
    a.pitch = depth_pitch_bytes;
    a.cap = h->g.kp_cap;
    a.base = base;
    a.step = step;
    rgbd_launch(depth_type, nframes, s, h->last_kps, h->last_counts, h->d_rg_ptrs, nullptr, a,
                (OrbKeyPoint*)d_keys_un, d_uright, d_depth_out);
    HIPCHK(hipGetLastError());
    return ORBFE_OK;
}

int orbfe_frame_rgbd(orbfe_extractor* h, const uint8_t* img, int width, int height, int stride, const void* depth,
                     int depth_type, int depth_stride_bytes, const orbfe_rgbd_params* p, orbfe_keypoint* kps,
                     orbfe_keypoint* kps_un, uint8_t* desc, int cap, int* n, float* uright, float* depth_out) {
    RgbdArgs a;
    if (!h || !n) return ORBFE_E_ARG;
    *n = 0;
    int rc = rgbd_args(p, depth_type, a);
    if (rc) return rc;
    if (!img || width <= 0 || height <= 0) return ORBFE_E_EMPTY;
    const size_t esz = depth_type == ORBFE_DEPTH_U16 ? 2 : 4;
    const size_t drow = (size_t)width * esz, dbytes = drow * height;
    if (stride < width || !depth || depth_stride_bytes < 0 || (size_t)depth_stride_bytes < drow) return ORBFE_E_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    rc = ensure(h, width, height, 1);
    if (rc) return rc;
    hipStream_t s = h->own_stream;
    const size_t bytes = (size_t)width * height;
    // the depth image goes to the device by a DMA copy beside the extraction; the A/B alternative
    // (k_rgbd reading the mapped pinned copy in place) measured 2 % slower per frame
    const bool dma = !h->rgbd_mapped;
    if (h->stage_bytes < bytes) {
        if (h->d_stage) HIPCHK(hipFree(h->d_stage));
        h->d_stage = nullptr;
        h->stage_bytes = 0;
        HIPCHK(hipMalloc(&h->d_stage, bytes));
        h->stage_bytes = bytes;
    }
    if (dma && h->rg_stage_bytes < dbytes) {
        if (h->d_rg_stage) HIPCHK(hipFree(h->d_rg_stage));
        h->d_rg_stage = nullptr;
        h->rg_stage_bytes = 0;
        HIPCHK(hipMalloc(&h->d_rg_stage, dbytes));
        h->rg_stage_bytes = dbytes;
    }
    // device results {mvKeysUn [kc] | mvuRight [kc] | mvDepth [kc]}: they stay for orbfe_frame_device_view
    const int kc = h->g.kp_cap;
    auto a16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t rg_ur = a16((size_t)kc * sizeof(OrbKeyPoint)), rg_bytes = a16(rg_ur + (size_t)kc * 8);
    if (!h->d_rg || h->rg_kp < kc) {
        if (h->d_rg) HIPCHK(hipFree(h->d_rg));
        h->d_rg = nullptr;
        h->d_rg_uright = nullptr;
        h->rg_kp = 0;
        HIPCHK(hipMalloc(&h->d_rg, rg_bytes));
        h->rg_kp = kc;
    }
    OrbKeyPoint* d_un = (OrbKeyPoint*)h->d_rg;
    float* d_ur = h->d_rg_uright = (float*)(h->d_rg + rg_ur);
    float* d_dp = d_ur + kc;
    // pinned: the gray image going up and the one-image output block coming back (as orbfe_extract),
    // then the RGB-D results coming back, then the depth image (tight rows) on its way to the device
    size_t o_kps, o_desc, o_end;
    out_layout(1, kc, &o_kps, &o_desc, &o_end);
    const size_t o_rg = a16(std::max(bytes, o_end)), o_dimg = o_rg + rg_bytes;
    const size_t pin_need = o_dimg + a16(dbytes);
    if (h->pin_bytes < pin_need) {
        if (h->h_pin) HIPCHK(hipHostFree(h->h_pin));
        h->h_pin = nullptr;
        h->pin_bytes = 0;
        HIPCHK(hipHostMalloc((void**)&h->h_pin, pin_need, hipHostMallocMapped | hipHostMallocCoherent));
        h->pin_bytes = pin_need;
    }
    const bool tm = h->timing;
    if (tm && !h->call_ev[0])
        for (auto& e : h->call_ev) HIPCHK(hipEventCreate(&e));
    uint8_t* hp = h->h_pin;
    uint8_t* hpd = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&hpd, hp, 0));
    // the previous call's result copies out of h_pin have completed (that call synchronised)
    if (stride == width) memcpy(hp, img, bytes);
    else
        for (int y = 0; y < height; y++) memcpy(hp + (size_t)y * width, img + (size_t)y * stride, width);
    if (tm) HIPCHK(hipEventRecord(h->call_ev[0], s));
    hipLaunchKernelGGL(k_push, dim3((unsigned)((bytes / 16 + 1 + 255) / 256)), dim3(256), 0, s, (const uint8_t*)hpd,
                       h->d_stage, bytes);
    HIPCHK(hipGetLastError());
    if (tm) HIPCHK(hipEventRecord(h->call_ev[1], s));
    const uint8_t* ptrs[1] = {h->d_stage};
    const int laps[2] = {0, 0};   // ExtractORB(0, imGray, 0, 0) (Frame.cc:223)
    h->timing = false;   // the call's own events bracket the kernels (the stage ring is for batches)
    rc = run_batch(h, 1, ptrs, width, laps, s, false);
    h->timing = tm;
    if (rc) return rc;
    if (tm) HIPCHK(hipEventRecord(h->call_ev[2], s));
    // the depth image into pinned memory while the GPU extracts
    if ((size_t)depth_stride_bytes == drow) memcpy(hp + o_dimg, depth, dbytes);
    else
        for (int y = 0; y < height; y++)
            memcpy(hp + o_dimg + (size_t)y * drow, (const uint8_t*)depth + (size_t)y * depth_stride_bytes, drow);
    const void* dsrc = hpd + o_dimg;
    if (dma) {   // on the side stream, beside the extraction kernels; k_rgbd waits for it
        HIPCHK(hipMemcpyAsync(h->d_rg_stage, hp + o_dimg, dbytes, hipMemcpyHostToDevice, h->side_stream));
        HIPCHK(hipEventRecord(h->ev_fork[0], h->side_stream));
        HIPCHK(hipStreamWaitEvent(s, h->ev_fork[0], 0));
        dsrc = h->d_rg_stage;
    }
    a.width = width;
    a.height = height;
    a.pitch = (int)drow;
    a.cap = kc;
    a.base = 0;
    a.step = 1;
    rgbd_launch(depth_type, 1, s, h->last_kps, h->last_counts, nullptr, dsrc, a, d_un, d_ur, d_dp);
    HIPCHK(hipGetLastError());
    if (tm) HIPCHK(hipEventRecord(h->call_ev[4], s));
    if (h->cap_b == 1) {   // the one-image output block and the RGB-D results: one kernel
        const int n0 = (int)(o_end / 16), n1 = (int)(rg_bytes / 16);
        hipLaunchKernelGGL(k_pull2, dim3((n0 + n1 + 255) / 256), dim3(256), 0, s, (const orbfe_u32x4*)h->d_out,
                           (orbfe_u32x4*)hpd, n0, (const orbfe_u32x4*)h->d_rg, (orbfe_u32x4*)(hpd + o_rg), n1);
        HIPCHK(hipGetLastError());
    } else {   // the handle's buffers are sized for a larger batch: its image-0 parts by copies
        HIPCHK(hipMemcpyAsync(hp, h->last_counts, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp + o_kps, h->last_kps, (size_t)kc * sizeof(OrbKeyPoint), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp + o_desc, h->last_desc, (size_t)kc * 32, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(hp + o_rg, h->d_rg, rg_bytes, hipMemcpyDeviceToHost, s));
    }
    if (tm) HIPCHK(hipEventRecord(h->call_ev[5], s));
    HIPCHK(hipStreamSynchronize(s));
    int cnt[2];
    memcpy(cnt, hp, 8);
    *n = cnt[0];
    if (cnt[0] > cap) return ORBFE_E_CAPACITY;
    // the frame stays in HBM for Tracking's searches (orbfe_frame_device_view)
    h->fs_id = h->frame_id;
    h->fs_n = cnt[0];
    h->fs_rgbd = true;
    if (cnt[0] > 0) {
        const size_t nn = (size_t)cnt[0];
        if (kps) memcpy(kps, hp + o_kps, nn * sizeof(OrbKeyPoint));
        if (desc) memcpy(desc, hp + o_desc, nn * 32);
        if (kps_un) memcpy(kps_un, hp + o_rg, nn * sizeof(OrbKeyPoint));
        if (uright) memcpy(uright, hp + o_rg + rg_ur, nn * 4);
        if (depth_out) memcpy(depth_out, hp + o_rg + rg_ur + (size_t)kc * 4, nn * 4);
    }
    if (tm) {   // {upload, extraction kernels, result copies, k_rgbd (with any wait for the host's depth copy), 0}
        HIPCHK(hipEventElapsedTime(&h->call_ms[0], h->call_ev[0], h->call_ev[1]));
        HIPCHK(hipEventElapsedTime(&h->call_ms[1], h->call_ev[1], h->call_ev[2]));
        HIPCHK(hipEventElapsedTime(&h->call_ms[3], h->call_ev[2], h->call_ev[4]));
        HIPCHK(hipEventElapsedTime(&h->call_ms[2], h->call_ev[4], h->call_ev[5]));
        h->call_ms[4] = 0.f;
    }
    return cnt[1];
}

}  // extern "C"
