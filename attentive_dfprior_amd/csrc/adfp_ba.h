// adfp_ba.h -- the Mapper's bundle adjustment on the device: the poses of the optimisation window's frames as parameters of the
// Mapper's Adam (the reference's parent project does this under mapping.BA; the reference dropped the code and left
// `camera_tensor_id = 0` at src/Mapper.py:413).  Batched glue around the fused Mapper iteration (mapping.MapperIteration):
//
//   k_ba_head                 per window frame: camera tensor -> c2w (k_camera_from_tensor) or the stored pose of the fixed frame,
//                             then the frame's n drawn pixels, their rays, sensor depth and colour (k_sample_keyframes)
//   k_ba_tail                 per window frame (one workgroup each): its rays' cotangents -> g_c2w (k_rays_from_uv_bwd) -> g_cam
//                             (k_camera_from_tensor_bwd) [-> the Adam step of its 7 parameters]
//   k_cameras_from_tensors    camera tensors -> c2w at F destinations (the write-back into the keyframe store's rows)
//
// The arithmetic is that of the per-frame kernels named above, operation by operation and in their summation order, so the
// results are equal bit for bit to calling those entries frame by frame, and reproducible from run to run.
#pragma once
#include "adfp_device.h"

__global__ __launch_bounds__(256) void k_ba_head(adfp_ba_head_args a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_frames * a.n) return;
    const int f = t / a.n, r = t - f * a.n;
    const adfp_ba_frame& fr = a.frames[f];
    float c2w[16];
    if (fr.free_pose) {
        camera_from_tensor_dev(a.cam + 7 * f, c2w);
    } else {                                                // the gauge: the stored matrix verbatim
#pragma unroll
        for (int m = 0; m < 16; ++m) c2w[m] = fr.c2w[m];
    }
    if (r == 0) {
#pragma unroll
        for (int m = 0; m < 16; ++m) a.c2w[16 * f + m] = c2w[m];
    }
    // k_sample_keyframes
    const int Ww = a.W1 - a.W0;
    const long long k = fr.idx[r];
    const int row = a.H0 + (int)(k / Ww), col = a.W0 + (int)(k % Ww);
    const long long p = (long long)row * a.W + col;
    a.gt_depth[t] = fr.depth_img[p];
    a.gt_color[3 * t] = fr.color_img[3 * p]; a.gt_color[3 * t + 1] = fr.color_img[3 * p + 1]; a.gt_color[3 * t + 2] = fr.color_img[3 * p + 2];
    const float pi = (float)col, pj = (float)row;
    a.pix_i[t] = pi; a.pix_j[t] = pj;
    const float dx = (pi - a.cx) / a.fx, dy = -(pj - a.cy) / a.fy, dz = -1.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        a.rays_d[3 * t + m] = __fadd_rn(__fadd_rn(__fmul_rn(dx, c2w[4 * m]), __fmul_rn(dy, c2w[4 * m + 1])), __fmul_rn(dz, c2w[4 * m + 2]));
        a.rays_o[3 * t + m] = c2w[4 * m + 3];
    }
}

// Workgroup f reduces rows [f n, (f + 1) n) with k_tracker_tail's partition (thread j takes rows j, j + 256, ... of the segment, then
// wave_sum, then the four waves' sums pairwise), so frame f's g_c2w / g_cam are what the single-frame entries give for that segment.
__global__ __launch_bounds__(256) void k_ba_tail(adfp_ba_tail_args a) {
    __shared__ float s[4][12];
    __shared__ float s_g[16];
    const int f = blockIdx.x;
    if (!a.free_flags[f]) {                     // the fixed frame: no gradient, tensor and moments untouched
        if (threadIdx.x < 16) a.g_c2w[16 * f + threadIdx.x] = 0.f;
        if (threadIdx.x < 7) a.g_cam[7 * f + threadIdx.x] = 0.f;
        return;
    }
    const long long base = (long long)f * a.n;
    const float* pix_i = a.pix_i + base; const float* pix_j = a.pix_j + base;
    const float* g_o = a.g_rays_o + 3 * base; const float* g_d = a.g_rays_d + 3 * base;
    float acc[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) acc[t] = 0.f;
    for (int i = threadIdx.x; i < a.n; i += 256) {
        const float dir[3] = {(pix_i[i] - a.cx) / a.fx, -(pix_j[i] - a.cy) / a.fy, -1.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gd = g_d[3 * i + k];
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[4 * k + m] = fmaf(gd, dir[m], acc[4 * k + m]);
            acc[4 * k + 3] += g_o[3 * i + k];
        }
    }
#pragma unroll
    for (int t = 0; t < 12; ++t) acc[t] = wave_sum(acc[t]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < 12; ++t) s[threadIdx.x >> 6][t] = acc[t];
    __syncthreads();
    if (threadIdx.x < 16) {
        const float v = threadIdx.x < 12 ? (s[0][threadIdx.x] + s[1][threadIdx.x]) + (s[2][threadIdx.x] + s[3][threadIdx.x]) : 0.f;
        s_g[threadIdx.x] = v; a.g_c2w[16 * f + threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // one thread from here on: 7 parameters
    float* cam = a.cam + 7 * f;
    float* g_cam = a.g_cam + 7 * f;
    float g[7];
    camera_from_tensor_bwd_dev(cam, s_g, g);
#pragma unroll
    for (int k = 0; k < 7; ++k) g_cam[k] = g[k];
    if (!a.step || (a.skip_flag && *a.skip_flag)) return;
    const float step_size = a.derived[0], sqrt_bc2 = a.derived[1];
    if (sqrt_bc2 == 0.f) return;                            // adam_prep_group's "skip this iteration"
    AdamArgs ad;
    ad.param = cam; ad.grad = g_cam; ad.exp_avg = a.exp_avg + 7 * f; ad.exp_avg_sq = a.exp_avg_sq + 7 * f; ad.mask = nullptr;
    ad.nvox = 7; ad.C = 1; ad.beta1 = a.beta1; ad.beta2 = a.beta2; ad.eps = a.eps; ad.step_size = 0.f; ad.sqrt_bc2 = 1.f; ad.derived = nullptr;
    for (int k = 0; k < 7; ++k) adam_one(ad, k, step_size, sqrt_bc2);
}

struct CamerasJobs { const float* cam; float* dst[ADFP_KEYFRAMES_MAX]; int n_frames; };
__global__ void k_cameras_from_tensors(CamerasJobs a) {
    const int f = threadIdx.x;
    if (blockIdx.x || f >= a.n_frames || !a.dst[f]) return;
    camera_from_tensor_dev(a.cam + 7 * f, a.dst[f]);
}

extern "C" int adfp_ba_head(const adfp_ba_head_args* a, void* stream) {
    if (!a || a->n_frames < 1 || a->n_frames > ADFP_KEYFRAMES_MAX || a->n < 1) return ADFP_E_ARG;
    if (a->H0 < 0 || a->W0 < 0 || a->H1 > a->H || a->W1 > a->W || a->H1 <= a->H0 || a->W1 <= a->W0) return ADFP_E_ARG;
    if (!a->cam || !a->c2w || !a->pix_i || !a->pix_j || !a->rays_o || !a->rays_d || !a->gt_depth || !a->gt_color) return ADFP_E_ARG;
    for (int f = 0; f < a->n_frames; ++f) {
        const adfp_ba_frame& k = a->frames[f];
        if (!k.idx || !k.depth_img || !k.color_img || (!k.free_pose && !k.c2w)) return ADFP_E_ARG;
    }
    if ((long long)a->n_frames * a->n > 0x7fffffffll / 4) return ADFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_ba_head, dim3((a->n_frames * a->n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_ba_tail(const adfp_ba_tail_args* a, void* stream) {
    if (!a || a->n_frames < 1 || a->n_frames > ADFP_KEYFRAMES_MAX || a->n < 1) return ADFP_E_ARG;
    if (!a->pix_i || !a->pix_j || !a->g_rays_o || !a->g_rays_d || !a->cam || !a->g_c2w || !a->g_cam || !a->free_flags) return ADFP_E_ARG;
    if (a->step && (!a->exp_avg || !a->exp_avg_sq || !a->derived)) return ADFP_E_ARG;
    if ((long long)a->n_frames * a->n > 0x7fffffffll / 4) return ADFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_ba_tail, dim3(a->n_frames), dim3(256), 0, (hipStream_t)stream, *a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_cameras_from_tensors(int n_frames, const float* cam, float* const* dst, void* stream) {
    if (n_frames < 1 || n_frames > ADFP_KEYFRAMES_MAX || !cam || !dst) return ADFP_E_ARG;
    CamerasJobs j;
    j.cam = cam; j.n_frames = n_frames;
    for (int f = 0; f < ADFP_KEYFRAMES_MAX; ++f) j.dst[f] = f < n_frames ? dst[f] : nullptr;
    hipLaunchKernelGGL(k_cameras_from_tensors, dim3(1), dim3(64), 0, (hipStream_t)stream, j);
    ADFP_CHECK_LAUNCH();
    return 0;
}
