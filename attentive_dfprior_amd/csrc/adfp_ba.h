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
// Each step is the function of adfp_camera.h that the per-frame kernel named above calls, so the results are equal bit for bit to
// calling those entries frame by frame, and reproducible from run to run.
#pragma once
#include "adfp_device.h"
#include "adfp_camera.h"

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
    float pi, pj;
    a.gt_depth[t] = window_sample(fr.idx[r], a.H0, a.W0, a.W1 - a.W0, a.W, fr.depth_img, fr.color_img, pi, pj, a.gt_color + 3 * t);
    a.pix_i[t] = pi; a.pix_j[t] = pj;
    ray_from_uv(pi, pj, a.fx, a.fy, a.cx, a.cy, c2w, a.rays_o + 3 * t, a.rays_d + 3 * t);
}

// Workgroup f reduces rows [f n, (f + 1) n), so frame f's g_c2w / g_cam are what the single-frame entries give for that segment.
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
    const float v = ray_cotangents_to_c2w(a.pix_i + base, a.pix_j + base, a.n, a.fx, a.fy, a.cx, a.cy, a.g_rays_o + 3 * base, a.g_rays_d + 3 * base, s);
    if (threadIdx.x < 16) { s_g[threadIdx.x] = v; a.g_c2w[16 * f + threadIdx.x] = v; }
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
    pose_adam(cam, g_cam, a.exp_avg + 7 * f, a.exp_avg_sq + 7 * f, 0, 7, a.derived[0], a.derived[1], a.beta1, a.beta2, a.eps);
}

struct CamerasJobs { const float* cam; float* dst[ADFP_KEYFRAMES_MAX]; int n_frames; };
__global__ void k_cameras_from_tensors(CamerasJobs a) {
    const int f = threadIdx.x;
    if (blockIdx.x || f >= a.n_frames || !a.dst[f]) return;
    camera_from_tensor_dev(a.cam + 7 * f, a.dst[f]);
}

extern "C" int adfp_ba_head(const adfp_ba_head_args* a, void* stream) {
    if (!a || a->n_frames < 1 || a->n_frames > ADFP_KEYFRAMES_MAX || a->n < 1) return ADFP_E_ARG;
    if (bad_window(a->H0, a->H1, a->W0, a->W1, a->H, a->W)) return ADFP_E_ARG;
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
