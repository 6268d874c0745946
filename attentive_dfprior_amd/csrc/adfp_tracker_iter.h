// adfp_tracker_iter.h -- the Tracker's per-iteration glue on the device (reference src/Tracker.py:75-134,
// Tracker.optimize_cam_in_batch), so that one camera-tracking iteration is a fixed sequence of kernels with no host read-back and
// can be replayed from a HIP graph (tracking.TrackerIteration), like adfp_mapper_iter.h does for the Mapper:
//
//   k_camera_from_tensor(_bwd)   quaternion + translation -> camera-to-world and back (src/common.py:139-178)
//   k_select_pixels              the sampled pixels' coordinates, sensor depth and colour (src/common.py:94-124)
//   k_sample_keyframes           the same and the rays, for every keyframe of the Mapper's window
//   k_tracker_loss               the tracking loss with its median-based outlier mask and the cotangents (src/Tracker.py:116-129)
//   k_keep_best                  the running "candidate_cam_tensor" of the iteration loop (src/Tracker.py:261-263)
//   k_tracker_head               one workgroup: camera tensor -> c2w, the drawn pixels, their rays, the pre-filter and its max depth
//   k_tracker_tail               one workgroup: ray cotangents -> g_c2w -> g_cam [-> keep-best, the Adam preparation and step]
//
// and their entries, at the end.  Head and tail merge the steps that are also entries of their own (adfp_select_pixels,
// adfp_rays_from_uv, adfp_prefilter_mask; adfp_rays_from_uv_backward, adfp_camera_from_tensor_backward, adfp_track_keep_best,
// adfp_adam_prep, adfp_masked_adam_multi on the 7 pose parameters) by calling the same functions of adfp_camera.h, so the two routes
// are equal bit for bit.  The render forward / backward with ray gradients between head and tail is the existing entry.
#pragma once
#include "adfp_device.h"
#include "adfp_camera.h"
#include "adfp_mapper_iter.h"    // AdamPrepArgs, adam_prep_group

__global__ void k_camera_from_tensor(const float* __restrict__ cam, float* __restrict__ c2w) {
    if (blockIdx.x || threadIdx.x) return;
    camera_from_tensor_dev(cam, c2w);
}
__global__ void k_camera_from_tensor_bwd(const float* __restrict__ cam, const float* __restrict__ g_c2w, float* __restrict__ g_cam) {
    if (blockIdx.x || threadIdx.x) return;
    camera_from_tensor_bwd_dev(cam, g_c2w, g_cam);
}

__global__ __launch_bounds__(256) void k_select_pixels(const long long* __restrict__ idx, int n, int H0, int W0, int Ww, int W,
                                                       const float* __restrict__ depth, const float* __restrict__ color,
                                                       float* __restrict__ pi, float* __restrict__ pj, float* __restrict__ gd, float* __restrict__ gc) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    gd[t] = window_sample(idx[t], H0, W0, Ww, W, depth, color, pi[t], pj[t], gc + 3 * t);
}

// The pixels and their rays for every keyframe of the Mapper's window in one launch (adfp_sample_keyframes): thread t = ray t % n
// of frame t / n, with the frame's pose from device memory (c2w[f]) or, where that is null, from the launch's arguments (pose[f]).
struct KeyframeJobs {
    const long long* idx[ADFP_KEYFRAMES_MAX]; const float* c2w[ADFP_KEYFRAMES_MAX]; const float* depth[ADFP_KEYFRAMES_MAX];
    const float* color[ADFP_KEYFRAMES_MAX]; float pose[ADFP_KEYFRAMES_MAX][12];
    int n_frames, n, H0, W0, Ww, W; float fx, fy, cx, cy;
    float* ro; float* rd; float* gd; float* gc;
};
__global__ __launch_bounds__(256) void k_sample_keyframes(KeyframeJobs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_frames * a.n) return;
    const int f = t / a.n;
    float pi, pj, c2w[12];
    a.gd[t] = window_sample(a.idx[f][t - f * a.n], a.H0, a.W0, a.Ww, a.W, a.depth[f], a.color[f], pi, pj, a.gc + 3 * t);
#pragma unroll
    for (int m = 0; m < 12; ++m) c2w[m] = a.c2w[f] ? a.c2w[f][m] : a.pose[f][m];
    ray_from_uv(pi, pj, a.fx, a.fy, a.cx, a.cy, c2w, a.ro + 3 * t, a.rd + 3 * t);
}

// loss = sum_mask |gt_d - d| / sqrt(unc + 1e-10)  +  w_color sum_mask |gt_c - c|,   mask = kept & (gt_d > 0) [& tmp < 10 median(tmp)]
// (handle_dynamic; torch.median = the lower middle element of the kept rays' tmp).  ONE workgroup: tracking batches are a few
// hundred to a few thousand rays.  uncertainty is detached in the reference (:115), so it gets no cotangent.
//
// The median is a radix SELECT over the values' bit patterns (tmp >= 0, so the IEEE-754 bits order like the values): ten bits
// per pass from the top, a 1 024-bin LDS histogram of the candidates that still share the selected prefix, one workgroup scan to
// find the bin holding the wanted rank.  The value is known as soon as one candidate is left (typically after three passes
// for ~1 000 distinct values: 9 exponent bits, then 2 + 8 mantissa bits, ...) or all 64 bits are fixed (ties: equal values, and
// only the VALUE matters).  A rank count over all pairs -- the first version -- cost 47 us at 1 000 rays, VALU-bound on f64
// compares; this is ~5 us.
#define ADFP_TRACK_MAX_RAYS 8192
// k_tracker_loss keeps the kept rays' 64-bit keys in LDS: 8192 x 8 B = 64 KB + a 4 KB histogram + scalars ~ 69 KB of static LDS.
// That is a gfx950 budget (160 KB per workgroup); gfx90a / gfx942 stop at 64 KB -- this library targets gfx950 only (build.sh).
static_assert(ADFP_TRACK_MAX_RAYS * 8 + 1024 * 4 + 16 * 4 + 16 * 8 + 64 <= 160 * 1024, "k_tracker_loss: static LDS beyond the gfx950 workgroup limit");
struct TrackLossArgs {
    int n, handle_dynamic; float w_color;
    const double* depth; const double* unc; const float* color; const float* gd; const float* gc; const unsigned char* keep;
    double* loss; double* g_depth; float* g_color;
};
__global__ __launch_bounds__(1024) void k_tracker_loss(TrackLossArgs a) {
    __shared__ unsigned long long s_key[ADFP_TRACK_MAX_RAYS];
    __shared__ int s_hist[1024];
    __shared__ int s_wtot[16];
    __shared__ double s_part[16];
    __shared__ unsigned long long s_medkey;
    __shared__ int s_kept, s_nan, s_digit, s_want, s_left;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) { s_kept = 0; s_nan = 0; s_medkey = 0ull; }
    __syncthreads();
    int kept = 0, nans = 0;
    for (int i = threadIdx.x; i < a.n; i += 1024) {
        unsigned long long key = ~0ull;                        // a dropped ray sorts last and is never selected
        if (!a.keep || a.keep[i]) {
            const double diff = (double)a.gd[i] - a.depth[i];
            const double t = (diff < 0 ? -diff : diff) / sqrt(a.unc[i] + 1e-10);
            ++kept;
            if (t != t) ++nans;
            key = (unsigned long long)__double_as_longlong(t) & 0x7fffffffffffffffull;      // -0.0 -> +0.0
        }
        s_key[i] = key;
    }
    if (kept) atomicAdd(&s_kept, kept);
    if (nans) atomicAdd(&s_nan, nans);
    __syncthreads();
    const int K = s_kept;
    const bool poisoned = s_nan != 0;                          // torch.median propagates NaN: every comparison with it is false
    if (a.handle_dynamic && K > 0 && !poisoned) {
        unsigned long long prefix = 0ull, fixed = 0ull;        // the selected bits so far and their mask
        int want = (K - 1) >> 1, left = K;
        for (int shift = 54; ; shift -= 10) {
            const int bits = shift >= 0 ? 10 : 10 + shift;     // the last pass takes the remaining 4 bits
            const int sh = shift >= 0 ? shift : 0;
            s_hist[threadIdx.x] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < a.n; i += 1024) {
                const unsigned long long k = s_key[i];
                if (((k ^ prefix) & fixed) == 0ull && k != ~0ull) atomicAdd(&s_hist[(int)((k >> sh) & ((1u << bits) - 1u))], 1);
            }
            __syncthreads();
            // inclusive scan of the 1 024 bins, one per thread
            const int mine = s_hist[threadIdx.x];
            int inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
            if (lane == 63) s_wtot[wv] = inc;
            __syncthreads();
            int base = 0;
            for (int w = 0; w < wv; ++w) base += s_wtot[w];
            inc += base;
            if (mine > 0 && want >= inc - mine && want < inc) { s_digit = threadIdx.x; s_want = want - (inc - mine); s_left = mine; }
            __syncthreads();
            prefix |= (unsigned long long)s_digit << sh;
            fixed |= (unsigned long long)((1u << bits) - 1u) << sh;
            want = s_want; left = s_left;
            if (left == 1 || sh == 0) break;
        }
        // the candidates that are left all carry the median's value (one candidate, or equal values): any of them writes it
        for (int i = threadIdx.x; i < a.n; i += 1024) {
            const unsigned long long k = s_key[i];
            if (((k ^ prefix) & fixed) == 0ull && k != ~0ull) s_medkey = k;
        }
        __syncthreads();
    }
    const double med = poisoned ? (double)NAN : __longlong_as_double((long long)s_medkey);
    const double lim = 10.0 * med;
    double part = 0.0;
    for (int i = threadIdx.x; i < a.n; i += 1024) {
        const bool k_ = !a.keep || a.keep[i];
        double g = 0.0;
        float gcol[3] = {0.f, 0.f, 0.f};
        if (k_ && a.gd[i] > 0.f) {
            const double diff = (double)a.gd[i] - a.depth[i];
            const double rs = sqrt(a.unc[i] + 1e-10);
            const double t = (diff < 0 ? -diff : diff) / rs;
            if (!a.handle_dynamic || t < lim) {
                part += t;
                g = (diff > 0 ? -1.0 : (diff < 0 ? 1.0 : 0.0)) / rs;
                for (int c = 0; c < 3; ++c) {
                    const float dc = a.gc[3 * i + c] - a.color[3 * i + c];
                    part += (double)(a.w_color * fabsf(dc));
                    gcol[c] = -a.w_color * (dc > 0.f ? 1.f : (dc < 0.f ? -1.f : 0.f));
                }
            }
        }
        a.g_depth[i] = g;
        a.g_color[3 * i] = gcol[0]; a.g_color[3 * i + 1] = gcol[1]; a.g_color[3 * i + 2] = gcol[2];
    }
    part = wave_sum(part);
    if (lane == 0) s_part[wv] = part;
    __syncthreads();
    if (threadIdx.x == 0 && a.loss) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += s_part[w];
        *a.loss = s;
    }
}

// if loss < best_loss: best_loss = loss, best_cam = cam   (NaN compares false, like the reference's `if loss < current_min_loss`)
__global__ void k_keep_best(const double* __restrict__ loss, const float* __restrict__ cam, double* __restrict__ best_loss, float* __restrict__ best_cam) {
    if (blockIdx.x || threadIdx.x >= 7) return;
    const bool better = *loss < *best_loss;
    const float v = cam[threadIdx.x];
    __syncthreads();                               // every lane has read best_loss before lane 0 overwrites it
    if (!better) return;
    best_cam[threadIdx.x] = v;
    if (threadIdx.x == 0) *best_loss = *loss;
}

// ---- the Tracker iteration's head and tail, one workgroup each ---------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_tracker_head(adfp_tracker_head_args a) {
    float c2w[16];
    camera_from_tensor_dev(a.cam, c2w);                     // every thread: 30 operations, the same values
    if (threadIdx.x < 16) a.c2w[threadIdx.x] = c2w[threadIdx.x];
    double b[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) b[k] = a.bound[k];
    float mx = -INFINITY;
    for (int t = threadIdx.x; t < a.n; t += 1024) {
        float pi, pj, ro[3], rd[3];
        const float dep = window_sample(a.idx[t], a.H0, a.W0, a.W1 - a.W0, a.W, a.depth_img, a.color_img, pi, pj, a.gt_color + 3 * t);
        a.pix_i[t] = pi; a.pix_j[t] = pj; a.gt_depth[t] = dep;
        ray_from_uv(pi, pj, a.fx, a.fy, a.cx, a.cy, c2w, ro, rd);
#pragma unroll
        for (int m = 0; m < 3; ++m) { a.rays_d[3 * t + m] = rd[m]; a.rays_o[3 * t + m] = ro[m]; }
        const bool k_ = ray_in_bound(b, ro, rd, dep);
        a.keep[t] = k_ ? 1 : 0;
        if (k_) mx = dep > mx ? dep : mx;
    }
    kept_depth_max_1024(mx, a.depth_max);
}
__global__ __launch_bounds__(256) void k_tracker_tail(adfp_tracker_tail_args a) {
    __shared__ float s[4][12];
    __shared__ float s_g[16];
    const float v = ray_cotangents_to_c2w(a.pix_i, a.pix_j, a.n, a.fx, a.fy, a.cx, a.cy, a.g_rays_o, a.g_rays_d, s);
    if (threadIdx.x < 16) { s_g[threadIdx.x] = v; a.g_c2w[threadIdx.x] = v; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // one thread from here on: 7 parameters
    float g_cam[7];
    camera_from_tensor_bwd_dev(a.cam, s_g, g_cam);
#pragma unroll
    for (int k = 0; k < 7; ++k) a.g_cam[k] = g_cam[k];
    if (!a.step) return;
    const bool better_before = *a.loss < *a.best_loss;
    if (a.n_groups == 2 && better_before) {                 // separate learning rates: the candidate is kept BEFORE the step
#pragma unroll
        for (int k = 0; k < 7; ++k) a.best_cam[k] = a.cam[k];
        *a.best_loss = *a.loss;
    }
    AdamPrepArgs pa;
    pa.steps = a.steps; pa.derived = a.derived; pa.n = a.n_groups; pa.beta1 = a.beta1; pa.beta2 = a.beta2; pa.skip = a.skip_flag;
    for (int g = 0; g < ADFP_ADAM_MAX_GROUPS; ++g) pa.lr[g] = g < a.n_groups ? a.lr[g] : -1.f;
    for (int g = 0; g < a.n_groups; ++g) adam_prep_group(pa, g);
    for (int g = 0; g < a.n_groups; ++g) {                  // two groups: the translation (4..6), then the quaternion (0..3)
        const int off = a.n_groups == 2 ? (g == 0 ? 4 : 0) : 0, cnt = a.n_groups == 2 ? (g == 0 ? 3 : 4) : 7;
        pose_adam(a.cam, a.g_cam, a.exp_avg, a.exp_avg_sq, off, cnt, a.derived[2 * g], a.derived[2 * g + 1], a.beta1, a.beta2, a.eps);
    }
    if (a.n_groups == 1 && better_before) {                 // one group: kept after the step, the stepped pose with this iteration's loss
#pragma unroll
        for (int k = 0; k < 7; ++k) a.best_cam[k] = a.cam[k];
        *a.best_loss = *a.loss;
    }
}

extern "C" int adfp_tracker_head(const adfp_tracker_head_args* a, void* stream) {
    if (!a || a->n < 0 || bad_window(a->H0, a->H1, a->W0, a->W1, a->H, a->W)) return ADFP_E_ARG;
    if (!a->cam || !a->c2w || !a->bound || !a->keep || !a->depth_max) return ADFP_E_ARG;
    if (a->n > 0 && (!a->idx || !a->depth_img || !a->color_img || !a->pix_i || !a->pix_j || !a->gt_depth || !a->gt_color || !a->rays_o || !a->rays_d)) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_tracker_head, dim3(1), dim3(1024), 0, (hipStream_t)stream, *a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_tracker_tail(const adfp_tracker_tail_args* a, void* stream) {
    if (!a || a->n < 0 || !a->cam || !a->g_c2w || !a->g_cam) return ADFP_E_ARG;
    if (a->n > 0 && (!a->pix_i || !a->pix_j)) return ADFP_E_ARG;
    if (a->step && (!a->exp_avg || !a->exp_avg_sq || !a->steps || !a->derived || a->n_groups < 1 || a->n_groups > 2 || !a->loss || !a->best_loss || !a->best_cam))
        return ADFP_E_ARG;
    hipLaunchKernelGGL(k_tracker_tail, dim3(1), dim3(256), 0, (hipStream_t)stream, *a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_camera_from_tensor(const float* cam, float* c2w, void* stream) {
    if (!cam || !c2w) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_camera_from_tensor, dim3(1), dim3(64), 0, (hipStream_t)stream, cam, c2w);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_camera_from_tensor_backward(const float* cam, const float* g_c2w, float* g_cam, void* stream) {
    if (!cam || !g_c2w || !g_cam) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_camera_from_tensor_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, cam, g_c2w, g_cam);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_select_pixels(const long long* idx, int n, int H0, int H1, int W0, int W1, int H, int W, const float* depth_img, const float* color_img,
                                  float* pix_i, float* pix_j, float* gt_depth, float* gt_color, void* stream) {
    if (n < 0 || bad_window(H0, H1, W0, W1, H, W)) return ADFP_E_ARG;
    if (n == 0) return 0;
    if (!idx || !depth_img || !color_img || !pix_i || !pix_j || !gt_depth || !gt_color) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_select_pixels, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, n, H0, W0, W1 - W0, W, depth_img, color_img,
                       pix_i, pix_j, gt_depth, gt_color);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_sample_keyframes(int n_frames, const adfp_keyframe* frames, int n, int H0, int H1, int W0, int W1, int H, int W, float fx, float fy,
                                     float cx, float cy, float* rays_o, float* rays_d, float* gt_depth, float* gt_color, void* stream) {
    if (n_frames < 0 || n_frames > ADFP_KEYFRAMES_MAX || n < 0 || bad_window(H0, H1, W0, W1, H, W)) return ADFP_E_ARG;
    if (n_frames == 0 || n == 0) return 0;
    if (!frames || !rays_o || !rays_d || !gt_depth || !gt_color) return ADFP_E_ARG;
    if ((long long)n_frames * n > 0x7fffffffll) return ADFP_E_UNSUPPORTED;
    KeyframeJobs a;
    for (int f = 0; f < ADFP_KEYFRAMES_MAX; ++f) {
        const adfp_keyframe& k = frames[f < n_frames ? f : 0];
        if (f < n_frames && (!k.idx || !k.depth_img || !k.color_img)) return ADFP_E_ARG;
        a.idx[f] = k.idx; a.c2w[f] = k.c2w; a.depth[f] = k.depth_img; a.color[f] = k.color_img;
        for (int m = 0; m < 12; ++m) a.pose[f][m] = k.c2w_host[m];
    }
    a.n_frames = n_frames; a.n = n; a.H0 = H0; a.W0 = W0; a.Ww = W1 - W0; a.W = W; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.ro = rays_o; a.rd = rays_d; a.gd = gt_depth; a.gc = gt_color;
    hipLaunchKernelGGL(k_sample_keyframes, dim3((n_frames * n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_track_keep_best(const double* loss, const float* cam, double* best_loss, float* best_cam, void* stream) {
    if (!loss || !cam || !best_loss || !best_cam) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_keep_best, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, cam, best_loss, best_cam);
    ADFP_CHECK_LAUNCH();
    return 0;
}
extern "C" int adfp_tracker_loss(const adfp_track_loss_args* l, void* stream) {
    if (!l || !l->depth || !l->uncertainty || !l->color || !l->gt_depth || !l->gt_color || !l->g_depth || !l->g_color || !l->loss || l->n_rays < 0) return ADFP_E_ARG;
    if (l->n_rays > ADFP_TRACK_MAX_RAYS) return ADFP_E_UNSUPPORTED;
    TrackLossArgs a;
    a.n = l->n_rays; a.handle_dynamic = l->handle_dynamic; a.w_color = l->w_color_loss;
    a.depth = l->depth; a.unc = l->uncertainty; a.color = l->color; a.gd = l->gt_depth; a.gc = l->gt_color; a.keep = l->keep;
    a.loss = l->loss; a.g_depth = l->g_depth; a.g_color = l->g_color;
    hipLaunchKernelGGL(k_tracker_loss, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
