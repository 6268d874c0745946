// adfp_camera.h -- the camera rules that the ray, pre-filter, Tracker, keyframe and bundle-adjustment kernels share: which pixel a
// window index names, the ray through a pixel, the Mapper's bounding-box keep test, the pose gradient taken through the rays, the
// camera tensor <-> camera-to-world maps and the Adam step of a pose.  ONE copy of each: a kernel that fuses several of these steps
// calls the function the single-purpose kernel calls, which is what makes the two equal bit for bit (build.sh compiles with
// -ffp-contract=off, so an inlined function rounds the same wherever it lands).  Device functions only, no kernels and no entries;
// the one host function is the window check at the end.
#pragma once
#include "adfp_device.h"
#include "adfp_mapping.h"        // AdamArgs, adam_one

// pixel k of the window [H0, H0 + Hw) x [W0, W0 + Ww) in row-major order (get_sample_uv's meshgrid flattened, src/common.py:112-124)
ADFP_DEV void window_pixel(long long k, int H0, int W0, int Ww, int& row, int& col) {
    row = H0 + (int)(k / Ww); col = W0 + (int)(k % Ww);
}
// ... its pixel coordinates (pi = column, pj = row), its colour from the [H,W,3] image and, returned, its depth from the [H,W] image
ADFP_DEV float window_sample(long long k, int H0, int W0, int Ww, int W, const float* __restrict__ depth, const float* __restrict__ color,
                             float& pi, float& pj, float* gc /*[3]*/) {
    int row, col;
    window_pixel(k, H0, W0, Ww, row, col);
    pi = (float)col; pj = (float)row;
    const long long p = (long long)row * W + col;
    gc[0] = color[3 * p]; gc[1] = color[3 * p + 1]; gc[2] = color[3 * p + 2];
    return depth[p];
}

// The ray through pixel (pi, pj) (column, row) of the camera c2w (rows 0-2 of a row-major [4,4] or [3,4]): get_rays and
// get_rays_from_uv (src/common.py:254-272, :76-91); also the sample points of the Mapper's keyframe selection (adfp_keyframes.h)
ADFP_DEV void ray_from_uv(float pi, float pj, float fx, float fy, float cx, float cy, const float* __restrict__ c2w, float* ro, float* rd) {
    const float dx = (pi - cx) / fx, dy = -(pj - cy) / fy, dz = -1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // torch.sum(dirs * c2w[:3,:3], -1): products then left-to-right adds
        rd[k] = __fadd_rn(__fadd_rn(__fmul_rn(dx, c2w[4 * k + 0]), __fmul_rn(dy, c2w[4 * k + 1])), __fmul_rn(dz, c2w[4 * k + 2]));
        ro[k] = c2w[4 * k + 3];
    }
}

// The Mapper's bounding-box pre-filter (src/Mapper.py:438-449): keep the ray iff min_axis max_side((bound - o) / d) >= gt_depth, in
// f64; b = {lo, hi} per axis
ADFP_DEV bool ray_in_bound(const double b[6], const float* ro, const float* rd, float depth) {
    double t = INFINITY; bool nan = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double o = (double)ro[k], d = (double)rd[k];
        const double t0 = (b[2 * k] - o) / d, t1 = (b[2 * k + 1] - o) / d;
        nan |= (t0 != t0) | (t1 != t1);            // torch.max / torch.min propagate NaN, and NaN >= depth is false: the ray is dropped
        const double tm = t0 > t1 ? t0 : t1;
        t = tm < t ? tm : t;
    }
    return !nan && (t >= (double)depth);
}
// max over a 1024-thread workgroup of each thread's maximum `mx` of its kept rays' depths (-inf: it kept none), stored by thread 0
ADFP_DEV void kept_depth_max_1024(float mx, float* depth_max) {
    __shared__ float s_m[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float v = __shfl_xor(mx, o); mx = v > mx ? v : mx; }
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = s_m[0];
        for (int w = 1; w < 16; ++w) m = s_m[w] > m ? s_m[w] : m;
        *depth_max = m;
    }
}

// The rays' cotangents -> the camera-to-world's, by a 256-thread workgroup with 4 x 12 floats of LDS:
//   g_c2w[k][m] = sum_n g_d[n][k] * dirs[n][m] (m < 3), g_c2w[k][3] = sum_n g_o[n][k]; row 3 of the 4x4 gets zero.
// Thread j takes rays j, j + 256, ..., then wave_sum, then the four waves' sums pairwise: a fixed order, so the result is
// reproducible from run to run.  Threads 0..15 return g_c2w[thread]; g_o / g_d may be null (= zeros).  Ends after a barrier.
ADFP_DEV float ray_cotangents_to_c2w(const float* __restrict__ pix_i, const float* __restrict__ pix_j, int n, float fx, float fy, float cx, float cy,
                                     const float* __restrict__ g_o, const float* __restrict__ g_d, float (*s)[12]) {
    float acc[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) acc[t] = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float dir[3] = {(pix_i[i] - cx) / fx, -(pix_j[i] - cy) / fy, -1.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gd = g_d ? g_d[3 * i + k] : 0.f;
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[4 * k + m] = fmaf(gd, dir[m], acc[4 * k + m]);
            acc[4 * k + 3] += g_o ? g_o[3 * i + k] : 0.f;
        }
    }
#pragma unroll
    for (int t = 0; t < 12; ++t) acc[t] = wave_sum(acc[t]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int t = 0; t < 12; ++t) s[threadIdx.x >> 6][t] = acc[t];
    __syncthreads();
    return threadIdx.x < 12 ? (s[0][threadIdx.x] + s[1][threadIdx.x]) + (s[2][threadIdx.x] + s[3][threadIdx.x]) : 0.f;
}

// R = I + two_s M(q), two_s = 2 / |q|^2, q = (r, i, j, k): quad2rotation of src/common.py:139-163, float32 like the reference
ADFP_DEV void quat_terms(const float* q, float& two_s, float M[9]) {
    const float qr = q[0], qi = q[1], qj = q[2], qk = q[3];
    two_s = 2.0f / (((qr * qr + qi * qi) + qj * qj) + qk * qk);
    M[0] = -(qj * qj + qk * qk); M[1] = qi * qj - qk * qr;   M[2] = qi * qk + qj * qr;
    M[3] = qi * qj + qk * qr;    M[4] = -(qi * qi + qk * qk); M[5] = qj * qk - qi * qr;
    M[6] = qi * qk - qj * qr;    M[7] = qj * qk + qi * qr;   M[8] = -(qi * qi + qj * qj);
}
// camera tensor (quaternion, translation) -> camera-to-world (get_camera_from_tensor, src/common.py:165-178)
ADFP_DEV void camera_from_tensor_dev(const float* __restrict__ cam, float* c2w /*[16]*/) {
    float two_s, M[9];
    quat_terms(cam, two_s, M);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) c2w[4 * a + b] = (a == b ? 1.0f : 0.0f) + two_s * M[3 * a + b];
        c2w[4 * a + 3] = cam[4 + a];
    }
    c2w[12] = 0.f; c2w[13] = 0.f; c2w[14] = 0.f; c2w[15] = 1.f;
}
// g_cam[0..3] = dL/dq, g_cam[4..6] = dL/dT from dL/d c2w (rows 0-2):
//   dL/dq_m = two_s sum_ab G_ab dM_ab/dq_m - two_s^2 q_m sum_ab G_ab M_ab       (d two_s / d q_m = -two_s^2 q_m)
ADFP_DEV void camera_from_tensor_bwd_dev(const float* __restrict__ cam, const float* g_c2w, float* g_cam) {
    float two_s, M[9], G[9];
    quat_terms(cam, two_s, M);
    float gm = 0.f;
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { G[3 * a + b] = g_c2w[4 * a + b]; gm += G[3 * a + b] * M[3 * a + b]; }
    const float qr = cam[0], qi = cam[1], qj = cam[2], qk = cam[3];
    const float dr = -qk * G[1] + qj * G[2] + qk * G[3] - qi * G[5] - qj * G[6] + qi * G[7];
    const float di = qj * G[1] + qk * G[2] + qj * G[3] - 2.f * qi * G[4] - qr * G[5] + qk * G[6] + qr * G[7] - 2.f * qi * G[8];
    const float dj = -2.f * qj * G[0] + qi * G[1] + qr * G[2] + qi * G[3] + qk * G[5] - qr * G[6] + qk * G[7] - 2.f * qj * G[8];
    const float dk = -2.f * qk * G[0] - qr * G[1] + qi * G[2] + qr * G[3] - 2.f * qk * G[4] + qj * G[5] + qi * G[6] + qj * G[7];
    const float t2 = two_s * two_s * gm;
    g_cam[0] = two_s * dr - t2 * qr; g_cam[1] = two_s * di - t2 * qi; g_cam[2] = two_s * dj - t2 * qj; g_cam[3] = two_s * dk - t2 * qk;
    g_cam[4] = g_c2w[3]; g_cam[5] = g_c2w[7]; g_cam[6] = g_c2w[11];
}

// torch.optim.Adam on parameters [off, off + cnt) of a 7-float camera tensor, by one thread; step_size and sqrt_bc2 are the group's
// pair from adam_prep_group (adfp_mapper_iter.h)
ADFP_DEV void pose_adam(float* cam, const float* g_cam, float* exp_avg, float* exp_avg_sq, int off, int cnt, float step_size, float sqrt_bc2,
                        float beta1, float beta2, float eps) {
    if (sqrt_bc2 == 0.f) return;                            // adam_prep_group's "skip this iteration"
    AdamArgs ad;
    ad.param = cam + off; ad.grad = g_cam + off; ad.exp_avg = exp_avg + off; ad.exp_avg_sq = exp_avg_sq + off; ad.mask = nullptr;
    ad.nvox = cnt; ad.C = 1; ad.beta1 = beta1; ad.beta2 = beta2; ad.eps = eps; ad.step_size = 0.f; ad.sqrt_bc2 = 1.f; ad.derived = nullptr;
    for (int k = 0; k < cnt; ++k) adam_one(ad, k, step_size, sqrt_bc2);
}

// host: is [H0, H1) x [W0, W1) not a non-empty window of an H x W image?
static bool bad_window(int H0, int H1, int W0, int W1, int H, int W) {
    return H0 < 0 || W0 < 0 || H1 > H || W1 > W || H1 <= H0 || W1 <= W0;
}
