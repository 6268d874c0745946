// adfp_keyframes.h -- the Mapper's overlap keyframe selection on the device (the reference's Mapper.keyframe_selection_overlap,
// src/Mapper.py:160-222): how many of the current frame's sample points each keyframe sees.
//
//   points (f32)      pixels * N_samples points along the rays of the drawn pixels, between 0.8 d and d + 0.5 of the pixel's sensor
//                     depth d: the ray is ray_from_uv's (adfp_rays_from_uv, bit for bit), t_vals the renderer's linspace01 (torch's
//                     CPU linspace)
//   test (f32 / f64)  per keyframe: w2c = inv(est_c2w) (f64, rounded to f32), camera coordinates in f32, x negated, projection by
//                     the f64 intrinsics, inside test against the image minus an edge
//
// One launch.  Each workgroup builds the point set (or a chunk of it) once into LDS and takes keyframes w, w + G, w + 2G, ...;
// each wave counts one keyframe at a time over every point with a 64-lane ballot.  The count is written by one lane with a plain
// store: no atomics, so the result does not depend on scheduling.  The exact contract is stated in include/adfp.h.
#pragma once
#include "adfp_device.h"

#define ADFP_KFO_THREADS 256                       // 4 waves
#define ADFP_KFO_WAVES (ADFP_KFO_THREADS / 64)
#define ADFP_KFO_CHUNK 4096                        // points held in LDS at a time: 48 KiB
#define ADFP_KFO_BATCH ADFP_KFO_THREADS            // keyframes inverted per pass, one per thread
#define ADFP_KFO_MAX_GRID 256                      // one workgroup per CU

struct KfoArgs {
    const long long* idx; int n; int S; int P;     // P = n S points; point q = sample q % S of ray q / S
    const float* depth; int H, W;
    const float* c2w;                              // the current pose, row-major [4,4]
    const float* poses; int K;                     // keyframe poses [K][4][4]
    double fx, fy, cx, cy;                         // the projection's intrinsics (f64, like the reference's K)
    float umin, umax, vmin, vmax;                  // edge < u < W - edge, edge < v < H - edge
    int* counts; float* pts_out;
};

// Rows 0-2 of the inverse of the row-major 4x4 m, by 2x2 minors in f64, rounded to f32.  A singular pose gives non-finite values,
// and then no point is inside.
ADFP_DEV void inverse_rows3(const float* __restrict__ m, float* out) {
    double a[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = (double)m[i];
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c0 = a[8] * a[13] - a[12] * a[9], c1 = a[8] * a[14] - a[12] * a[10], c2 = a[8] * a[15] - a[12] * a[11];
    const double c3 = a[9] * a[14] - a[13] * a[10], c4 = a[9] * a[15] - a[13] * a[11], c5 = a[10] * a[15] - a[14] * a[11];
    const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const double b[12] = {a[5] * c5 - a[6] * c4 + a[7] * c3,    -a[1] * c5 + a[2] * c4 - a[3] * c3,
                          a[13] * s5 - a[14] * s4 + a[15] * s3, -a[9] * s5 + a[10] * s4 - a[11] * s3,
                          -a[4] * c5 + a[6] * c2 - a[7] * c1,   a[0] * c5 - a[2] * c2 + a[3] * c1,
                          -a[12] * s5 + a[14] * s2 - a[15] * s1, a[8] * s5 - a[10] * s2 + a[11] * s1,
                          a[4] * c4 - a[5] * c2 + a[7] * c0,    -a[0] * c4 + a[1] * c2 - a[3] * c0,
                          a[12] * s4 - a[13] * s2 + a[15] * s0, -a[8] * s4 + a[9] * s2 - a[11] * s0};
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = (float)(b[i] / det);
}

// Point q of the sample set (src/Mapper.py:179-191), every product and sum rounded on its own (the build has -ffp-contract=off).  A
// drawn index outside the image gives a NaN point, which no keyframe sees.
ADFP_DEV void overlap_point(const KfoArgs& a, int q, float* p) {
    const int r = q / a.S, s = q - r * a.S;
    const long long k = a.idx[r];
    if (k < 0 || k >= (long long)a.H * a.W) { p[0] = p[1] = p[2] = __builtin_nanf(""); return; }
    const int row = (int)(k / a.W), col = (int)(k - (long long)row * a.W);
    float ro[3], rd[3];
    ray_from_uv((float)col, (float)row, (float)a.fx, (float)a.fy, (float)a.cx, (float)a.cy, a.c2w, ro, rd);
    const float d = a.depth[k];
    const float t = linspace01(s, a.S);
    const float near = d * 0.8f, far = d + 0.5f;
    const float z = near * (1.f - t) + far * t;
#pragma unroll
    for (int m = 0; m < 3; ++m) p[m] = ro[m] + rd[m] * z;
}

// Whether keyframe w2c (rows 0-2, f32) sees the point (src/Mapper.py:193-214): camera coordinates in f32 with x negated, then
// u = (fx (-x) + cx z) / (z + 1e-5), v = (fy y + cy z) / (z + 1e-5) in f64, rounded to f32, and z + 1e-5 < 0.
ADFP_DEV bool overlap_inside(const KfoArgs& a, const float* w, float x, float y, float z) {
    float cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = ((w[4 * r] * x + w[4 * r + 1] * y) + w[4 * r + 2] * z) + w[4 * r + 3];
    const double X = -(double)cam[0], Y = (double)cam[1], Z = (double)cam[2];
    const double zz = Z + 1e-5;
    const float u = (float)((a.fx * X + a.cx * Z) / zz), v = (float)((a.fy * Y + a.cy * Z) / zz);
    return u < a.umax && u > a.umin && v < a.vmax && v > a.vmin && zz < 0.0;
}

__global__ __launch_bounds__(ADFP_KFO_THREADS) void k_keyframe_overlap(KfoArgs a) {
    __shared__ float s_p[3][ADFP_KFO_CHUNK];                  // x, y, z of the chunk's points
    __shared__ float s_w2c[ADFP_KFO_BATCH][12];
    __shared__ int s_cnt[ADFP_KFO_BATCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int G = gridDim.x, wg = blockIdx.x;
    const int mine = (a.K - wg + G - 1) / G;                  // this workgroup's keyframes: wg + G m, m < mine
    const int nchunks = (a.P + ADFP_KFO_CHUNK - 1) / ADFP_KFO_CHUNK;
    for (int m0 = 0; m0 < mine; m0 += ADFP_KFO_BATCH) {
        const int nb = mine - m0 < ADFP_KFO_BATCH ? mine - m0 : ADFP_KFO_BATCH;
        if (tid < nb) inverse_rows3(a.poses + 16ll * (wg + (long long)G * (m0 + tid)), s_w2c[tid]);
        for (int ch = 0; ch < nchunks; ++ch) {
            const int q0 = ch * ADFP_KFO_CHUNK, nq = a.P - q0 < ADFP_KFO_CHUNK ? a.P - q0 : ADFP_KFO_CHUNK;
            if (nchunks > 1 || m0 == 0) {                     // one chunk: built once for every batch
                __syncthreads();                              // the previous chunk's counting is done
                const bool emit = a.pts_out && wg == 0 && m0 == 0;
                for (int i = tid; i < nq; i += ADFP_KFO_THREADS) {
                    float p[3];
                    overlap_point(a, q0 + i, p);
                    s_p[0][i] = p[0]; s_p[1][i] = p[1]; s_p[2][i] = p[2];
                    if (emit) {
                        float* o = a.pts_out + 3ll * (q0 + i);
                        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
                    }
                }
            }
            __syncthreads();                                  // the points and this batch's w2c are in LDS
            for (int m = wave; m < nb; m += ADFP_KFO_WAVES) {
                const float* w = s_w2c[m];
                int c = 0;                                    // wave-uniform
                for (int i0 = 0; i0 < nq; i0 += 64) {
                    const int i = i0 + lane;
                    const bool in = i < nq && overlap_inside(a, w, s_p[0][i], s_p[1][i], s_p[2][i]);
                    c += __popcll(__ballot(in));
                }
                if (lane == 0) s_cnt[m] = (ch ? s_cnt[m] : 0) + c;
            }
        }
        __syncthreads();
        if (tid < nb) a.counts[wg + (long long)G * (m0 + tid)] = s_cnt[tid];
    }
}

extern "C" int adfp_keyframe_overlap(const long long* idx, int n, const float* depth_img, int H, int W, const float* c2w, int N_samples,
                                     const float* poses, int K, double fx, double fy, double cx, double cy, int edge, int* counts,
                                     float* pts_out, void* stream) {
    if (K < 0 || n <= 0 || N_samples < 1 || H < 1 || W < 1) return ADFP_E_ARG;
    if (!idx || !depth_img || !c2w || !counts || (K > 0 && !poses)) return ADFP_E_ARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if ((long long)n * N_samples > 0x7fffffffll - ADFP_KFO_CHUNK) return ADFP_E_UNSUPPORTED;
    if (K == 0) return 0;
    KfoArgs a;
    a.idx = idx; a.n = n; a.S = N_samples; a.P = n * N_samples;
    a.depth = depth_img; a.H = H; a.W = W; a.c2w = c2w; a.poses = poses; a.K = K;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.umin = (float)edge; a.umax = (float)(W - edge); a.vmin = (float)edge; a.vmax = (float)(H - edge);
    a.counts = counts; a.pts_out = pts_out;
    const int per_wg = ADFP_KFO_WAVES;                        // one keyframe per wave before the grid widens past the CUs
    int grid = (K + per_wg - 1) / per_wg;
    if (grid > ADFP_KFO_MAX_GRID) grid = ADFP_KFO_MAX_GRID;
    hipLaunchKernelGGL(k_keyframe_overlap, dim3(grid), dim3(ADFP_KFO_THREADS), 0, (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
