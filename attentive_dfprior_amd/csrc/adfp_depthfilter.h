// adfp_depthfilter.h -- the bilateral filter of a sensor depth image that KinectFusion's pipeline starts with (icp.depth_bilateral,
// DepthICP(bilateral=...)): k_depth_normals takes one-pixel differences of the depth, which amplifies sensor noise more than anything
// else in the chain, and a noisy normal fails the step's cos_tol gate.  The contract is stated in include/adfp.h ("Depth bilateral
// filter") and, in numpy, in tests/depth_filter_ref.py.
//
//   k_depth_bilateral   a 16 x 16 tile of one image per 256-thread workgroup, grid (ceil(W / 16), ceil(H / 16), V).  The tile and its
//                       halo, (16 + 2 R)^2 <= 32 x 32 texels, are staged once in LDS: each lane loads up to four texels, row pieces
//                       of 16 + 2 R consecutive floats.  Validity (finite and > 0, inside the image) is decided there, once per staged
//                       texel: anything else is stored as +0, so a tap asks `d > 0` of a register and nothing more.  The rows are 48
//                       floats apart: the 32 lanes that a ds_read_b32 serves together are two tile rows of 16 lanes, which land on
//                       banks 0-15 and 16-31 of the 32.  A lane then walks its window row by row, column by column (the rule's order
//                       of addition), one f64 exp per tap that passes the range gate, two f64 sums, one division, one f32 store.
//                       The window's bounds are kernel arguments, not template parameters: the loops index LDS only, no array lives
//                       in registers, so nothing goes to scratch.  No atomics; the order of every addition is the window's own.
#pragma once
#include "adfp_device.h"

#define ADFP_BILATERAL_TILE 16
#define ADFP_BILATERAL_MAX_RADIUS 8
#define ADFP_BILATERAL_PITCH 48          // floats between staged rows: >= 16 + 2 * 8, and 16 mod 32 (see above)
#define ADFP_BILATERAL_MAX_DIM 32768

__global__ __launch_bounds__(256) void k_depth_bilateral(const float* __restrict__ depth, int H, int W, int R, double a, double sigma_depth,
                                                         double sigma_depth_z2, float* __restrict__ out) {
    __shared__ float s_d[(ADFP_BILATERAL_TILE + 2 * ADFP_BILATERAL_MAX_RADIUS) * ADFP_BILATERAL_PITCH];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int u0 = blockIdx.x * ADFP_BILATERAL_TILE - R, v0 = blockIdx.y * ADFP_BILATERAL_TILE - R;      // the staged window's corner
    const int side = ADFP_BILATERAL_TILE + 2 * R;
    const long long image = (long long)blockIdx.z * H * W;
    for (int i = t; i < side * side; i += 256) {
        const int ly = i / side, lx = i - ly * side;
        const int gv = v0 + ly, gu = u0 + lx;
        float d = 0.f;
        if (gv >= 0 && gv < H && gu >= 0 && gu < W) {
            const float g = depth[image + (long long)gv * W + gu];
            if (icp_depth_ok(g)) d = g;
        }
        s_d[ly * ADFP_BILATERAL_PITCH + lx] = d;
    }
    __syncthreads();
    const int u = u0 + R + tx, v = v0 + R + ty;
    if (u >= W || v >= H) return;
    const float dpf = s_d[(ty + R) * ADFP_BILATERAL_PITCH + tx + R];
    float res = 0.f;
    if (dpf > 0.f) {
        const double dp = (double)dpf;
        const double sp = sigma_depth + sigma_depth_z2 * (dp * dp);
        const double b = 1.0 / ((2.0 * sp) * sp), gate = 3.0 * sp;
        double num = 0.0, den = 0.0;
        for (int j = 0; j <= 2 * R; ++j) {
            const float* row = s_d + (ty + j) * ADFP_BILATERAL_PITCH + tx;
            const int dv = j - R;
            for (int i = 0; i <= 2 * R; ++i) {
                const float dqf = row[i];
                if (!(dqf > 0.f)) continue;                        // invalid, or outside the image: not part of the window
                const double dq = (double)dqf, e = dq - dp;
                if (fabs(e) > gate) continue;
                const int du = i - R;
                const double w = exp(-((double)(du * du + dv * dv) * a + (e * e) * b));
                num += w * dq;
                den += w;
            }
        }
        res = (float)(num / den);
    }
    out[image + (long long)v * W + u] = res;
}

extern "C" int adfp_depth_bilateral(const float* depth, int V, int H, int W, int radius, double sigma_space, double sigma_depth,
                                    double sigma_depth_z2, float* out, void* stream) {
    if (!depth || !out || out == depth || V < 1 || H < 1 || W < 1 || radius < 1) return ADFP_E_ARG;
    if (!(sigma_space > 0.0) || !(sigma_depth > 0.0) || !(sigma_depth_z2 >= 0.0)) return ADFP_E_ARG;          // a NaN fails each
    if (radius > ADFP_BILATERAL_MAX_RADIUS || H > ADFP_BILATERAL_MAX_DIM || W > ADFP_BILATERAL_MAX_DIM || V > 65535) return ADFP_E_UNSUPPORTED;
    const double a = 1.0 / ((2.0 * sigma_space) * sigma_space);
    const dim3 grid((unsigned)((W + ADFP_BILATERAL_TILE - 1) / ADFP_BILATERAL_TILE), (unsigned)((H + ADFP_BILATERAL_TILE - 1) / ADFP_BILATERAL_TILE),
                    (unsigned)V);
    hipLaunchKernelGGL(k_depth_bilateral, grid, dim3(256), 0, (hipStream_t)stream, depth, H, W, radius, a, sigma_depth, sigma_depth_z2, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}
