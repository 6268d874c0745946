// adfp_meshcolor.h -- mesh colours from the keyframes' images: every vertex projected into every keyframe, the keyframe's own depth
// image deciding visibility, the surviving views blended.  Contract and the rule, operation for operation: include/adfp.h, "mesh
// colours from the keyframes".  tests/project_colors_ref.py restates the rule in numpy.
//
//   one lane per vertex, no workspace.  The poses (12 floats) and camera centres (3 floats) go through LDS ADFP_MPC_TILE keyframes at
//   a time, so a wave reads them as broadcasts.  The frame test (k_cull_seen's projection, cull_project<true>) comes before any
//   image load: most vertex-keyframe pairs end there.  A pair that passes reads four depths, and only if all four agree with the
//   vertex's depth the four 12-byte colour pixels, as dwords (two runs of six: pixels x0 and x0 + 1 are adjacent in a row).  Marching
//   cubes emits vertices in lattice order, so a wave's gathers fall on neighbouring pixels.  The keyframes are walked in ascending
//   index by every lane: the sums of the WEIGHTED blend have one order, nothing is decided by an atomic.
#pragma once
#include "adfp_device.h"

#define ADFP_MPC_THREADS 256
#define ADFP_MPC_TILE 32           // keyframes per LDS stage: 32 x 15 floats
#define ADFP_MPC_POSE 15           // 12 of w2c, 3 of the centre

struct MpcArgs {
    const float* v; const float* n; int nv;                // [nv][3] vertices, [nv][3] normals or NULL
    const float* w2c; const float* center; int K;          // [K][12], [K][3]
    const float* depth; const float* color;                // [K][H][W], [K][H][W][3]
    float fx, fy, cx, cy;
    int W, H;
    float u_lo, u_hi, v_lo, v_hi;                          // border, W - 1 - border, border, H - 1 - border as f32 (exact)
    float tol;
    float* rgb; float* wsum; int* count; int* best;
};

template <int BLEND, bool NORMALS>
__global__ __launch_bounds__(ADFP_MPC_THREADS) void k_mesh_project_colors(MpcArgs a) {
    __shared__ float s_pose[ADFP_MPC_TILE * ADFP_MPC_POSE];
    const int i = blockIdx.x * ADFP_MPC_THREADS + threadIdx.x;
    const bool on = i < a.nv;
    float x = 0.f, y = 0.f, z = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (on) {
        x = a.v[3 * (long long)i]; y = a.v[3 * (long long)i + 1]; z = a.v[3 * (long long)i + 2];
        if (NORMALS) { nx = a.n[3 * (long long)i]; ny = a.n[3 * (long long)i + 1]; nz = a.n[3 * (long long)i + 2]; }
    }
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wacc = 0.f;    // WEIGHTED: the sums; BEST: the best view's colour and weight
    int cnt = 0, best = -1;
    float wbest = 0.f;
    const long long plane = (long long)a.H * a.W;
    for (int k0 = 0; k0 < a.K; k0 += ADFP_MPC_TILE) {
        const int m = a.K - k0 < ADFP_MPC_TILE ? a.K - k0 : ADFP_MPC_TILE;
        __syncthreads();
        for (int e = threadIdx.x; e < ADFP_MPC_POSE * m; e += ADFP_MPC_THREADS) {
            const int k = e / ADFP_MPC_POSE, c = e - k * ADFP_MPC_POSE;
            s_pose[e] = c < 12 ? a.w2c[12 * (long long)(k0 + k) + c] : a.center[3 * (long long)(k0 + k) + (c - 12)];
        }
        __syncthreads();
        if (!on) continue;
        for (int k = 0; k < m; ++k) {
            const float* w = s_pose + ADFP_MPC_POSE * k;
            float u, v, Z;
            // k_cull_seen's projection; its open frustum test is not ours, so only u, v, Z are taken (zz < 0 is recomputed)
            cull_project<true>(w, x, y, z, a.fx, a.fy, a.cx, a.cy, 0.f, 0.f, u, v, Z);
            const float zz = Z + 1e-8f;
            if (!(zz < 0.f && u >= a.u_lo && u <= a.u_hi && v >= a.v_lo && v <= a.v_hi)) continue;       // a NaN fails
            int x0 = (int)floorf(u), y0 = (int)floorf(v);
            x0 = x0 < a.W - 2 ? x0 : a.W - 2;
            y0 = y0 < a.H - 2 ? y0 : a.H - 2;
            const float ax = u - (float)x0, ay = v - (float)y0, zc = -Z;
            const long long pix = (long long)(k0 + k) * plane + (long long)y0 * a.W + x0;      // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2
            const float* d0 = a.depth + pix;
            const float* d1 = d0 + a.W;
            const float d00 = d0[0], d01 = d0[1], d10 = d1[0], d11 = d1[1];
            const bool vis = d00 > 0.f && fabsf(d00 - zc) <= a.tol && d01 > 0.f && fabsf(d01 - zc) <= a.tol &&
                             d10 > 0.f && fabsf(d10 - zc) <= a.tol && d11 > 0.f && fabsf(d11 - zc) <= a.tol;
            if (!vis) continue;
            const float tx = w[12] - x, ty = w[13] - y, tz = w[14] - z;
            float cosv = 1.f;
            if (NORMALS) {
                const float dist = sqrtf((tx * tx + ty * ty) + tz * tz);
                cosv = fabsf((tx * nx + ty * ny) + tz * nz) / fmaxf(dist, 1e-12f);
            }
            const float wt = cosv / fmaxf(zc * zc, 1e-12f);
            if (!(wt > 0.f)) continue;                                                          // a zero or NaN normal
            ++cnt;
            const bool better = best < 0 || wt > wbest;
            if (better) { best = k0 + k; wbest = wt; }
            if (BLEND == ADFP_BLEND_BEST && !better) continue;
            const float* c0 = a.color + 3 * pix;                                                // two pixels = six dwords per row
            const float* c1 = c0 + 3 * (long long)a.W;
            const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
            const float r = ((w00 * c0[0] + w01 * c0[3]) + w10 * c1[0]) + w11 * c1[3];
            const float g = ((w00 * c0[1] + w01 * c0[4]) + w10 * c1[1]) + w11 * c1[4];
            const float b = ((w00 * c0[2] + w01 * c0[5]) + w10 * c1[2]) + w11 * c1[5];
            if (BLEND == ADFP_BLEND_WEIGHTED) { acc0 += wt * r; acc1 += wt * g; acc2 += wt * b; wacc += wt; }
            else { acc0 = r; acc1 = g; acc2 = b; wacc = wt; }
        }
    }
    if (!on) return;
    if (BLEND == ADFP_BLEND_WEIGHTED && cnt > 0) { acc0 = acc0 / wacc; acc1 = acc1 / wacc; acc2 = acc2 / wacc; }
    a.rgb[3 * (long long)i] = acc0; a.rgb[3 * (long long)i + 1] = acc1; a.rgb[3 * (long long)i + 2] = acc2;
    a.wsum[i] = wacc;
    a.count[i] = cnt;
    a.best[i] = best;
}

extern "C" {

int adfp_mesh_project_colors(const float* verts, const float* normals, long long n_verts, const float* w2c, const float* center,
                             const float* depth, const float* color, long long n_keyframes, float fx, float fy, float cx, float cy, int W,
                             int H, float depth_tol, int border, int blend, float* rgb, float* wsum, int* count, int* best, void* stream) {
    if (n_verts < 0 || n_keyframes < 0 || W < 1 || H < 1 || border < 0) return ADFP_E_ARG;
    if (blend != ADFP_BLEND_WEIGHTED && blend != ADFP_BLEND_BEST) return ADFP_E_ARG;
    if (!(depth_tol >= 0.f) || !isfinite(depth_tol)) return ADFP_E_ARG;
    if (W >= 2 && H >= 2 && 2 * (long long)border > (long long)(W < H ? W : H) - 2) return ADFP_E_ARG;
    if (n_verts == 0) return 0;
    if (!verts || !rgb || !wsum || !count || !best) return ADFP_E_ARG;
    if (n_keyframes > 0 && (!w2c || !center || !depth || !color)) return ADFP_E_ARG;
    if (W < 2 || H < 2 || W > 32768 || H > 32768 || n_keyframes > 32768 || n_verts > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    MpcArgs a;
    a.v = verts; a.n = normals; a.nv = (int)n_verts; a.w2c = w2c; a.center = center; a.K = (int)n_keyframes;
    a.depth = depth; a.color = color; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.W = W; a.H = H;
    a.u_lo = (float)border; a.u_hi = (float)(W - 1 - border); a.v_lo = (float)border; a.v_hi = (float)(H - 1 - border);
    a.tol = depth_tol; a.rgb = rgb; a.wsum = wsum; a.count = count; a.best = best;
    const dim3 grid((unsigned)ceil_div(n_verts, ADFP_MPC_THREADS)), block(ADFP_MPC_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (blend == ADFP_BLEND_WEIGHTED) {
        if (normals) hipLaunchKernelGGL((k_mesh_project_colors<ADFP_BLEND_WEIGHTED, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mesh_project_colors<ADFP_BLEND_WEIGHTED, false>), grid, block, 0, st, a);
    } else {
        if (normals) hipLaunchKernelGGL((k_mesh_project_colors<ADFP_BLEND_BEST, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_mesh_project_colors<ADFP_BLEND_BEST, false>), grid, block, 0, st, a);
    }
    ADFP_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
