// adfp_rgbd.h -- RGB-D ICP: adfp_icp.h's frame-to-model point-to-plane step with a photometric term against the last tracked frame
// (the "keyframe": its colour, its sensor depth, its final pose) added to the same 6 x 6 normal equations, as Kintinuous,
// ElasticFusion and DVO pair the two.  Texture pins the directions a wall's depth leaves free, and a frame-to-frame term needs no
// prior.  The contract is stated in include/adfp.h ("RGB-D ICP") and, in numpy, in tests/rgbd_icp_ref.py.
//
//   k_rgbd_frame_map  one lane per pixel, a row of the image per blockIdx.y (k_depth_normals' shape): colour and depth -> one
//                     16-byte texel (I, gx, gy, d).  A lane recomputes its four neighbours' intensities from their colours in f64, so
//                     the central differences are of unrounded values and every load is a coalesced row piece; one float4 store.
//   k_rgbd_step       k_icp_step's shape (256 threads, grid-stride, the grid sized to the compute units, wave_sum, 4 x 31 doubles of
//                     LDS, one row per workgroup, no atomics).  Per strided pixel the geometric pair first -- icp_geo_pair, the very
//                     function k_icp_step calls -- then the photometric one: the sensor point into the keyframe's image, the four
//                     texels of the bilinear footprint as four independent 16-byte loads behind the bounds gate, then the depth
//                     gates, the interpolation, r and J.
//   k_icp_solve<31>   adfp_icp.h's solve over two more sums.
//
// With rgb_weight 0 or no keyframe the host passes key = nullptr: no photometric pair is evaluated, sums 29 and 30 are 0 and sums
// 0..28 are adfp_icp_step's bytes (same grid, same additions in the same order).
#pragma once
#include "adfp_icp.h"

static_assert(ADFP_RGBD_SUMS == ADFP_ICP_SUMS + 2, "the joint sums are the depth ICP's and two photometric ones");

ADFP_DEV double rgbd_intensity(const float* __restrict__ color, long long p) {
    return (0.299 * (double)color[3 * p] + 0.587 * (double)color[3 * p + 1]) + 0.114 * (double)color[3 * p + 2];
}

// grid (ceil(W / 256), H)
__global__ __launch_bounds__(256) void k_rgbd_frame_map(const float* __restrict__ color, const float* __restrict__ depth, int H, int W,
                                                        float4* __restrict__ map) {
    const int u = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (u >= W) return;
    const long long base = (long long)v * W + u;
    const double I = rgbd_intensity(color, base);
    double gx = 0.0, gy = 0.0;
    if (u >= 1 && u + 1 < W) gx = (rgbd_intensity(color, base + 1) - rgbd_intensity(color, base - 1)) / 2.0;
    if (v >= 1 && v + 1 < H) gy = (rgbd_intensity(color, base + W) - rgbd_intensity(color, base - W)) / 2.0;
    map[base] = make_float4((float)I, (float)gx, (float)gy, depth[base]);
}

struct RgbdStepArgs {
    IcpStepArgs g;                         // the geometric step's; g.ds is not read (the sensor depth is cur's fourth channel)
    const float4* cur; const float4* key;  // key == nullptr: no photometric term
    const float* pkey;
    double lam, rgb_tol;
};

// a keyframe texel takes part when its depth is valid and agrees with the projected point's
ADFP_DEV bool rgbd_texel_ok(const float4& m, double z, double tol) { return icp_depth_ok(m.w) && fabs((double)m.w - z) <= tol; }

// The photometric pair of the sensor point x (intensity Is) with the keyframe.  K: the keyframe's pose.  false: no pair.
ADFP_DEV bool rgbd_photo_pair(const RgbdStepArgs& a, const double K[12], const double x[3], double Is, double J[6], double& r) {
    const IcpStepArgs& g = a.g;
    const double e[3] = {x[0] - K[3], x[1] - K[7], x[2] - K[11]};
    double y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) y[k] = (K[k] * e[0] + K[4 + k] * e[1]) + K[8 + k] * e[2];
    const double z = -y[2];
    if (!(z > 0.0)) return false;
    const double pa = ((g.fx * y[0]) / z) + g.cx, pb = ((-g.fy * y[1]) / z) + g.cy;
    const double u0 = floor(pa), v0 = floor(pb);
    // all four footprint pixels carry central differences; a NaN fails here, so the conversions below are of in-range values
    if (!(u0 >= 1.0 && u0 <= (double)(g.W - 3) && v0 >= 1.0 && v0 <= (double)(g.H - 3))) return false;
    const long long k0 = (long long)(int)v0 * g.W + (int)u0;      // k0 + W + 1 <= (H - 2) W + W - 2: inside the map
    const float4 m00 = a.key[k0], m01 = a.key[k0 + 1], m10 = a.key[k0 + g.W], m11 = a.key[k0 + g.W + 1];
    const bool seen = rgbd_texel_ok(m00, z, g.dist_tol) & rgbd_texel_ok(m01, z, g.dist_tol) & rgbd_texel_ok(m10, z, g.dist_tol)
                      & rgbd_texel_ok(m11, z, g.dist_tol);
    if (!seen) return false;
    const double s = pa - u0, t = pb - v0;
    const double w00 = (1.0 - s) * (1.0 - t), w01 = s * (1.0 - t), w10 = (1.0 - s) * t, w11 = s * t;
    const double I = (w00 * (double)m00.x + w01 * (double)m01.x) + (w10 * (double)m10.x + w11 * (double)m11.x);
    const double gx = (w00 * (double)m00.y + w01 * (double)m01.y) + (w10 * (double)m10.y + w11 * (double)m11.y);
    const double gy = (w00 * (double)m00.z + w01 * (double)m01.z) + (w10 * (double)m10.z + w11 * (double)m11.z);
    r = Is - I;
    if (!(fabs(r) <= a.rgb_tol)) return false;
    const double gfx = gx * g.fx, gfy = gy * g.fy;
    const double c[3] = {gfx / z, -gfy / z, (gfx * y[0] - gfy * y[1]) / (z * z)};     // the intensity's gradient at y, keyframe camera frame
    double n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] = (K[4 * k] * c[0] + K[4 * k + 1] * c[1]) + K[4 * k + 2] * c[2];
    J[0] = x[1] * n[2] - x[2] * n[1]; J[1] = x[2] * n[0] - x[0] * n[2]; J[2] = x[0] * n[1] - x[1] * n[0];
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    return true;
}

__global__ __launch_bounds__(ADFP_ICP_THREADS) void k_rgbd_step(RgbdStepArgs a) {
    __shared__ double s_part[4][ADFP_RGBD_SUMS];
    const IcpStepArgs& g = a.g;
    if (g.state->status != (double)ADFP_ICP_OK) return;          // kernel-uniform: k_icp_solve returns on the same word
    const bool photo = a.key != nullptr;
    double T[12], P[12], K[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T[k] = g.state->T[k]; P[k] = (double)g.pref[k]; K[k] = photo ? (double)a.pkey[k] : 0.0; }
    double acc[ADFP_RGBD_SUMS];
#pragma unroll
    for (int k = 0; k < ADFP_RGBD_SUMS; ++k) acc[k] = 0.0;
    const long long step = (long long)gridDim.x * ADFP_ICP_THREADS;
    for (long long i = (long long)blockIdx.x * ADFP_ICP_THREADS + threadIdx.x; i < g.n; i += step) {
        const int vs = (int)(i / g.wn) * g.stride, us = (int)(i % g.wn) * g.stride;
        const long long si = (long long)vs * g.W + us;
        const float4 c = a.cur[si];
        const double Ns[3] = {(double)g.ns[3 * si], (double)g.ns[3 * si + 1], (double)g.ns[3 * si + 2]};
        const bool geo = !(Ns[0] == 0.0 && Ns[1] == 0.0 && Ns[2] == 0.0);
        const bool pho = photo && icp_depth_ok(c.w) && fabsf(c.x) <= 3.4028234663852886e38f;      // a NaN or infinite intensity fails
        if (!geo && !pho) continue;
        double x[3], J[6], r;
        icp_sensor_point(g, T, us, vs, (double)c.w, x);
        if (geo && icp_geo_pair(g, T, P, x, Ns, J, r)) icp_add_pair<false>(acc, J, r, 1.0, 27);
        if (pho && rgbd_photo_pair(a, K, x, (double)c.x, J, r)) icp_add_pair<true>(acc, J, r, a.lam, 29);
    }
    icp_block_sums<ADFP_RGBD_SUMS>(acc, s_part, g.part);
}

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
extern "C" size_t adfp_rgbd_workspace_bytes(int H, int W) {
    return (size_t)icp_blocks_max(H, W) * ADFP_RGBD_SUMS * sizeof(double);
}

extern "C" int adfp_rgbd_frame_map(const float* color, const float* depth, int H, int W, float* map, void* stream) {
    if (!color || !depth || !map || H < 1 || W < 1 || (((unsigned long long)map) & 15ull)) return ADFP_E_ARG;
    if (H > ADFP_ICP_MAX_DIM || W > ADFP_ICP_MAX_DIM) return ADFP_E_UNSUPPORTED;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H);
    hipLaunchKernelGGL(k_rgbd_frame_map, grid, dim3(256), 0, (hipStream_t)stream, color, depth, H, W, (float4*)map);
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_rgbd_step(const float* cur_map, const float* normals_s, const float* depth_m, const float* normals_m, const float* p_ref,
                              const float* key_map, const float* p_key, int H, int W, float fx, float fy, float cx, float cy, int stride,
                              double dist_tol, double cos_tol, double rgb_weight, double rgb_tol, double min_pivot, double min_pairs, void* state,
                              double* stats, double* rgb_stats, int stats_rows, int row, double* sums, void* workspace, size_t workspace_bytes,
                              void* stream) {
    if (!cur_map || !normals_s || !depth_m || !normals_m || !p_ref || !state || !stats || !rgb_stats || !workspace) return ADFP_E_ARG;
    if ((key_map == nullptr) != (p_key == nullptr)) return ADFP_E_ARG;
    if (H < 1 || W < 1 || stride < 1 || stats_rows < 1 || row < 0 || row >= stats_rows) return ADFP_E_ARG;
    if (!(dist_tol == dist_tol) || !(cos_tol == cos_tol) || !(min_pivot == min_pivot) || !(min_pairs == min_pairs)) return ADFP_E_ARG;
    if (!(rgb_weight >= 0.0) || !(rgb_tol == rgb_tol)) return ADFP_E_ARG;
    if (!(fx == fx) || !(fy == fy) || fx == 0.f || fy == 0.f || !(cx == cx) || !(cy == cy)) return ADFP_E_ARG;
    if ((((unsigned long long)cur_map) & 15ull) || (((unsigned long long)key_map) & 15ull)) return ADFP_E_ARG;
    if ((((unsigned long long)state) & 7ull) || (((unsigned long long)workspace) & 7ull) || (((unsigned long long)stats) & 7ull)
        || (((unsigned long long)rgb_stats) & 7ull))
        return ADFP_E_ARG;
    if (H > ADFP_ICP_MAX_DIM || W > ADFP_ICP_MAX_DIM) return ADFP_E_UNSUPPORTED;
    const size_t need = adfp_rgbd_workspace_bytes(H, W);
    if (need == 0 || workspace_bytes < need) return ADFP_E_ARG;
    RgbdStepArgs a;
    IcpStepArgs& g = a.g;
    g.ds = nullptr; g.ns = normals_s; g.dm = depth_m; g.nm = normals_m; g.pref = p_ref; g.state = (const IcpState*)state;
    g.H = H; g.W = W; g.stride = stride;
    g.wn = (W + stride - 1) / stride;
    g.n = (long long)g.wn * ((H + stride - 1) / stride);
    g.fx = fx; g.fy = fy; g.cx = cx; g.cy = cy; g.dist_tol = dist_tol; g.cos_tol = cos_tol;
    g.part = (double*)workspace;
    const bool photo = key_map && rgb_weight > 0.0;
    a.cur = (const float4*)cur_map; a.key = photo ? (const float4*)key_map : nullptr; a.pkey = photo ? p_key : nullptr;
    a.lam = rgb_weight; a.rgb_tol = rgb_tol;
    long long blocks = (g.n + ADFP_ICP_THREADS - 1) / ADFP_ICP_THREADS;        // adfp_icp_step's grid rule
    const long long cap = 2ll * num_cu();
    if (blocks > cap) blocks = cap;
    if (blocks > ADFP_ICP_MAX_BLOCKS) blocks = ADFP_ICP_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_rgbd_step, dim3((unsigned)blocks), dim3(ADFP_ICP_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_icp_solve<ADFP_RGBD_SUMS>), dim3(1), dim3(64), 0, st, (const double*)workspace, (int)blocks, (IcpState*)state, min_pivot,
                       min_pairs, stats + (long long)row * ADFP_ICP_STATS, rgb_stats + (long long)row * ADFP_RGBD_STATS, sums);
    ADFP_CHECK_LAUNCH();
    return 0;
}
