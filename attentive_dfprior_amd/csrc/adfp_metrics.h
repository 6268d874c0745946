// adfp_metrics.h -- one frame's rendering metrics on the device (render_eval.FrameMetrics): the sensor images and the images
// render_img returned go in as they lie in device memory, and one row of ADFP_FRAME_METRICS doubles comes out at an address the
// caller chooses -- the Visualizer's stats sums (adfp_vis.h) and, per level of the MS-SSIM pyramid and per channel, the sums of
// the SSIM map and of the contrast-structure map.  Nothing is read back in between; the contract is stated in include/adfp.h
// ("rendering metrics") and, in numpy, in tests/render_ref.py.
//
//   k_vis_reduce  adfp_vis.h's own kernel, launched as adfp_vis_panels launches it (its grid is a function of H W alone): the
//                 five sums come out with the bits the Visualizer gives them because the same code makes them.  Its partials
//                 (six doubles per workgroup, the maximum of gt_depth first, which nothing here reads) open the workspace.
//   k_met_ssim    one workgroup per 16 x 32 tile of window positions and channel.  The tile plus its 10-pixel apron of x and y
//                 is staged in LDS as doubles (level 0 converts there: gt_color widened, color clipped to [0, 1] with NaN as 0);
//                 the row pass leaves the five moment maps E[x], E[y], E[xx], E[yy], E[xy] of 26 x 32 entries in LDS; the column
//                 pass, the two quotients and the mask of a partial tile stay in registers, two positions per thread; the
//                 workgroup reduces to one partial pair (ssim, cs).  LDS: 2 x 26 x 42 x 8 + 5 x 26 x 32 x 8 = 50 752 bytes.
//   k_met_pool    level k + 1 from level k: one thread per pooled pixel and channel, x and y both, f64 into the workspace.  A
//                 launch of its own rather than a rider of k_met_ssim: the pooled pixels of a tile do not line up with the
//                 tile's window positions once a level is odd (the zero padding shifts them by one), and a separate kernel of
//                 ten lines keeps both simple.
//   k_met_final   one workgroup per row entry walks that entry's partial list in fixed index order and writes it; levels at or
//                 beyond geom.levels get exactly 0.
// No float atomics anywhere: every call gives the same bits.  All arithmetic is f64 and the build forbids contraction.
#pragma once
#include "adfp_device.h"

#define ADFP_MET_THREADS 256
#define ADFP_MET_STATS 5           // row entries [0..4]
#define ADFP_MET_LEVELS 5
#define ADFP_MET_TAPS 11
#define ADFP_MET_TH 16             // window positions per tile: rows
#define ADFP_MET_TW 32             //                            columns
#define ADFP_MET_SH (ADFP_MET_TH + ADFP_MET_TAPS - 1)      // staged rows: 26
#define ADFP_MET_SW (ADFP_MET_TW + ADFP_MET_TAPS - 1)      // staged columns: 42
#define ADFP_MET_MAX_DIM 32768
#define ADFP_MET_C1 1e-4           // (0.01 L)^2 and (0.03 L)^2 at data range L = 1
#define ADFP_MET_C2 9e-4

static_assert(ADFP_MET_THREADS == ADFP_VIS_THREADS, "k_met_final folds k_vis_reduce's partials as k_vis_panels does");
static_assert(ADFP_MET_TH * ADFP_MET_TW == 2 * ADFP_MET_THREADS, "two window positions per thread");

struct MetWindow { double g[ADFP_MET_TAPS]; };

// a level's two images, element i of [H][W][3]
template <typename GT>
struct MetLevel0 {                                 // the frame itself
    const GT* x; const float* y;
    ADFP_DEV double X(long long i) const { return (double)x[i]; }
    ADFP_DEV double Y(long long i) const {        // the RGB panel's rule: clip(color, 0, 1), NaN = 0
        const float v = y[i];
        return v != v ? 0.0 : (double)(v < 0.f ? 0.f : (v > 1.f ? 1.f : v));
    }
};
struct MetLevelK {                                 // a pooled level in the workspace
    const double* x; const double* y;
    ADFP_DEV double X(long long i) const { return x[i]; }
    ADFP_DEV double Y(long long i) const { return y[i]; }
};

// grid (tiles_x, tiles_y, 3): partial pair ((channel tiles_y + tile_y) tiles_x + tile_x) of a level [H][W][3]
template <typename SRC>
__global__ __launch_bounds__(ADFP_MET_THREADS) void k_met_ssim(SRC src, int H, int W, MetWindow win, double* __restrict__ part) {
    __shared__ double s_x[ADFP_MET_SH * ADFP_MET_SW], s_y[ADFP_MET_SH * ADFP_MET_SW];
    __shared__ double s_m[5][ADFP_MET_SH * ADFP_MET_TW];
    __shared__ double s_wave[ADFP_MET_THREADS / 64];
    const int ch = blockIdx.z;
    const int r0 = blockIdx.y * ADFP_MET_TH, c0 = blockIdx.x * ADFP_MET_TW;
    // the tile and its apron; pixels beyond the level are zeros that only masked positions read
    for (int i = threadIdx.x; i < ADFP_MET_SH * ADFP_MET_SW; i += ADFP_MET_THREADS) {
        const int r = r0 + i / ADFP_MET_SW, c = c0 + i % ADFP_MET_SW;
        double x = 0.0, y = 0.0;
        if (r < H && c < W) {
            const long long e = ((long long)r * W + c) * 3 + ch;
            x = src.X(e); y = src.Y(e);
        }
        s_x[i] = x; s_y[i] = y;
    }
    __syncthreads();
    // the row pass: consecutive lanes, consecutive columns
    for (int i = threadIdx.x; i < ADFP_MET_SH * ADFP_MET_TW; i += ADFP_MET_THREADS) {
        const int o = (i / ADFP_MET_TW) * ADFP_MET_SW + i % ADFP_MET_TW;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int k = 0; k < ADFP_MET_TAPS; ++k) {
            const double w = win.g[k], x = s_x[o + k], y = s_y[o + k];
            mx += w * x; my += w * y; xx += w * (x * x); yy += w * (y * y); xy += w * (x * y);
        }
        s_m[0][i] = mx; s_m[1][i] = my; s_m[2][i] = xx; s_m[3][i] = yy; s_m[4][i] = xy;
    }
    __syncthreads();
    // the column pass and the quotients: thread t takes positions (t / 32, t % 32) and (t / 32 + 8, t % 32) of the tile
    double sum_ssim = 0.0, sum_cs = 0.0;
    const int col = threadIdx.x % ADFP_MET_TW;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = threadIdx.x / ADFP_MET_TW + j * (ADFP_MET_TH / 2);
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < ADFP_MET_TAPS; ++k) {
            const double w = win.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += w * s_m[q][(row + k) * ADFP_MET_TW + col];
        }
        const double mx = m[0], my = m[1];
        const double sxx = m[2] - mx * mx, syy = m[3] - my * my, sxy = m[4] - mx * my;
        const double cs = (2.0 * sxy + ADFP_MET_C2) / (sxx + syy + ADFP_MET_C2);
        const double ssim = (2.0 * mx * my + ADFP_MET_C1) / (mx * mx + my * my + ADFP_MET_C1) * cs;
        if (r0 + row < H - (ADFP_MET_TAPS - 1) && c0 + col < W - (ADFP_MET_TAPS - 1)) { sum_ssim += ssim; sum_cs += cs; }
    }
    sum_ssim = red_block_sum(sum_ssim, s_wave);
    sum_cs = red_block_sum(sum_cs, s_wave);
    if (threadIdx.x == 0) {
        double* p = part + 2 * (((long long)ch * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        p[0] = sum_ssim; p[1] = sum_cs;
    }
}

// F.avg_pool2d(level, 2, padding=(H % 2, W % 2)): output (i, j) averages rows 2 i - H % 2, + 1 and columns 2 j - W % 2, + 1; what
// falls outside the level is a zero that counts in the average
template <typename SRC>
__global__ __launch_bounds__(ADFP_MET_THREADS) void k_met_pool(SRC src, int H, int W, double* __restrict__ ox, double* __restrict__ oy, int Ho, int Wo) {
    const long long e = (long long)blockIdx.x * ADFP_MET_THREADS + threadIdx.x;
    if (e >= (long long)Ho * Wo * 3) return;
    const int ch = (int)(e % 3);
    const long long p = e / 3;
    const int i = (int)(p / Wo), j = (int)(p - (long long)i * Wo);
    const int r = 2 * i - (H & 1), c = 2 * j - (W & 1);
    double x[4], y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int rr = r + (k >> 1), cc = c + (k & 1);
        x[k] = 0.0; y[k] = 0.0;
        if (rr >= 0 && rr < H && cc >= 0 && cc < W) {
            const long long s = ((long long)rr * W + cc) * 3 + ch;
            x[k] = src.X(s); y[k] = src.Y(s);
        }
    }
    ox[e] = (((x[0] + x[1]) + x[2]) + x[3]) * 0.25;
    oy[e] = (((y[0] + y[1]) + y[2]) + y[3]) * 0.25;
}

struct MetPlan {
    int H, W, levels, nblk;
    int h[ADFP_MET_LEVELS], w[ADFP_MET_LEVELS];                    // level sizes
    int ty[ADFP_MET_LEVELS], tx[ADFP_MET_LEVELS];                  // tiles of window positions
    long long part[ADFP_MET_LEVELS];                               // workspace offsets in doubles: the level's partial pairs ...
    long long img[ADFP_MET_LEVELS];                                // ... and its x image, y behind it (levels >= 1)
    long long total;                                               // doubles; k_vis_reduce's partials sit at 0
};

struct MetFinalArgs { const double* ws; double* row; MetPlan p; };

// thread-strided walk in index order, then the workgroup's fixed tree: k_vis_panels' pass over its partial sums
ADFP_DEV double met_fold(const double* __restrict__ v, long long n, int stride, double* s_wave) {
    double s = 0.0;
    for (long long b = threadIdx.x; b < n; b += ADFP_MET_THREADS) s += v[b * stride];
    return red_block_sum(s, s_wave);
}

// workgroup e writes row[e]
__global__ __launch_bounds__(ADFP_MET_THREADS) void k_met_final(MetFinalArgs a) {
    __shared__ double s_wave[ADFP_MET_THREADS / 64];
    const int e = blockIdx.x;
    double v = 0.0;
    if (e < ADFP_MET_STATS) {                                      // block-uniform, like every branch here
        const int c = e == 3 ? 5 : (e == 4 ? 4 : e + 1);                       // k_vis_reduce's partial: max, n_valid, two sums, n_nonfinite, n_color
        v = met_fold(a.ws + c, a.p.nblk, ADFP_VIS_PART, s_wave);
    } else {
        const int k = (e - ADFP_MET_STATS) / 6, ch = (e - ADFP_MET_STATS) % 6 / 2, q = (e - ADFP_MET_STATS) & 1;
        if (k < a.p.levels) {
            const long long tiles = (long long)a.p.ty[k] * a.p.tx[k];
            v = met_fold(a.ws + a.p.part[k] + 2 * (ch * tiles) + q, tiles, 2, s_wave);
        }
    }
    if (threadIdx.x == 0) a.row[e] = v;
}

// 0, or the error of a geometry; fills the plan
static int met_plan(const adfp_metrics_geom* g, MetPlan& p) {
    if (!g) return ADFP_E_ARG;
    if (g->H < 1 || g->W < 1 || g->levels < 0 || g->levels > ADFP_MET_LEVELS || (unsigned)g->gt_color_f64 > 1u) return ADFP_E_ARG;
    if (g->H > ADFP_MET_MAX_DIM || g->W > ADFP_MET_MAX_DIM) return ADFP_E_UNSUPPORTED;
    p.H = g->H; p.W = g->W; p.levels = g->levels;
    const long long n = (long long)g->H * g->W, b = (n + ADFP_VIS_THREADS - 1) / ADFP_VIS_THREADS;
    p.nblk = (int)(b < ADFP_VIS_MAX_BLOCKS ? b : ADFP_VIS_MAX_BLOCKS);                  // vis_geometry's
    long long at = (long long)p.nblk * ADFP_VIS_PART;
    int h = g->H, w = g->W;
    for (int k = 0; k < ADFP_MET_LEVELS; ++k) {
        p.h[k] = p.w[k] = p.ty[k] = p.tx[k] = 0; p.part[k] = p.img[k] = 0;
        if (k >= g->levels) continue;
        if (h < ADFP_MET_TAPS || w < ADFP_MET_TAPS) return ADFP_E_ARG;
        p.h[k] = h; p.w[k] = w;
        p.ty[k] = (h - (ADFP_MET_TAPS - 1) + ADFP_MET_TH - 1) / ADFP_MET_TH;
        p.tx[k] = (w - (ADFP_MET_TAPS - 1) + ADFP_MET_TW - 1) / ADFP_MET_TW;
        p.part[k] = at; at += 6ll * p.ty[k] * p.tx[k];
        if (k > 0) { p.img[k] = at; at += 6ll * h * w; }
        h = (h + 2 * (h & 1) - 2) / 2 + 1; w = (w + 2 * (w & 1) - 2) / 2 + 1;
    }
    p.total = at;
    return 0;
}

extern "C" size_t adfp_frame_metrics_workspace_bytes(const adfp_metrics_geom* geom) {
    MetPlan p;
    if (met_plan(geom, p)) return 0;
    return ((size_t)p.total * sizeof(double) + 255) / 256 * 256;
}

extern "C" int adfp_frame_metrics_windows(const adfp_metrics_geom* geom, long long windows[5]) {
    MetPlan p;
    const int rc = met_plan(geom, p);
    if (rc) return rc;
    if (!windows) return ADFP_E_ARG;
    for (int k = 0; k < ADFP_MET_LEVELS; ++k)
        windows[k] = k < p.levels ? (long long)(p.h[k] - (ADFP_MET_TAPS - 1)) * (p.w[k] - (ADFP_MET_TAPS - 1)) : 0;
    return 0;
}

template <typename GT>
static void met_launch(const MetPlan& p, const MetWindow& win, const float* gt_depth, const GT* gt_color, const double* depth, const float* color,
                       double* row, double* ws, hipStream_t st) {
    const dim3 block(ADFP_MET_THREADS);
    VisArgs va{};                                  // k_vis_reduce reads the four images, part, H, W and nblk
    va.gt_depth = gt_depth; va.gt_color = gt_color; va.depth = depth; va.color = color; va.part = ws;
    va.H = p.H; va.W = p.W; va.nblk = p.nblk;
    hipLaunchKernelGGL(k_vis_reduce<GT>, dim3((unsigned)p.nblk), block, 0, st, va);
    const MetLevel0<GT> frame{gt_color, color};
    for (int k = 0; k < p.levels; ++k) {
        const MetLevelK lk{ws + p.img[k], ws + p.img[k] + 3ll * p.h[k] * p.w[k]};
        const dim3 grid((unsigned)p.tx[k], (unsigned)p.ty[k], 3u);
        if (k == 0) hipLaunchKernelGGL(k_met_ssim<MetLevel0<GT>>, grid, block, 0, st, frame, p.h[k], p.w[k], win, ws + p.part[k]);
        else hipLaunchKernelGGL(k_met_ssim<MetLevelK>, grid, block, 0, st, lk, p.h[k], p.w[k], win, ws + p.part[k]);
        if (k + 1 < p.levels) {
            const long long n = 3ll * p.h[k + 1] * p.w[k + 1];
            double* ox = ws + p.img[k + 1];
            const dim3 pgrid((unsigned)((n + ADFP_MET_THREADS - 1) / ADFP_MET_THREADS));
            if (k == 0) hipLaunchKernelGGL(k_met_pool<MetLevel0<GT>>, pgrid, block, 0, st, frame, p.h[k], p.w[k], ox, ox + n, p.h[k + 1], p.w[k + 1]);
            else hipLaunchKernelGGL(k_met_pool<MetLevelK>, pgrid, block, 0, st, lk, p.h[k], p.w[k], ox, ox + n, p.h[k + 1], p.w[k + 1]);
        }
    }
    MetFinalArgs fa{ws, row, p};
    hipLaunchKernelGGL(k_met_final, dim3(ADFP_FRAME_METRICS), block, 0, st, fa);
}

extern "C" int adfp_frame_metrics(const adfp_metrics_geom* geom, const float* gt_depth, const void* gt_color, const double* depth, const float* color,
                                  double* row, void* workspace, size_t workspace_bytes, void* stream) {
    MetPlan p;
    const int rc = met_plan(geom, p);
    if (rc) return rc;
    if (!gt_depth || !gt_color || !depth || !color || !row || !workspace) return ADFP_E_ARG;
    if ((((unsigned long long)row) & 7ull) || (((unsigned long long)workspace) & 7ull)) return ADFP_E_ARG;
    if (workspace_bytes < adfp_frame_metrics_workspace_bytes(geom)) return ADFP_E_ARG;
    MetWindow win;                                 // 11 taps, sigma 1.5, normalised to sum 1
    double sum = 0.0;
    for (int k = 0; k < ADFP_MET_TAPS; ++k) { const double d = (double)(k - ADFP_MET_TAPS / 2); win.g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5)); sum += win.g[k]; }
    for (int k = 0; k < ADFP_MET_TAPS; ++k) win.g[k] /= sum;
    if (geom->gt_color_f64) met_launch<double>(p, win, gt_depth, (const double*)gt_color, depth, color, row, (double*)workspace, (hipStream_t)stream);
    else met_launch<float>(p, win, gt_depth, (const float*)gt_color, depth, color, row, (double*)workspace, (hipStream_t)stream);
    ADFP_CHECK_LAUNCH();
    return 0;
}
