// adfp_ingest.h -- frame ingestion on the device (the reference's BaseDataset.__getitem__, src/utils/datasets.py:77-113): the decoded
// uint8 colour image and the raw depth image go in as they are, and one launch writes the colour [H,W,3] (f32 or f64) and depth
// [H,W] (f32) tensors the reference returns, for every frame of a batch.
//
// Per output pixel, with no intermediate image in memory (the exact contract is stated in include/adfp.h):
//   A  colour byte / 255 in f64, channels in RGB order
//   B  cv2.resize(img_f64, (depth_w, depth_h)): bilinear, half-pixel centres, float coefficients, f64 products; horizontal pass first
//   C  cfg cam.crop_size: F.interpolate(bilinear, align_corners=True) of the f64 colour, F.interpolate(nearest) of the depth
//   D  cfg cam.crop_edge: [edge:-edge, edge:-edge]
//   depth = ((float)raw / png_depth_scale) * scale, two f32 roundings
//   U  (adfp_ingest_frames_undistort) lens undistortion in front of A: the source byte of pixel (y, x) is the fixed-point bilinear
//      remap of the decoded image through a 1/32-pixel map (adfp_undistort_map), pure integer arithmetic
//
// The stages a geometry needs are chosen per launch (a template argument): 1 colour tap (same size, no crop_size: Replica), 4 taps
// (resize only: ScanNet), or the general chain (crop_size: 4 taps of stage C, each 1 or 4 taps of stage B).  Threads run along the
// flattened output rows: a wave's stores are contiguous, its byte reads fall into a few contiguous segments of source rows, and a
// thread writes the three channels of its pixel.  The frame index is blockIdx.y.
#pragma once
#include <limits.h>
#include <math.h>
#include "adfp_device.h"

#define ADFP_ING_THREADS 256

enum { ING_COPY = 0, ING_RESIZE = 1, ING_GENERAL = 2 };

struct IngestArgs {
    const unsigned char* color[ADFP_INGEST_MAX_JOBS]; const void* depth[ADFP_INGEST_MAX_JOBS];
    void* color_out[ADFP_INGEST_MAX_JOBS]; float* depth_out[ADFP_INGEST_MAX_JOBS];
    int ch, cw, dh, dw;                            // decoded colour and depth images
    int mh, mw;                                    // the frame before the edge crop: crop_size, or the depth frame
    int oh, ow, edge;                              // output = [edge : mh - edge, edge : mw - edge]
    int resize, bgr, depth_f32;                    // uniform flags
    float png_depth_scale, scale;
    const int* map;                                // stage U: [ch][cw][2] fixed-point source positions, or null
};

// OpenCV's linear coefficient of destination index d (resize.cpp): the source position in f64, rounded to float; its floor and the
// float remainder.  The position is written as include/adfp.h states it; OpenCV multiplies by 1. / ((double)dst_n / src_n) instead,
// which gives the same float for the shipped geometries and the tests' shapes (adfp.h).
ADFP_DEV void ing_cv_coef(int d, int src_n, int dst_n, int& s, float& f) {
    f = (float)((d + 0.5) * (double)src_n / dst_n - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    f -= fl;
}

// Stage U: byte k of the undistorted pixel (y, x) of an [h][w][3] image.  The four taps of the map entry, each 0 outside the
// image, weighted in 1/1024ths.  The shifts come first: the sentinel (INT32_MIN) and any entry far outside give sx, sy whose
// successors cannot overflow, and the unsigned compares put them outside the image, so such an entry is 0 with no case of its own.
ADFP_DEV int ing_remap(const unsigned char* __restrict__ src, const int* __restrict__ map, int h, int w, int y, int x, int k) {
    const int2 m = ((const int2*)map)[(long long)y * w + x];
    const int sx = m.x >> 5, sy = m.y >> 5, fa = m.x & 31, fb = m.y & 31;
    const bool x0 = (unsigned)sx < (unsigned)w, x1 = (unsigned)(sx + 1) < (unsigned)w;
    const bool y0 = (unsigned)sy < (unsigned)h, y1 = (unsigned)(sy + 1) < (unsigned)h;
    const long long o = 3ll * ((long long)sy * w + sx) + k, row = 3ll * w;               // offsets; read only when inside
    const int p00 = y0 && x0 ? src[o] : 0, p01 = y0 && x1 ? src[o + 3] : 0;
    const int p10 = y1 && x0 ? src[o + row] : 0, p11 = y1 && x1 ? src[o + row + 3] : 0;
    return ((32 - fa) * (32 - fb) * p00 + fa * (32 - fb) * p01 + (32 - fa) * fb * p10 + fa * fb * p11 + 512) >> 10;
}

// Stage A: channel c (RGB order) of source pixel (y, x).
template <bool UNDISTORT>
ADFP_DEV double ing_byte(const IngestArgs& a, const unsigned char* __restrict__ src, int y, int x, int c) {
    if (UNDISTORT) return (double)ing_remap(src, a.map, a.ch, a.cw, y, x, a.bgr ? 2 - c : c) / 255.0;
    return (double)src[3ll * ((long long)y * a.cw + x) + (a.bgr ? 2 - c : c)] / 255.0;
}

// Stages A and B: the colour of depth-frame pixel (y, x).  In x a position left of the first or at / right of the last source
// column takes that column alone (sx = 0 or cw - 1, fx = 0); in y the two rows are clamped and keep their weights.
template <bool RESIZE, bool UNDISTORT>
ADFP_DEV void ing_base(const IngestArgs& a, const unsigned char* __restrict__ src, int y, int x, double* out) {
    if (!RESIZE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = ing_byte<UNDISTORT>(a, src, y, x, c);
        return;
    }
    int sx, sy; float fx, fy;
    ing_cv_coef(x, a.cw, a.dw, sx, fx);
    ing_cv_coef(y, a.ch, a.dh, sy, fy);
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= a.cw - 1) { sx = a.cw - 1; fx = 0.f; }
    const int sx1 = sx + 1 < a.cw ? sx + 1 : a.cw - 1;
    const int y0 = sy < 0 ? 0 : (sy > a.ch - 1 ? a.ch - 1 : sy);
    const int y1 = sy + 1 < 0 ? 0 : (sy + 1 > a.ch - 1 ? a.ch - 1 : sy + 1);
    const double a0 = (double)(1.f - fx), a1 = (double)fx, b0 = (double)(1.f - fy), b1 = (double)fy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double h0 = ing_byte<UNDISTORT>(a, src, y0, sx, c) * a0 + ing_byte<UNDISTORT>(a, src, y0, sx1, c) * a1;
        const double h1 = ing_byte<UNDISTORT>(a, src, y1, sx, c) * a0 + ing_byte<UNDISTORT>(a, src, y1, sx1, c) * a1;
        out[c] = h0 * b0 + h1 * b1;
    }
}

// torch's align_corners=True source index and weights for f64 (UpSample.h: compute_source_index_and_lambda).
ADFP_DEV void ing_torch_coef(int d, int in_n, int out_n, int& i0, int& i1, double& l0, double& l1) {
    if (in_n == out_n) { i0 = i1 = d; l0 = 1.0; l1 = 0.0; return; }
    const double ratio = out_n > 1 ? (double)(in_n - 1) / (double)(out_n - 1) : 0.0;
    const double real = ratio * d;
    i0 = (int)real;
    if (i0 > in_n - 1) i0 = in_n - 1;
    i1 = i0 + (i0 < in_n - 1 ? 1 : 0);
    l1 = real - (double)i0;
    l1 = l1 < 0.0 ? 0.0 : (l1 > 1.0 ? 1.0 : l1);
    l0 = 1.0 - l1;
}

// torch's nearest source index (UpSample.h: nearest_neighbor_compute_source_index with the float scale in / out).
ADFP_DEV int ing_nearest(int d, int in_n, int out_n) {
    const int s = (int)floorf((float)d * ((float)in_n / (float)out_n));
    return s < in_n - 1 ? s : in_n - 1;
}

template <int CASE, typename OutT, bool UNDISTORT>
__global__ __launch_bounds__(ADFP_ING_THREADS) void k_ingest(IngestArgs a) {
    const int p = blockIdx.x * ADFP_ING_THREADS + threadIdx.x;
    if (p >= a.oh * a.ow) return;
    const int job = blockIdx.y;
    const unsigned char* __restrict__ src = a.color[job];
    const int oy = p / a.ow, ox = p - oy * a.ow;
    const int my = oy + a.edge, mx = ox + a.edge;              // the pixel before the edge crop
    double rgb[3];
    int dy = my, dx = mx;                                      // the depth pixel it takes
    if (CASE == ING_COPY) {
        ing_base<false, UNDISTORT>(a, src, my, mx, rgb);
    } else if (CASE == ING_RESIZE) {
        ing_base<true, UNDISTORT>(a, src, my, mx, rgb);
    } else {
        int y0, y1, x0, x1; double hl0, hl1, wl0, wl1;
        ing_torch_coef(my, a.dh, a.mh, y0, y1, hl0, hl1);
        ing_torch_coef(mx, a.dw, a.mw, x0, x1, wl0, wl1);
        double v00[3], v01[3], v10[3], v11[3];
        if (UNDISTORT) {
            // One stage-C tap at a time, the sum in the order below: with all four unrolled, up to 16 remapped pixels of four
            // byte loads and three channels each are in flight and the kernel needs every VGPR there is.
#pragma unroll 1
            for (int t = 0; t < 4; ++t) {
                const int ty = t & 2 ? y1 : y0, tx = t & 1 ? x1 : x0;
                if (a.resize) ing_base<true, true>(a, src, ty, tx, v00);
                else ing_base<false, true>(a, src, ty, tx, v00);
                const double w = (t & 2 ? hl1 : hl0) * (t & 1 ? wl1 : wl0);
#pragma unroll
                for (int c = 0; c < 3; ++c) rgb[c] = t ? rgb[c] + w * v00[c] : w * v00[c];
            }
        } else {
            if (a.resize) {
                ing_base<true, false>(a, src, y0, x0, v00); ing_base<true, false>(a, src, y0, x1, v01);
                ing_base<true, false>(a, src, y1, x0, v10); ing_base<true, false>(a, src, y1, x1, v11);
            } else {
                ing_base<false, false>(a, src, y0, x0, v00); ing_base<false, false>(a, src, y0, x1, v01);
                ing_base<false, false>(a, src, y1, x0, v10); ing_base<false, false>(a, src, y1, x1, v11);
            }
            const double w00 = hl0 * wl0, w01 = hl0 * wl1, w10 = hl1 * wl0, w11 = hl1 * wl1;
#pragma unroll
            for (int c = 0; c < 3; ++c) rgb[c] = ((w00 * v00[c] + w01 * v01[c]) + w10 * v10[c]) + w11 * v11[c];
        }
        dy = ing_nearest(my, a.dh, a.mh);
        dx = ing_nearest(mx, a.dw, a.mw);
    }
    OutT* __restrict__ co = (OutT*)a.color_out[job] + 3ll * p;
    co[0] = (OutT)rgb[0]; co[1] = (OutT)rgb[1]; co[2] = (OutT)rgb[2];
    const long long di = (long long)dy * a.dw + dx;
    const float raw = a.depth_f32 ? ((const float*)a.depth[job])[di] : (float)((const unsigned short*)a.depth[job])[di];
    a.depth_out[job][p] = (raw / a.png_depth_scale) * a.scale;
}

// 0, or the error of a geometry; fills the sizes of a
static int ing_geometry(const adfp_ingest_geom* g, IngestArgs& a) {
    if (!g) return ADFP_E_ARG;
    if (g->color_h < 1 || g->color_w < 1 || g->depth_h < 1 || g->depth_w < 1) return ADFP_E_ARG;
    if (g->crop_h < 0 || g->crop_w < 0 || (g->crop_h == 0) != (g->crop_w == 0) || g->crop_edge < 0) return ADFP_E_ARG;
    if ((unsigned)g->color_order > 1u || (unsigned)g->depth_kind > 1u || (unsigned)g->color_out > 1u) return ADFP_E_ARG;
    const float s = g->png_depth_scale;
    if (!(s == s) || s - s != 0.f || s == 0.f) return ADFP_E_ARG;
    if (g->color_h > 32768 || g->color_w > 32768 || g->depth_h > 32768 || g->depth_w > 32768 || g->crop_h > 32768 || g->crop_w > 32768)
        return ADFP_E_UNSUPPORTED;
    a.ch = g->color_h; a.cw = g->color_w; a.dh = g->depth_h; a.dw = g->depth_w;
    a.mh = g->crop_h ? g->crop_h : g->depth_h; a.mw = g->crop_w ? g->crop_w : g->depth_w;
    a.edge = g->crop_edge;
    if (2 * a.edge >= a.mh || 2 * a.edge >= a.mw) return ADFP_E_ARG;
    a.oh = a.mh - 2 * a.edge; a.ow = a.mw - 2 * a.edge;
    a.resize = a.ch != a.dh || a.cw != a.dw;
    a.bgr = g->color_order == 0; a.depth_f32 = g->depth_kind == 1;
    a.png_depth_scale = g->png_depth_scale; a.scale = g->scale;
    return 0;
}

template <typename OutT, bool UNDISTORT>
static void ing_launch(const IngestArgs& a, int crop, dim3 grid, hipStream_t st) {
    if (crop) hipLaunchKernelGGL((k_ingest<ING_GENERAL, OutT, UNDISTORT>), grid, dim3(ADFP_ING_THREADS), 0, st, a);
    else if (a.resize) hipLaunchKernelGGL((k_ingest<ING_RESIZE, OutT, UNDISTORT>), grid, dim3(ADFP_ING_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_ingest<ING_COPY, OutT, UNDISTORT>), grid, dim3(ADFP_ING_THREADS), 0, st, a);
}

extern "C" int adfp_ingest_out_shape(const adfp_ingest_geom* geom, int* H, int* W) {
    IngestArgs a;
    const int rc = ing_geometry(geom, a);
    if (rc) return rc;
    if (!H || !W) return ADFP_E_ARG;
    *H = a.oh; *W = a.ow;
    return 0;
}

extern "C" int adfp_ingest_frames_undistort(const adfp_ingest_geom* geom, const int* map, int n_jobs, const adfp_ingest_job* jobs,
                                            void* stream) {
    IngestArgs a;
    const int rc = ing_geometry(geom, a);
    if (rc) return rc;
    if (n_jobs < 0 || ((uintptr_t)map & 7)) return ADFP_E_ARG;
    if (n_jobs > ADFP_INGEST_MAX_JOBS) return ADFP_E_UNSUPPORTED;
    if (n_jobs == 0) return 0;
    if (!jobs) return ADFP_E_ARG;
    for (int j = 0; j < ADFP_INGEST_MAX_JOBS; ++j) {
        const adfp_ingest_job& b = jobs[j < n_jobs ? j : 0];
        if (j < n_jobs && (!b.color || !b.depth || !b.color_out || !b.depth_out)) return ADFP_E_ARG;
        a.color[j] = b.color; a.depth[j] = b.depth; a.color_out[j] = b.color_out; a.depth_out[j] = b.depth_out;
    }
    a.map = map;
    const dim3 grid((unsigned)((a.oh * a.ow + ADFP_ING_THREADS - 1) / ADFP_ING_THREADS), (unsigned)n_jobs);
    const hipStream_t st = (hipStream_t)stream;
    if (map) {
        if (geom->color_out == 1) ing_launch<double, true>(a, geom->crop_h, grid, st);
        else ing_launch<float, true>(a, geom->crop_h, grid, st);
    } else {
        if (geom->color_out == 1) ing_launch<double, false>(a, geom->crop_h, grid, st);
        else ing_launch<float, false>(a, geom->crop_h, grid, st);
    }
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_ingest_frames(const adfp_ingest_geom* geom, int n_jobs, const adfp_ingest_job* jobs, void* stream) {
    return adfp_ingest_frames_undistort(geom, nullptr, n_jobs, jobs, stream);
}

// Stage U on its own: dst [h][w][3] = the remap of src [h][w][3]; a thread per pixel, its three bytes.
__global__ __launch_bounds__(ADFP_ING_THREADS) void k_undistort_image(const unsigned char* __restrict__ src, const int* __restrict__ map,
                                                                      int h, int w, unsigned char* __restrict__ dst) {
    const int p = blockIdx.x * ADFP_ING_THREADS + threadIdx.x;
    if (p >= h * w) return;
    const int y = p / w, x = p - y * w;
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[3ll * p + k] = (unsigned char)ing_remap(src, map, h, w, y, x, k);
}

extern "C" int adfp_undistort_image(const unsigned char* src, const int* map, int h, int w, unsigned char* dst, void* stream) {
    if (!src || !map || !dst || h < 1 || w < 1 || ((uintptr_t)map & 7)) return ADFP_E_ARG;
    if (h > 32768 || w > 32768) return ADFP_E_UNSUPPORTED;
    const dim3 grid((unsigned)((h * w + ADFP_ING_THREADS - 1) / ADFP_ING_THREADS));
    hipLaunchKernelGGL(k_undistort_image, grid, dim3(ADFP_ING_THREADS), 0, (hipStream_t)stream, src, map, h, w, dst);
    ADFP_CHECK_LAUNCH();
    return 0;
}

// The 1/32-pixel map of include/adfp.h "lens undistortion": every operation an f64 one in the order stated there, no contraction.
extern "C" int adfp_undistort_map(int color_h, int color_w, double fx, double fy, double cx, double cy, const double* dist, int n_dist,
                                  int* map) {
#pragma clang fp contract(off)
    if (!dist || !map || color_h < 1 || color_w < 1) return ADFP_E_ARG;
    if (!(fx - fx == 0.0) || !(fy - fy == 0.0) || !(cx - cx == 0.0) || !(cy - cy == 0.0) || fx == 0.0 || fy == 0.0) return ADFP_E_ARG;
    if ((n_dist != 4 && n_dist != 5 && n_dist != 8) || color_h > 32768 || color_w > 32768) return ADFP_E_UNSUPPORTED;
    double k[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n_dist; ++i) k[i] = dist[i];
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    const double lim = 1073741824.0;                                         // 2^30: clamped before the conversion to int
    for (int v = 0; v < color_h; ++v) {
        for (int u = 0; u < color_w; ++u) {
            const double x = ((double)u - cx) / fx, y = ((double)v - cy) / fy, r2 = x * x + y * y;
            const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * (2.0 * x * y) + p2 * (r2 + 2.0 * (x * x));
            const double yd = y * kr + p1 * (r2 + 2.0 * (y * y)) + p2 * (2.0 * x * y);
            const double U = fx * xd + cx, V = fy * yd + cy;
            int* m = map + 2ll * ((long long)v * color_w + u);
            if (!(U - U == 0.0) || !(V - V == 0.0)) { m[0] = m[1] = INT_MIN; continue; }
            const double su = 32.0 * U, sv = 32.0 * V;
            m[0] = (int)rint(su < -lim ? -lim : (su > lim ? lim : su));      // nearest-even under the default rounding mode
            m[1] = (int)rint(sv < -lim ? -lim : (sv > lim ? lim : sv));
        }
    }
    return 0;
}
