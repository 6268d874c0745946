// adfp_segments.h -- 3D line segments drawn into mesh views with the mesh in the way: trajectories and camera frusta over
// render_mesh.MeshViews' pictures.  Contract: include/adfp.h, "mesh views", adfp_draw_segments; tests/segments_ref.py restates it in
// numpy.  Every operation of the contract is one f64 operation in the order written (the build has no contraction), so the bytes
// are a function of the inputs alone: no float atomics, no global bins, one write per pixel.
//
//   k_seg_project   one lane per (view, slot of the view's list): the slot's segment (the ranges walked in order, a segment an
//                   earlier range holds already dropped), both endpoints to camera space, the near clip, the screen; a 64-byte
//                   record (u0, v0, w0, u1 - u0, v1 - v0, w1 - w0, L, index), index -1 for a slot that draws nothing
//   k_seg_draw      one 256-lane workgroup per 16 x 16 pixel tile and view; the view's records 256 at a time: each lane loads one
//                   and drops it when its box misses the tile's box grown by half_width + 1 (only for coordinates below 2^40, where
//                   the coverage test's own rounding is far below the pixel of margin: dropping never changes a byte), the rest
//                   are packed into LDS by wave ballots (at most 256 a pass: nothing can overflow); then every pixel tests the
//                   packed records and keeps (z, index) in registers.  The winner is the minimum of (z, index) over a set, so it
//                   does not depend on the order the records arrive in.
#pragma once
#include "adfp_device.h"

#define ADFP_SEG_THREADS 256
#define ADFP_SEG_TILE 16
#define ADFP_SEG_MAX_RANGES 8
#define ADFP_SEG_EXACT_BOX 1099511627776.0                // 2^40: below it a coordinate's rounding stays under 2^-12 pixel
#define ADFP_SEG_MAX_RECORDS (1ll << 34)                   // views x slots of one call: a terabyte of records

struct SegRecord { double u0, v0, w0, ax, ay, dw, L; int k, pad; };     // 64 bytes

struct SegArgs {
    unsigned char* rgb; const float* depth; int* seg;        // [views][H][W][3], [views][H][W] or NULL, [views][H][W] or NULL
    int H, W, nbx, view0;
    const double* c2w; double fx, fy, cx, cy;                 // [views][12]
    const double* segments; const unsigned char* colors; int n_seg;
    const long long* ranges; int n_ranges; int n_listed;      // [views][n_ranges][2] or NULL
    double hw2, margin, near_clip, bias_rel, bias_abs, alpha;
    SegRecord* rec;                                           // [views][n_listed]
};

ADFP_DEV bool seg_pose_ok(const double* m) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 12; ++c) ok = ok && isfinite(m[c]);
    return ok;
}

// the vertex transform of the depth render: e = P - o, cam_c = ((R0c e0 + R1c e1) + R2c e2)
ADFP_DEV void seg_to_camera(const double* m, const double* P, double* cam) {
    const double e0 = P[0] - m[3], e1 = P[1] - m[7], e2 = P[2] - m[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) cam[c] = (m[c] * e0 + m[4 + c] * e1) + m[8 + c] * e2;
}

// slot j of view v's list -> its segment index, or -1: past the list's end, or held by an earlier range already
ADFP_DEV int seg_of_slot(const SegArgs& a, long long view, int j) {
    if (!a.ranges) return j < a.n_seg ? j : -1;
    const long long* r = a.ranges + view * a.n_ranges * 2;
    long long left = j;
    for (int q = 0; q < a.n_ranges; ++q) {
        long long b = r[2 * q], e = r[2 * q + 1];
        b = b < 0 ? 0 : b;
        e = e > a.n_seg ? a.n_seg : e;
        const long long len = e > b ? e - b : 0;
        if (left < len) {
            const long long k = b + left;
            for (int p = 0; p < q; ++p)
                if (k >= r[2 * p] && k < r[2 * p + 1]) return -1;
            return (int)k;
        }
        left -= len;
    }
    return -1;
}

__global__ __launch_bounds__(ADFP_SEG_THREADS) void k_seg_project(SegArgs a) {
    const int j = (int)(blockIdx.x * ADFP_SEG_THREADS + threadIdx.x);
    if (j >= a.n_listed) return;
    const long long view = (long long)a.view0 + blockIdx.y;
    SegRecord out;
    out.u0 = out.v0 = out.w0 = out.ax = out.ay = out.dw = out.L = 0.0;
    out.k = -1; out.pad = 0;
    SegRecord* dst = a.rec + view * a.n_listed + j;
    const double* m = a.c2w + 12 * view;
    const int k = seg_pose_ok(m) ? seg_of_slot(a, view, j) : -1;
    if (k < 0) { *dst = out; return; }
    const double* P = a.segments + 6 * (long long)k;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) ok = ok && isfinite(P[c]);
    double A[3], B[3];
    seg_to_camera(m, P, A);
    seg_to_camera(m, P + 3, B);
    const double nc = a.near_clip;
    if (A[2] < nc && B[2] < nc) ok = false;
    if (ok && A[2] < nc) {
        const double t = (nc - A[2]) / (B[2] - A[2]);
        A[0] = A[0] + t * (B[0] - A[0]); A[1] = A[1] + t * (B[1] - A[1]); A[2] = nc;
    } else if (ok && B[2] < nc) {
        const double t = (nc - B[2]) / (A[2] - B[2]);
        B[0] = B[0] + t * (A[0] - B[0]); B[1] = B[1] + t * (A[1] - B[1]); B[2] = nc;
    }
    const double u0 = a.fx * (A[0] / A[2]) + a.cx, v0 = a.fy * (A[1] / A[2]) + a.cy, w0 = 1.0 / A[2];
    const double u1 = a.fx * (B[0] / B[2]) + a.cx, v1 = a.fy * (B[1] / B[2]) + a.cy, w1 = 1.0 / B[2];
    ok = ok && isfinite(u0) && isfinite(v0) && isfinite(w0) && isfinite(u1) && isfinite(v1) && isfinite(w1);
    if (ok) {
        out.u0 = u0; out.v0 = v0; out.w0 = w0;
        out.ax = u1 - u0; out.ay = v1 - v0; out.dw = w1 - w0;
        out.L = out.ax * out.ax + out.ay * out.ay;
        out.k = k;
    }
    *dst = out;
}

__global__ __launch_bounds__(ADFP_SEG_THREADS) void k_seg_draw(SegArgs a) {
    __shared__ SegRecord s_rec[ADFP_SEG_THREADS];
    __shared__ int s_wave[ADFP_SEG_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long view = (long long)a.view0 + blockIdx.y;
    const int by = (int)blockIdx.x / a.nbx, bx = (int)blockIdx.x - by * a.nbx;
    const int row = by * ADFP_SEG_TILE + (tid >> 4), col = bx * ADFP_SEG_TILE + (tid & 15);
    const bool inside = row < a.H && col < a.W;
    const long long px = (view * a.H + row) * a.W + col;
    if (!seg_pose_ok(a.c2w + 12 * view)) {                    // the whole workgroup takes this branch or none of it
        if (inside && a.seg) a.seg[px] = -1;
        return;
    }
    // the tile's pixel centres, grown: a covered pixel lies within half_width of a point of the segment's box
    const double tx0 = (double)(bx * ADFP_SEG_TILE) - a.margin, tx1 = (double)(bx * ADFP_SEG_TILE + ADFP_SEG_TILE - 1) + a.margin;
    const double ty0 = (double)(by * ADFP_SEG_TILE) - a.margin, ty1 = (double)(by * ADFP_SEG_TILE + ADFP_SEG_TILE - 1) + a.margin;
    const double pj = (double)col, pi = (double)row;
    double best_z = 0.0;
    int best_k = -1;
    const SegRecord* rec = a.rec + view * a.n_listed;
    for (int base = 0; base < a.n_listed; base += ADFP_SEG_THREADS) {
        double u0 = 0.0, v0 = 0.0, w0 = 0.0, ax = 0.0, ay = 0.0, dw = 0.0, L = 0.0;
        int k = -1;
        if (base + tid < a.n_listed) {
            const SegRecord* g = rec + base + tid;
            u0 = g->u0; v0 = g->v0; w0 = g->w0; ax = g->ax; ay = g->ay; dw = g->dw; L = g->L; k = g->k;
        }
        bool keep = k >= 0;
        if (keep) {
            const double u1 = u0 + ax, v1 = v0 + ay;
            const double big = ADFP_SEG_EXACT_BOX;
            if (fabs(u0) < big && fabs(v0) < big && fabs(u1) < big && fabs(v1) < big) {
                const double lo_u = fmin(u0, u1), hi_u = fmax(u0, u1), lo_v = fmin(v0, v1), hi_v = fmax(v0, v1);
                if (hi_u < tx0 || lo_u > tx1 || hi_v < ty0 || lo_v > ty1) keep = false;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wave[wv] = __popcll(mask);
        __syncthreads();                                       // s_wave is complete; every wave is done with the last pass's s_rec
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < ADFP_SEG_THREADS / 64; ++w) {
            const int c = s_wave[w];
            before += w < wv ? c : 0;
            total += c;
        }
        if (keep) {
            SegRecord* d = s_rec + before + __popcll(mask & ((1ull << lane) - 1ull));
            d->u0 = u0; d->v0 = v0; d->w0 = w0; d->ax = ax; d->ay = ay; d->dw = dw; d->L = L; d->k = k;
        }
        __syncthreads();                                       // s_rec is complete; s_wave is free for the next pass
        if (inside) {
            for (int n = 0; n < total; ++n) {
                const SegRecord& e = s_rec[n];                 // the same address in every lane: a broadcast
                const double qx0 = pj - e.u0, qy0 = pi - e.v0;
                double s = e.L == 0.0 ? 0.0 : (qx0 * e.ax + qy0 * e.ay) / e.L;
                s = s > 0.0 ? s : 0.0;                         // NaN goes to 0
                s = s > 1.0 ? 1.0 : s;
                const double qx = qx0 - s * e.ax, qy = qy0 - s * e.ay;
                if (qx * qx + qy * qy <= a.hw2) {
                    const double z = 1.0 / (e.w0 + s * e.dw);
                    if (best_k < 0 || z < best_z || (z == best_z && e.k < best_k)) { best_z = z; best_k = e.k; }
                }
            }
        }
    }
    if (!inside) return;
    if (a.seg) a.seg[px] = best_k;
    if (best_k < 0) return;
    bool visible = true;
    if (a.depth) {
        const double D = (double)a.depth[px];
        visible = D == 0.0 || best_z <= D * (1.0 + a.bias_rel) + a.bias_abs;
    }
    const unsigned char* c = a.colors + 3 * (long long)best_k;
    unsigned char* p = a.rgb + 3 * px;
    if (visible) {
        p[0] = c[0]; p[1] = c[1]; p[2] = c[2];
    } else if (a.alpha > 0.0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = (unsigned char)floor((a.alpha * (double)c[q] + (1.0 - a.alpha) * (double)p[q]) + 0.5);
    }
}

// ---- host side: the launcher ----
extern "C" {

static SegRecord* seg_layout(Arena& A, long long n_views, long long n_listed) {
    return A.take<SegRecord>((size_t)n_views * (size_t)n_listed);
}
size_t adfp_draw_segments_workspace_bytes(long long n_views, long long n_listed) {
    if (n_views <= 0 || n_listed <= 0 || n_views > RECON_MAX_N || n_listed > RECON_MAX_N) return 0;
    if (n_views * n_listed > ADFP_SEG_MAX_RECORDS) return 0;
    return layout_bytes(seg_layout, n_views, n_listed);
}

int adfp_draw_segments(unsigned char* rgb, const float* depth, int* seg, long long n_views, int H, int W, const double* c2w,
                       double fx, double fy, double cx, double cy, const double* segments, const unsigned char* colors,
                       long long n_seg, const long long* ranges, int n_ranges, long long n_listed, double half_width,
                       double near_clip, double bias_rel, double bias_abs, double hidden_alpha, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!rgb || !c2w || n_views < 0 || n_seg < 0 || H <= 0 || W <= 0) return ADFP_E_ARG;
    if (n_seg > 0 && (!segments || !colors)) return ADFP_E_ARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if (!(half_width > 0.0) || !(half_width <= 64.0)) return ADFP_E_ARG;
    if (!(near_clip > 0.0) || !isfinite(near_clip)) return ADFP_E_ARG;
    if (!(bias_rel >= 0.0) || !(bias_abs >= 0.0) || !isfinite(bias_rel) || !isfinite(bias_abs)) return ADFP_E_ARG;
    if (!(hidden_alpha >= 0.0) || !(hidden_alpha <= 1.0)) return ADFP_E_ARG;
    if (ranges && (n_ranges < 1 || n_ranges > ADFP_SEG_MAX_RANGES || n_listed < 0)) return ADFP_E_ARG;
    if (H > RT_MAX_SIDE || W > RT_MAX_SIDE || n_views > RECON_MAX_N || n_seg > RECON_MAX_N || (ranges && n_listed > RECON_MAX_N))
        return ADFP_E_UNSUPPORTED;
    if (!ranges) n_listed = n_seg;
    if (n_views * n_listed > ADFP_SEG_MAX_RECORDS) return ADFP_E_UNSUPPORTED;
    if (n_views == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_seg == 0 || n_listed == 0) {                          // nothing listed anywhere: rgb as it is, seg = -1
        hipError_t e = seg ? hipMemsetAsync(seg, 0xff, (size_t)n_views * H * W * sizeof(int), st) : hipSuccess;
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!workspace || workspace_bytes < adfp_draw_segments_workspace_bytes(n_views, n_listed)) return ADFP_E_ARG;
    Arena A(workspace);
    SegArgs a;
    a.rgb = rgb; a.depth = depth; a.seg = seg; a.H = H; a.W = W; a.nbx = (int)ceil_div(W, ADFP_SEG_TILE);
    a.c2w = c2w; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.segments = segments; a.colors = colors; a.n_seg = (int)n_seg;
    a.ranges = ranges; a.n_ranges = ranges ? n_ranges : 0; a.n_listed = (int)n_listed;
    a.hw2 = half_width * half_width; a.margin = half_width + 1.0; a.near_clip = near_clip;
    a.bias_rel = bias_rel; a.bias_abs = bias_abs; a.alpha = hidden_alpha;
    a.rec = seg_layout(A, n_views, n_listed);
    const unsigned nslot = (unsigned)ceil_div(n_listed, ADFP_SEG_THREADS);
    const unsigned ntile = (unsigned)a.nbx * (unsigned)ceil_div(H, ADFP_SEG_TILE);
    for (long long v0 = 0; v0 < n_views; v0 += RT_VIEWS_PER_LAUNCH) {
        const long long nv = n_views - v0 < RT_VIEWS_PER_LAUNCH ? n_views - v0 : RT_VIEWS_PER_LAUNCH;
        a.view0 = (int)v0;
        hipLaunchKernelGGL(k_seg_project, dim3(nslot, (unsigned)nv), dim3(ADFP_SEG_THREADS), 0, st, a);
        ADFP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_seg_draw, dim3(ntile, (unsigned)nv), dim3(ADFP_SEG_THREADS), 0, st, a);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

}   // extern "C"
