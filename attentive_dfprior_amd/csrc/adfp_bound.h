// adfp_bound.h -- the mesh bound on the device: the point work of a quickhull in rounds over the keyframes' camera centres and
// back-projected valid depth pixels (mesher.Mesher.get_bound_planes does it with numpy and Qhull on the host).  Contracts and the
// fixed formulae: include/adfp.h, "mesh bound".  The facet topology of the few hundred hull vertices stays with Qhull on the host
// (mesh.depth_hull); the points are never stored: every kernel recomputes a point from its id, the depth block and the poses.
//
//   support     tiles of 1024 consecutive ids; a workgroup stages the tile's coordinates in LDS (NaN for ids that are no point),
//               then lane <-> direction: every lane walks the tile's points in ascending id against ITS direction, so the LDS reads
//               are broadcasts and the running best needs no reduction inside the loop.  Per-workgroup bests go to the workspace,
//               a second launch folds them in a fixed order: no atomics.
//   classify    count / scan / emit: one pass evaluates every candidate against the planes (planes in LDS in chunks of 512, four
//               candidates per lane per plane read) and leaves one bit per candidate and a count per tile of 1024; one workgroup
//               scans the tile counts (adfp_scan.h: k_tile_scan); the emit pass writes the surviving ids in ascending position.  The
//               per-facet farthest is two passes over the survivors: the distance's bit pattern (positive, so monotone as an
//               integer) through an LDS max per workgroup and one 64-bit vector atomic max per touched facet per workgroup, then
//               the lowest id among the survivors that attain it (atomic min).  Max and min of integers: the order the atomics
//               land in decides nothing.
#pragma once
#include "adfp_device.h"
#include "adfp_scan.h"

#define ADFP_BND_THREADS 256
#define ADFP_BND_PER 4
#define ADFP_BND_TILE (ADFP_BND_THREADS * ADFP_BND_PER)
#define ADFP_BND_SCAN_PER 8           // tile counts per lane and round of the one-workgroup scan (adfp_scan.h: k_tile_scan)
#define ADFP_BND_PLANES 512              // planes per LDS chunk (16 KB)
#define ADFP_BND_FARS 4096               // facets whose farthest distance is reduced in LDS first (32 KB); the rest go to memory directly
#define ADFP_BND_SUP_BLOCKS 1024         // workgroups (per 256 directions) of the support pass
#define ADFP_BND_FAR_BLOCKS 2048         // workgroups of the farthest passes

struct BndScene { const float* depth; const float* poses; long long K; int H, W; long long HW1; long long n_ids; double fx, fy, cx, cy; };

// The point of an id (include/adfp.h, "mesh bound": pose, validity, camera point, world point).  false: the id names no point (out
// of range, or a pixel without a valid depth); nothing is read for an id out of range.
ADFP_DEV bool bnd_point(const BndScene& s, long long id, double p[3]) {
    if (id < 0 || id >= s.n_ids) return false;
    const long long k = id / s.HW1, j = id - k * s.HW1;
    const float* __restrict__ P = s.poses + 16 * k;
    if (j == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = (double)P[4 * c + 3];
        return true;
    }
    const unsigned pix = (unsigned)(j - 1);
    const unsigned row = pix / (unsigned)s.W, col = pix - row * (unsigned)s.W;
    const double d = (double)s.depth[k * (s.HW1 - 1) + pix];
    if (!(d > 0.0 && d < 1000.0)) return false;
    const double x = (((double)col - s.cx) / s.fx) * d, y = (((double)row - s.cy) / s.fy) * d;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        p[c] = (((double)P[4 * c] * x + (-(double)P[4 * c + 1]) * y) + (-(double)P[4 * c + 2]) * d) + (double)P[4 * c + 3];
    return true;
}
ADFP_DEV bool bnd_finite(const double p[3]) { return fabs(p[0]) < INFINITY && fabs(p[1]) < INFINITY && fabs(p[2]) < INFINITY; }

// ---- support pass ----
struct BndSupport { BndScene s; const double* dirs; int D; long long n_tiles; int nbx;
                    double* part_dot; long long* part_id;        // [nbx][D]
                    double* part_box; long long* part_cnt;       // [nbx][6], [nbx][2]
                    long long* best_id; double* aabb; long long* counts; };

__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_support(BndSupport a) {
    __shared__ double sp[3 * ADFP_BND_TILE];
    __shared__ long long s_id[ADFP_BND_THREADS];
    __shared__ long long s_cnt[2 * ADFP_BND_THREADS];
    const int c0 = blockIdx.y * ADFP_BND_THREADS;
    const int nd = a.D - c0 < ADFP_BND_THREADS ? a.D - c0 : ADFP_BND_THREADS;
    const int S = ADFP_BND_THREADS / nd;                       // slices of the tile: lane = (slice, direction)
    const bool active = (int)threadIdx.x < S * nd;
    const int dd = threadIdx.x % nd, slice = threadIdx.x / nd;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (active) { dx = a.dirs[3 * (c0 + dd)]; dy = a.dirs[3 * (c0 + dd) + 1]; dz = a.dirs[3 * (c0 + dd) + 2]; }
    double best = -INFINITY;
    long long bid = -1;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long nv = 0, nn = 0;
    for (long long t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        __syncthreads();                                       // the previous tile has been read
#pragma unroll
        for (int q = 0; q < ADFP_BND_PER; ++q) {
            const int i = q * ADFP_BND_THREADS + threadIdx.x;
            double p[3];
            const bool ok = bnd_point(a.s, t * ADFP_BND_TILE + i, p);
            const bool fin = ok && bnd_finite(p);
            if (fin) {
                ++nv;
#pragma unroll
                for (int c = 0; c < 3; ++c) { lo[c] = p[c] < lo[c] ? p[c] : lo[c]; hi[c] = p[c] > hi[c] ? p[c] : hi[c]; }
            } else if (ok) ++nn;
#pragma unroll
            for (int c = 0; c < 3; ++c) sp[c * ADFP_BND_TILE + i] = fin ? p[c] : (double)NAN;
        }
        __syncthreads();
        if (active) {
            const long long id0 = t * ADFP_BND_TILE;
            for (int i = slice; i < ADFP_BND_TILE; i += S) {   // ascending id: a strict > keeps the lowest id among equals
                const double dot = (dx * sp[i] + dy * sp[ADFP_BND_TILE + i]) + dz * sp[2 * ADFP_BND_TILE + i];
                if (dot > best) { best = dot; bid = id0 + i; }
            }
        }
    }
    __syncthreads();
    // fold the slices of each direction (ids of different slices interleave: compare the ids)
    sp[threadIdx.x] = best;
    s_id[threadIdx.x] = bid;
    __syncthreads();
    if (active && slice == 0) {
        for (int sl = 1; sl < S; ++sl) {
            const double o = sp[sl * nd + dd];
            const long long oi = s_id[sl * nd + dd];
            if (o > best || (o == best && (unsigned long long)oi < (unsigned long long)bid)) { best = o; bid = oi; }
        }
        a.part_dot[(long long)blockIdx.x * a.D + c0 + dd] = best;
        a.part_id[(long long)blockIdx.x * a.D + c0 + dd] = bid;
    }
    if (blockIdx.y != 0) return;                               // block-uniform
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) { sp[c * ADFP_BND_THREADS + threadIdx.x] = lo[c]; sp[(3 + c) * ADFP_BND_THREADS + threadIdx.x] = hi[c]; }
    s_cnt[threadIdx.x] = nv;
    s_cnt[ADFP_BND_THREADS + threadIdx.x] = nn;
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool mx = threadIdx.x >= 3;
        double r = sp[threadIdx.x * ADFP_BND_THREADS];
        for (int i = 1; i < ADFP_BND_THREADS; ++i) {
            const double o = sp[threadIdx.x * ADFP_BND_THREADS + i];
            r = mx ? (o > r ? o : r) : (o < r ? o : r);
        }
        a.part_box[(long long)blockIdx.x * 6 + threadIdx.x] = r;
    } else if (threadIdx.x < 8) {
        long long r = 0;
        for (int i = 0; i < ADFP_BND_THREADS; ++i) r += s_cnt[(threadIdx.x - 6) * ADFP_BND_THREADS + i];
        a.part_cnt[(long long)blockIdx.x * 2 + threadIdx.x - 6] = r;
    }
}

// workgroup b < D: the best of direction b over the nbx partials (the lowest id among equal dots); workgroup D: box and counts
__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_support_fold(BndSupport a) {
    __shared__ double s_dot[ADFP_BND_THREADS];
    __shared__ long long s_id[ADFP_BND_THREADS];
    if ((int)blockIdx.x == a.D) {
        if (threadIdx.x < 6) {
            const bool mx = threadIdx.x >= 3;
            double r = mx ? -INFINITY : INFINITY;
            for (int i = 0; i < a.nbx; ++i) {
                const double o = a.part_box[(long long)i * 6 + threadIdx.x];
                r = mx ? (o > r ? o : r) : (o < r ? o : r);
            }
            a.aabb[threadIdx.x] = r;
        } else if (threadIdx.x < 8) {
            long long r = 0;
            for (int i = 0; i < a.nbx; ++i) r += a.part_cnt[(long long)i * 2 + threadIdx.x - 6];
            a.counts[threadIdx.x - 6] = r;
        }
        return;
    }
    double best = -INFINITY;
    long long bid = -1;
    for (int i = threadIdx.x; i < a.nbx; i += ADFP_BND_THREADS) {
        const double o = a.part_dot[(long long)i * a.D + blockIdx.x];
        const long long oi = a.part_id[(long long)i * a.D + blockIdx.x];
        if (o > best || (o == best && (unsigned long long)oi < (unsigned long long)bid)) { best = o; bid = oi; }
    }
    s_dot[threadIdx.x] = best;
    s_id[threadIdx.x] = bid;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < ADFP_BND_THREADS; ++i) {
            const double o = s_dot[i];
            const long long oi = s_id[i];
            if (o > best || (o == best && (unsigned long long)oi < (unsigned long long)bid)) { best = o; bid = oi; }
        }
        a.best_id[blockIdx.x] = bid;
    }
}

// ---- classify ----
struct BndClassify { BndScene s; const long long* ids_in; long long n_in; const double* planes; int F; double eps;
                     unsigned long long* mask; unsigned* tile_counts; const long long* tile_offsets;
                     long long* ids_out; long long ids_cap; const long long* count;
                     unsigned long long* far_bits; unsigned long long* far_id; };

// m[q] = max_f s_f of the lane's four points, formed by `s > m` from -inf in facet order, so that fac[q] is the lowest facet that
// attains it (-1 and -inf for a NaN point).  Every lane of the workgroup calls it (barriers inside); sp: ADFP_BND_PLANES x 4 doubles.
ADFP_DEV void bnd_planes_max(const double* __restrict__ planes, int F, double* sp, const double (*p)[3], double* m, int* fac) {
#pragma unroll
    for (int q = 0; q < ADFP_BND_PER; ++q) { m[q] = -INFINITY; fac[q] = -1; }
    for (int f0 = 0; f0 < F; f0 += ADFP_BND_PLANES) {
        const int nf = F - f0 < ADFP_BND_PLANES ? F - f0 : ADFP_BND_PLANES;
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * nf; i += ADFP_BND_THREADS) sp[i] = planes[4 * (long long)f0 + i];
        __syncthreads();
        for (int f = 0; f < nf; ++f) {
            const double nx = sp[4 * f], ny = sp[4 * f + 1], nz = sp[4 * f + 2], d = sp[4 * f + 3];
#pragma unroll
            for (int q = 0; q < ADFP_BND_PER; ++q) {
                const double s = ((nx * p[q][0] + ny * p[q][1]) + nz * p[q][2]) + d;
                if (s > m[q]) { m[q] = s; fac[q] = f0 + f; }
            }
        }
    }
}

// candidate i of the call: its id (ids_in, or i itself) and its point (NaN when it is none)
ADFP_DEV long long bnd_candidate(const BndScene& s, const long long* ids, long long i, long long n, double p[3]) {
    long long id = -1;
    if (i < n) id = ids ? ids[i] : i;
    if (!bnd_point(s, id, p)) p[0] = p[1] = p[2] = (double)NAN;
    return id;
}

// count pass: one bit per candidate (bit i & 63 of word i >> 6), one count per tile
__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_flag(BndClassify a) {
    __shared__ double sp[4 * ADFP_BND_PLANES];
    __shared__ unsigned s_c[ADFP_BND_THREADS / 64];
    const long long i0 = (long long)blockIdx.x * ADFP_BND_TILE;
    double p[ADFP_BND_PER][3], m[ADFP_BND_PER];
    int fac[ADFP_BND_PER];
#pragma unroll
    for (int q = 0; q < ADFP_BND_PER; ++q) bnd_candidate(a.s, a.ids_in, i0 + q * ADFP_BND_THREADS + threadIdx.x, a.n_in, p[q]);
    bnd_planes_max(a.planes, a.F, sp, p, m, fac);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < ADFP_BND_PER; ++q) {
        const unsigned long long b = __ballot(m[q] > a.eps);
        if (lane == 0) a.mask[(long long)blockIdx.x * (ADFP_BND_TILE / 64) + q * (ADFP_BND_THREADS / 64) + wave] = b;
        c += (unsigned)__popcll(b);
    }
    if (lane == 0) s_c[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) a.tile_counts[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

// emit pass: the surviving ids at tile_offsets[tile] + the set bits before them; nothing is written at or past ids_cap
__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_emit(BndClassify a) {
    __shared__ unsigned long long s_w[ADFP_BND_TILE / 64];
    if (threadIdx.x < ADFP_BND_TILE / 64) s_w[threadIdx.x] = a.mask[(long long)blockIdx.x * (ADFP_BND_TILE / 64) + threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = a.tile_offsets[blockIdx.x];
#pragma unroll
    for (int q = 0; q < ADFP_BND_PER; ++q) {
        const int w = q * (ADFP_BND_THREADS / 64) + wave;
        const unsigned long long word = s_w[w];
        if (!((word >> lane) & 1ull)) continue;
        long long pos = base + __popcll(word & ((1ull << lane) - 1ull));
        for (int u = 0; u < w; ++u) pos += __popcll(s_w[u]);
        const long long i = (long long)blockIdx.x * ADFP_BND_TILE + q * ADFP_BND_THREADS + threadIdx.x;
        if (pos < a.ids_cap) a.ids_out[pos] = a.ids_in ? a.ids_in[i] : i;
    }
}

// PASS 0: far_bits[f] = the largest bit pattern of m over the survivors assigned to facet f; PASS 1: far_id[f] = the lowest id among
// those that attain it.  Workgroups stride over the tiles of the survivor list, whose length is read from the device.
template <int PASS>
__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_far(BndClassify a) {
    __shared__ double sp[4 * ADFP_BND_PLANES];
    __shared__ unsigned long long s_far[PASS == 0 ? ADFP_BND_FARS : 1];
    long long n = a.count[0];
    n = n < a.ids_cap ? n : a.ids_cap;
    const int nl = a.F < ADFP_BND_FARS ? a.F : ADFP_BND_FARS;
    if (PASS == 0) for (int i = threadIdx.x; i < nl; i += ADFP_BND_THREADS) s_far[i] = 0ull;
    const long long n_tiles = (n + ADFP_BND_TILE - 1) / ADFP_BND_TILE;
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {          // block-uniform trip count (barriers inside)
        double p[ADFP_BND_PER][3], m[ADFP_BND_PER];
        int fac[ADFP_BND_PER];
        long long id[ADFP_BND_PER];
#pragma unroll
        for (int q = 0; q < ADFP_BND_PER; ++q) id[q] = bnd_candidate(a.s, a.ids_out, t * ADFP_BND_TILE + q * ADFP_BND_THREADS + threadIdx.x, n, p[q]);
        bnd_planes_max(a.planes, a.F, sp, p, m, fac);                       // its first barrier also orders the zeroing of s_far
#pragma unroll
        for (int q = 0; q < ADFP_BND_PER; ++q) {
            if (fac[q] < 0 || !(m[q] > a.eps)) continue;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(m[q]);
            if (PASS == 0) {
                if (fac[q] < ADFP_BND_FARS) atomicMax(&s_far[fac[q]], bits);
                else atomicMax(&a.far_bits[fac[q]], bits);
            } else if (a.far_bits[fac[q]] == bits) atomicMin(&a.far_id[fac[q]], (unsigned long long)id[q]);
        }
    }
    if (PASS == 0) {
        __syncthreads();
        for (int i = threadIdx.x; i < nl; i += ADFP_BND_THREADS) {
            const unsigned long long v = s_far[i];
            if (v) atomicMax(&a.far_bits[i], v);
        }
    }
}

// coordinates of n ids: out [n][3]; NaN for an id that names no point
__global__ __launch_bounds__(ADFP_BND_THREADS) void k_bnd_points(BndScene s, const long long* __restrict__ ids, long long n, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ADFP_BND_THREADS + threadIdx.x;
    if (i >= n) return;
    double p[3];
    if (!bnd_point(s, ids[i], p)) p[0] = p[1] = p[2] = (double)NAN;
    out[3 * i] = p[0]; out[3 * i + 1] = p[1]; out[3 * i + 2] = p[2];
}

// ---- host side: the launchers ----
static const long long BND_MAX_IDS = 1ll << 40;                    // tile numbers stay int
static long long bnd_tiles(long long n) { return ceil_div(n, ADFP_BND_TILE); }
static bool bnd_finite_host(double x) { return x == x && x - x == 0.0; }
// 0, or the error of a scene description; fills s
static int bnd_scene(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy, BndScene& s) {
    if (K < 0 || H < 1 || W < 1) return ADFP_E_ARG;
    if (!bnd_finite_host(fx) || !bnd_finite_host(fy) || fx == 0.0 || fy == 0.0 || !bnd_finite_host(cx) || !bnd_finite_host(cy)) return ADFP_E_ARG;
    if (K > 0 && (!depth || !poses)) return ADFP_E_ARG;
    if (H > 32768 || W > 32768) return ADFP_E_UNSUPPORTED;
    s.depth = depth; s.poses = poses; s.K = K; s.H = H; s.W = W; s.HW1 = (long long)H * W + 1;
    if (K > BND_MAX_IDS / s.HW1) return ADFP_E_UNSUPPORTED;
    s.n_ids = K * s.HW1; s.fx = fx; s.fy = fy; s.cx = cx; s.cy = cy;
    return 0;
}
static int bnd_sup_blocks(long long n_ids) { const long long t = bnd_tiles(n_ids); return (int)(t < ADFP_BND_SUP_BLOCKS ? t : ADFP_BND_SUP_BLOCKS); }

extern "C" {

// the partials of the support pass's a.nbx workgroups
static void bnd_support_layout(Arena& A, BndSupport& a) {
    const size_t nb = (size_t)a.nbx;
    a.part_dot = A.take<double>(nb * a.D);
    a.part_id = A.take<long long>(nb * a.D);
    a.part_box = A.take<double>(nb * 6);
    a.part_cnt = A.take<long long>(nb * 2);
}
size_t adfp_bound_support_workspace_bytes(long long K, int H, int W, int D) {
    if (K <= 0 || H < 1 || W < 1 || H > 32768 || W > 32768 || D < 1 || D > ADFP_BOUND_MAX_DIRECTIONS) return 0;
    if (K > BND_MAX_IDS / ((long long)H * W + 1)) return 0;
    BndSupport a;
    a.D = D; a.nbx = bnd_sup_blocks(K * ((long long)H * W + 1));
    return layout_bytes(bnd_support_layout, a);
}

int adfp_bound_support(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                       const double* directions, int D, void* workspace, size_t workspace_bytes, long long* best_id, double* aabb,
                       long long* counts, void* stream) {
    BndSupport a;
    const int rc = bnd_scene(depth, poses, K, H, W, fx, fy, cx, cy, a.s);
    if (rc) return rc;
    if (D < 1 || D > ADFP_BOUND_MAX_DIRECTIONS || !directions || !best_id || !aabb || !counts) return ADFP_E_ARG;
    if (K == 0) return 0;
    if (!workspace) return ADFP_E_ARG;
    if (workspace_bytes < adfp_bound_support_workspace_bytes(K, H, W, D)) return ADFP_E_WORKSPACE;
    a.dirs = directions; a.D = D; a.n_tiles = bnd_tiles(a.s.n_ids); a.nbx = bnd_sup_blocks(a.s.n_ids);
    Arena A(workspace);
    bnd_support_layout(A, a);
    a.best_id = best_id; a.aabb = aabb; a.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bnd_support, dim3((unsigned)a.nbx, (unsigned)ceil_div(D, ADFP_BND_THREADS)), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bnd_support_fold, dim3((unsigned)D + 1), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

// the inside mask (a bit per id), the tile counts and their exclusive prefix; returns the prefix, which the kernels only read
static long long* bnd_classify_layout(Arena& A, long long n_in, BndClassify& a) {
    const size_t T = (size_t)bnd_tiles(n_in);
    a.mask = A.take<unsigned long long>(T * (ADFP_BND_TILE / 64));
    a.tile_counts = A.take<unsigned>(T);
    long long* tile_offsets = A.take<long long>(T);
    a.tile_offsets = tile_offsets;
    return tile_offsets;
}
size_t adfp_bound_classify_workspace_bytes(long long n_in) {
    BndClassify a;
    return n_in <= 0 || n_in > BND_MAX_IDS ? 0 : layout_bytes(bnd_classify_layout, n_in, a);
}

int adfp_bound_classify(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                        const long long* ids_in, long long n_in, const double* planes, int F, double eps, void* workspace,
                        size_t workspace_bytes, long long* ids_out, long long ids_cap, long long* count, long long* far_id, double* far_dist,
                        void* stream) {
    BndClassify a;
    const int rc = bnd_scene(depth, poses, K, H, W, fx, fy, cx, cy, a.s);
    if (rc) return rc;
    if (n_in < 0 || ids_cap < 0 || F < 1 || !planes || !count || !far_id || !far_dist || !(eps >= 0.0) || !bnd_finite_host(eps)) return ADFP_E_ARG;
    if (!ids_in && n_in != a.s.n_ids) return ADFP_E_ARG;                // NULL: all ids of the scene
    if (n_in > BND_MAX_IDS) return ADFP_E_UNSUPPORTED;
    if (n_in > 0 && (!workspace || (ids_cap > 0 && !ids_out))) return ADFP_E_ARG;
    if (n_in > 0 && workspace_bytes < adfp_bound_classify_workspace_bytes(n_in)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(far_id, 0xff, (size_t)F * 8, st);     // -1: no point
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(far_dist, 0, (size_t)F * 8, st);
    if (e != hipSuccess) return (int)e;
    if (n_in == 0) { e = hipMemsetAsync(count, 0, sizeof(long long), st); return e == hipSuccess ? 0 : (int)e; }
    const long long T = bnd_tiles(n_in);
    Arena A(workspace);
    long long* tile_offsets = bnd_classify_layout(A, n_in, a);
    a.ids_in = ids_in; a.n_in = n_in; a.planes = planes; a.F = F; a.eps = eps;
    a.ids_out = ids_out; a.ids_cap = ids_cap; a.count = count;
    a.far_bits = (unsigned long long*)far_dist; a.far_id = (unsigned long long*)far_id;
    hipLaunchKernelGGL(k_bnd_flag, dim3((unsigned)T), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_tile_scan<ADFP_BND_THREADS, ADFP_BND_SCAN_PER>), dim3(1), dim3(ADFP_BND_THREADS), 0, st, a.tile_counts, T, tile_offsets, count);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bnd_emit, dim3((unsigned)T), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    if (ids_cap == 0) return 0;
    const long long cap_tiles = bnd_tiles(n_in < ids_cap ? n_in : ids_cap);
    const unsigned fb = (unsigned)(cap_tiles < ADFP_BND_FAR_BLOCKS ? cap_tiles : ADFP_BND_FAR_BLOCKS);
    a.ids_in = nullptr;                                                  // the farthest passes read ids_out
    hipLaunchKernelGGL(k_bnd_far<0>, dim3(fb), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_bnd_far<1>, dim3(fb), dim3(ADFP_BND_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_bound_points(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                      const long long* ids, long long n, double* out, void* stream) {
    BndScene s;
    const int rc = bnd_scene(depth, poses, K, H, W, fx, fy, cx, cy, s);
    if (rc) return rc;
    if (n < 0) return ADFP_E_ARG;
    if (n == 0) return 0;
    if (!ids || !out) return ADFP_E_ARG;
    if (n > BND_MAX_IDS) return ADFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_bnd_points, dim3((unsigned)ceil_div(n, ADFP_BND_THREADS)), dim3(ADFP_BND_THREADS), 0, (hipStream_t)stream,
                       s, ids, n, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}

}   // extern "C"
