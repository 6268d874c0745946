// adfp_recon.h -- reconstruction evaluation on the device (src/tools/eval_recon.py and src/tools/cull_mesh.py of the reference):
//
//   exact nearest neighbour (f64)   a Morton-ordered leaf sequence of ADFP_NN_LEAF points, an implicit complete binary tree of
//                                   leaf boxes over it (node k has children 2k, 2k+1; padding leaves carry inverted boxes), and a
//                                   stackless query: one lane per query point, a 32-bit trail of "sibling done" bits
//   deterministic reductions (f64)  per-workgroup partials over a grid that depends on n only, then one fixed-order pass: the
//                                   metric sums and the 17 ICP moments; no float atomics
//   surface sampling (f64)          trimesh.sample.sample_surface on caller-drawn uniforms: areas, a fixed-order inclusive scan,
//                                   searchsorted(side='left'), the folded barycentric pair
//   frustum culling (f32)           cull_mesh.py:49-75 over every pose in one launch, the poses staged through LDS in chunks
//
// The library is built -ffp-contract=off: every squared distance is ((dx*dx + dy*dy) + dz*dz) with separate roundings, the
// arithmetic of scipy's cKDTree (sqeuclidean_distance_double for m = 3).
#pragma once
#include "adfp_device.h"

#ifndef ADFP_NN_LEAF
#define ADFP_NN_LEAF 16            // points per leaf: 200 k x 200 k query 2.9 ms, against 4.0 ms with 32 (tools/recon_bench.py)
#endif
#define ADFP_NN_THREADS 256
#define ADFP_NN_BB_BLOCKS 256      // workgroups of the bounding-box pass (fixed: the partials are reduced by every Morton workgroup)
#define ADFP_RED_THREADS 256
#define ADFP_RED_MAX_BLOCKS 1024   // partials of a reduction: min(ceil(n / 256), 1024) workgroups, a function of n alone
#define ADFP_SCAN_TILE 2048        // elements per workgroup of the area scan (256 threads x 8)
#define ADFP_CULL_CHUNK 256        // poses per LDS stage of the cull

// squared distance of (x, y, z) to an axis-aligned box [lo, hi]; +inf for an inverted (empty) box.  Never above the squared
// distance, computed the same way, to any point inside the box: rounding is monotone.
ADFP_DEV double nn_box_d2(const double* b, double x, double y, double z) {
    const double dx = fmax(fmax(b[0] - x, x - b[3]), 0.0);
    const double dy = fmax(fmax(b[1] - y, y - b[4]), 0.0);
    const double dz = fmax(fmax(b[2] - z, z - b[5]), 0.0);
    return (dx * dx + dy * dy) + dz * dz;
}

ADFP_DEV unsigned nn_spread10(unsigned v) {       // 10 bits -> every third bit
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// per-workgroup bounding boxes: part[6 * b + (0..5)] = (lo xyz, hi xyz) of the points b, b + NB, ... (grid-stride)
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_bbox_partial(const double* __restrict__ p, int n, double* __restrict__ part) {
    __shared__ double s[6][ADFP_NN_THREADS];
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x; i < n; i += ADFP_NN_BB_BLOCKS * ADFP_NN_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = p[3 * (long long)i + c];
            m[c] = fmin(m[c], v);
            m[3 + c] = fmax(m[3 + c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c][threadIdx.x] = m[c];
    __syncthreads();
    for (int h = ADFP_NN_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s[c][threadIdx.x] = fmin(s[c][threadIdx.x], s[c][threadIdx.x + h]);
                s[3 + c][threadIdx.x] = fmax(s[3 + c][threadIdx.x], s[3 + c][threadIdx.x + h]);
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[6 * blockIdx.x + threadIdx.x] = s[threadIdx.x][0];
}

// every workgroup folds the ADFP_NN_BB_BLOCKS partial boxes itself (no host round trip, no extra launch), then writes the 30-bit
// Morton code of its points on a 1024^3 lattice over the box, and the identity permutation for the sort
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_morton(const double* __restrict__ p, int n, const double* __restrict__ part,
                                                                int* __restrict__ key, int* __restrict__ val) {
    static_assert(ADFP_NN_BB_BLOCKS == ADFP_NN_THREADS, "one partial box per thread");
    __shared__ double s[6][ADFP_NN_THREADS];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c][threadIdx.x] = part[6 * threadIdx.x + c];
    __syncthreads();
    for (int h = ADFP_NN_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                s[c][threadIdx.x] = fmin(s[c][threadIdx.x], s[c][threadIdx.x + h]);
                s[3 + c][threadIdx.x] = fmax(s[3 + c][threadIdx.x], s[3 + c][threadIdx.x + h]);
            }
        }
        __syncthreads();
    }
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned code = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lo = s[c][0], ext = s[3 + c][0] - lo;
        double t = ext > 0.0 ? (p[3 * (long long)i + c] - lo) * (1024.0 / ext) : 0.0;
        t = fmin(fmax(t, 0.0), 1023.0);                    // NaN -> 0 (fmax), the top edge -> the last cell
        code |= nn_spread10((unsigned)t) << c;
    }
    key[i] = (int)code;
    val[i] = i;
}

// the sorted points (AoS f64) and their original indices
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_gather(const double* __restrict__ p, int n, const int* __restrict__ perm,
                                                                double* __restrict__ sp, int* __restrict__ orig) {
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int j = perm[i];
    sp[3 * (long long)i] = p[3 * (long long)j];
    sp[3 * (long long)i + 1] = p[3 * (long long)j + 1];
    sp[3 * (long long)i + 2] = p[3 * (long long)j + 2];
    orig[i] = j;
}

// leaf j of [0, P): the box of sorted points [j B, min(j B + B, n)), inverted when empty; written at node P + j.  fmin / fmax drop a
// NaN coordinate.  A triangle index calls it on its 3 nf vertices with B = 3 leaf.
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_leaves(const double* __restrict__ sp, long long n, int B, long long P,
                                                                double* __restrict__ box) {
    const long long j = (long long)blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (j >= P) return;
    double m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const long long a = j * B, e = a + B < n ? a + B : n;
    for (long long s = a; s < e; ++s) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = sp[3 * s + c];
            m[c] = fmin(m[c], v);
            m[3 + c] = fmax(m[3 + c], v);
        }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) box[6 * (P + j) + c] = m[c];
}

// one level of the tree: nodes [first, 2 first) = the union of their two children
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_level(long long first, double* __restrict__ box) {
    const long long k = first + (long long)blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (k >= 2 * first) return;
    const double* a = box + 12 * k;                       // children 2k and 2k + 1 are adjacent
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        box[6 * k + c] = fmin(a[c], a[6 + c]);
        box[6 * k + 3 + c] = fmax(a[3 + c], a[9 + c]);
    }
}

// The stackless walk of an implicit tree of boxes (the root is node 1, the leaves are the nodes [P, 2 P) at depth D), shared by
// the NN query and the two ray walks of adfp_raycast.h.  The visitor says what a box and a leaf mean:
//   v.enter(box6, &key) -> bool   may the walk enter this box, by the visitor's bound as it stands now; key orders two children
//   v.leaf(j) -> bool             visit leaf j of [0, P); true ends the walk (any-hit), and bvh_walk returns true
// `trail` bit d = the sibling of the current node at depth d is done (visited or pruned).  Descend into an enterable child, of two
// the one with the smaller key when ORDERED (the left one on a tie, and always when not); on the way up, climb past every level
// whose bit is set, then step to the sibling and test its box again, against the bound the visitor has reached by then.
template <bool ORDERED, class V>
ADFP_DEV bool bvh_walk(const double* box, long long P, int D, V& v) {
    unsigned long long k = 1;
    int depth = 0;
    unsigned trail = 0;
    double key0, key1;
    bool alive = v.enter(box + 6, &key0);
    while (alive) {
        bool up = true;
        if (depth == D) {
            if (v.leaf((long long)(k - (unsigned long long)P))) return true;
        } else {
            const bool h0 = v.enter(box + 12 * k, &key0);          // children 2k and 2k + 1 are adjacent
            const bool h1 = v.enter(box + 12 * k + 6, &key1);
            if (h0 || h1) {
                const bool first = h0 && (!ORDERED || !h1 || key0 <= key1);
                k = 2 * k + (first ? 0 : 1);
                ++depth;
                trail = h0 && h1 ? (trail & ~(1u << depth)) : (trail | (1u << depth));
                up = false;
            }
        }
        if (up) {
            for (;;) {
                while (depth > 0 && ((trail >> depth) & 1u)) { k >>= 1; --depth; }
                if (depth == 0) { alive = false; break; }
                k ^= 1ull;
                trail |= 1u << depth;
                if (v.enter(box + 6 * k, &key0)) break;
            }
        }
    }
    return false;
}

struct NnQueryArgs {
    const double* sp; const int* orig; const double* box; int n_ref; long long P; int D;
    const double* q; int nq; const int* order;            // order: lane i takes query order[i] (Morton order), or NULL
    int has_t; double t[12];                               // optional 3x4 row-major transform of the queries
    double best0;                                          // r^2 (radius) or +inf
    double* dist; int* idx;
};

// the nearest point so far: a box is entered while its squared distance is below `best`, the nearer child first
struct NnNearest {
    const double* sp; int n_ref; double x, y, z, best; long long bi;
    ADFP_DEV bool enter(const double* b, double* d2) { *d2 = nn_box_d2(b, x, y, z); return *d2 < best; }
    ADFP_DEV bool leaf(long long j) {
        const long long s0 = j * ADFP_NN_LEAF, s1 = s0 + ADFP_NN_LEAF < n_ref ? s0 + ADFP_NN_LEAF : n_ref;
        for (long long s = s0; s < s1; ++s) {
            const double dx = sp[3 * s] - x, dy = sp[3 * s + 1] - y, dz = sp[3 * s + 2] - z;
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < best) { best = d; bi = s; }
        }
        return false;
    }
};

// One lane, one query: bvh_walk with the NnNearest visitor
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_nn_query(NnQueryArgs a) {
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (i >= a.nq) return;
    const int qi = a.order ? a.order[i] : i;
    double x = a.q[3 * (long long)qi], y = a.q[3 * (long long)qi + 1], z = a.q[3 * (long long)qi + 2];
    if (a.has_t) {
        const double tx = ((a.t[0] * x + a.t[1] * y) + a.t[2] * z) + a.t[3];
        const double ty = ((a.t[4] * x + a.t[5] * y) + a.t[6] * z) + a.t[7];
        const double tz = ((a.t[8] * x + a.t[9] * y) + a.t[10] * z) + a.t[11];
        x = tx; y = ty; z = tz;
    }
    NnNearest v = {a.sp, a.n_ref, x, y, z, a.best0, -1};
    bvh_walk<true>(a.box, a.P, a.D, v);
    a.dist[qi] = v.bi >= 0 ? sqrt(v.best) : INFINITY;
    a.idx[qi] = v.bi >= 0 ? a.orig[v.bi] : -1;
}

// ---- deterministic f64 reductions ----
// a fixed-shape sum over the workgroup: wave shuffles in a fixed pattern, then the four wave sums in order
ADFP_DEV double red_block_sum(double v, double* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                       // s_wave may still be read from the previous call
    if (lane == 0) s_wave[w] = v;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

struct MetricArgs { const double* d; int n; double th; int nblk; double* part; double* out; };

// partial b: sum of d and count of d < th over elements b * 256 + t + k * (nblk * 256)
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_metric_partial(MetricArgs a) {
    __shared__ double s_wave[ADFP_RED_THREADS / 64];
    double sum = 0.0, cnt = 0.0;
    for (int i = blockIdx.x * ADFP_RED_THREADS + threadIdx.x; i < a.n; i += a.nblk * ADFP_RED_THREADS) {
        const double d = a.d[i];
        sum += d;
        cnt += d < a.th ? 1.0 : 0.0;                       // exact: whole numbers far below 2^53
    }
    sum = red_block_sum(sum, s_wave);
    cnt = red_block_sum(cnt, s_wave);
    if (threadIdx.x == 0) { a.part[2 * blockIdx.x] = sum; a.part[2 * blockIdx.x + 1] = cnt; }
}

// the fixed-order pass over the partials of a reduction of `width` doubles each: out[c] = sum_b part[width b + c].  Workgroup g
// (grid x) reduces batch g: nblk partials from part + g * WIDTH * nblk into out + g * WIDTH.
template <int WIDTH>
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_red_final(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    __shared__ double s_wave[ADFP_RED_THREADS / 64];
    part += (long long)blockIdx.x * WIDTH * nblk;
    out += (long long)blockIdx.x * WIDTH;
    for (int c = 0; c < WIDTH; ++c) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblk; b += ADFP_RED_THREADS) v += part[WIDTH * b + c];
        v = red_block_sum(v, s_wave);
        if (threadIdx.x == 0) out[c] = v;
    }
}

#define ADFP_ICP_MOMENTS 17
struct IcpArgs {
    const double* src; int n_src; double t[12]; double org[3];
    const double* tgt; int n_tgt; const int* idx;
    int nblk; double* part;
};

// the ICP moments over correspondences i (idx[i] in [0, n_tgt)): count, sum d^2, sum p, sum q, sum p q^T (row-major), where
// p = T src_i - org, q = tgt_idx[i] - org and d^2 is the query's squared distance of T src_i to tgt_idx[i]
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_icp_partial(IcpArgs a) {
    __shared__ double s_wave[ADFP_RED_THREADS / 64];
    double m[ADFP_ICP_MOMENTS];
#pragma unroll
    for (int c = 0; c < ADFP_ICP_MOMENTS; ++c) m[c] = 0.0;
    for (int i = blockIdx.x * ADFP_RED_THREADS + threadIdx.x; i < a.n_src; i += a.nblk * ADFP_RED_THREADS) {
        const int j = a.idx[i];
        if (j < 0 || j >= a.n_tgt) continue;
        const double x = a.src[3 * (long long)i], y = a.src[3 * (long long)i + 1], z = a.src[3 * (long long)i + 2];
        const double px = ((a.t[0] * x + a.t[1] * y) + a.t[2] * z) + a.t[3];
        const double py = ((a.t[4] * x + a.t[5] * y) + a.t[6] * z) + a.t[7];
        const double pz = ((a.t[8] * x + a.t[9] * y) + a.t[10] * z) + a.t[11];
        const double qx = a.tgt[3 * (long long)j], qy = a.tgt[3 * (long long)j + 1], qz = a.tgt[3 * (long long)j + 2];
        const double dx = qx - px, dy = qy - py, dz = qz - pz;
        const double p[3] = {px - a.org[0], py - a.org[1], pz - a.org[2]};
        const double q[3] = {qx - a.org[0], qy - a.org[1], qz - a.org[2]};
        m[0] += 1.0;
        m[1] += (dx * dx + dy * dy) + dz * dz;
#pragma unroll
        for (int c = 0; c < 3; ++c) { m[2 + c] += p[c]; m[5 + c] += q[c]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) m[8 + 3 * r + c] += p[r] * q[c];
    }
#pragma unroll
    for (int c = 0; c < ADFP_ICP_MOMENTS; ++c) {
        const double v = red_block_sum(m[c], s_wave);
        if (threadIdx.x == 0) a.part[ADFP_ICP_MOMENTS * blockIdx.x + c] = v;
    }
}

// ---- area-weighted surface sampling ----
struct SurfSampleArgs {
    const double* v; int nv; const int* f; int nf;
    const double* u_face; const double* u_bary; int count;
    double* cum; double* tile_sum; double* tile_max; int ntiles;
    double* pts; int* face_index;
};

// area of face i: |cross(v1 - v0, v2 - v0)| / 2 (trimesh.triangles.area); a face with an index out of range has area 0
ADFP_DEV double tri_area(const SurfSampleArgs& a, int i) {
    const int i0 = a.f[3 * (long long)i], i1 = a.f[3 * (long long)i + 1], i2 = a.f[3 * (long long)i + 2];
    if ((unsigned)i0 >= (unsigned)a.nv || (unsigned)i1 >= (unsigned)a.nv || (unsigned)i2 >= (unsigned)a.nv) return 0.0;
    const double* v0 = a.v + 3 * (long long)i0; const double* v1 = a.v + 3 * (long long)i1; const double* v2 = a.v + 3 * (long long)i2;
    const double ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
    const double bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return sqrt((cx * cx + cy * cy) + cz * cz) * 0.5;
}

// tile t: the sum of its ADFP_SCAN_TILE areas, thread r summing its 8 consecutive ones, then the workgroup in a fixed tree
ADFP_DEV double scan_block_inclusive(double v, double* s) {      // Hillis-Steele over the 256 thread values, fixed order
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < ADFP_RED_THREADS; o <<= 1) {
        const double add = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0.0;
        __syncthreads();
        v += add;
        s[threadIdx.x] = v;
        __syncthreads();
    }
    return v;
}

#define ADFP_SCAN_PER_THREAD (ADFP_SCAN_TILE / ADFP_RED_THREADS)
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_area_tiles(SurfSampleArgs a) {
    __shared__ double s[ADFP_RED_THREADS];
    const long long base = (long long)blockIdx.x * ADFP_SCAN_TILE + (long long)threadIdx.x * ADFP_SCAN_PER_THREAD;
    double v = 0.0;
    for (int k = 0; k < ADFP_SCAN_PER_THREAD; ++k) {
        const long long i = base + k;
        if (i < a.nf) {
            const double ar = tri_area(a, (int)i);
            a.cum[i] = ar;
            v += ar;
        }
    }
    v = scan_block_inclusive(v, s);
    if (threadIdx.x == ADFP_RED_THREADS - 1) a.tile_sum[blockIdx.x] = v;
}

// one workgroup: exclusive prefix of the tile sums, in chunks of 256 with a carried total; tile_sum[ntiles] = the total area
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_area_tile_scan(SurfSampleArgs a) {
    __shared__ double s[ADFP_RED_THREADS];
    double carry = 0.0;
    for (int c0 = 0; c0 < a.ntiles; c0 += ADFP_RED_THREADS) {
        const int t = c0 + threadIdx.x;
        const double v = t < a.ntiles ? a.tile_sum[t] : 0.0;
        const double inc = scan_block_inclusive(v, s);
        if (t < a.ntiles) a.tile_sum[t] = carry + (inc - v);      // exclusive
        const double last = s[ADFP_RED_THREADS - 1];
        __syncthreads();
        carry += last;
    }
    if (threadIdx.x == 0) a.tile_sum[a.ntiles] = carry;
}

// within each tile: cum[i] = tile prefix + thread prefix + the running sum of the thread's own areas
ADFP_DEV double scan_block_max_inclusive(double v, double* s) {  // the same walk with fmax: exact, so order does not matter
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < ADFP_RED_THREADS; o <<= 1) {
        const double other = (int)threadIdx.x >= o ? s[threadIdx.x - o] : -INFINITY;
        __syncthreads();
        v = fmax(v, other);
        s[threadIdx.x] = v;
        __syncthreads();
    }
    return v;
}

// within each tile: cum[i] = tile prefix + thread prefix + the running sum of the thread's own areas.  A thread's running sum never
// decreases (areas are >= 0), but its starting prefix comes from a differently rounded scan and can lie an ulp or so below where
// the previous thread ended.  So every value is raised to the largest value before it in the tile (a max-scan, exact), and the
// tile's last value goes to tile_max for the same fix across tiles (k_area_tile_max, applied on read by k_sample): the cumulative
// sums the search sees never decrease, and searchsorted(side='left') keeps its meaning at every boundary.
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_area_apply(SurfSampleArgs a) {
    __shared__ double s[ADFP_RED_THREADS];
    const long long base = (long long)blockIdx.x * ADFP_SCAN_TILE + (long long)threadIdx.x * ADFP_SCAN_PER_THREAD;
    double v = 0.0;
    for (int k = 0; k < ADFP_SCAN_PER_THREAD; ++k) {
        const long long i = base + k;
        if (i < a.nf) v += a.cum[i];
    }
    const double inc = scan_block_inclusive(v, s);
    double run = a.tile_sum[blockIdx.x] + (inc - v);
    for (int k = 0; k < ADFP_SCAN_PER_THREAD; ++k) {
        const long long i = base + k;
        if (i < a.nf) { run += a.cum[i]; a.cum[i] = run; }
    }
    __syncthreads();                                       // s is reused by the max-scan
    const double incmax = scan_block_max_inclusive(run, s);
    const double before = threadIdx.x > 0 ? s[threadIdx.x - 1] : -INFINITY;
    for (int k = 0; k < ADFP_SCAN_PER_THREAD; ++k) {
        const long long i = base + k;
        if (i < a.nf) a.cum[i] = fmax(a.cum[i], before);
    }
    if (threadIdx.x == ADFP_RED_THREADS - 1) a.tile_max[blockIdx.x] = incmax;
}

// one workgroup: tile_max[t] <- the largest cumulative value of the tiles before t (-inf for the first), in chunks of 256 with a
// carried maximum
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_area_tile_max(SurfSampleArgs a) {
    __shared__ double s[ADFP_RED_THREADS];
    double carry = -INFINITY;
    for (int c0 = 0; c0 < a.ntiles; c0 += ADFP_RED_THREADS) {
        const int t = c0 + threadIdx.x;
        const double v = t < a.ntiles ? a.tile_max[t] : -INFINITY;
        scan_block_max_inclusive(v, s);
        const double before = fmax(carry, threadIdx.x > 0 ? s[threadIdx.x - 1] : -INFINITY);
        const double last = s[ADFP_RED_THREADS - 1];
        __syncthreads();
        if (t < a.ntiles) a.tile_max[t] = before;
        carry = fmax(carry, last);
    }
}

// the non-decreasing cumulative sum the search reads
ADFP_DEV double cum_at(const SurfSampleArgs& a, int i) { return fmax(a.cum[i], a.tile_max[i / ADFP_SCAN_TILE]); }

// draw i: face = first f with cum[f] >= u_face[i] * total (searchsorted side='left'); (a, b) = u_bary[i]; if a + b > 1 both
// minus 1, then absolute values; point = (a (v1 - v0) + b (v2 - v0)) + v0 (trimesh's order of operations)
__global__ __launch_bounds__(ADFP_RED_THREADS) void k_sample(SurfSampleArgs a) {
    const int i = blockIdx.x * ADFP_RED_THREADS + threadIdx.x;
    if (i >= a.count) return;
    const double u = a.u_face[i] * cum_at(a, a.nf - 1);      // weight_cum[-1], as trimesh scales the draw
    int lo = 0, hi = a.nf;                                 // first index in [lo, hi) with cum >= u; nf when none
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cum_at(a, mid) < u) lo = mid + 1; else hi = mid;
    }
    const int fi = lo < a.nf ? lo : a.nf - 1;
    double ra = a.u_bary[2 * (long long)i], rb = a.u_bary[2 * (long long)i + 1];
    if (ra + rb > 1.0) { ra -= 1.0; rb -= 1.0; }
    ra = fabs(ra); rb = fabs(rb);
    const int i0 = a.f[3 * (long long)fi], i1 = a.f[3 * (long long)fi + 1], i2 = a.f[3 * (long long)fi + 2];
    double* o = a.pts + 3 * (long long)i;
    if ((unsigned)i0 >= (unsigned)a.nv || (unsigned)i1 >= (unsigned)a.nv || (unsigned)i2 >= (unsigned)a.nv) {
        o[0] = o[1] = o[2] = NAN;                          // only reachable when every face is degenerate or out of range
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v0 = a.v[3 * (long long)i0 + c];
            o[c] = (ra * (a.v[3 * (long long)i1 + c] - v0) + rb * (a.v[3 * (long long)i2 + c] - v0)) + v0;
        }
    }
    a.face_index[i] = fi;
}

// ---- frustum culling ----
// Which test k_cull_seen restates: cull_mesh.py's over f64 vertices, or one of the three branches of the Mesher's point_masks
// (src/utils/Mesher.py:58-217, the *seen* mask only) over f32 vertices.  The values 0..2 are ADFP_SEEN_* of include/adfp.h.
#define ADFP_CULL_RULE_CULL_MESH (-1)
#define ADFP_CULL_RULE_FRUSTUM   0      // get_mask_use_all_frames: the frustum only
#define ADFP_CULL_RULE_MAX_DEPTH 1      // depth_test = False: and -cam.z < dmax[k] (the caller's 1.1 max(depth_k))
#define ADFP_CULL_RULE_DEPTH_TEST 2     // depth_test = True: and |(-cam.z) - depth_k(uv)| < 2.4 (bilinear sample)
struct CullArgs {
    const double* v; int nv; const float* w2c; int np;     // w2c: [np][12], the top three rows of inv(c2w) (f32)
    float fx, fy, cx, cy, W, H;
    unsigned char* seen;
    // the Mesher's rules only
    const float* vf;                                       // [nv][3] f32 vertices
    const float* depth; const float* dmax;                 // [np][Hi][Wi] depth images / [np] depth bounds
    int Wi, Hi; float rW, rH;                              // rW = 1 / (W - 1), rH = 1 / (H - 1), rounded to f32 on the host
};

// pose w (12 f32: the top three rows of inv(c2w)) applied to (x, y, z): cam = w [p, 1], cam.x *= -1, uv = K cam, zz = uv.z + eps,
// uv /= zz, all in f32.  Returns the frustum test.  MESHER = false: cull_mesh.py:49-71 (eps 1e-5, 0 <= -zz); true: Mesher._project
// (eps 1e-8, zz < 0).  Z = cam.z, before eps.
template <bool MESHER>
ADFP_DEV bool cull_project(const float* w, float x, float y, float z, float fx, float fy, float cx, float cy, float W, float H,
                           float& u, float& v, float& Z) {
    const float X = -(((w[0] * x + w[1] * y) + w[2] * z) + w[3]);
    const float Y = ((w[4] * x + w[5] * y) + w[6] * z) + w[7];
    Z = ((w[8] * x + w[9] * y) + w[10] * z) + w[11];
    const float zz = Z + (MESHER ? 1e-8f : 1e-5f);
    u = (fx * X + cx * Z) / zz;
    v = (fy * Y + cy * Z) / zz;
    const bool front = MESHER ? zz < 0.f : 0.f <= -zz;
    return front && u < W && u > 0.f && v < H && v > 0.f;
}
// does pose w project (x, y, z) into the image, by cull_mesh.py's rule
ADFP_DEV bool cull_sees(const float* w, float x, float y, float z, float fx, float fy, float cx, float cy, float W, float H) {
    float u, v, Z;
    return cull_project<false>(w, x, y, z, fx, fy, cx, cy, W, H, u, v, Z);
}

// F.grid_sample(depth[1,1,H,W], grid, 'bilinear', padding_mode='zeros', align_corners=True) at pixel (u, v), with the grid the
// Mesher forms (Mesher.py:118-121): g = u * (1 / (W - 1)) * 2 - 1 (torch divides by a host scalar through its reciprocal),
// ix = ((g + 1) / 2) * (W - 1), the four corner weights from the integer corners, corners outside the image contribute nothing,
// summed nw, ne, sw, se.  Called only with 0 < u < W, 0 < v < H, so the integer conversions are in range.
ADFP_DEV float cull_depth_sample(const float* img, float u, float v, int W, int H, float rW, float rH) {
    const float gx = (u * rW) * 2.f - 1.f, gy = (v * rH) * 2.f - 1.f;
    const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1), iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    const int x0 = (int)floorf(ix), y0 = (int)floorf(iy), x1 = x0 + 1, y1 = y0 + 1;
    const float nw = ((float)x1 - ix) * ((float)y1 - iy), ne = (ix - (float)x0) * ((float)y1 - iy);
    const float sw = ((float)x1 - ix) * (iy - (float)y0), se = (ix - (float)x0) * (iy - (float)y0);
    const bool xa = x0 >= 0 && x0 < W, xb = x1 >= 0 && x1 < W, ya = y0 >= 0 && y0 < H, yb = y1 >= 0 && y1 < H;
    float out = 0.f;
    if (xa && ya) out += img[(long long)y0 * W + x0] * nw;
    if (xb && ya) out += img[(long long)y0 * W + x1] * ne;
    if (xa && yb) out += img[(long long)y1 * W + x0] * sw;
    if (xb && yb) out += img[(long long)y1 * W + x1] * se;
    return out;
}

// seen[i] = 1 iff some pose sees vertex i by RULE: one lane per vertex, the poses staged through LDS ADFP_CULL_CHUNK at a time
template <int RULE>
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_cull_seen(CullArgs a) {
    constexpr bool MESHER = RULE != ADFP_CULL_RULE_CULL_MESH;
    __shared__ float s_pose[ADFP_CULL_CHUNK * 12];
    __shared__ float s_far[RULE == ADFP_CULL_RULE_MAX_DEPTH ? ADFP_CULL_CHUNK : 1];
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    const bool on = i < a.nv;
    float x = 0.f, y = 0.f, z = 0.f;
    if (on) {
        if (MESHER) { x = a.vf[3 * (long long)i]; y = a.vf[3 * (long long)i + 1]; z = a.vf[3 * (long long)i + 2]; }
        else { x = (float)a.v[3 * (long long)i]; y = (float)a.v[3 * (long long)i + 1]; z = (float)a.v[3 * (long long)i + 2]; }
    }
    bool seen = false;
    for (int p0 = 0; p0 < a.np; p0 += ADFP_CULL_CHUNK) {
        const int m = a.np - p0 < ADFP_CULL_CHUNK ? a.np - p0 : ADFP_CULL_CHUNK;
        __syncthreads();
        for (int e = threadIdx.x; e < 12 * m; e += ADFP_NN_THREADS) s_pose[e] = a.w2c[12 * (long long)p0 + e];
        if (RULE == ADFP_CULL_RULE_MAX_DEPTH)
            for (int e = threadIdx.x; e < m; e += ADFP_NN_THREADS) s_far[e] = a.dmax[p0 + e];
        __syncthreads();
        if (!on || seen) continue;
        for (int k = 0; k < m; ++k) {
            float u, v, Z;
            bool s = cull_project<MESHER>(s_pose + 12 * k, x, y, z, a.fx, a.fy, a.cx, a.cy, a.W, a.H, u, v, Z);
            if (RULE == ADFP_CULL_RULE_MAX_DEPTH) s = s && -Z < s_far[k];
            if (RULE == ADFP_CULL_RULE_DEPTH_TEST) {
                if (s) {
                    const float d = cull_depth_sample(a.depth + (long long)(p0 + k) * a.Hi * a.Wi, u, v, a.Wi, a.Hi, a.rW, a.rH);
                    s = -Z < d + 2.4f && d - 2.4f < -Z;
                }
            }
            if (s) { seen = true; break; }
        }
    }
    if (on) a.seen[i] = seen ? 1 : 0;
}

// keep[f] = 1 unless all three vertices of face f are unseen (cull_mesh.py:72-74); an out-of-range index counts as unseen
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_cull_faces(const unsigned char* __restrict__ seen, int nv, const int* __restrict__ f,
                                                                 int nf, unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (i >= nf) return;
    unsigned char k = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int j = f[3 * (long long)i + c];
        k |= ((unsigned)j < (unsigned)nv) ? seen[j] : (unsigned char)0;
    }
    keep[i] = k;
}

// ---- host side: the launchers ----
// An index (the NN index over points, the BVH over triangles in adfp_raycast.h): `items` objects of `width` doubles in Morton order,
// each one's position in the caller's order, and the boxes of a complete binary tree over leaves of `leaf` objects (P leaves, depth D).
struct BvhLayout { long long P; int D; double* sorted; int* orig; double* box; };
static BvhLayout bvh_layout(Arena& A, long long items, int width, int leaf) {
    BvhLayout L;
    L.P = 1; L.D = 0;
    while (L.P < ceil_div(items, leaf)) { L.P <<= 1; ++L.D; }
    L.sorted = A.take<double>((size_t)items * width);
    L.orig = A.take<int>((size_t)items);
    L.box = A.take_tail<double>((size_t)(2 * L.P) * 6);
    return L;
}
static unsigned nn_blocks(long long n) { return (unsigned)ceil_div(n, ADFP_NN_THREADS); }

// the Morton ordering of a cloud: bounding-box partials, codes, the stable radix sort; perm <- the sorted order
struct MortonWork { double* part; int* key; int* val; int* key2; int* val2; int* table; };
static MortonWork morton_layout(Arena& A, long long n) {
    MortonWork m;
    m.part = A.take<double>(ADFP_NN_BB_BLOCKS * 6);
    m.key = A.take<int>((size_t)n); m.val = A.take<int>((size_t)n); m.key2 = A.take<int>((size_t)n); m.val2 = A.take<int>((size_t)n);
    m.table = (int*)A.take<char>(adfp_sort_workspace_bytes(n));
    return m;
}
static int morton_order(const double* p, int n, Arena& A, const int** perm, hipStream_t st) {
    const MortonWork m = morton_layout(A, n);
    hipLaunchKernelGGL(k_nn_bbox_partial, dim3(ADFP_NN_BB_BLOCKS), dim3(ADFP_NN_THREADS), 0, st, p, n, m.part);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_nn_morton, dim3(nn_blocks(n)), dim3(ADFP_NN_THREADS), 0, st, p, n, m.part, m.key, m.val);
    ADFP_CHECK_LAUNCH();
    const int* kf;
    return radix_sort_pairs(m.key, m.val, m.key2, m.val2, n, 30, m.table, &kf, perm, st);
}
static size_t morton_ws_bytes(long long n) { return layout_bytes(morton_layout, n); }

// the boxes of an index over the sorted points sp[0, n): leaves of B points each at the nodes [P, 2 P), then every level above
static int nn_boxes(const double* sp, long long n, int B, long long P, double* box, hipStream_t st) {
    hipLaunchKernelGGL(k_nn_leaves, dim3(nn_blocks(P)), dim3(ADFP_NN_THREADS), 0, st, sp, n, B, P, box);
    ADFP_CHECK_LAUNCH();
    for (long long first = P >> 1; first >= 1; first >>= 1) {
        hipLaunchKernelGGL(k_nn_level, dim3(nn_blocks(first)), dim3(ADFP_NN_THREADS), 0, st, first, box);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

size_t adfp_nn_index_bytes(long long n_ref) { return n_ref <= 0 || n_ref > RECON_MAX_N ? 0 : layout_bytes(bvh_layout, n_ref, 3, ADFP_NN_LEAF); }
size_t adfp_nn_build_workspace_bytes(long long n_ref) { return n_ref <= 0 || n_ref > RECON_MAX_N ? 0 : morton_ws_bytes(n_ref); }

int adfp_nn_build(const double* ref, long long n_ref, void* index, size_t index_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_ref < 0) return ADFP_E_ARG;
    if (n_ref == 0) return 0;
    if (!ref || !index || !workspace) return ADFP_E_ARG;
    if (n_ref > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (index_bytes < adfp_nn_index_bytes(n_ref) || workspace_bytes < adfp_nn_build_workspace_bytes(n_ref)) return ADFP_E_WORKSPACE;
    Arena I(index), A(workspace);
    const BvhLayout L = bvh_layout(I, n_ref, 3, ADFP_NN_LEAF);
    const int n = (int)n_ref;
    hipStream_t st = (hipStream_t)stream;
    const int* perm;
    int rc = morton_order(ref, n, A, &perm, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_nn_gather, dim3(nn_blocks(n)), dim3(ADFP_NN_THREADS), 0, st, ref, n, perm, L.sorted, L.orig);
    ADFP_CHECK_LAUNCH();
    return nn_boxes(L.sorted, n, ADFP_NN_LEAF, L.P, L.box, st);
}

size_t adfp_nn_query_workspace_bytes(long long n_query, int flags) {
    if (n_query <= 0 || n_query > RECON_MAX_N || !(flags & ADFP_NN_SORT_QUERIES)) return 0;
    return morton_ws_bytes(n_query);
}

int adfp_nn_query(const void* index, size_t index_bytes, long long n_ref, const double* query, long long n_query, const double* transform,
                  double radius, int flags, void* workspace, size_t workspace_bytes, double* dist, int* idx, void* stream) {
    if (n_ref < 0 || n_query < 0 || (flags & ~ADFP_NN_SORT_QUERIES)) return ADFP_E_ARG;
    if (!(radius > 0.0)) return ADFP_E_ARG;                                // NaN, zero or negative
    if (n_query == 0) return 0;
    if (n_ref == 0 || !index || !query || !dist || !idx) return ADFP_E_ARG;
    if ((flags & ADFP_NN_SORT_QUERIES) && !workspace) return ADFP_E_ARG;
    if (n_ref > RECON_MAX_N || n_query > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (index_bytes < adfp_nn_index_bytes(n_ref) || workspace_bytes < adfp_nn_query_workspace_bytes(n_query, flags)) return ADFP_E_WORKSPACE;
    Arena I(index), A(workspace);
    const BvhLayout L = bvh_layout(I, n_ref, 3, ADFP_NN_LEAF);
    hipStream_t st = (hipStream_t)stream;
    NnQueryArgs a;
    a.sp = L.sorted; a.orig = L.orig; a.box = L.box;
    a.n_ref = (int)n_ref; a.P = L.P; a.D = L.D;
    a.q = query; a.nq = (int)n_query; a.order = nullptr;
    a.has_t = transform != nullptr;
    for (int k = 0; k < 12; ++k) a.t[k] = transform ? transform[k] : 0.0;
    a.best0 = radius * radius;                              // +inf stays +inf
    a.dist = dist; a.idx = idx;
    if (flags & ADFP_NN_SORT_QUERIES) {
        int rc = morton_order(query, (int)n_query, A, &a.order, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_nn_query, dim3(nn_blocks(n_query)), dim3(ADFP_NN_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

static int red_blocks(long long n) {
    const long long b = ceil_div(n, ADFP_RED_THREADS);
    return (int)(b < 1 ? 1 : (b > ADFP_RED_MAX_BLOCKS ? ADFP_RED_MAX_BLOCKS : b));
}
size_t adfp_recon_reduce_workspace_bytes(long long n) {
    if (n < 0 || n > RECON_MAX_N) return 0;
    return (size_t)red_blocks(n) * ADFP_ICP_MOMENTS * 8;
}

int adfp_nn_metric_sums(const double* dist, long long n, double threshold, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (n < 0 || !out || !workspace || (n > 0 && !dist)) return ADFP_E_ARG;
    if (n > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_recon_reduce_workspace_bytes(n)) return ADFP_E_WORKSPACE;
    MetricArgs a;
    a.d = dist; a.n = (int)n; a.th = threshold; a.nblk = red_blocks(n); a.part = (double*)workspace; a.out = out;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_metric_partial, dim3((unsigned)a.nblk), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_red_final<2>, dim3(1), dim3(ADFP_RED_THREADS), 0, st, a.part, a.nblk, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_icp_moments(const double* src, long long n_src, const double* transform, const double* origin, const double* tgt, long long n_tgt,
                     const int* idx, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (n_src < 0 || n_tgt < 0 || !transform || !origin || !out || !workspace) return ADFP_E_ARG;
    if (n_src > 0 && (!src || !idx || (n_tgt > 0 && !tgt))) return ADFP_E_ARG;
    if (n_src > RECON_MAX_N || n_tgt > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_recon_reduce_workspace_bytes(n_src)) return ADFP_E_WORKSPACE;
    IcpArgs a;
    a.src = src; a.n_src = (int)n_src; a.tgt = tgt; a.n_tgt = (int)n_tgt; a.idx = idx;
    for (int k = 0; k < 12; ++k) a.t[k] = transform[k];
    for (int k = 0; k < 3; ++k) a.org[k] = origin[k];
    a.nblk = red_blocks(n_src); a.part = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_icp_partial, dim3((unsigned)a.nblk), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_red_final<ADFP_ICP_MOMENTS>, dim3(1), dim3(ADFP_RED_THREADS), 0, st, a.part, a.nblk, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}

// cum [F]; then tile_sum [tiles + 1] and tile_max [tiles] in one block
static void surf_layout(Arena& A, long long n_faces, SurfSampleArgs& a) {
    a.ntiles = (int)ceil_div(n_faces, ADFP_SCAN_TILE);
    a.cum = A.take<double>((size_t)n_faces);
    a.tile_sum = A.take_tail<double>(2 * (size_t)a.ntiles + 1);
    a.tile_max = a.tile_sum + a.ntiles + 1;
}
size_t adfp_sample_surface_workspace_bytes(long long n_faces) {
    SurfSampleArgs a;
    return n_faces <= 0 || n_faces > RECON_MAX_N ? 0 : layout_bytes(surf_layout, n_faces, a);
}

int adfp_sample_surface(const double* verts, long long n_verts, const int* faces, long long n_faces, const double* u_face, const double* u_bary,
                        long long count, void* workspace, size_t workspace_bytes, double* points, int* face_index, void* stream) {
    if (n_verts < 0 || n_faces < 0 || count < 0) return ADFP_E_ARG;
    if (count == 0) return 0;
    if (n_faces == 0 || n_verts == 0 || !verts || !faces || !u_face || !u_bary || !workspace || !points || !face_index) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_faces > RECON_MAX_N || count > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_sample_surface_workspace_bytes(n_faces)) return ADFP_E_WORKSPACE;
    SurfSampleArgs a;
    a.v = verts; a.nv = (int)n_verts; a.f = faces; a.nf = (int)n_faces;
    a.u_face = u_face; a.u_bary = u_bary; a.count = (int)count;
    Arena A(workspace);
    surf_layout(A, n_faces, a);
    a.pts = points; a.face_index = face_index;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_area_tiles, dim3((unsigned)a.ntiles), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_area_tile_scan, dim3(1), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_area_apply, dim3((unsigned)a.ntiles), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_area_tile_max, dim3(1), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sample, dim3((unsigned)ceil_div(count, ADFP_RED_THREADS)), dim3(ADFP_RED_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_cull_vertices(const double* verts, long long n_verts, const float* w2c, long long n_poses, float fx, float fy, float cx, float cy,
                       int W, int H, unsigned char* seen, void* stream) {
    if (n_verts < 0 || n_poses < 0) return ADFP_E_ARG;
    if (n_verts == 0) return 0;
    if (!verts || !seen || (n_poses > 0 && !w2c)) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_poses > RECON_MAX_N / 12) return ADFP_E_UNSUPPORTED;
    CullArgs a;
    a.v = verts; a.nv = (int)n_verts; a.w2c = w2c; a.np = (int)n_poses;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.W = (float)W; a.H = (float)H; a.seen = seen;
    a.vf = nullptr; a.depth = nullptr; a.dmax = nullptr; a.Wi = W; a.Hi = H; a.rW = 0.f; a.rH = 0.f;
    hipLaunchKernelGGL(k_cull_seen<ADFP_CULL_RULE_CULL_MESH>, dim3(nn_blocks(n_verts)), dim3(ADFP_NN_THREADS), 0,
                       (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_cull_faces(const unsigned char* seen, long long n_verts, const int* faces, long long n_faces, unsigned char* keep, void* stream) {
    if (n_verts < 0 || n_faces < 0) return ADFP_E_ARG;
    if (n_faces == 0) return 0;
    if (!faces || !keep || (n_verts > 0 && !seen)) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_faces > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_cull_faces, dim3(nn_blocks(n_faces)), dim3(ADFP_NN_THREADS), 0,
                       (hipStream_t)stream, seen, (int)n_verts, faces, (int)n_faces, keep);
    ADFP_CHECK_LAUNCH();
    return 0;
}
