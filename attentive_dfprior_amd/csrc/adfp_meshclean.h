// adfp_meshclean.h -- the Mesher's clean-up after marching cubes on the device (src/utils/Mesher.py:492-513 does it with trimesh
// on the host): face components through two-face edges, component areas, the keep rule, compaction, the merge of coincident
// vertices and the colour bytes.  The seen mask is k_cull_seen (adfp_recon.h).  Contracts: include/adfp.h, "mesh clean-up".
//
//   components   3 F half-edges keyed (min vertex, max vertex), ordered by two stable radix sorts (adfp_sort.h); a run of exactly
//                two equal keys makes its two faces mates.  parent[f] starts at f; a round hooks, for every mate pair with
//                different roots, the larger root under the smaller (atomicMin) and then points every face at its root.  parent[x]
//                <= x always, so every walk descends and ends; a round that hooks nothing leaves parent = the smallest face index
//                of each component, whatever order the atomics landed in.  A root that is the larger end of some edge stops
//                being a root in that round, and of the roots that stay (local minima) at most half can stay once more, so
//                2 log2(F) + 2 rounds are the worst case: the host caps at 128.
//   areas        f64 as numpy forms them; faces ordered by label (one more sort), a segmented scan of fixed shape (8 items per
//                lane in order, 256 lanes by doubling steps, the tiles in order) sums each component: no float atomics.
//   compaction   flags -> exclusive scan (tile counts, one workgroup over the tiles, positions) -> gathers.
#pragma once
#include "adfp_device.h"

#define ADFP_MCL_THREADS 256
#define ADFP_MCL_PER 8
#define ADFP_MCL_TILE (ADFP_MCL_THREADS * ADFP_MCL_PER)

// ---- exclusive scan of byte flags: pos[i] = number of set flags before i; total[0] = their number (long long) ----
struct MclScan { const unsigned char* flag; int n; int ntiles; unsigned* tile_counts; long long* tile_offsets; int* pos; long long* total; };

__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_tile_count(MclScan a) {
    __shared__ unsigned lds[ADFP_MCL_THREADS / 64];
    const long long first = (long long)blockIdx.x * ADFP_MCL_TILE + (long long)threadIdx.x * ADFP_MCL_PER;
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) c += (first + q < a.n && a.flag[first + q]) ? 1u : 0u;
    unsigned tot;
    mc_block_scan<unsigned, ADFP_MCL_THREADS>(c, tot, lds);
    if (threadIdx.x == 0) a.tile_counts[blockIdx.x] = tot;
}

// one workgroup: exclusive prefix of the tile counts
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_tile_scan(MclScan a) {
    __shared__ unsigned long long lds[ADFP_MCL_THREADS / 64];
    unsigned long long carry = 0;
    const long long per_round = (long long)ADFP_MCL_THREADS * ADFP_MCL_PER;
    for (long long t0 = 0; t0 < a.ntiles; t0 += per_round) {
        const long long first = t0 + (long long)threadIdx.x * ADFP_MCL_PER;
        unsigned cv[ADFP_MCL_PER];
        unsigned long long s = 0;
#pragma unroll
        for (int q = 0; q < ADFP_MCL_PER; ++q) {
            cv[q] = first + q < a.ntiles ? a.tile_counts[first + q] : 0u;
            s += cv[q];
        }
        unsigned long long tot;
        unsigned long long o = carry + mc_block_scan<unsigned long long, ADFP_MCL_THREADS>(s, tot, lds);
#pragma unroll
        for (int q = 0; q < ADFP_MCL_PER; ++q) {
            if (first + q < a.ntiles) a.tile_offsets[first + q] = (long long)o;
            o += cv[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) a.total[0] = (long long)carry;
}

__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_positions(MclScan a) {
    __shared__ unsigned lds[ADFP_MCL_THREADS / 64];
    const long long first = (long long)blockIdx.x * ADFP_MCL_TILE + (long long)threadIdx.x * ADFP_MCL_PER;
    bool h[ADFP_MCL_PER];
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) {
        h[q] = first + q < a.n && a.flag[first + q];
        c += h[q] ? 1u : 0u;
    }
    unsigned tot;
    long long p = a.tile_offsets[blockIdx.x] + mc_block_scan<unsigned, ADFP_MCL_THREADS>(c, tot, lds);
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) {
        if (first + q < a.n) a.pos[first + q] = (int)p;
        p += h[q] ? 1 : 0;
    }
}

// ---- components ----
ADFP_DEV bool mcl_face_ok(const int* f, int i, int nv, const unsigned char* keep) {
    if (keep && !keep[i]) return false;
    const int a = f[3 * (long long)i], b = f[3 * (long long)i + 1], c = f[3 * (long long)i + 2];
    return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv;
}

// half-edge e = 3 f + c joins vertices f[c], f[(c + 1) % 3]: hi[e] = the larger, lo[e] = the smaller, val[e] = e.  A face that is
// not kept or has an index outside [0, nv) gets lo = hi = nv on all three (sorted last, never mated) and parent -1, else parent f.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_edges(const int* __restrict__ f, int nf, int nv, const unsigned char* __restrict__ keep,
                                                                 int* __restrict__ lo, int* __restrict__ hi, int* __restrict__ val,
                                                                 int* __restrict__ parent) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf) return;
    const bool ok = mcl_face_ok(f, i, nv, keep);
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = f[3 * (long long)i + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int a = v[c], b = v[(c + 1) % 3];
        const long long e = 3 * (long long)i + c;
        lo[e] = ok ? (a < b ? a : b) : nv;
        hi[e] = ok ? (a < b ? b : a) : nv;
        val[e] = (int)e;
    }
    parent[i] = ok ? i : -1;
}

// key[i] = src[perm[i]]: the key of the sort's next pass
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_gather(const int* __restrict__ src, const int* __restrict__ perm, int n,
                                                                  int* __restrict__ key) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) key[i] = src[perm[i]];
}

// perm: the half-edges ordered by (lo, hi).  mate[e] = the face of the other half-edge when e's key occurs exactly twice, else -1.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_mates(const int* __restrict__ lo, const int* __restrict__ hi,
                                                                 const int* __restrict__ perm, int n, int nv, int* __restrict__ mate) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int e = perm[i];
    const int l = lo[e], h = hi[e];
    int m = -1;
    if (l < nv) {
        const int ep = i > 0 ? perm[i - 1] : -1, en = i + 1 < n ? perm[i + 1] : -1;
        const bool same_p = ep >= 0 && lo[ep] == l && hi[ep] == h;
        const bool same_n = en >= 0 && lo[en] == l && hi[en] == h;
        if (same_n && !same_p) {                       // first of a run: of exactly two?
            const int e2 = i + 2 < n ? perm[i + 2] : -1;
            if (!(e2 >= 0 && lo[e2] == l && hi[e2] == h)) m = en / 3;
        } else if (same_p && !same_n) {                // last of a run: of exactly two?
            const int e0 = i > 1 ? perm[i - 2] : -1;
            if (!(e0 >= 0 && lo[e0] == l && hi[e0] == h)) m = ep / 3;
        }
    }
    mate[e] = m;
}

// the root above x: parent values only descend, so the walk ends; the count is a second bound
ADFP_DEV int mcl_root(const int* parent, int x, int nf) {
    for (int it = 0; it < nf; ++it) {
        const int p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
        if (p == x) break;
        x = p;
    }
    return x;
}

__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_hook(const int* __restrict__ mate, int* parent, int nf, int* changed) {
    const int f = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (f >= nf) return;
    if (__atomic_load_n(parent + f, __ATOMIC_RELAXED) < 0) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int g = mate[3 * (long long)f + c];
        if (g <= f) continue;                          // none, or the pair is the other face's to hook
        const int rf = mcl_root(parent, f, nf), rg = mcl_root(parent, g, nf);
        if (rf == rg) continue;
        atomicMin(parent + (rf > rg ? rf : rg), rf > rg ? rg : rf);
        *changed = 1;
    }
}

__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_compress(int* parent, int nf) {
    const int f = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (f >= nf) return;
    if (__atomic_load_n(parent + f, __ATOMIC_RELAXED) < 0) return;
    const int r = mcl_root(parent, f, nf);
    __atomic_store_n(parent + f, r, __ATOMIC_RELAXED);
}

// ---- areas and the keep rule ----
// area[f] = 0.5 * |cross(v1 - v0, v2 - v0)| in f64, numpy's order: cross = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), each
// product rounded, norm = sqrt((x x + y y) + z z).  key[f] = label (nf for a face without one), val[f] = f.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_areas(const float* __restrict__ v, const int* __restrict__ f, int nf,
                                                                 const int* __restrict__ label, double* __restrict__ area,
                                                                 int* __restrict__ key, int* __restrict__ val) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf) return;
    const int l = label[i];
    double ar = 0.0;
    if (l >= 0) {                                       // a labelled face has its indices in range (k_mcl_edges)
        const long long i0 = f[3 * (long long)i], i1 = f[3 * (long long)i + 1], i2 = f[3 * (long long)i + 2];
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p0 = (double)v[3 * i0 + c];
            a[c] = (double)v[3 * i1 + c] - p0;
            b[c] = (double)v[3 * i2 + c] - p0;
        }
        const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
        ar = 0.5 * sqrt((x * x + y * y) + z * z);
    }
    area[i] = ar;
    key[i] = l >= 0 ? l : nf;
    val[i] = i;
}

// Segmented sums over the faces in label order (key sorted, perm the faces): (flag, sum) pairs under (f1, s1) + (f2, s2) =
// (f1 | f2, f2 ? s2 : s1 + s2).  PASS 0: the tile's aggregate.  PASS 1: with the sum open at the tile's start (carry), the sum of
// every run at its last element -> comp_area[label].
struct MclSeg { const int* key; const int* perm; const double* area; int n; int nf; int ntiles;
                unsigned char* tile_flag; double* tile_sum; double* carry; double* comp_area; };

template <int PASS>
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_seg(MclSeg a) {
    __shared__ double s_sum[2][ADFP_MCL_THREADS];
    __shared__ unsigned char s_flag[2][ADFP_MCL_THREADS];
    const int t = threadIdx.x;
    const long long first = (long long)blockIdx.x * ADFP_MCL_TILE + (long long)t * ADFP_MCL_PER;
    int k[ADFP_MCL_PER + 1];
    double ar[ADFP_MCL_PER];
    const int kprev = first > 0 && first - 1 < a.n ? a.key[first - 1] : -1;
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) {
        const bool in = first + q < a.n;
        k[q] = in ? a.key[first + q] : -2 - q;                         // past the end: every item a run of its own
        ar[q] = in ? a.area[a.perm[first + q]] : 0.0;
    }
    k[ADFP_MCL_PER] = first + ADFP_MCL_PER < a.n ? a.key[first + ADFP_MCL_PER] : -1;
    bool fl = false;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) {
        const bool head = k[q] != (q ? k[q - 1] : kprev) || first + q == 0;
        if (head) { fl = true; s = ar[q]; } else s += ar[q];
    }
    // inclusive scan of the lanes' pairs by doubling
    int cur = 0;
    s_sum[0][t] = s; s_flag[0][t] = fl ? 1 : 0;
    __syncthreads();
    for (int o = 1; o < ADFP_MCL_THREADS; o <<= 1) {
        double ns = s_sum[cur][t];
        unsigned char nfl = s_flag[cur][t];
        if (t >= o) {
            if (!nfl) ns = s_sum[cur][t - o] + ns;
            nfl |= s_flag[cur][t - o];
        }
        s_sum[cur ^ 1][t] = ns; s_flag[cur ^ 1][t] = nfl;
        cur ^= 1;
        __syncthreads();
    }
    if (PASS == 0) {
        if (t == ADFP_MCL_THREADS - 1) { a.tile_flag[blockIdx.x] = s_flag[cur][t]; a.tile_sum[blockIdx.x] = s_sum[cur][t]; }
        return;
    }
    // what is open when this lane starts: the lanes before it, and before them the tile's carry
    double open = a.carry[blockIdx.x];
    if (t > 0) open = s_flag[cur][t - 1] ? s_sum[cur][t - 1] : open + s_sum[cur][t - 1];
#pragma unroll
    for (int q = 0; q < ADFP_MCL_PER; ++q) {
        const bool head = k[q] != (q ? k[q - 1] : kprev) || first + q == 0;
        open = head ? ar[q] : open + ar[q];
        if (first + q < a.n && k[q] != k[q + 1] && k[q] < a.nf) a.comp_area[k[q]] = open;
    }
}

// one lane: carry[t] = the sum open at the start of tile t
__global__ void k_mcl_seg_carry(MclSeg a) {
    if (threadIdx.x || blockIdx.x) return;
    double c = 0.0;
    for (int t = 0; t < a.ntiles; ++t) {
        a.carry[t] = c;
        c = a.tile_flag[t] ? a.tile_sum[t] : c + a.tile_sum[t];
    }
}

// the component of largest area, the smallest label among equals: (area, label) of the best root of each workgroup's faces
// (labels != NULL: the roots label[f] == f, their area comp_area[f]) or of earlier partials (labels == NULL: val / lab arrays)
struct MclBest { const int* labels; const double* val; const int* lab; int n; double* out_val; int* out_lab; };
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_best(MclBest a) {
    __shared__ double s_v[ADFP_MCL_THREADS];
    __shared__ int s_l[ADFP_MCL_THREADS];
    double bv = 0.0;
    int bl = -1;
    for (long long i = (long long)blockIdx.x * ADFP_MCL_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * ADFP_MCL_THREADS) {
        const int l = a.labels ? (a.labels[i] == (int)i ? (int)i : -1) : a.lab[i];
        if (l < 0) continue;
        const double v = a.val[i];
        if (bl < 0 || v > bv || (v == bv && l < bl)) { bv = v; bl = l; }
    }
    s_v[threadIdx.x] = bv; s_l[threadIdx.x] = bl;
    __syncthreads();
    for (int h = ADFP_MCL_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            const double v = s_v[threadIdx.x + h];
            const int l = s_l[threadIdx.x + h];
            if (l >= 0 && (s_l[threadIdx.x] < 0 || v > s_v[threadIdx.x] || (v == s_v[threadIdx.x] && l < s_l[threadIdx.x]))) {
                s_v[threadIdx.x] = v; s_l[threadIdx.x] = l;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { a.out_val[blockIdx.x] = s_v[0]; a.out_lab[blockIdx.x] = s_l[0]; }
}

// keep[f] = 1 iff f has a label and (best != NULL: label == *best; else: comp_area[label] > threshold)
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_keep(const int* __restrict__ label, int nf, const double* __restrict__ comp_area,
                                                                const int* __restrict__ best, double threshold, unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf) return;
    const int l = label[i];
    keep[i] = l >= 0 && (best ? l == best[0] : comp_area[l] > threshold) ? 1 : 0;
}

// ---- compaction ----
// used[v] = 1 for every vertex of a kept face (plain stores of 1); a kept face with an index outside [0, nv) is not kept (fkeep 0)
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_mark(const int* __restrict__ f, int nf, int nv, const unsigned char* __restrict__ keep,
                                                                unsigned char* __restrict__ fkeep, unsigned char* used) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf) return;
    const bool ok = mcl_face_ok(f, i, nv, keep);
    fkeep[i] = ok ? 1 : 0;
    if (!ok) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) used[f[3 * (long long)i + c]] = 1;
}

// rows of three f32 (and of three colour bytes when cin is given): out[pos[i]] = in[i] for every i with flag[i]
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_take_rows(const float* __restrict__ in, const unsigned char* __restrict__ cin, int n,
                                                                     const unsigned char* __restrict__ flag, const int* __restrict__ pos,
                                                                     float* __restrict__ out, unsigned char* __restrict__ cout) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const long long o = pos[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * o + c] = in[3 * (long long)i + c];
    if (cin) {
#pragma unroll
        for (int c = 0; c < 3; ++c) cout[3 * o + c] = cin[3 * (long long)i + c];
    }
}

// kept faces in order, re-indexed: out[fpos[i]][c] = vmap[f[i][c]]; fflag == NULL: every face
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_take_faces(const int* __restrict__ f, int nf, const unsigned char* __restrict__ fflag,
                                                                      const int* __restrict__ fpos, const int* __restrict__ vmap, int nv,
                                                                      int* __restrict__ out) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf || (fflag && !fflag[i])) return;
    const long long o = fflag ? fpos[i] : i;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int j = f[3 * (long long)i + c];
        out[3 * o + c] = (unsigned)j < (unsigned)nv ? vmap[j] : -1;
    }
}

// ---- coincident vertices ----
// key[i] = 16 bits (from bit `shift`) of word `word` of vertex perm[i]'s three f32 bit patterns
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_bits_key(const unsigned* __restrict__ v, const int* __restrict__ perm, int n,
                                                                    int word, int shift, int* __restrict__ key) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) key[i] = (int)((v[3 * (long long)perm[i] + word] >> shift) & 0xffffu);
}
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_iota(int* p, int n) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) p[i] = i;
}
ADFP_DEV bool mcl_same_bits(const unsigned* v, int a, int b) {
    return v[3 * (long long)a] == v[3 * (long long)b] && v[3 * (long long)a + 1] == v[3 * (long long)b + 1] &&
           v[3 * (long long)a + 2] == v[3 * (long long)b + 2];
}
// perm: the vertices grouped by bit pattern, ascending index inside a group.  head[i] = 1 iff sorted position i starts a group.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_heads(const unsigned* __restrict__ v, const int* __restrict__ perm, int n,
                                                                 unsigned char* __restrict__ head) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) head[i] = i == 0 || !mcl_same_bits(v, perm[i], perm[i - 1]) ? 1 : 0;
}
// gid[i] = heads before i (exclusive): a head writes first[gid] = its vertex
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_group_first(const int* __restrict__ perm, int n, const unsigned char* __restrict__ head,
                                                                       const int* __restrict__ gid, int* __restrict__ first) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n && head[i]) first[gid[i]] = perm[i];
}
// rep[vertex] = the first vertex of its group; survive[vertex] = 1 iff it is that vertex
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_rep(const int* __restrict__ perm, int n, const unsigned char* __restrict__ head,
                                                               const int* __restrict__ gid, const int* __restrict__ first,
                                                               int* __restrict__ rep, unsigned char* __restrict__ survive) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int g = head[i] ? gid[i] : gid[i] - 1;       // the exclusive count steps after the head
    rep[perm[i]] = first[g];
    survive[perm[i]] = head[i];
}
// vmap[v] = pos[rep[v]]: the merged index of every vertex
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_vmap(const int* __restrict__ rep, const int* __restrict__ pos, int n, int* __restrict__ vmap) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) vmap[i] = pos[rep[i]];
}

// ---- colours: (clip(c, 0, 1) * 255) truncated to a byte, f32 (Mesher.py:523-524 in numpy); rows of `stride` floats, 3 used ----
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_mcl_color_bytes(const float* __restrict__ rgb, long long n, int stride,
                                                                       unsigned char* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = rgb[i * stride + c];
        const float y = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);             // NaN passes through both, as np.clip leaves it
        out[3 * i + c] = y == y ? (unsigned char)(int)(y * 255.f) : (unsigned char)0;
    }
}
