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
//   compaction   flags -> exclusive scan (adfp_scan.h: k_scan_count, k_tile_scan, k_scan_place) -> gathers.
#pragma once
#include "adfp_device.h"
#include "adfp_scan.h"

#define ADFP_MCL_THREADS 256
#define ADFP_MCL_PER 8
#define ADFP_MCL_TILE (ADFP_MCL_THREADS * ADFP_MCL_PER)
static_assert(ADFP_MCL_THREADS == ADFP_SCAN_THREADS, "flags are scanned in tiles of ADFP_MCL_TILE items");

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

// ---- host side: the launchers ----
static unsigned mcl_blocks(long long n) { return (unsigned)ceil_div(n, ADFP_MCL_THREADS); }
static size_t mcl_tiles(long long n) { return (size_t)ceil_div(n, ADFP_MCL_TILE); }
static int mcl_bits(long long top) { int b = 1; while (b < 31 && (top >> b) != 0) ++b; return b; }     // top < 2^bits
// pos[i] = set flags before i, total[0] = their number; tc / to: mcl_tiles(n) entries each
static int mcl_scan(const unsigned char* flag, long long n, unsigned* tc, long long* to, int* pos, long long* total, hipStream_t st) {
    return scan_items<ADFP_MCL_PER, ADFP_MCL_THREADS, ADFP_MCL_PER, false>(FlagSet{flag}, n, tc, to, pos, total, st);
}

extern "C" {

int adfp_mesh_seen_mask(const float* verts, long long n_verts, const float* w2c, long long n_poses, int rule, const float* depth,
                        const float* depth_max, float fx, float fy, float cx, float cy, int W, int H, unsigned char* seen, void* stream) {
    if (n_verts < 0 || n_poses < 0 || W < 1 || H < 1) return ADFP_E_ARG;
    if (rule != ADFP_SEEN_FRUSTUM && rule != ADFP_SEEN_MAX_DEPTH && rule != ADFP_SEEN_DEPTH_TEST) return ADFP_E_ARG;
    if (n_verts == 0) return 0;
    if (!verts || !seen || (n_poses > 0 && !w2c)) return ADFP_E_ARG;
    if (n_poses > 0 && ((rule == ADFP_SEEN_MAX_DEPTH && !depth_max) || (rule == ADFP_SEEN_DEPTH_TEST && !depth))) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_poses > RECON_MAX_N / 12 || W > 32768 || H > 32768) return ADFP_E_UNSUPPORTED;
    if (rule == ADFP_SEEN_DEPTH_TEST && (W < 2 || H < 2)) return ADFP_E_UNSUPPORTED;       // the sample grid divides by W - 1, H - 1
    CullArgs a;
    a.v = nullptr; a.vf = verts; a.nv = (int)n_verts; a.w2c = w2c; a.np = (int)n_poses;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.W = (float)W; a.H = (float)H; a.seen = seen;
    a.depth = depth; a.dmax = depth_max; a.Wi = W; a.Hi = H;
    a.rW = W > 1 ? 1.0f / (float)(W - 1) : 0.f; a.rH = H > 1 ? 1.0f / (float)(H - 1) : 0.f;
    const dim3 grid(mcl_blocks(n_verts)), block(ADFP_NN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (rule == ADFP_SEEN_FRUSTUM) hipLaunchKernelGGL(k_cull_seen<ADFP_CULL_RULE_FRUSTUM>, grid, block, 0, st, a);
    else if (rule == ADFP_SEEN_MAX_DEPTH) hipLaunchKernelGGL(k_cull_seen<ADFP_CULL_RULE_MAX_DEPTH>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_cull_seen<ADFP_CULL_RULE_DEPTH_TEST>, grid, block, 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

static bool mcl_mesh_too_large(long long n_verts, long long n_faces) { return n_verts > RECON_MAX_N || n_faces > RECON_MAX_N / 3; }

// half-edge workspace: lo, hi, key, key_tmp, perm, perm_tmp [3 F] ints, the sort's
struct MclEdges { int* lo; int* hi; int* key; int* key_tmp; int* perm; int* perm_tmp; void* sort_ws; };
static MclEdges mcl_edges_layout(Arena& A, long long nf) {
    MclEdges m;
    int** ints[6] = {&m.lo, &m.hi, &m.key, &m.key_tmp, &m.perm, &m.perm_tmp};
    for (int k = 0; k < 6; ++k) *ints[k] = A.take<int>(3 * (size_t)nf);
    m.sort_ws = A.take<char>(adfp_sort_workspace_bytes(3 * nf));
    return m;
}
size_t adfp_mesh_face_labels_workspace_bytes(long long n_faces) {
    return n_faces <= 0 || n_faces > RECON_MAX_N / 3 ? 0 : layout_bytes(mcl_edges_layout, n_faces);
}

int adfp_mesh_face_labels_begin(const int* faces, long long n_faces, long long n_verts, const unsigned char* keep, int* mate, int* labels,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (n_faces < 0 || n_verts < 0) return ADFP_E_ARG;
    if (n_faces == 0) return 0;
    if (!faces || !mate || !labels || !workspace) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_face_labels_workspace_bytes(n_faces)) return ADFP_E_WORKSPACE;
    const long long ne = 3 * n_faces;
    Arena A(workspace);
    const MclEdges m = mcl_edges_layout(A, n_faces);
    const size_t swb = adfp_sort_workspace_bytes(ne);
    hipStream_t st = (hipStream_t)stream;
    const int bits = mcl_bits(n_verts);                                     // keys lie in [0, n_verts]
    hipLaunchKernelGGL(k_mcl_edges, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, faces, (int)n_faces, (int)n_verts, keep, m.lo, m.hi,
                       m.perm, labels);
    ADFP_CHECK_LAUNCH();
    const int* src[2] = {m.hi, m.lo};                                         // by the larger vertex, then (stable) by the smaller
    for (int ps = 0; ps < 2; ++ps) {
        hipLaunchKernelGGL(k_mcl_gather, dim3(mcl_blocks(ne)), dim3(ADFP_MCL_THREADS), 0, st, src[ps], m.perm, (int)ne, m.key);
        ADFP_CHECK_LAUNCH();
        int rc = adfp_sort_pairs(m.key, m.perm, m.key_tmp, m.perm_tmp, ne, bits, m.sort_ws, swb, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mcl_mates, dim3(mcl_blocks(ne)), dim3(ADFP_MCL_THREADS), 0, st, m.lo, m.hi, m.perm, (int)ne, (int)n_verts, mate);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_mesh_face_labels_rounds(const int* mate, int* labels, long long n_faces, int rounds, int* changed, void* stream) {
    if (n_faces < 0 || rounds < 1 || !changed) return ADFP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_faces == 0) { hipError_t e = hipMemsetAsync(changed, 0, sizeof(int), st); return e == hipSuccess ? 0 : (int)e; }
    if (!mate || !labels) return ADFP_E_ARG;
    if (n_faces > RECON_MAX_N / 3) return ADFP_E_UNSUPPORTED;
    for (int r = 0; r < rounds; ++r) {
        hipError_t e = hipMemsetAsync(changed, 0, sizeof(int), st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_mcl_hook, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, mate, labels, (int)n_faces, changed);
        ADFP_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mcl_compress, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, labels, (int)n_faces);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

#define MCL_BEST_BLOCKS 1024
// component workspace: area, comp_area [F] doubles, key, key_tmp, perm, perm_tmp [F] ints, the segmented scan's tiles, the partials
// and the result of the largest-component search, the sort's
struct MclKeep { double* area; double* comp_area; int* key; int* key_tmp; int* perm; int* perm_tmp; unsigned char* tile_flag; double* tile_sum;
                 double* carry; double* part_val; int* part_lab; double* best_val; int* best_lab; void* sort_ws; };
static MclKeep mcl_keep_layout(Arena& A, long long nf) {
    MclKeep m;
    const size_t f = (size_t)nf, T = mcl_tiles(nf);
    m.area = A.take<double>(f); m.comp_area = A.take<double>(f);
    m.key = A.take<int>(f); m.key_tmp = A.take<int>(f); m.perm = A.take<int>(f); m.perm_tmp = A.take<int>(f);
    m.tile_flag = A.take<unsigned char>(T); m.tile_sum = A.take<double>(T); m.carry = A.take<double>(T);
    m.part_val = A.take<double>(MCL_BEST_BLOCKS); m.part_lab = A.take<int>(MCL_BEST_BLOCKS);
    m.best_val = A.take<double>(1); m.best_lab = A.take<int>(1);
    m.sort_ws = A.take<char>(adfp_sort_workspace_bytes(nf));
    return m;
}
size_t adfp_mesh_component_keep_workspace_bytes(long long n_faces) {
    return n_faces <= 0 || n_faces > RECON_MAX_N / 3 ? 0 : layout_bytes(mcl_keep_layout, n_faces);
}

int adfp_mesh_component_keep(const float* verts, long long n_verts, const int* faces, long long n_faces, const int* labels, int largest,
                             double threshold, unsigned char* keep, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_faces < 0 || n_verts < 0 || (largest != 0 && largest != 1) || (!largest && threshold != threshold)) return ADFP_E_ARG;
    if (n_faces == 0) return 0;
    if (!faces || !labels || !keep || !workspace || (n_verts > 0 && !verts)) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_component_keep_workspace_bytes(n_faces)) return ADFP_E_WORKSPACE;
    Arena A(workspace);
    const MclKeep m = mcl_keep_layout(A, n_faces);
    const unsigned T = (unsigned)mcl_tiles(n_faces);
    hipStream_t st = (hipStream_t)stream;
    const int nf = (int)n_faces;
    const dim3 grid(mcl_blocks(n_faces)), block(ADFP_MCL_THREADS);
    hipLaunchKernelGGL(k_mcl_areas, grid, block, 0, st, verts, faces, nf, labels, m.area, m.key, m.perm);
    ADFP_CHECK_LAUNCH();
    int rc = adfp_sort_pairs(m.key, m.perm, m.key_tmp, m.perm_tmp, n_faces, mcl_bits(n_faces), m.sort_ws, adfp_sort_workspace_bytes(n_faces), stream);
    if (rc) return rc;
    MclSeg s;
    s.key = m.key; s.perm = m.perm; s.area = m.area; s.n = nf; s.nf = nf; s.ntiles = (int)T; s.comp_area = m.comp_area;
    s.tile_flag = m.tile_flag; s.tile_sum = m.tile_sum; s.carry = m.carry;
    hipLaunchKernelGGL(k_mcl_seg<0>, dim3(T), block, 0, st, s);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mcl_seg_carry, dim3(1), dim3(64), 0, st, s);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mcl_seg<1>, dim3(T), block, 0, st, s);
    ADFP_CHECK_LAUNCH();
    if (largest) {
        MclBest b;
        const unsigned nb = grid.x < MCL_BEST_BLOCKS ? grid.x : MCL_BEST_BLOCKS;
        b.labels = labels; b.val = m.comp_area; b.lab = nullptr; b.n = nf; b.out_val = m.part_val; b.out_lab = m.part_lab;
        hipLaunchKernelGGL(k_mcl_best, dim3(nb), block, 0, st, b);
        ADFP_CHECK_LAUNCH();
        b.labels = nullptr; b.val = m.part_val; b.lab = m.part_lab; b.n = (int)nb; b.out_val = m.best_val; b.out_lab = m.best_lab;
        hipLaunchKernelGGL(k_mcl_best, dim3(1), block, 0, st, b);
        ADFP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_mcl_keep, grid, block, 0, st, labels, nf, m.comp_area, largest ? m.best_lab : (const int*)nullptr, threshold, keep);
    ADFP_CHECK_LAUNCH();
    return 0;
}

// compaction workspace: fkeep [F], used [V] (bytes), fpos [F], vpos [V] (ints), tile counts / offsets for the longer of the two
struct MclCompact { unsigned char* fkeep; unsigned char* used; int* fpos; int* vpos; unsigned* tc; long long* to; };
static MclCompact mcl_compact_layout(Arena& A, long long nv, long long nf) {
    MclCompact c;
    const size_t T = mcl_tiles(nv > nf ? nv : nf);
    c.fkeep = A.take<unsigned char>((size_t)nf);
    c.used = A.take<unsigned char>((size_t)nv);
    c.fpos = A.take<int>((size_t)nf);
    c.vpos = A.take<int>((size_t)nv);
    c.tc = A.take<unsigned>(T);
    c.to = A.take<long long>(T);
    return c;
}
size_t adfp_mesh_compact_workspace_bytes(long long n_verts, long long n_faces) {
    return n_verts < 0 || n_faces < 0 || mcl_mesh_too_large(n_verts, n_faces) ? 0 : layout_bytes(mcl_compact_layout, n_verts, n_faces);
}

int adfp_mesh_compact_plan(const int* faces, long long n_faces, long long n_verts, const unsigned char* keep, void* workspace,
                           size_t workspace_bytes, long long* totals, void* stream) {
    if (n_faces < 0 || n_verts < 0 || !totals) return ADFP_E_ARG;
    if (n_faces > 0 && (!faces || !keep)) return ADFP_E_ARG;
    if ((n_faces > 0 || n_verts > 0) && !workspace) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_compact_workspace_bytes(n_verts, n_faces)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Arena A(workspace);
    const MclCompact c = mcl_compact_layout(A, n_verts, n_faces);
    if (n_verts > 0) { hipError_t e = hipMemsetAsync(c.used, 0, (size_t)n_verts, st); if (e != hipSuccess) return (int)e; }
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_mcl_mark, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, faces, (int)n_faces, (int)n_verts, keep, c.fkeep,
                           c.used);
        ADFP_CHECK_LAUNCH();
    }
    int rc = mcl_scan(c.used, n_verts, c.tc, c.to, c.vpos, totals, st);
    if (rc) return rc;
    return mcl_scan(c.fkeep, n_faces, c.tc, c.to, c.fpos, totals + 1, st);
}

int adfp_mesh_compact_emit(const float* verts, long long n_verts, const int* faces, long long n_faces, const void* workspace,
                           size_t workspace_bytes, float* verts_out, long long n_verts_out, int* faces_out, long long n_faces_out, void* stream) {
    if (n_faces < 0 || n_verts < 0 || n_verts_out < 0 || n_faces_out < 0 || n_verts_out > n_verts || n_faces_out > n_faces) return ADFP_E_ARG;
    if (n_verts_out == 0 && n_faces_out == 0) return 0;
    if (!workspace || !verts || (n_faces_out > 0 && (!faces || !faces_out)) || (n_verts_out > 0 && !verts_out)) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_compact_workspace_bytes(n_verts, n_faces)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Arena A(workspace);
    const MclCompact c = mcl_compact_layout(A, n_verts, n_faces);
    if (n_verts_out > 0) {
        hipLaunchKernelGGL(k_mcl_take_rows, dim3(mcl_blocks(n_verts)), dim3(ADFP_MCL_THREADS), 0, st, verts, (const unsigned char*)nullptr,
                           (int)n_verts, c.used, c.vpos, verts_out, (unsigned char*)nullptr);
        ADFP_CHECK_LAUNCH();
    }
    if (n_faces_out > 0) {
        hipLaunchKernelGGL(k_mcl_take_faces, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, faces, (int)n_faces, c.fkeep, c.fpos, c.vpos,
                           (int)n_verts, faces_out);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

// merge workspace: key, key_tmp, perm, perm_tmp, gid, first, rep, pos, vmap [V] ints, head, survive [V] bytes, tiles, the sort's
struct MclMerge { int* key; int* key_tmp; int* perm; int* perm_tmp; int* gid; int* first; int* rep; int* pos; int* vmap;
                  unsigned char* head; unsigned char* survive; unsigned* tc; long long* to; void* sort_ws; };
static MclMerge mcl_merge_layout(Arena& A, long long nv) {
    MclMerge m;
    int** ints[9] = {&m.key, &m.key_tmp, &m.perm, &m.perm_tmp, &m.gid, &m.first, &m.rep, &m.pos, &m.vmap};
    for (int k = 0; k < 9; ++k) *ints[k] = A.take<int>((size_t)nv);
    m.head = A.take<unsigned char>((size_t)nv);
    m.survive = A.take<unsigned char>((size_t)nv);
    m.tc = A.take<unsigned>(mcl_tiles(nv));
    m.to = A.take<long long>(mcl_tiles(nv));
    m.sort_ws = A.take<char>(adfp_sort_workspace_bytes(nv));
    return m;
}
size_t adfp_mesh_merge_workspace_bytes(long long n_verts) {
    return n_verts <= 0 || n_verts > RECON_MAX_N ? 0 : layout_bytes(mcl_merge_layout, n_verts);
}

int adfp_mesh_merge_plan(const float* verts, long long n_verts, void* workspace, size_t workspace_bytes, long long* total, void* stream) {
    if (n_verts < 0 || !total) return ADFP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_verts == 0) { hipError_t e = hipMemsetAsync(total, 0, sizeof(long long), st); return e == hipSuccess ? 0 : (int)e; }
    if (!verts || !workspace) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_merge_workspace_bytes(n_verts)) return ADFP_E_WORKSPACE;
    Arena A(workspace);
    const MclMerge m = mcl_merge_layout(A, n_verts);
    const int n = (int)n_verts;
    const dim3 grid(mcl_blocks(n_verts)), block(ADFP_MCL_THREADS);
    const unsigned* bits = (const unsigned*)verts;
    const size_t swb = adfp_sort_workspace_bytes(n_verts);
    hipLaunchKernelGGL(k_mcl_iota, grid, block, 0, st, m.perm, n);
    ADFP_CHECK_LAUNCH();
    for (int ps = 0; ps < 6; ++ps) {                       // 96 key bits in stable passes of 16, the lowest first
        hipLaunchKernelGGL(k_mcl_bits_key, grid, block, 0, st, bits, m.perm, n, 2 - ps / 2, 16 * (ps & 1), m.key);
        ADFP_CHECK_LAUNCH();
        int rc = adfp_sort_pairs(m.key, m.perm, m.key_tmp, m.perm_tmp, n_verts, 16, m.sort_ws, swb, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mcl_heads, grid, block, 0, st, bits, m.perm, n, m.head);
    ADFP_CHECK_LAUNCH();
    int rc = mcl_scan(m.head, n_verts, m.tc, m.to, m.gid, total, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mcl_group_first, grid, block, 0, st, m.perm, n, m.head, m.gid, m.first);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mcl_rep, grid, block, 0, st, m.perm, n, m.head, m.gid, m.first, m.rep, m.survive);
    ADFP_CHECK_LAUNCH();
    rc = mcl_scan(m.survive, n_verts, m.tc, m.to, m.pos, total, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_mcl_vmap, grid, block, 0, st, m.rep, m.pos, n, m.vmap);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_mesh_merge_emit(const float* verts, const unsigned char* colors, long long n_verts, const int* faces, long long n_faces,
                         const void* workspace, size_t workspace_bytes, float* verts_out, unsigned char* colors_out, long long n_verts_out,
                         int* faces_out, void* stream) {
    if (n_verts < 0 || n_faces < 0 || n_verts_out < 0 || n_verts_out > n_verts) return ADFP_E_ARG;
    if (n_verts == 0 && n_faces == 0) return 0;
    if ((n_verts > 0 && (!workspace || !verts || !verts_out)) || (n_faces > 0 && (!faces || !faces_out))) return ADFP_E_ARG;
    if ((colors != nullptr) != (colors_out != nullptr)) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_merge_workspace_bytes(n_verts)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    MclMerge m;
    memset(&m, 0, sizeof(m));
    if (n_verts > 0) {
        Arena A(workspace);
        m = mcl_merge_layout(A, n_verts);
        hipLaunchKernelGGL(k_mcl_take_rows, dim3(mcl_blocks(n_verts)), dim3(ADFP_MCL_THREADS), 0, st, verts, colors, (int)n_verts, m.survive, m.pos,
                           verts_out, colors_out);
        ADFP_CHECK_LAUNCH();
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_mcl_take_faces, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, faces, (int)n_faces,
                           (const unsigned char*)nullptr, (const int*)nullptr, m.vmap, (int)n_verts, faces_out);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

int adfp_mesh_color_bytes(const float* rgb, long long n, int stride, unsigned char* out, void* stream) {
    if (n < 0 || stride < 3) return ADFP_E_ARG;
    if (n == 0) return 0;
    if (!rgb || !out) return ADFP_E_ARG;
    if (n > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_mcl_color_bytes, dim3(mcl_blocks(n)), dim3(ADFP_MCL_THREADS), 0, (hipStream_t)stream, rgb, n, stride, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}

}   // extern "C"
