// adfp_meshsimplify.h -- vertex clustering of a triangle mesh on the device (what open3d users call simplify_vertex_clustering):
// one vertex per occupied voxel cell, placed at the cell's average or by its faces' quadric, the faces re-indexed, collapsed and
// duplicate faces dropped, unreferenced clusters dropped.  Contract: include/adfp.h, "mesh simplification".
//
//   cells        the vertices as f64 points through the voxel down-sample's own kernels (adfp_refuse.h: k_vds_keys, k_vds_segment,
//                the stable passes of adfp_sort_pairs, VdsHead under the scan of adfp_scan.h, k_vds_mean): cluster k = the k-th
//                occupied cell in ascending key order, mean[k] its f64 average in input order.
//   clusters     one lane per cell: the vertex -> cluster map, the integer colour sums, the average as f32.
//   quadrics     3 F contributions (cluster of corner c of face f) in face-major order, sorted stably by cluster, so that a
//                cluster's run is in ascending (face, corner) order; one lane per cluster finds its run by bisection, sums A and b
//                over it in that order, diagonalises A with eight cyclic Jacobi sweeps in f64 and moves along the directions with
//                lambda > tau lambda_max.  No float atomics.
//   faces        rotated cluster triples (smallest index first; a collapsed face = (V, V, V)), grouped with the vertex merge's
//                kernels (k_mcl_bits_key, k_mcl_heads: stable 16-bit passes over the three words); the head of a group is its
//                earliest input face.  keep[] then goes through adfp_mesh_compact_plan on a sub-workspace: used clusters, the two
//                flag scans, totals; _emit gathers with k_mcl_take_rows / k_mcl_take_faces.
//
// One lane per cell walks its whole run, in k_vds_mean, k_msp_cells and k_msp_quadric: a voxel as large as the model makes those
// three loops as long as the mesh (DESIGN 5.4 states what such a call costs).
#pragma once
#include "adfp_meshclean.h"
#include "adfp_refuse.h"

#define ADFP_MSP_TAU 1e-3
#define ADFP_MSP_SWEEPS 8

struct MspArgs {
    const float* v; const int* f; const unsigned char* col; int nv, nf; double vs;
    const double* p64; const int* perm; const int* start; const long long* ncl;      // the cells: sorted order, run starts, their number
    const double* mean; int* cl; float* cpos; unsigned char* ccol;
    int* key; int* val;                                                              // [3 F] contributions, sorted by cluster
    int* tri; int* fperm;
};

// p64[i] = (double)v[i] over the 3 V components
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_f64(const float* __restrict__ v, long long n, double* __restrict__ p64) {
    const long long i = (long long)blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i < n) p64[i] = (double)v[i];
}

// one lane per cell k: cl[vertex] = k over its run, cpos[k] = the average rounded to f32, ccol[k] = (2 sum + n) / (2 n) per channel
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_cells(MspArgs a) {
    const long long k = (long long)blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    const long long M = a.ncl[0];
    if (k >= M) return;
    const int s = a.start[k], e = k + 1 < M ? a.start[k + 1] : a.nv;
    unsigned long long sum[3] = {0ull, 0ull, 0ull};
    for (int j = s; j < e; ++j) {
        const long long i = a.perm[j];
        a.cl[i] = (int)k;
        if (a.col) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] += a.col[3 * i + c];
        }
    }
    const unsigned long long n = (unsigned long long)(e - s);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.cpos[3 * k + c] = (float)a.mean[3 * k + c];
        if (a.col) a.ccol[3 * k + c] = (unsigned char)((2ull * sum[c] + n) / (2ull * n));
    }
}

// contribution e = 3 f + c: key[e] = the cluster of corner c (nv for a face with an index outside [0, nv): sorted last), val[e] = e
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_contrib(MspArgs a) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= a.nf) return;
    const bool ok = mcl_face_ok(a.f, i, a.nv, nullptr);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long e = 3 * (long long)i + c;
        a.key[e] = ok ? a.cl[a.f[e]] : a.nv;
        a.val[e] = (int)e;
    }
}

// one Jacobi rotation of a symmetric 3x3 in the plane (p, q), r the third index: zeroes a_pq; vkp, vkq = columns p, q of the vectors
ADFP_DEV void msp_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p, double& v1q,
                      double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double th = (aqq - app) / (2.0 * apq);
    const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));       // th = +-inf: t = 0, no rotation
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app -= t * apq; aqq += t * apq; apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y; arq = s * x + c * y;
    x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
    x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
    x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
}

// one lane per cluster k: A, b over its contributions in ascending (face, corner) order, relative to mean[k]; the truncated solve
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_quadric(MspArgs a) {
    const long long k = (long long)blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (k >= a.ncl[0]) return;
    const long long ne = 3 * (long long)a.nf;
    long long lo = 0, hi = ne;                              // the first contribution with key >= k
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a.key[mid] < (int)k) lo = mid + 1; else hi = mid;
    }
    const double m0 = a.mean[3 * k], m1 = a.mean[3 * k + 1], m2 = a.mean[3 * k + 2];
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (long long j = lo; j < ne && a.key[j] == (int)k; ++j) {
        const long long f = a.val[j] / 3;
        const long long i0 = a.f[3 * f], i1 = a.f[3 * f + 1], i2 = a.f[3 * f + 2];
        const double p0 = a.p64[3 * i0], p1 = a.p64[3 * i0 + 1], p2 = a.p64[3 * i0 + 2];
        const double u0 = a.p64[3 * i1] - p0, u1 = a.p64[3 * i1 + 1] - p1, u2 = a.p64[3 * i1 + 2] - p2;
        const double w0 = a.p64[3 * i2] - p0, w1 = a.p64[3 * i2 + 1] - p1, w2 = a.p64[3 * i2 + 2] - p2;
        const double g0 = u1 * w2 - u2 * w1, g1 = u2 * w0 - u0 * w2, g2 = u0 * w1 - u1 * w0;
        const double l = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
        if (!(l > 0.0) || !isfinite(l)) continue;
        const double n0 = g0 / l, n1 = g1 / l, n2 = g2 / l, w = 0.5 * l;
        const double d = -((n0 * (p0 - m0) + n1 * (p1 - m1)) + n2 * (p2 - m2));
        a00 += w * n0 * n0; a01 += w * n0 * n1; a02 += w * n0 * n2;
        a11 += w * n1 * n1; a12 += w * n1 * n2; a22 += w * n2 * n2;
        b0 += w * d * n0; b1 += w * d * n1; b2 += w * d * n2;
    }
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sw = 0; sw < ADFP_MSP_SWEEPS; ++sw) {
        msp_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);       // (0, 1), r = 2
        msp_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);       // (0, 2), r = 1
        msp_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);       // (1, 2), r = 0
    }
    const double lmax = fmax(a00, fmax(a11, a22));
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (lmax > 0.0) {
        const double cut = ADFP_MSP_TAU * lmax;
        if (a00 > cut) { const double q = -((v00 * b0 + v10 * b1) + v20 * b2) / a00; x0 += v00 * q; x1 += v10 * q; x2 += v20 * q; }
        if (a11 > cut) { const double q = -((v01 * b0 + v11 * b1) + v21 * b2) / a11; x0 += v01 * q; x1 += v11 * q; x2 += v21 * q; }
        if (a22 > cut) { const double q = -((v02 * b0 + v12 * b1) + v22 * b2) / a22; x0 += v02 * q; x1 += v12 * q; x2 += v22 * q; }
        if (!(fmax(fabs(x0), fmax(fabs(x1), fabs(x2))) <= a.vs)) { x0 = 0.0; x1 = 0.0; x2 = 0.0; }      // too far (or NaN): the average
    }
    a.cpos[3 * k] = (float)(m0 + x0); a.cpos[3 * k + 1] = (float)(m1 + x1); a.cpos[3 * k + 2] = (float)(m2 + x2);
}

// tri[f] = the face's clusters rotated so that the smallest is first; (nv, nv, nv) for a face with two equal clusters or an index
// outside [0, nv): grouped last, never kept.  fperm[f] = f.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_tri(MspArgs a) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= a.nf) return;
    int t0 = a.nv, t1 = a.nv, t2 = a.nv;
    if (mcl_face_ok(a.f, i, a.nv, nullptr)) {
        const int c0 = a.cl[a.f[3 * (long long)i]], c1 = a.cl[a.f[3 * (long long)i + 1]], c2 = a.cl[a.f[3 * (long long)i + 2]];
        if (c0 != c1 && c1 != c2 && c0 != c2) {
            if (c0 < c1 && c0 < c2) { t0 = c0; t1 = c1; t2 = c2; }
            else if (c1 < c2) { t0 = c1; t1 = c2; t2 = c0; }
            else { t0 = c2; t1 = c0; t2 = c1; }
        }
    }
    a.tri[3 * (long long)i] = t0; a.tri[3 * (long long)i + 1] = t1; a.tri[3 * (long long)i + 2] = t2;
    a.fperm[i] = i;
}

// fperm: the faces grouped by triple, ascending index inside a group.  keep[face] = 1 iff it heads its group and is not collapsed.
__global__ __launch_bounds__(ADFP_MCL_THREADS) void k_msp_keep(const int* __restrict__ tri, const int* __restrict__ fperm, int nf, int nv,
                                                                const unsigned char* __restrict__ head, unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * ADFP_MCL_THREADS + threadIdx.x;
    if (i >= nf) return;
    const int f = fperm[i];
    keep[f] = head[i] && tri[3 * (long long)f] < nv ? 1 : 0;
}

// ---- host side ----
// workspace: the cells' (p64 [3 V], key64, key, key_tmp, perm, perm_tmp, start [V], the scan's tiles, ncl, mean [3 V], counts [V]),
// cl [V], cpos [3 V] f32, ccol [3 V] bytes; ckey, ckey_tmp, cval, cval_tmp [3 F] (the faces' sort uses their first F entries);
// tri [3 F], head, keep [F] bytes; the sort's table for max(V, 3 F) keys; the compaction's workspace
struct MspWork { VdsArgs vds; int* key_tmp; int* perm_tmp; unsigned* tile_counts; long long* tile_offsets; long long* ncl; double* p64;
                 int* cl; float* cpos; unsigned char* ccol; int* ckey; int* ckey_tmp; int* cval; int* cval_tmp; int* tri;
                 unsigned char* head; unsigned char* keep; void* sort_ws; void* compact_ws; };
static MspWork msp_layout(Arena& A, long long nv, long long nf) {
    MspWork w;
    const size_t V = (size_t)nv, F = (size_t)nf, T = (size_t)ceil_div(nv, ADFP_VDS_TILE);
    w.p64 = A.take<double>(3 * V);
    w.vds.key64 = A.take<unsigned long long>(V);
    w.vds.key = A.take<int>(V); w.key_tmp = A.take<int>(V);
    w.vds.perm = A.take<int>(V); w.perm_tmp = A.take<int>(V);
    w.vds.start = A.take<int>(V);
    w.tile_counts = A.take<unsigned>(T);
    w.tile_offsets = A.take<long long>(T);
    w.ncl = A.take<long long>(1);
    w.vds.out = A.take<double>(3 * V);
    w.vds.counts = A.take<int>(V);
    w.cl = A.take<int>(V);
    w.cpos = A.take<float>(3 * V);
    w.ccol = A.take<unsigned char>(3 * V);
    w.ckey = A.take<int>(3 * F); w.ckey_tmp = A.take<int>(3 * F);
    w.cval = A.take<int>(3 * F); w.cval_tmp = A.take<int>(3 * F);
    w.tri = A.take<int>(3 * F);
    w.head = A.take<unsigned char>(F);
    w.keep = A.take<unsigned char>(F);
    w.sort_ws = A.take<char>(adfp_sort_workspace_bytes(nv > 3 * nf ? nv : 3 * nf));
    w.compact_ws = A.take<char>(adfp_mesh_compact_workspace_bytes(nv, nf));
    return w;
}

extern "C" {

size_t adfp_mesh_simplify_workspace_bytes(long long n_verts, long long n_faces) {
    return n_verts <= 0 || n_faces <= 0 || mcl_mesh_too_large(n_verts, n_faces) ? 0 : layout_bytes(msp_layout, n_verts, n_faces);
}

int adfp_mesh_simplify_plan(const float* verts, long long n_verts, const int* faces, long long n_faces, const unsigned char* colors,
                            double voxel_size, int contraction, const double min_bound[3], const double max_bound[3], void* workspace,
                            size_t workspace_bytes, long long* totals, void* stream) {
    if (n_verts < 0 || n_faces < 0 || !totals || !(voxel_size > 0.0) || !isfinite(voxel_size)) return ADFP_E_ARG;
    if (contraction != ADFP_SIMPLIFY_AVERAGE && contraction != ADFP_SIMPLIFY_QUADRIC) return ADFP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n_verts == 0 || n_faces == 0) {
        hipError_t e = hipMemsetAsync(totals, 0, 2 * sizeof(long long), st);
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!verts || !faces || !min_bound || !max_bound || !workspace) return ADFP_E_ARG;
    MspWork w;
    unsigned long long ncell = 1;
    double vmin[3];
    long long dim[3];
    for (int c = 0; c < 3; ++c) {                           // adfp_voxel_down_sample's cells
        if (!isfinite(min_bound[c]) || !isfinite(max_bound[c]) || !(min_bound[c] <= max_bound[c])) return ADFP_E_ARG;
        vmin[c] = min_bound[c] - voxel_size * 0.5;
        const double f = floor((max_bound[c] - vmin[c]) / voxel_size);
        if (!(f < (double)VDS_MAX_CELLS_PER_AXIS)) return ADFP_E_UNSUPPORTED;
        dim[c] = (long long)f + 1;
        ncell *= (unsigned long long)dim[c];
    }
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_simplify_workspace_bytes(n_verts, n_faces)) return ADFP_E_WORKSPACE;
    Arena A(workspace);
    w = msp_layout(A, n_verts, n_faces);
    const long long ne = 3 * n_faces;
    const dim3 block(ADFP_MCL_THREADS), gv(mcl_blocks(n_verts)), gf(mcl_blocks(n_faces));
    // the cells
    VdsArgs& d = w.vds;
    d.p = w.p64; d.n = (int)n_verts; d.vs = voxel_size; d.total = w.ncl;
    for (int c = 0; c < 3; ++c) { d.vmin[c] = vmin[c]; d.dim[c] = dim[c]; }
    hipLaunchKernelGGL(k_msp_f64, dim3(mcl_blocks(3 * n_verts)), block, 0, st, verts, 3 * n_verts, w.p64);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vds_keys, gv, block, 0, st, d);
    ADFP_CHECK_LAUNCH();
    int bits = 0;
    while (bits < 64 && ((ncell - 1) >> bits) != 0ull) ++bits;
    if (bits == 0) bits = 1;
    const size_t swb_v = adfp_sort_workspace_bytes(n_verts);
    for (int shift = 0; shift < bits; shift += 31) {
        hipLaunchKernelGGL(k_vds_segment, gv, block, 0, st, d, shift);
        ADFP_CHECK_LAUNCH();
        int rc = adfp_sort_pairs(d.key, d.perm, w.key_tmp, w.perm_tmp, n_verts, bits - shift < 31 ? bits - shift : 31, w.sort_ws, swb_v, stream);
        if (rc) return rc;
    }
    const VdsHead vhead = {d.key64, d.perm};
    int rc = scan_items<ADFP_VDS_PER_THREAD, ADFP_VDS_SCAN_THREADS, ADFP_VDS_SCAN_PER_THREAD, true>(vhead, n_verts, w.tile_counts, w.tile_offsets,
                                                                                                      d.start, w.ncl, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vds_mean, gv, block, 0, st, d);
    ADFP_CHECK_LAUNCH();
    // the clusters
    MspArgs a;
    a.v = verts; a.f = faces; a.col = colors; a.nv = (int)n_verts; a.nf = (int)n_faces; a.vs = voxel_size;
    a.p64 = w.p64; a.perm = d.perm; a.start = d.start; a.ncl = w.ncl; a.mean = d.out; a.cl = w.cl; a.cpos = w.cpos; a.ccol = w.ccol;
    a.key = w.ckey; a.val = w.cval; a.tri = w.tri; a.fperm = w.cval;
    hipLaunchKernelGGL(k_msp_cells, gv, block, 0, st, a);
    ADFP_CHECK_LAUNCH();
    const int vbits = mcl_bits(n_verts);                    // cluster indices and the sentinel lie in [0, n_verts]
    if (contraction == ADFP_SIMPLIFY_QUADRIC) {
        hipLaunchKernelGGL(k_msp_contrib, gf, block, 0, st, a);
        ADFP_CHECK_LAUNCH();
        rc = adfp_sort_pairs(w.ckey, w.cval, w.ckey_tmp, w.cval_tmp, ne, vbits, w.sort_ws, adfp_sort_workspace_bytes(ne), stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_msp_quadric, gv, block, 0, st, a);
        ADFP_CHECK_LAUNCH();
    }
    // the faces
    hipLaunchKernelGGL(k_msp_tri, gf, block, 0, st, a);
    ADFP_CHECK_LAUNCH();
    const size_t swb_f = adfp_sort_workspace_bytes(n_faces);
    for (int ps = 0; ps < 6; ++ps) {                       // the three words in stable passes of 16 bits, the lowest first
        const int shift = 16 * (ps & 1), kb = vbits - shift < 16 ? vbits - shift : 16;
        if (kb <= 0) continue;                              // no index reaches the upper half
        hipLaunchKernelGGL(k_mcl_bits_key, gf, block, 0, st, (const unsigned*)w.tri, w.cval, (int)n_faces, 2 - ps / 2, shift, w.ckey);
        ADFP_CHECK_LAUNCH();
        rc = adfp_sort_pairs(w.ckey, w.cval, w.ckey_tmp, w.cval_tmp, n_faces, kb, w.sort_ws, swb_f, stream);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_mcl_heads, gf, block, 0, st, (const unsigned*)w.tri, w.cval, (int)n_faces, w.head);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_msp_keep, gf, block, 0, st, w.tri, w.cval, (int)n_faces, (int)n_verts, w.head, w.keep);
    ADFP_CHECK_LAUNCH();
    // used clusters, positions of the survivors, totals
    return adfp_mesh_compact_plan(w.tri, n_faces, n_verts, w.keep, w.compact_ws, adfp_mesh_compact_workspace_bytes(n_verts, n_faces), totals, stream);
}

int adfp_mesh_simplify_emit(long long n_verts, long long n_faces, const void* workspace, size_t workspace_bytes, float* verts_out,
                            unsigned char* colors_out, long long n_verts_out, int* faces_out, long long n_faces_out, void* stream) {
    if (n_verts < 0 || n_faces < 0 || n_verts_out < 0 || n_faces_out < 0 || n_verts_out > n_verts || n_faces_out > n_faces) return ADFP_E_ARG;
    if (n_verts_out == 0 && n_faces_out == 0) return 0;
    if (!workspace || (n_verts_out > 0 && !verts_out) || (n_faces_out > 0 && !faces_out)) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_mesh_simplify_workspace_bytes(n_verts, n_faces)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Arena A(workspace);
    const MspWork w = msp_layout(A, n_verts, n_faces);
    Arena B(w.compact_ws);
    const MclCompact c = mcl_compact_layout(B, n_verts, n_faces);
    if (n_verts_out > 0) {
        hipLaunchKernelGGL(k_mcl_take_rows, dim3(mcl_blocks(n_verts)), dim3(ADFP_MCL_THREADS), 0, st, w.cpos,
                           colors_out ? (const unsigned char*)w.ccol : (const unsigned char*)nullptr, (int)n_verts, c.used, c.vpos, verts_out, colors_out);
        ADFP_CHECK_LAUNCH();
    }
    if (n_faces_out > 0) {
        hipLaunchKernelGGL(k_mcl_take_faces, dim3(mcl_blocks(n_faces)), dim3(ADFP_MCL_THREADS), 0, st, w.tri, (int)n_faces, c.fkeep, c.fpos, c.vpos,
                           (int)n_verts, faces_out);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

}   // extern "C"
