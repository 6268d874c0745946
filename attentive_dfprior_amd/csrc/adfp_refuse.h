// adfp_refuse.h -- ScanNet mesh evaluation on the device (the reference's src/tools/evaluate_scannet.py):
//
//   unit touch marks (f64)   open3d ScalableTSDFVolume::Integrate's voxel-unit allocation as we read it: every stride-th pixel's
//                            depth point, back-projected in f64, marks the 16^3-voxel units within sdf_trunc of it, per view
//   unit-gated fusion (f32)  one workgroup per touched unit, one lane per (x, y) column holding its 16 tsdf and 16 weight values in
//                            VGPRs across a whole chunk of views, applied in view order (IntegrateWithDepthToCameraDistanceMultiplier)
//   voxel downsample (f64)   PointCloud::voxel_down_sample: linear cell keys, stable radix passes, one lane per cell summing its
//                            points in input order
//
// The culled depth render is adfp_raycast.h's kernel with a cull mode.  The exact contract of each entry is stated in
// include/adfp.h; tests/refuse_ref.py restates it in numpy.
#pragma once
#include "adfp_raycast.h"
#include "adfp_scan.h"

#define ADFP_UNIT 16               // voxels per unit edge (open3d's ScalableTSDFVolume volume_unit_resolution)
#define ADFP_TOUCH_THREADS 256
#define ADFP_FUSE_THREADS 256      // 16 x 16 columns of one unit
#define ADFP_VDS_THREADS 256
#define ADFP_VDS_PER_THREAD 4
#define ADFP_VDS_TILE (ADFP_VDS_THREADS * ADFP_VDS_PER_THREAD)
static_assert(ADFP_VDS_THREADS == ADFP_SCAN_THREADS, "the cells are scanned in tiles of ADFP_VDS_TILE points");
#define ADFP_VDS_SCAN_THREADS 1024
#define ADFP_VDS_SCAN_PER_THREAD 8

struct TouchArgs {
    const float* depth; int H, W, stride, nsx, nsy;           // depth [views][H][W]; the strided pixel grid is nsx x nsy
    const double* c2w; double fx, fy, cx, cy;                 // c2w [views][12] (f64)
    float depth_trunc; double trunc, unit;
    int lo[3], dim[3]; long long nunits;                      // the unit box: world unit indices lo .. lo + dim - 1
    unsigned char* touched; int* outside; int view0;          // touched [views][nunits]
};

// One lane per strided pixel of view view0 + grid y.  d in (0, depth_trunc]; p = ((m0 x + m1 y) + m2 d) + m3 per row in f64 with
// x = ((u - cx) d) / fx, y = ((v - cy) d) / fy; units floor((p - trunc) / unit) .. floor((p + trunc) / unit) per axis.  A
// non-finite bound touches nothing; a range reaching outside the box counts once in *outside and marks its part inside.
__global__ __launch_bounds__(ADFP_TOUCH_THREADS) void k_refuse_touch(TouchArgs a) {
    const int t = blockIdx.x * ADFP_TOUCH_THREADS + threadIdx.x;
    if (t >= a.nsx * a.nsy) return;
    const int u = (t % a.nsx) * a.stride, v = (t / a.nsx) * a.stride;
    const long long p = (long long)a.view0 + blockIdx.y;
    const float df = a.depth[(p * a.H + v) * (long long)a.W + u];
    if (!(df > 0.f && df <= a.depth_trunc)) return;
    const double d = df;
    const double x = (((double)u - a.cx) * d) / a.fx, y = (((double)v - a.cy) * d) / a.fy;
    const double* m = a.c2w + 12 * p;
    int i0[3], i1[3];
    bool out = false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double q = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * d) + m[4 * r + 3];
        const double f0 = floor((q - a.trunc) / a.unit), f1 = floor((q + a.trunc) / a.unit);
        if (!isfinite(f0) || !isfinite(f1)) return;           // no float-to-int conversion of NaN or inf
        const double lo = (double)a.lo[r], hi = (double)a.lo[r] + (double)(a.dim[r] - 1);
        out = out || f0 < lo || f1 > hi;
        i0[r] = (int)(fmin(fmax(f0, lo), hi + 1.0) - lo);     // clamped to the box before the conversion: an empty range
        i1[r] = (int)(fmax(fmin(f1, hi), lo - 1.0) - lo);     // when the point's range misses the box
    }
    if (out) atomicAdd(a.outside, 1);
    unsigned char* T = a.touched + p * a.nunits;
    for (int ix = i0[0]; ix <= i1[0]; ++ix)
        for (int iy = i0[1]; iy <= i1[1]; ++iy)
            for (int iz = i0[2]; iz <= i1[2]; ++iz) T[((long long)ix * a.dim[1] + iy) * a.dim[2] + iz] = 1;   // idempotent
}

struct FuseArgs {
    float* tsdf; float* weight;                               // [nx][ny][nz], z fastest, n_ = 16 dim_
    int dim[3]; long long ny, nz; long long nunits;
    const int* units;                                         // the units to visit (linear unit ids)
    const float* depth; const float* w2c; const unsigned char* touched; int n_views, H, W;
    float fx, fy, cx, cy, trunc, inv_trunc, depth_trunc, safe_w, safe_h;
    long long org[3]; double voxel;                           // world voxel index of the box's first voxel; voxel length
};

// One workgroup per listed unit, lane = (x, y) column; every view of the chunk in order, skipped for the whole unit (a uniform,
// scalar branch) when it did not touch the unit.  Per voxel and view, in f32: cam = ((r0 x + r1 y) + r2 z) + t; cam.z <= 0 skips;
// u_f = ((cam.x fx) / cam.z + cx) + 0.5, inside [0.0001, W - 0.0001) (the same for v), u = (int)u_f; d = depth[v][u] in
// (0, depth_trunc]; sdf = (d - cam.z) sqrt((du du + dv dv) + 1), du = (u - cx) / fx, dv = (v - cy) / fy; if sdf > -trunc:
// t = min(1, sdf inv_trunc), tsdf = (tsdf w + t) / (w + 1), w = w + 1.
__global__ __launch_bounds__(ADFP_FUSE_THREADS) void k_refuse_integrate(FuseArgs a) {
    const int unit = a.units[blockIdx.x];
    if (unit < 0 || (long long)unit >= a.nunits) return;                 // uniform; no barrier below
    const int uz = unit % a.dim[2], uy = (unit / a.dim[2]) % a.dim[1], ux = unit / (a.dim[2] * a.dim[1]);
    const int X = ux * ADFP_UNIT + (threadIdx.x >> 4), Y = uy * ADFP_UNIT + (threadIdx.x & 15), Z0 = uz * ADFP_UNIT;
    const long long base = ((long long)X * a.ny + Y) * a.nz + Z0;          // a multiple of 16: 64-byte aligned columns
    float ts[ADFP_UNIT], wt[ADFP_UNIT], zc[ADFP_UNIT];
#pragma unroll
    for (int q = 0; q < ADFP_UNIT; q += 4) {
        const float4 t4 = *(const float4*)(a.tsdf + base + q);
        const float4 w4 = *(const float4*)(a.weight + base + q);
        ts[q] = t4.x; ts[q + 1] = t4.y; ts[q + 2] = t4.z; ts[q + 3] = t4.w;
        wt[q] = w4.x; wt[q + 1] = w4.y; wt[q + 2] = w4.z; wt[q + 3] = w4.w;
    }
    const float xc = (float)(((double)(a.org[0] + X) + 0.5) * a.voxel);
    const float yc = (float)(((double)(a.org[1] + Y) + 0.5) * a.voxel);
#pragma unroll
    for (int q = 0; q < ADFP_UNIT; ++q) zc[q] = (float)(((double)(a.org[2] + Z0 + q) + 0.5) * a.voxel);
    for (int k = 0; k < a.n_views; ++k) {
        if (!a.touched[(long long)k * a.nunits + unit]) continue;          // uniform: the whole unit skips the view
        const float* m = a.w2c + 12 * k;                                    // uniform address: scalar loads
        const float* img = a.depth + (long long)k * a.H * a.W;
        const float px = m[0] * xc + m[1] * yc, py = m[4] * xc + m[5] * yc, pz = m[8] * xc + m[9] * yc;
#pragma unroll
        for (int q = 0; q < ADFP_UNIT; ++q) {
            const float cz = (pz + m[10] * zc[q]) + m[11];
            if (!(cz > 0.f)) continue;
            const float cx = (px + m[2] * zc[q]) + m[3], cy = (py + m[6] * zc[q]) + m[7];
            const float uf = ((cx * a.fx) / cz + a.cx) + 0.5f, vf = ((cy * a.fy) / cz + a.cy) + 0.5f;
            if (!(uf >= 0.0001f && uf < a.safe_w && vf >= 0.0001f && vf < a.safe_h)) continue;
            const int u = (int)uf, v = (int)vf;                             // u in [0, W), v in [0, H)
            const float d = img[(long long)v * a.W + u];
            if (!(d > 0.f && d <= a.depth_trunc)) continue;
            const float du = ((float)u - a.cx) / a.fx, dv = ((float)v - a.cy) / a.fy;
            const float sdf = (d - cz) * sqrtf((du * du + dv * dv) + 1.f);
            if (sdf > -a.trunc) {
                const float tn = fminf(1.f, sdf * a.inv_trunc);
                ts[q] = (ts[q] * wt[q] + tn) / (wt[q] + 1.f);
                wt[q] = wt[q] + 1.f;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < ADFP_UNIT; q += 4) {
        *(float4*)(a.tsdf + base + q) = make_float4(ts[q], ts[q + 1], ts[q + 2], ts[q + 3]);
        *(float4*)(a.weight + base + q) = make_float4(wt[q], wt[q + 1], wt[q + 2], wt[q + 3]);
    }
}

// ---- voxel downsample ----
struct VdsArgs {
    const double* p; int n; double vmin[3]; double vs; long long dim[3];
    unsigned long long* key64; int* key; int* perm;
    int* start; long long* total;                  // start[cell] = the sorted position of the cell's first point, total[0] = the cells
    double* out; int* counts;
};

// key64[i] = (ix dim1 + iy) dim2 + iz, i_c = floor((p_c - vmin_c) / vs) (clamped to the box: only a guard, the caller's bounds
// contain every point); perm[i] = i
__global__ __launch_bounds__(ADFP_VDS_THREADS) void k_vds_keys(VdsArgs a) {
    const int i = blockIdx.x * ADFP_VDS_THREADS + threadIdx.x;
    if (i >= a.n) return;
    long long ix[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double f = floor((a.p[3 * (long long)i + c] - a.vmin[c]) / a.vs);
        ix[c] = f >= 0.0 ? (f < (double)(a.dim[c] - 1) ? (long long)f : a.dim[c] - 1) : 0;   // NaN -> 0
    }
    a.key64[i] = (unsigned long long)((ix[0] * a.dim[1] + ix[1]) * a.dim[2] + ix[2]);
    a.perm[i] = i;
}

// key[i] = bits [shift, shift + 31) of key64[perm[i]]: one LSD pass of the stable sort
__global__ __launch_bounds__(ADFP_VDS_THREADS) void k_vds_segment(VdsArgs a, int shift) {
    const int i = blockIdx.x * ADFP_VDS_THREADS + threadIdx.x;
    if (i >= a.n) return;
    a.key[i] = (int)((a.key64[a.perm[i]] >> shift) & 0x7fffffffull);
}

// the scan's predicate (adfp_scan.h): sorted position i is the first point of its cell
struct VdsHead {
    const unsigned long long* key64; const int* perm;
    ADFP_DEV bool operator()(long long i) const { return i == 0 || key64[perm[i]] != key64[perm[i - 1]]; }
};

// one lane per cell c < total: the f64 sum of its points in sorted (= input, the sort is stable) order over the count
__global__ __launch_bounds__(ADFP_VDS_THREADS) void k_vds_mean(VdsArgs a) {
    const long long c = (long long)blockIdx.x * ADFP_VDS_THREADS + threadIdx.x;
    const long long M = a.total[0];
    if (c >= M) return;
    const int s = a.start[c], e = c + 1 < M ? a.start[c + 1] : a.n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = s; j < e; ++j) {
        const long long i = a.perm[j];
        sx += a.p[3 * i]; sy += a.p[3 * i + 1]; sz += a.p[3 * i + 2];
    }
    const double k = (double)(e - s);
    a.out[3 * c] = sx / k; a.out[3 * c + 1] = sy / k; a.out[3 * c + 2] = sz / k;
    a.counts[c] = e - s;
}

// ---- host side: the launchers ----
static bool box_ok(const int lo[3], const int dim[3], long long* nunits) {
    long long n = 1;
    for (int c = 0; c < 3; ++c) {
        if (dim[c] <= 0) return false;
        n *= dim[c];
        if (n > 0x7fffffffll) { *nunits = -1; return true; }
    }
    *nunits = n;
    return true;
}

int adfp_refuse_touch(const float* depth, long long n_views, int H, int W, const double* c2w, double fx, double fy, double cx, double cy,
                      int stride, float depth_trunc, double sdf_trunc, double unit_length, const int unit_lo[3], const int unit_dim[3],
                      unsigned char* touched, int* outside, void* stream) {
    if (n_views < 0 || H <= 0 || W <= 0 || stride < 1 || !unit_lo || !unit_dim) return ADFP_E_ARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if (!(sdf_trunc >= 0.0) || !isfinite(sdf_trunc) || !(unit_length > 0.0) || !isfinite(unit_length) || !(depth_trunc > 0.f))
        return ADFP_E_ARG;
    long long nunits = 0;
    if (!box_ok(unit_lo, unit_dim, &nunits)) return ADFP_E_ARG;
    if (n_views == 0) return 0;
    if (!depth || !c2w || !touched || !outside) return ADFP_E_ARG;
    if (nunits < 0 || H > RT_MAX_SIDE || W > RT_MAX_SIDE || n_views > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(touched, 0, (size_t)n_views * (size_t)nunits, st);
    if (e != hipSuccess) return (int)e;
    TouchArgs a;
    a.depth = depth; a.H = H; a.W = W; a.stride = stride; a.nsx = (int)ceil_div(W, stride); a.nsy = (int)ceil_div(H, stride);
    a.c2w = c2w; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.depth_trunc = depth_trunc; a.trunc = sdf_trunc; a.unit = unit_length;
    for (int c = 0; c < 3; ++c) { a.lo[c] = unit_lo[c]; a.dim[c] = unit_dim[c]; }
    a.nunits = nunits; a.touched = touched; a.outside = outside;
    const unsigned nblk = (unsigned)ceil_div((long long)a.nsx * a.nsy, ADFP_TOUCH_THREADS);
    for (long long v0 = 0; v0 < n_views; v0 += RT_VIEWS_PER_LAUNCH) {
        const long long nv = n_views - v0 < RT_VIEWS_PER_LAUNCH ? n_views - v0 : RT_VIEWS_PER_LAUNCH;
        a.view0 = (int)v0;
        hipLaunchKernelGGL(k_refuse_touch, dim3(nblk, (unsigned)nv), dim3(ADFP_TOUCH_THREADS), 0, st, a);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

#define FUSE_MAX_VIEWS 65536
int adfp_refuse_integrate(float* tsdf, float* weight, const int unit_lo[3], const int unit_dim[3], double voxel, const int* units,
                          long long n_units, const float* depth, const float* w2c, const unsigned char* touched, long long n_views, int H,
                          int W, float fx, float fy, float cx, float cy, float sdf_trunc, float depth_trunc, void* stream) {
    if (n_units < 0 || n_views < 0 || H <= 0 || W <= 0 || !unit_lo || !unit_dim) return ADFP_E_ARG;
    if (!(voxel > 0.0) || !isfinite(voxel) || !(sdf_trunc > 0.f) || !isfinite(sdf_trunc) || !(depth_trunc > 0.f)) return ADFP_E_ARG;
    if (!(fx != 0.f) || !(fy != 0.f) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    long long nunits = 0;
    if (!box_ok(unit_lo, unit_dim, &nunits)) return ADFP_E_ARG;
    if (n_units == 0 || n_views == 0) return 0;
    if (!tsdf || !weight || !units || !depth || !w2c || !touched) return ADFP_E_ARG;
    if (nunits < 0 || n_units > nunits || n_views > FUSE_MAX_VIEWS || H > RT_MAX_SIDE || W > RT_MAX_SIDE) return ADFP_E_UNSUPPORTED;
    FuseArgs a;
    a.tsdf = tsdf; a.weight = weight;
    for (int c = 0; c < 3; ++c) { a.dim[c] = unit_dim[c]; a.org[c] = (long long)unit_lo[c] * ADFP_UNIT; }
    a.ny = (long long)unit_dim[1] * ADFP_UNIT; a.nz = (long long)unit_dim[2] * ADFP_UNIT; a.nunits = nunits;
    a.units = units; a.depth = depth; a.w2c = w2c; a.touched = touched; a.n_views = (int)n_views; a.H = H; a.W = W;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.trunc = sdf_trunc; a.inv_trunc = 1.0f / sdf_trunc; a.depth_trunc = depth_trunc;
    a.safe_w = (float)W - 0.0001f; a.safe_h = (float)H - 0.0001f; a.voxel = voxel;
    hipLaunchKernelGGL(k_refuse_integrate, dim3((unsigned)n_units), dim3(ADFP_FUSE_THREADS), 0, (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

#define VDS_MAX_CELLS_PER_AXIS (1ll << 21)
struct VdsWork { int* key_tmp; int* perm_tmp; unsigned* tile_counts; long long* tile_offsets; void* sort_ws; };
static VdsWork vds_layout(Arena& A, long long n, VdsArgs& a) {
    VdsWork w;
    const size_t N = (size_t)n, T = (size_t)ceil_div(n, ADFP_VDS_TILE);
    a.key64 = A.take<unsigned long long>(N);
    a.key = A.take<int>(N); w.key_tmp = A.take<int>(N);
    a.perm = A.take<int>(N); w.perm_tmp = A.take<int>(N);
    a.start = A.take<int>(N);
    w.tile_counts = A.take<unsigned>(T);
    w.tile_offsets = A.take<long long>(T);
    w.sort_ws = A.take<char>(adfp_sort_workspace_bytes(n));
    return w;
}
size_t adfp_voxel_down_sample_workspace_bytes(long long n) {
    VdsArgs a;
    return n <= 0 || n > RECON_MAX_N ? 0 : layout_bytes(vds_layout, n, a);
}

int adfp_voxel_down_sample(const double* points, long long n, double voxel_size, const double min_bound[3], const double max_bound[3],
                           void* workspace, size_t workspace_bytes, double* out, int* counts, long long* total, void* stream) {
    if (n < 0 || !(voxel_size > 0.0) || !isfinite(voxel_size) || !total) return ADFP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        hipError_t e = hipMemsetAsync(total, 0, sizeof(long long), st);
        return e == hipSuccess ? 0 : (int)e;
    }
    if (!points || !min_bound || !max_bound || !workspace || !out || !counts) return ADFP_E_ARG;
    VdsArgs a;
    unsigned long long ncell = 1;
    for (int c = 0; c < 3; ++c) {
        if (!isfinite(min_bound[c]) || !isfinite(max_bound[c]) || !(min_bound[c] <= max_bound[c])) return ADFP_E_ARG;
        a.vmin[c] = min_bound[c] - voxel_size * 0.5;
        const double f = floor((max_bound[c] - a.vmin[c]) / voxel_size);
        if (!(f < (double)VDS_MAX_CELLS_PER_AXIS)) return ADFP_E_UNSUPPORTED;
        a.dim[c] = (long long)f + 1;
        ncell *= (unsigned long long)a.dim[c];
    }
    if (n > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_voxel_down_sample_workspace_bytes(n)) return ADFP_E_WORKSPACE;
    Arena A(workspace);
    const VdsWork w = vds_layout(A, n, a);
    const size_t sort_wsb = adfp_sort_workspace_bytes(n);
    a.p = points; a.n = (int)n; a.vs = voxel_size; a.total = total; a.out = out; a.counts = counts;
    int bits = 0;
    while (bits < 64 && ((ncell - 1) >> bits) != 0ull) ++bits;
    if (bits == 0) bits = 1;
    const unsigned nb = (unsigned)ceil_div(n, ADFP_VDS_THREADS);
    hipLaunchKernelGGL(k_vds_keys, dim3(nb), dim3(ADFP_VDS_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    for (int shift = 0; shift < bits; shift += 31) {                     // LSD: low segment first, every pass stable
        hipLaunchKernelGGL(k_vds_segment, dim3(nb), dim3(ADFP_VDS_THREADS), 0, st, a, shift);
        ADFP_CHECK_LAUNCH();
        const int kb = bits - shift < 31 ? bits - shift : 31;
        int rc = adfp_sort_pairs(a.key, a.perm, w.key_tmp, w.perm_tmp, n, kb, w.sort_ws, sort_wsb, stream);
        if (rc) return rc;
    }
    const VdsHead head = {a.key64, a.perm};
    int rc = scan_items<ADFP_VDS_PER_THREAD, ADFP_VDS_SCAN_THREADS, ADFP_VDS_SCAN_PER_THREAD, true>(head, n, w.tile_counts, w.tile_offsets,
                                                                                                      a.start, total, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vds_mean, dim3(nb), dim3(ADFP_VDS_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}
