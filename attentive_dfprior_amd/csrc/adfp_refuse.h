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

#define ADFP_UNIT 16               // voxels per unit edge (open3d's ScalableTSDFVolume volume_unit_resolution)
#define ADFP_TOUCH_THREADS 256
#define ADFP_FUSE_THREADS 256      // 16 x 16 columns of one unit
#define ADFP_VDS_THREADS 256
#define ADFP_VDS_PER_THREAD 4
#define ADFP_VDS_TILE (ADFP_VDS_THREADS * ADFP_VDS_PER_THREAD)
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
    unsigned* tile_counts; long long* tile_offsets; int ntiles; int* start; long long* total;
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

ADFP_DEV bool vds_head(const VdsArgs& a, int i) { return i == 0 || a.key64[a.perm[i]] != a.key64[a.perm[i - 1]]; }

// heads (first point of a cell in sorted order) per tile of ADFP_VDS_TILE sorted points
__global__ __launch_bounds__(ADFP_VDS_THREADS) void k_vds_tile_heads(VdsArgs a) {
    __shared__ unsigned lds[ADFP_VDS_THREADS / 64];
    const long long first = (long long)blockIdx.x * ADFP_VDS_TILE + (long long)threadIdx.x * ADFP_VDS_PER_THREAD;
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < ADFP_VDS_PER_THREAD; ++q) c += (first + q < a.n && vds_head(a, (int)(first + q))) ? 1u : 0u;
    unsigned tot;
    mc_block_scan<unsigned, ADFP_VDS_THREADS>(c, tot, lds);
    if (threadIdx.x == 0) a.tile_counts[blockIdx.x] = tot;
}

// one workgroup: exclusive prefix of the tile counts; total[0] = the number of cells
__global__ __launch_bounds__(ADFP_VDS_SCAN_THREADS) void k_vds_tile_scan(VdsArgs a) {
    __shared__ unsigned long long lds[ADFP_VDS_SCAN_THREADS / 64];
    unsigned long long carry = 0;
    const long long per_round = (long long)ADFP_VDS_SCAN_THREADS * ADFP_VDS_SCAN_PER_THREAD;
    for (long long t0 = 0; t0 < a.ntiles; t0 += per_round) {
        const long long first = t0 + (long long)threadIdx.x * ADFP_VDS_SCAN_PER_THREAD;
        unsigned cv[ADFP_VDS_SCAN_PER_THREAD];
        unsigned long long s = 0;
#pragma unroll
        for (int q = 0; q < ADFP_VDS_SCAN_PER_THREAD; ++q) {
            cv[q] = first + q < a.ntiles ? a.tile_counts[first + q] : 0u;
            s += cv[q];
        }
        unsigned long long tot;
        unsigned long long o = carry + mc_block_scan<unsigned long long, ADFP_VDS_SCAN_THREADS>(s, tot, lds);
#pragma unroll
        for (int q = 0; q < ADFP_VDS_SCAN_PER_THREAD; ++q) {
            if (first + q < a.ntiles) a.tile_offsets[first + q] = (long long)o;
            o += cv[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) a.total[0] = (long long)carry;
}

// start[cell] = the sorted position of the cell's first point
__global__ __launch_bounds__(ADFP_VDS_THREADS) void k_vds_starts(VdsArgs a) {
    __shared__ unsigned lds[ADFP_VDS_THREADS / 64];
    const long long first = (long long)blockIdx.x * ADFP_VDS_TILE + (long long)threadIdx.x * ADFP_VDS_PER_THREAD;
    bool h[ADFP_VDS_PER_THREAD];
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < ADFP_VDS_PER_THREAD; ++q) {
        h[q] = first + q < a.n && vds_head(a, (int)(first + q));
        c += h[q] ? 1u : 0u;
    }
    unsigned tot;
    long long cell = a.tile_offsets[blockIdx.x] + mc_block_scan<unsigned, ADFP_VDS_THREADS>(c, tot, lds);
#pragma unroll
    for (int q = 0; q < ADFP_VDS_PER_THREAD; ++q)
        if (h[q]) a.start[cell++] = (int)(first + q);
}

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
