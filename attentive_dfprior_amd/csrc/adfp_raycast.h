// adfp_raycast.h -- depth rendering of triangle meshes on the device (calc_2d_metric of the reference's src/tools/eval_recon.py):
//
//   triangle BVH (f64)      the NN index's construction over triangles: Morton codes of the centroids (adfp_recon.h's box and
//                           code kernels, the radix sort), leaves of `leaf` triangles holding their nine vertex coordinates and
//                           original face indices, an implicit complete binary tree of leaf boxes (padding leaves inverted)
//   ray (f64)               RtRay, filled from a pose and an image-plane point by rt_ray; rt_box, the slab test against a padded
//                           box; rt_tri, Woop, Benthin & Wald's watertight test.  Both walks below are adfp_recon.h's bvh_walk
//                           with a visitor made of these: RtNearest (closed, shrinking bound) and RtAny (open, fixed bound)
//   depth render (f64)      one lane per pixel, a wave per 8x8 tile, four tiles per workgroup, views along grid y; the walk
//                           ordered by entry t, the nearest hit
//   views in sight (f32)    check_proj of eval_recon.py:70-96 for a batch of poses: k_cull_seen's test, a wave ballot per pose
//                           and one integer atomic OR
//   points visible          points x poses: k_cull_seen's f32 frustum test per pair, then for the pairs that pass an any-hit shadow
//                           ray in the renderer's f64 arithmetic (one lane per point, poses through LDS), the left child first
//   depth L1 sums (f64)     per view, sum |a - b| of two f32 depth images: k_l1_partial, then k_red_final<1> with a view per workgroup
//
// The exact contract (camera, intersection, clipping, pruning) is stated in include/adfp.h; tests/depth_ref.py restates it in numpy.
#pragma once
#include "adfp_recon.h"

// triangles per leaf: 4, 8 or 16 at run time.  ADFP_TRI_LEAF_DEFAULT (include/adfp.h) is 4: 100 views at 500 x 500 of a 1.18 M-face
// room render in 50.6 ms with leaves of 4, 58.5 ms with 8 and 73.0 ms with 16 (tools/recon_bench.py --2d, medians)
#define ADFP_RT_THREADS 256        // four waves: a 16 x 16 pixel block of four 8 x 8 tiles
#define ADFP_RT_BOX_PAD 0x1p-24    // boxes grow by this times (max |mesh coordinate| + max |camera origin|) at query time

// triangle i's centroid ((v0 + v1) + v2) / 3, NaN for a face with an index outside [0, nv): the box pass (fmin / fmax) skips it
// and the Morton pass sends it to code 0
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_tri_centroids(const double* __restrict__ v, int nv, const int* __restrict__ f, int nf,
                                                                     double* __restrict__ c) {
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (i >= nf) return;
    const int i0 = f[3 * (long long)i], i1 = f[3 * (long long)i + 1], i2 = f[3 * (long long)i + 2];
    const bool ok = (unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        c[3 * (long long)i + k] = ok ? ((v[3 * (long long)i0 + k] + v[3 * (long long)i1 + k]) + v[3 * (long long)i2 + k]) / 3.0 : NAN;
}

// the sorted triangles: tri[9 s .. 9 s + 9) = v0, v1, v2 of face perm[s] (NaN for an out-of-range face: never hit), orig[s] = perm[s]
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_tri_gather(const double* __restrict__ v, int nv, const int* __restrict__ f, int nf,
                                                                  const int* __restrict__ perm, double* __restrict__ tri, int* __restrict__ orig) {
    const int s = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    if (s >= nf) return;
    const int j = perm[s];
    int id[3];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        id[c] = f[3 * (long long)j + c];
        ok = ok && (unsigned)id[c] < (unsigned)nv;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) tri[9 * (long long)s + 3 * c + k] = ok ? v[3 * (long long)id[c] + k] : NAN;
    orig[s] = j;
}

// where the pieces of a triangle BVH live (the host's make_tri): sorted triangles, node boxes, the leaves [P, 2 P) at depth D
struct TriDev { const double* tri; const double* box; int nf; int leaf; long long P; int D; };

// the ray o + t Dw, Dw = R (dx, dy, 1), of pose [R | o] through the image-plane point (dx, dy); inv = 1 / Dw, or 0 on an axis the
// ray is parallel to; pad = what the boxes grow by
struct RtRay { double R[9], o[3], dx, dy, Dw[3], inv[3], pad; };

// m: 12 f64, [R | o] row-major; rb: the root box (the mesh's)
ADFP_DEV void rt_ray(RtRay& r, const double* m, double dx, double dy, const double* rb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int c = 0; c < 3; ++c) r.R[3 * i + c] = m[4 * i + c];
        r.o[i] = m[4 * i + 3];
    }
    r.dx = dx; r.dy = dy;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = (r.R[3 * i] * dx + r.R[3 * i + 1] * dy) + r.R[3 * i + 2];
        if (fabs(t) < 1e-200) t = 0.0;                       // parallel to the axis: a containment test, never 0 x inf
        r.Dw[i] = t;
        r.inv[i] = t != 0.0 ? 1.0 / t : 0.0;
    }
    const double M = fmax(fmax(fmax(fabs(rb[0]), fabs(rb[3])), fmax(fabs(rb[1]), fabs(rb[4]))), fmax(fabs(rb[2]), fabs(rb[5])));
    r.pad = ADFP_RT_BOX_PAD * (M + fmax(fmax(fabs(r.o[0]), fabs(r.o[1])), fabs(r.o[2])));
}

// Does the ray meet box b, grown by pad, at some t in [near, best]?  Inverted boxes never do.  An axis with Dw = 0 is a
// containment test (no 0 x inf); elsewhere the slab of each axis is [(lo - o) inv, (hi - o) inv] sorted, with finite factors.
// *tin = the entry t.  The pad is far above the rounding of both this test and the triangle test (include/adfp.h).
ADFP_DEV bool rt_box(const RtRay& r, const double* b, double near, double best, double* tin) {
    if (!(b[0] <= b[3])) return false;
    double tn = -INFINITY, tf = INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lo = b[c] - r.pad, hi = b[3 + c] + r.pad;
        if (r.Dw[c] == 0.0) {
            if (r.o[c] < lo || r.o[c] > hi) return false;
        } else {
            const double t0 = (lo - r.o[c]) * r.inv[c], t1 = (hi - r.o[c]) * r.inv[c];
            tn = fmax(tn, fmin(t0, t1));
            tf = fmin(tf, fmax(t0, t1));
        }
    }
    *tin = tn;
    return tn <= tf && tn <= best && tf >= near;
}

// Does the ray's line meet triangle t (v0, v1, v2)?  A vertex goes to camera space as cam_c = ((R0c e0 + R1c e1) + R2c e2),
// e = v - o; the shear A' = (Ax - dx Az, Ay - dy Az); U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; a miss when their
// signs are mixed or det = (U + V) + W is 0; *z = ((U Az + V Bz) + W Cz) / det, NaN for an out-of-range face: it fails the caller's
// range test.  CULL (ADFP_CULL_*): BACK keeps only det > 0, FRONT only det < 0 (det = -(n . R d), n = (v1 - v0) x (v2 - v0):
// det > 0 is a face whose normal points toward the camera).
template <int CULL>
ADFP_DEV bool rt_tri(const RtRay& r, const double* t, double* z) {
    double cam[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double e0 = t[3 * q] - r.o[0], e1 = t[3 * q + 1] - r.o[1], e2 = t[3 * q + 2] - r.o[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) cam[3 * q + c] = (r.R[c] * e0 + r.R[3 + c] * e1) + r.R[6 + c] * e2;
    }
    const double Ax = cam[0] - r.dx * cam[2], Ay = cam[1] - r.dy * cam[2];
    const double Bx = cam[3] - r.dx * cam[5], By = cam[4] - r.dy * cam[5];
    const double Cx = cam[6] - r.dx * cam[8], Cy = cam[7] - r.dy * cam[8];
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if ((U < 0.0 || V < 0.0 || W < 0.0) && (U > 0.0 || V > 0.0 || W > 0.0)) return false;
    const double det = (U + V) + W;
    if (det == 0.0) return false;
    if (CULL == ADFP_CULL_BACK && !(det > 0.0)) return false;
    if (CULL == ADFP_CULL_FRONT && !(det < 0.0)) return false;
    *z = ((U * cam[2] + V * cam[5]) + W * cam[8]) / det;
    return true;
}

// bvh_walk's visitor for the nearest hit: the least z in [near, best], best shrinking with every hit (a closed bound: an equal
// z is a hit again, and a box entered exactly at best is still walked)
template <int CULL>
struct RtNearest {
    const RtRay& r; const TriDev& t; double near, best; bool found;
    ADFP_DEV bool enter(const double* b, double* tin) { return rt_box(r, b, near, best, tin); }
    ADFP_DEV bool leaf(long long j) {
        const long long s0 = j * t.leaf, s1 = s0 + t.leaf < t.nf ? s0 + t.leaf : t.nf;
        for (long long s = s0; s < s1; ++s) {
            double z;
            if (rt_tri<CULL>(r, t.tri + 9 * s, &z) && z >= near && z <= best) { best = z; found = true; }
        }
        return false;
    }
};

// bvh_walk's visitor for a shadow ray: is there any hit (back faces included) with near <= z < best?  The bound is open and fixed,
// so a box entered at or beyond it is pruned too, and the first hit ends the walk: existence over a set does not depend on order
struct RtAny {
    const RtRay& r; const TriDev& t; double near, best;
    ADFP_DEV bool enter(const double* b, double* tin) { return rt_box(r, b, near, best, tin) && *tin < best; }
    ADFP_DEV bool leaf(long long j) {
        const long long s0 = j * t.leaf, s1 = s0 + t.leaf < t.nf ? s0 + t.leaf : t.nf;
        for (long long s = s0; s < s1; ++s) {
            double z;
            if (rt_tri<ADFP_CULL_NONE>(r, t.tri + 9 * s, &z) && z >= near && z < best) return true;
        }
        return false;
    }
};

struct RenderArgs {
    TriDev t;
    const double* c2w; const double* near; double far;       // c2w [views][12] (3x4 row-major), near [views]
    int H, W, nbx; double fx, fy, cx, cy;
    int view0;                                                // first view of this launch
    float* depth;                                             // [views][H][W]
};

// One lane, one pixel (row i, col j) of view p: the ray through d = ((j - cx) / fx, (i - cy) / fy, 1); the depth is the least z of
// a hit (rt_tri<CULL>) with near <= z <= far, rounded to f32, or 0.  The culled modes write 0 for a view whose pose holds a
// non-finite entry.
template <int CULL>
__global__ __launch_bounds__(ADFP_RT_THREADS) void k_render_depth(RenderArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)a.nbx), by = (int)(blockIdx.x / (unsigned)a.nbx);
    const int col = bx * 16 + (w & 1) * 8 + (lane & 7);
    const int row = by * 16 + (w >> 1) * 8 + (lane >> 3);
    if (row >= a.H || col >= a.W) return;                   // no barrier below
    const long long p = (long long)a.view0 + blockIdx.y;
    const double* m = a.c2w + 12 * p;
    float* out = a.depth + (p * a.H + row) * (long long)a.W + col;
    if (CULL != ADFP_CULL_NONE) {                           // uniform over the workgroup: one view per grid row
        bool fin = true;
#pragma unroll
        for (int e = 0; e < 12; ++e) fin = fin && isfinite(m[e]);
        if (!fin) { *out = 0.f; return; }
    }
    RtRay r;
    rt_ray(r, m, ((double)col - a.cx) / a.fx, ((double)row - a.cy) / a.fy, a.t.box + 6);
    RtNearest<CULL> v = {r, a.t, a.near[p], a.far, false};
    if (a.t.nf > 0) bvh_walk<true>(a.t.box, a.t.P, a.t.D, v);
    *out = v.found ? (float)v.best : 0.f;
}

// ---- hit render: the nearest hit's depth, original face index and barycentric weights ----
// bvh_walk's visitor for the nearest hit and its identity: RtNearest's closed, shrinking bound, so every triangle whose z equals
// the least one is visited, and among those the smallest original face index wins -- a function of the set of hits, not of the
// walk.  The winner travels as its sorted slot and its original index (two 32-bit registers, the slot doubling as RtNearest's
// `found`); U, V, W are not kept but formed once more after the walk (rt_bary).
template <int CULL>
struct RtHit {
    const RtRay& r; const TriDev& t; const int* orig; double near, best; int slot, face;      // slot < 0: no hit yet
    ADFP_DEV bool enter(const double* b, double* tin) { return rt_box(r, b, near, best, tin); }
    ADFP_DEV bool leaf(long long j) {
        const long long s0 = j * t.leaf, s1 = s0 + t.leaf < t.nf ? s0 + t.leaf : t.nf;
        for (long long s = s0; s < s1; ++s) {
            double z;
            if (rt_tri<CULL>(r, t.tri + 9 * s, &z) && z >= near && z <= best) {
                const int o = orig[s];
                if (slot < 0 || z < best || o < face) { slot = (int)s; face = o; }
                best = z;
            }
        }
        return false;
    }
};

// (V / det, W / det) of triangle t for ray r, rounded to f32: rt_tri's arithmetic again, operation for operation, for a
// triangle that rt_tri has accepted (det != 0)
ADFP_DEV void rt_bary(const RtRay& r, const double* t, float* b1, float* b2) {
    double cam[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const double e0 = t[3 * q] - r.o[0], e1 = t[3 * q + 1] - r.o[1], e2 = t[3 * q + 2] - r.o[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) cam[3 * q + c] = (r.R[c] * e0 + r.R[3 + c] * e1) + r.R[6 + c] * e2;
    }
    const double Ax = cam[0] - r.dx * cam[2], Ay = cam[1] - r.dy * cam[2];
    const double Bx = cam[3] - r.dx * cam[5], By = cam[4] - r.dy * cam[5];
    const double Cx = cam[6] - r.dx * cam[8], Cy = cam[7] - r.dy * cam[8];
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const double det = (U + V) + W;
    *b1 = (float)(V / det);
    *b2 = (float)(W / det);
}

struct HitArgs {
    TriDev t; const int* orig;                                // orig [nf]: the original face index of each sorted slot
    const double* c2w; const double* near; double far;
    int H, W, nbx; double fx, fy, cx, cy;
    int view0;
    float* depth; int* face; float* bary;                     // [views][H][W], [views][H][W], [views][H][W][2]; each may be NULL
};

// k_render_depth's lane, pixel and ray; depth is its value bit for bit, face the original index of the nearest hit (the smallest
// among hits of equal z) or -1, bary = (V / det, W / det) of that triangle or (0, 0)
template <int CULL>
__global__ __launch_bounds__(ADFP_RT_THREADS) void k_render_hits(HitArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int bx = (int)(blockIdx.x % (unsigned)a.nbx), by = (int)(blockIdx.x / (unsigned)a.nbx);
    const int col = bx * 16 + (w & 1) * 8 + (lane & 7);
    const int row = by * 16 + (w >> 1) * 8 + (lane >> 3);
    if (row >= a.H || col >= a.W) return;                   // no barrier below
    const long long p = (long long)a.view0 + blockIdx.y;
    const double* m = a.c2w + 12 * p;
    const long long px = (p * a.H + row) * (long long)a.W + col;
    float z = 0.f, b1 = 0.f, b2 = 0.f;
    int face = -1;
    bool fin = true;
    if (CULL != ADFP_CULL_NONE) {                           // uniform over the workgroup: one view per grid row
#pragma unroll
        for (int e = 0; e < 12; ++e) fin = fin && isfinite(m[e]);
    }
    if (fin) {
        RtRay r;
        rt_ray(r, m, ((double)col - a.cx) / a.fx, ((double)row - a.cy) / a.fy, a.t.box + 6);
        RtHit<CULL> v = {r, a.t, a.orig, a.near[p], a.far, -1, -1};
        bvh_walk<true>(a.t.box, a.t.P, a.t.D, v);
        if (v.slot >= 0) {
            z = (float)v.best; face = v.face;
            if (a.bary) rt_bary(r, a.t.tri + 9 * (long long)v.slot, &b1, &b2);
        }
    }
    if (a.depth) a.depth[px] = z;
    if (a.face) a.face[px] = face;
    if (a.bary) { a.bary[2 * px] = b1; a.bary[2 * px + 1] = b2; }
}

// any[p] |= 1 iff pose p projects some point into the image (k_cull_seen's f32 test, cull_mesh.py:49-71 = eval_recon.py:70-96);
// any[] is zeroed by the entry before the launch
struct SightArgs {
    const double* v; int nv; const float* w2c; int np;
    float fx, fy, cx, cy, W, H;
    int* any;
};

__global__ __launch_bounds__(ADFP_NN_THREADS) void k_views_in_sight(SightArgs a) {
    __shared__ float s_pose[ADFP_CULL_CHUNK * 12];
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    const bool on = i < a.nv;
    const float x = on ? (float)a.v[3 * (long long)i] : 0.f;
    const float y = on ? (float)a.v[3 * (long long)i + 1] : 0.f;
    const float z = on ? (float)a.v[3 * (long long)i + 2] : 0.f;
    for (int p0 = 0; p0 < a.np; p0 += ADFP_CULL_CHUNK) {
        const int m = a.np - p0 < ADFP_CULL_CHUNK ? a.np - p0 : ADFP_CULL_CHUNK;
        __syncthreads();
        for (int e = threadIdx.x; e < 12 * m; e += ADFP_NN_THREADS) s_pose[e] = a.w2c[12 * (long long)p0 + e];
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const bool s = on && cull_sees(s_pose + 12 * k, x, y, z, a.fx, a.fy, a.cx, a.cy, a.W, a.H);
            if (__ballot(s) && (threadIdx.x & 63) == 0) atomicOr(a.any + p0 + k, 1);
        }
    }
}

// ---- occlusion-aware visibility: points x poses ----
struct VisibleArgs {
    TriDev t;
    const double* pts; int n;                                 // [n][3] f64
    const float* w2c; const double* c2w; int np;              // [np][12] f32 (k_cull_seen's rows) / [np][12] f64 (k_render_depth's rows)
    float fx, fy, cx, cy, W, H;
    double near, eps;
    unsigned char* seen;                                      // [n]
};

// Does pose m (12 f64, [R | o] row-major, here in LDS) see the point p unoccluded?  p goes to camera space as a mesh vertex does;
// z_p = cam z; not seen when m holds a non-finite entry, when z_p <= 0 or is not finite, or when d = (cam x / z_p, cam y / z_p)
// is not finite.  Else occluded iff the ray through d has a hit (RtAny) at near <= z < z_p - eps.
ADFP_DEV bool vis_unoccluded(const VisibleArgs& a, const double* m, double px, double py, double pz) {
    bool fin = true;
#pragma unroll
    for (int e = 0; e < 12; ++e) fin = fin && isfinite(m[e]);
    if (!fin) return false;
    const double e0 = px - m[3], e1 = py - m[7], e2 = pz - m[11];
    double pc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pc[c] = (m[c] * e0 + m[4 + c] * e1) + m[8 + c] * e2;
    const double zp = pc[2];
    if (!(zp > 0.0) || !isfinite(zp)) return false;
    const double dx = pc[0] / zp, dy = pc[1] / zp;
    if (!isfinite(dx) || !isfinite(dy)) return false;
    RtRay r;
    rt_ray(r, m, dx, dy, a.t.box + 6);
    RtAny v = {r, a.t, a.near, zp - a.eps};
    return !bvh_walk<false>(a.t.box, a.t.P, a.t.D, v);
}

// seen[i] = 1 iff some pose k has point i in its frustum (cull_sees on the f32 rounding of the point: k_cull_seen's test) and sees
// it unoccluded (vis_unoccluded).  One lane per point; the poses pass through LDS ADFP_CULL_CHUNK at a time, the f64 rows beside
// the f32 ones; a lane whose point is seen skips the remaining poses but takes part in every barrier.  Letting each lane run ahead
// to its next in-frustum pose, so that a wave's walks run side by side, was measured and dropped: 149.5 ms against 130.3 ms
// for 1 M points x 2 000 poses -- the launch lasts as long as the few points that no pose sees.
__global__ __launch_bounds__(ADFP_NN_THREADS) void k_points_visible(VisibleArgs a) {
    __shared__ float s_w2c[ADFP_CULL_CHUNK * 12];
    __shared__ double s_c2w[ADFP_CULL_CHUNK * 12];
    const int i = blockIdx.x * ADFP_NN_THREADS + threadIdx.x;
    const bool on = i < a.n;
    const double px = on ? a.pts[3 * (long long)i] : 0.0;
    const double py = on ? a.pts[3 * (long long)i + 1] : 0.0;
    const double pz = on ? a.pts[3 * (long long)i + 2] : 0.0;
    const float x = (float)px, y = (float)py, z = (float)pz;
    bool seen = false;
    for (int p0 = 0; p0 < a.np; p0 += ADFP_CULL_CHUNK) {
        const int m = a.np - p0 < ADFP_CULL_CHUNK ? a.np - p0 : ADFP_CULL_CHUNK;
        __syncthreads();
        for (int e = threadIdx.x; e < 12 * m; e += ADFP_NN_THREADS) {
            s_w2c[e] = a.w2c[12 * (long long)p0 + e];
            s_c2w[e] = a.c2w[12 * (long long)p0 + e];
        }
        __syncthreads();
        if (!on || seen) continue;
        for (int k = 0; k < m; ++k) {
            if (!cull_sees(s_w2c + 12 * k, x, y, z, a.fx, a.fy, a.cx, a.cy, a.W, a.H)) continue;
            if (vis_unoccluded(a, s_c2w + 12 * k, px, py, pz)) { seen = true; break; }
        }
    }
    if (on) a.seen[i] = seen ? 1 : 0;
}

// per view p (grid y): partial b = sum of (double)|a - b| (the f32 difference) over pixels b * 256 + t + k * (nblk * 256)
struct L1Args { const float* a; const float* b; long long n; int nblk; double* part; double* out; };

__global__ __launch_bounds__(ADFP_RED_THREADS) void k_l1_partial(L1Args a) {
    __shared__ double s_wave[ADFP_RED_THREADS / 64];
    const long long base = (long long)blockIdx.y * a.n;
    double sum = 0.0;
    for (long long i = (long long)blockIdx.x * ADFP_RED_THREADS + threadIdx.x; i < a.n; i += (long long)a.nblk * ADFP_RED_THREADS)
        sum += (double)fabsf(a.a[base + i] - a.b[base + i]);
    sum = red_block_sum(sum, s_wave);
    if (threadIdx.x == 0) a.part[(long long)blockIdx.y * a.nblk + blockIdx.x] = sum;
}

// ---- host side: the launchers ----
static bool tri_leaf_ok(int leaf) { return leaf == 4 || leaf == 8 || leaf == 16; }
// a triangle is nine doubles (adfp_recon.h: bvh_layout)
static BvhLayout tri_layout(Arena& A, long long nf, int leaf) { return bvh_layout(A, nf, 9, leaf); }

static TriDev make_tri(const void* bvh, long long n_faces, int leaf, const int** orig = nullptr) {
    Arena A(bvh);
    const BvhLayout L = tri_layout(A, n_faces, leaf);
    TriDev d; d.tri = L.sorted; d.box = L.box;
    d.nf = (int)n_faces; d.leaf = leaf; d.P = L.P; d.D = L.D;
    if (orig) *orig = L.orig;
    return d;
}

size_t adfp_tri_bvh_bytes(long long n_faces, int leaf) {
    return n_faces <= 0 || n_faces > RECON_MAX_N || !tri_leaf_ok(leaf) ? 0 : layout_bytes(tri_layout, n_faces, leaf);
}
// the face centroids [F][3], then the Morton workspace
size_t adfp_tri_bvh_build_workspace_bytes(long long n_faces) {
    if (n_faces <= 0 || n_faces > RECON_MAX_N) return 0;
    Arena A;
    A.take<double>(3 * (size_t)n_faces);
    morton_layout(A, n_faces);
    return A.bytes();
}

int adfp_tri_bvh_build(const double* verts, long long n_verts, const int* faces, long long n_faces, int leaf, void* bvh, size_t bvh_bytes,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (n_verts < 0 || n_faces < 0 || !tri_leaf_ok(leaf)) return ADFP_E_ARG;
    if (n_faces == 0) return 0;
    if (!faces || !bvh || !workspace || (n_verts > 0 && !verts)) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_faces > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (bvh_bytes < adfp_tri_bvh_bytes(n_faces, leaf) || workspace_bytes < adfp_tri_bvh_build_workspace_bytes(n_faces)) return ADFP_E_WORKSPACE;
    Arena I(bvh), A(workspace);
    const BvhLayout L = tri_layout(I, n_faces, leaf);
    const int nf = (int)n_faces, nv = (int)n_verts;
    hipStream_t st = (hipStream_t)stream;
    double* cen = A.take<double>(3 * (size_t)nf);
    const unsigned nb = nn_blocks(nf);
    hipLaunchKernelGGL(k_tri_centroids, dim3(nb), dim3(ADFP_NN_THREADS), 0, st, verts, nv, faces, nf, cen);
    ADFP_CHECK_LAUNCH();
    const int* perm;
    int rc = morton_order(cen, nf, A, &perm, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_tri_gather, dim3(nb), dim3(ADFP_NN_THREADS), 0, st, verts, nv, faces, nf, perm, L.sorted, L.orig);
    ADFP_CHECK_LAUNCH();
    return nn_boxes(L.sorted, 3ll * nf, 3 * leaf, L.P, L.box, st);      // a triangle is three consecutive points
}

#define RT_MAX_SIDE 32768
#define RT_VIEWS_PER_LAUNCH 32768                    // grid y
static int render_depth_launch(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near,
                               double far, long long n_views, int H, int W, double fx, double fy, double cx, double cy, int cull,
                               float* depth, void* stream) {
    if (n_faces < 0 || n_views < 0 || !tri_leaf_ok(leaf) || H <= 0 || W <= 0) return ADFP_E_ARG;
    if (cull != ADFP_CULL_NONE && cull != ADFP_CULL_BACK && cull != ADFP_CULL_FRONT) return ADFP_E_ARG;
    if (!(far > 0.0) || !(fx != 0.0) || !(fy != 0.0) || !isfinite(far) || !isfinite(fx) || !isfinite(fy) ||
        !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if (n_views == 0) return 0;
    if (!depth || (n_faces > 0 && (!bvh || !c2w || !near))) return ADFP_E_ARG;
    if (n_faces > RECON_MAX_N || H > RT_MAX_SIDE || W > RT_MAX_SIDE || n_views > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (n_faces > 0 && bvh_bytes < adfp_tri_bvh_bytes(n_faces, leaf)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n_faces == 0) {
        hipError_t e = hipMemsetAsync(depth, 0, (size_t)n_views * H * W * sizeof(float), st);
        return e == hipSuccess ? 0 : (int)e;
    }
    RenderArgs a;
    a.t = make_tri(bvh, n_faces, leaf);
    a.c2w = c2w; a.near = near; a.far = far;
    a.H = H; a.W = W; a.nbx = (int)ceil_div(W, 16); a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.depth = depth;
    const unsigned nblk = (unsigned)a.nbx * (unsigned)ceil_div(H, 16);
    void (*const kern)(RenderArgs) = cull == ADFP_CULL_BACK ? k_render_depth<ADFP_CULL_BACK>
                                     : cull == ADFP_CULL_FRONT ? k_render_depth<ADFP_CULL_FRONT> : k_render_depth<ADFP_CULL_NONE>;
    for (long long v0 = 0; v0 < n_views; v0 += RT_VIEWS_PER_LAUNCH) {
        const long long nv = n_views - v0 < RT_VIEWS_PER_LAUNCH ? n_views - v0 : RT_VIEWS_PER_LAUNCH;
        a.view0 = (int)v0;
        hipLaunchKernelGGL(kern, dim3(nblk, (unsigned)nv), dim3(ADFP_RT_THREADS), 0, st, a);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

int adfp_render_depth(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near, double far,
                      long long n_views, int H, int W, double fx, double fy, double cx, double cy, float* depth, void* stream) {
    return render_depth_launch(bvh, bvh_bytes, n_faces, leaf, c2w, near, far, n_views, H, W, fx, fy, cx, cy, ADFP_CULL_NONE, depth,
                               stream);
}

int adfp_render_depth_cull(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near,
                           double far, long long n_views, int H, int W, double fx, double fy, double cx, double cy, int cull,
                           float* depth, void* stream) {
    return render_depth_launch(bvh, bvh_bytes, n_faces, leaf, c2w, near, far, n_views, H, W, fx, fy, cx, cy, cull, depth, stream);
}

int adfp_render_hits(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near, double far,
                     long long n_views, int H, int W, double fx, double fy, double cx, double cy, int cull, float* depth, int* face,
                     float* bary, void* stream) {
    if (n_faces < 0 || n_views < 0 || !tri_leaf_ok(leaf) || H <= 0 || W <= 0) return ADFP_E_ARG;
    if (cull != ADFP_CULL_NONE && cull != ADFP_CULL_BACK && cull != ADFP_CULL_FRONT) return ADFP_E_ARG;
    if (!(far > 0.0) || !(fx != 0.0) || !(fy != 0.0) || !isfinite(far) || !isfinite(fx) || !isfinite(fy) ||
        !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if (n_views == 0) return 0;
    if ((!depth && !face && !bary) || (n_faces > 0 && (!bvh || !c2w || !near))) return ADFP_E_ARG;
    if (n_faces > RECON_MAX_N || H > RT_MAX_SIDE || W > RT_MAX_SIDE || n_views > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (n_faces > 0 && bvh_bytes < adfp_tri_bvh_bytes(n_faces, leaf)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n_faces == 0) {                                  // no hit anywhere: 0 / -1 / (0, 0)
        const size_t npix = (size_t)n_views * H * W;
        hipError_t e = hipSuccess;
        if (depth) e = hipMemsetAsync(depth, 0, npix * sizeof(float), st);
        if (e == hipSuccess && face) e = hipMemsetAsync(face, 0xff, npix * sizeof(int), st);
        if (e == hipSuccess && bary) e = hipMemsetAsync(bary, 0, npix * 2 * sizeof(float), st);
        return e == hipSuccess ? 0 : (int)e;
    }
    HitArgs a;
    a.t = make_tri(bvh, n_faces, leaf, &a.orig);
    a.c2w = c2w; a.near = near; a.far = far;
    a.H = H; a.W = W; a.nbx = (int)ceil_div(W, 16); a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.depth = depth; a.face = face; a.bary = bary;
    const unsigned nblk = (unsigned)a.nbx * (unsigned)ceil_div(H, 16);
    void (*const kern)(HitArgs) = cull == ADFP_CULL_BACK ? k_render_hits<ADFP_CULL_BACK>
                                  : cull == ADFP_CULL_FRONT ? k_render_hits<ADFP_CULL_FRONT> : k_render_hits<ADFP_CULL_NONE>;
    for (long long v0 = 0; v0 < n_views; v0 += RT_VIEWS_PER_LAUNCH) {
        const long long nv = n_views - v0 < RT_VIEWS_PER_LAUNCH ? n_views - v0 : RT_VIEWS_PER_LAUNCH;
        a.view0 = (int)v0;
        hipLaunchKernelGGL(kern, dim3(nblk, (unsigned)nv), dim3(ADFP_RT_THREADS), 0, st, a);
        ADFP_CHECK_LAUNCH();
    }
    return 0;
}

int adfp_views_in_sight(const double* points, long long n_points, const float* w2c, long long n_poses, float fx, float fy, float cx, float cy,
                        int W, int H, int* any, void* stream) {
    if (n_points < 0 || n_poses < 0) return ADFP_E_ARG;
    if (n_poses == 0) return 0;
    if (!w2c || !any || (n_points > 0 && !points)) return ADFP_E_ARG;
    if (n_points > RECON_MAX_N || n_poses > RECON_MAX_N / 12) return ADFP_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(any, 0, (size_t)n_poses * sizeof(int), st);
    if (e != hipSuccess) return (int)e;
    if (n_points == 0) return 0;
    SightArgs a;
    a.v = points; a.nv = (int)n_points; a.w2c = w2c; a.np = (int)n_poses;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.W = (float)W; a.H = (float)H; a.any = any;
    hipLaunchKernelGGL(k_views_in_sight, dim3(nn_blocks(n_points)), dim3(ADFP_NN_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_points_visible(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* points, long long n_points,
                        const float* w2c, const double* c2w, long long n_poses, float fx, float fy, float cx, float cy, int W, int H,
                        double near, double eps, unsigned char* seen, void* stream) {
    if (n_faces < 0 || n_points < 0 || n_poses < 0 || !tri_leaf_ok(leaf)) return ADFP_E_ARG;
    if (!(eps >= 0.0) || !isfinite(eps) || !(near >= 0.0) || !isfinite(near) || !(fx != 0.f) || !(fy != 0.f)) return ADFP_E_ARG;
    if (n_points == 0) return 0;
    if (!points || !seen || (n_poses > 0 && !w2c) || (n_poses > 0 && n_faces > 0 && (!bvh || !c2w))) return ADFP_E_ARG;
    if (n_faces > RECON_MAX_N || n_points > RECON_MAX_N || n_poses > RECON_MAX_N / 12) return ADFP_E_UNSUPPORTED;
    if (n_faces > 0 && bvh_bytes < adfp_tri_bvh_bytes(n_faces, leaf)) return ADFP_E_WORKSPACE;
    if (n_faces == 0 || n_poses == 0)                     // nothing occludes (or nothing looks): the frustum-only kernel itself
        return adfp_cull_vertices(points, n_points, w2c, n_poses, fx, fy, cx, cy, W, H, seen, stream);
    VisibleArgs a;
    a.t = make_tri(bvh, n_faces, leaf);
    a.pts = points; a.n = (int)n_points; a.w2c = w2c; a.c2w = c2w; a.np = (int)n_poses;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.W = (float)W; a.H = (float)H;
    a.near = near; a.eps = eps; a.seen = seen;
    hipLaunchKernelGGL(k_points_visible, dim3(nn_blocks(n_points)), dim3(ADFP_NN_THREADS), 0,
                       (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

size_t adfp_depth_l1_workspace_bytes(long long n_views, long long n_pixels) {
    if (n_views < 0 || n_pixels < 0 || n_pixels > RECON_MAX_N || n_views > RECON_MAX_N) return 0;
    return (size_t)n_views * red_blocks(n_pixels) * 8;
}

int adfp_depth_l1_sums(const float* a, const float* b, long long n_views, long long n_pixels, void* workspace, size_t workspace_bytes,
                       double* out, void* stream) {
    if (n_views < 0 || n_pixels < 0) return ADFP_E_ARG;
    if (n_views == 0) return 0;
    if (!out || !workspace || (n_pixels > 0 && (!a || !b))) return ADFP_E_ARG;
    if (n_pixels > RECON_MAX_N || n_views > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    if (workspace_bytes < adfp_depth_l1_workspace_bytes(n_views, n_pixels)) return ADFP_E_WORKSPACE;
    L1Args r;
    r.a = a; r.b = b; r.n = n_pixels; r.nblk = red_blocks(n_pixels); r.part = (double*)workspace; r.out = out;
    hipStream_t st = (hipStream_t)stream;
    for (long long v0 = 0; v0 < n_views; v0 += RT_VIEWS_PER_LAUNCH) {
        const long long nv = n_views - v0 < RT_VIEWS_PER_LAUNCH ? n_views - v0 : RT_VIEWS_PER_LAUNCH;
        L1Args c = r;
        c.a = a + v0 * n_pixels; c.b = b + v0 * n_pixels; c.part = r.part + v0 * r.nblk;
        hipLaunchKernelGGL(k_l1_partial, dim3((unsigned)r.nblk, (unsigned)nv), dim3(ADFP_RED_THREADS), 0, st, c);
        ADFP_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_red_final<1>, dim3((unsigned)n_views), dim3(ADFP_RED_THREADS), 0, st, r.part, r.nblk, out);
    ADFP_CHECK_LAUNCH();
    return 0;
}
