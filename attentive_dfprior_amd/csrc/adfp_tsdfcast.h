// adfp_tsdfcast.h -- raycast of the TSDF prior: the depth image of the prior's surface from any pose (KinectFusion's raycast),
// which is the `gt_depth` the depth-guided sampler wants for a view that has no sensor image (Renderer.render_novel).  The
// contract is stated in include/adfp.h ("TSDF raycast") and, in torch on the CPU, in tests/tsdfcast_ref.py.
//
//   k_tsdf_bricks   the empty-space bitmap: one bit per brick of 8^3 voxels, set unless EVERY voxel of the brick, padded by one
//                   voxel on every side and clipped to the volume, is >= 2^-100 (see (b) for why not "> 0").  One wave per
//                   32-bit word, no atomics, the same bits on every call.
//   k_tsdf_raycast  one lane per pixel, one wave per 8 x 8 pixel tile, four waves per 16 x 16 workgroup tile: neighbouring rays
//                   stay within a few voxels of each other along the whole march, so the 64 lookups of a wave instruction land
//                   in a handful of sectors.  64 pixels of one row would fan out eight times as wide in one direction.
//
// The march.  Sample k sits at t_k = tn + k dt, computed from k (a double: exact far beyond any sample count) and never
// accumulated, so a sample's position does not depend on which samples were looked at before it.  The first sample with
// f <= 0 ends the ray: depth = t_{k-1} + dt f_{k-1} / (f_{k-1} - f_k), or 0 when k = 0.  The result is a function of (k, f_{k-1},
// f_k) alone, which is what lets the skip below leave every bit of the image alone.
//
// The skip.  A sample whose cell (the f32 cell index tri_axis gives the lookup) lies in a brick with a clear bit is not looked
// up; the march then jumps k over the samples that are certain to be in the same case.  Two claims carry this.
//
//  (a) The one-voxel pad covers the f32 cell index against the f64 brick box.  The jump is computed in f64 on the line
//      u(t) = U0 + U1 t, the sample's voxel coordinate per axis; the lookup takes its cell from f32 arithmetic on the rounded
//      normalised position, c = ((pn + 1) / 2) (size - 1).  pn is one rounding of a value in [-1, 1] (2^-24), pn + 1 another
//      (2^-24), the product with size - 1 a third: |c - u| < 2^-22 size, which is 2^-7 voxel at the largest volume the entries
//      accept (32768 per side) and 2^-12 at 1024.  The jump only passes samples whose u lies in the SHRUNK box
//      [8 B - 1 + m, 8 B + 8 - m] per axis with m = 1/16 voxel, eight times that error at the largest size.  Such a sample has
//      c in (8 B - 1, 8 B + 8), so its cell index i0 = floor(c) is in [8 B - 1, 8 B + 7] and its upper corner i0 + 1 in
//      [8 B, 8 B + 8]: all eight corners lie in brick B padded by one voxel, which is the set of voxels the bit vouches for.
//      (Clamping c to [0, size - 1] only moves it inside the clipped pad.)  The sample that triggers the jump is vouched for by
//      its OWN f32 cell, whatever its u; when its u lies outside the shrunk box (within m of the upper face) the march advances
//      by one sample and asks again.  The exit parameter is turned into a sample index as floor((t_out - tn) / dt) - 1: the
//      quotient is off by a few 2^-53 of itself, the - 1 is a whole sample.
//  (b) The blend of positive values is positive.  The weights are w0 = (f + 1) - c and w1 = c - f with f = floor(c) <= c <= f + 1,
//      both >= 0 (a clipped upper corner gets exactly 0), so every product (wx wy) wz is >= 0 and every term of the fmaf chain
//      is >= 0: the sum cannot fall below its largest term.  On each axis the larger weight is >= 1/2 up to rounding, so one of
//      the eight products is >= 1/8 up to rounding, and its corner value v gives a term >= v / 8 up to rounding.  With v >= 2^-100
//      that term is a normal number far above 0 whatever the denormal mode, which is why the bit is cleared on ">= 2^-100" and
//      not on "> 0": a value in (0, 2^-100) could underflow in the product.  No TSDF holds such values (they are multiples of
//      sdf / trunc); the stricter rule only ever sets more bits, and a set bit changes no pixel.  A NaN voxel sets the bit too.
//      So a skipped sample has f > 0 and could not have ended the ray.
//
// When a ray is ended by sample k > 0 and sample k - 1 was skipped, that one sample is looked up then (at most once per ray):
// t_{k-1} is computed from k - 1, so f_{k-1} has the bits the plain march carries over.  With the skip on, the image is byte for
// byte the image with ADFP_CAST_NO_SKIP.
//
// The bitmap stays in global memory (L2), not LDS: it is 49 KB for room0 and 93 KB for office0, a workgroup's 256 rays touch a few
// hundred of its words, and staging all of it would cost each of the 1 200 workgroups of a 640 x 480 frame a 49-93 KB copy and
// cap a CU at one or two workgroups (160 KB of LDS).  Read on demand it is a 4-byte load that neighbouring lanes share.
//
// A ray that comes through unobserved space (f = -1 voxels) behind a surface reports a crossing at the truncation boundary: the
// rule is on interpolated values and has no band test on f_{k-1}, as KinectFusion's has none.
#pragma once
#include "adfp_device.h"

#define ADFP_CAST_THREADS 256
#define ADFP_CAST_TILE 16              // workgroup tile; a wave takes an 8 x 8 quarter
#define ADFP_BRICK 8
#define ADFP_BRICK_MARGIN 0.0625       // m of (a), in voxels
#define ADFP_BRICK_MIN 0x1p-100f       // (b)
#define ADFP_CAST_MAX_DIM 32768
#define ADFP_CAST_MAX_SAMPLES 16777216   // per ray: a step below diagonal / 2^24 is refused

struct CastArgs {
    TsdfDev t; NormDev nt;
    double lo[3], hi[3];               // tsdf_bnds per axis x, y, z
    double s1[3];                      // (double)(size - 1) per axis x, y, z
    const unsigned* bricks; int nby, nbz;
    const float* c2w; int H, W; float fx, fy, cx, cy;
    double near, far, step;
    float* depth; unsigned long long* lookups;
};

ADFP_DEV float cast_lookup(const TsdfDev& t, const float pn[3]) {
    if (t.cb) {                        // kernel-uniform
        TriBlock tb;
        trilerp_block_prepare(t, pn, tb);
        const f32x4 lo = tb.a[0], hi = tb.a[1];
        return trilerp_block_finish(tb, lo, hi);
    }
    return trilerp_scalar(t, pn);
}

// the sample at parameter t: position o + d t in f64, normalised in f64, then .float()
ADFP_DEV void cast_point(const CastArgs& a, const double o[3], const double d[3], double t, float pn[3]) {
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = __dadd_rn(o[k], __dmul_rn(d[k], t));
    normalize3(a.nt, p, pn);
}

// grid (tiles_x, tiles_y, V)
template <bool SKIP, bool COUNT>
__global__ __launch_bounds__(ADFP_CAST_THREADS) void k_tsdf_raycast(CastArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int px = blockIdx.x * ADFP_CAST_TILE + (wave & 1) * 8 + (lane & 7);
    const int py = blockIdx.y * ADFP_CAST_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (px >= a.W || py >= a.H) return;
    const int view = blockIdx.z;
    float rof[3], rdf[3];
    ray_from_uv((float)px, (float)py, a.fx, a.fy, a.cx, a.cy, a.c2w + 16 * view, rof, rdf);
    double o[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[k] = (double)rof[k]; d[k] = (double)rdf[k]; }
    // slab entry and exit against tsdf_bnds; an axis the ray does not move along only says in or out
    double tn = -__builtin_inf(), tf = __builtin_inf();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (d[k] != 0.0) {
            const double t1 = (a.lo[k] - o[k]) / d[k], t2 = (a.hi[k] - o[k]) / d[k];
            const double ta = t1 < t2 ? t1 : t2, tb = t1 < t2 ? t2 : t1;
            tn = ta > tn ? ta : tn;
            tf = tb < tf ? tb : tf;
        } else if (!(o[k] >= a.lo[k] && o[k] <= a.hi[k])) {
            tn = __builtin_inf(); tf = -__builtin_inf();
        }
    }
    tn = a.near > tn ? a.near : tn;
    tn = 0.0 > tn ? 0.0 : tn;
    if (a.far > 0.0) tf = a.far < tf ? a.far : tf;
    float depth = 0.f;
    unsigned looked = 0;
    if (!(tf < tn)) {
        const double dt = a.step / sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        // the line u(t) = U0 + U1 t in voxel coordinates and what turns a brick face into a sample index (skip only)
        double U0[3], U1[3], iU1[3], idt = 0.0;
        if (SKIP) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                U0[k] = ((o[k] - a.lo[k]) * a.nt.inv[k]) * a.s1[k];
                U1[k] = (d[k] * a.nt.inv[k]) * a.s1[k];
                iU1[k] = 1.0 / U1[k];
            }
            idt = 1.0 / dt;
        }
        double k = 0.0, kprev = -1.0;
        float fprev = 0.f;
        for (;;) {
            const double t = tn + k * dt;
            if (!(t <= tf)) break;
            float pn[3];
            cast_point(a, o, d, t, pn);
            if (SKIP) {
                int c0[3], c1; float w0, w1;
                tri_axis(pn[0], a.t.X, c0[0], c1, w0, w1);
                tri_axis(pn[1], a.t.Y, c0[1], c1, w0, w1);
                tri_axis(pn[2], a.t.Z, c0[2], c1, w0, w1);
                const int b[3] = {c0[0] >> 3, c0[1] >> 3, c0[2] >> 3};
                const unsigned bit = ((unsigned)b[0] * (unsigned)a.nby + (unsigned)b[1]) * (unsigned)a.nbz + (unsigned)b[2];
                if (!((a.bricks[bit >> 5] >> (bit & 31u)) & 1u)) {
                    bool in = true;
                    double tout = __builtin_inf();
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const double bl = (double)(ADFP_BRICK * b[q] - 1) + ADFP_BRICK_MARGIN;
                        const double bh = (double)(ADFP_BRICK * b[q] + ADFP_BRICK) - ADFP_BRICK_MARGIN;
                        const double u = U0[q] + U1[q] * t;
                        in = in && u >= bl && u <= bh;
                        if (U1[q] != 0.0) {
                            const double te = ((U1[q] > 0.0 ? bh : bl) - U0[q]) * iU1[q];
                            tout = te < tout ? te : tout;
                        }
                    }
                    const double j = in ? floor((tout - tn) * idt) - 1.0 : k;      // the last sample known to be passable
                    k = (j > k ? j : k) + 1.0;
                    continue;
                }
            }
            const float f = cast_lookup(a.t, pn);
            ++looked;
            if (f <= 0.f) {
                if (k > 0.0) {
                    const double tp = tn + (k - 1.0) * dt;
                    float fp = fprev;
                    if (SKIP && kprev != k - 1.0) {        // sample k - 1 was skipped: the one lookup that gives f_{k-1}
                        float pp[3];
                        cast_point(a, o, d, tp, pp);
                        fp = cast_lookup(a.t, pp);
                        ++looked;
                    }
                    depth = (float)(tp + (dt * (double)fp) / ((double)fp - (double)f));
                }
                break;
            }
            fprev = f; kprev = k;
            k += 1.0;
        }
    }
    a.depth[((long long)view * a.H + py) * a.W + px] = depth;
    if (COUNT) atomicAdd(a.lookups, (unsigned long long)looked);
}

// one wave per word of the bitmap: bit b of word w is brick 32 w + b, bricks numbered (bx nby + by) nbz + bz
__global__ __launch_bounds__(64) void k_tsdf_bricks(TsdfDev t, int nby, int nbz, unsigned n_bricks, unsigned* __restrict__ out) {
    const unsigned w = blockIdx.x;
    unsigned word = 0u;
    for (int b = 0; b < 32; ++b) {
        const unsigned idx = w * 32u + (unsigned)b;
        if (idx >= n_bricks) break;                                            // wave-uniform
        const int bz = (int)(idx % (unsigned)nbz), by = (int)((idx / (unsigned)nbz) % (unsigned)nby), bx = (int)(idx / ((unsigned)nbz * (unsigned)nby));
        const int x0 = max(ADFP_BRICK * bx - 1, 0), x1 = min(ADFP_BRICK * bx + ADFP_BRICK, t.X - 1);
        const int y0 = max(ADFP_BRICK * by - 1, 0), y1 = min(ADFP_BRICK * by + ADFP_BRICK, t.Y - 1);
        const int z0 = max(ADFP_BRICK * bz - 1, 0), z1 = min(ADFP_BRICK * bz + ADFP_BRICK, t.Z - 1);
        const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
        bool any = false;
        for (int i = threadIdx.x; i < nx * ny * nz; i += 64) {                 // z fastest, like the reference's volume
            const int z = z0 + i % nz, y = y0 + (i / nz) % ny, x = x0 + i / (nz * ny);
            const float v = t.data[z * t.sZ + y * t.sY + x * t.sX];
            any = any || !(v >= ADFP_BRICK_MIN);
        }
        if (__any(any)) word |= 1u << b;
    }
    if (threadIdx.x == 0) out[w] = word;
}

// the number of bricks of a volume and per axis (x, y, z); 0 for a bad size
static long long cast_bricks(int Z, int Y, int X, int nb[3]) {
    if (Z < 1 || Y < 1 || X < 1 || Z > ADFP_CAST_MAX_DIM || Y > ADFP_CAST_MAX_DIM || X > ADFP_CAST_MAX_DIM) return 0;
    nb[0] = (X + ADFP_BRICK - 1) / ADFP_BRICK; nb[1] = (Y + ADFP_BRICK - 1) / ADFP_BRICK; nb[2] = (Z + ADFP_BRICK - 1) / ADFP_BRICK;
    const long long n = (long long)nb[0] * nb[1] * nb[2];
    return n < (1ll << 31) ? n : 0;
}

extern "C" size_t adfp_tsdf_bricks_bytes(int Z, int Y, int X) {
    int nb[3];
    const long long n = cast_bricks(Z, Y, X, nb);
    return (size_t)((n + 31) / 32) * 4;
}

extern "C" int adfp_tsdf_bricks_build(const adfp_tsdf* tsdf, void* bricks, size_t bricks_bytes, void* stream) {
    if (!tsdf || !tsdf->data || !bricks || tsdf->X < 1 || tsdf->Y < 1 || tsdf->Z < 1) return ADFP_E_ARG;
    int nb[3];
    const long long n = cast_bricks(tsdf->Z, tsdf->Y, tsdf->X, nb);
    if (n == 0) return ADFP_E_UNSUPPORTED;
    if ((((unsigned long long)bricks) & 3ull) || bricks_bytes < adfp_tsdf_bricks_bytes(tsdf->Z, tsdf->Y, tsdf->X)) return ADFP_E_ARG;
    adfp_tsdf src = *tsdf; src.corner_blocks = nullptr;
    hipLaunchKernelGGL(k_tsdf_bricks, dim3((unsigned)((n + 31) / 32)), dim3(64), 0, (hipStream_t)stream, make_tsdf(src), nb[1], nb[2], (unsigned)n,
                       (unsigned*)bricks);
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_tsdf_raycast(const adfp_tsdf* tsdf, const double tsdf_bnds[3][2], const void* bricks, size_t bricks_bytes, const float* c2w,
                                 int V, int H, int W, float fx, float fy, float cx, float cy, double near, double far, double step, int options,
                                 float* depth, unsigned long long* lookups, void* stream) {
    if (!tsdf || !tsdf->data || !tsdf_bnds || !c2w || !depth || tsdf->X < 1 || tsdf->Y < 1 || tsdf->Z < 1) return ADFP_E_ARG;
    if (V < 1 || H < 1 || W < 1 || !(step > 0.0) || !(near == near) || !(far == far) || (options & ~ADFP_CAST_NO_SKIP)) return ADFP_E_ARG;
    for (int k = 0; k < 3; ++k)
        if (!(tsdf_bnds[k][1] > tsdf_bnds[k][0])) return ADFP_E_ARG;
    const bool skip = !(options & ADFP_CAST_NO_SKIP);
    int nb[3];
    const long long n = cast_bricks(tsdf->Z, tsdf->Y, tsdf->X, nb);
    if (n == 0 || V > 65535 || H > ADFP_CAST_MAX_DIM || W > ADFP_CAST_MAX_DIM) return ADFP_E_UNSUPPORTED;
    double diag = 0.0;                             // no ray takes more samples than the volume's diagonal holds steps
    for (int k = 0; k < 3; ++k) diag += (tsdf_bnds[k][1] - tsdf_bnds[k][0]) * (tsdf_bnds[k][1] - tsdf_bnds[k][0]);
    if (!(sqrt(diag) / step <= (double)ADFP_CAST_MAX_SAMPLES)) return ADFP_E_UNSUPPORTED;
    if (skip && (!bricks || (((unsigned long long)bricks) & 3ull) || bricks_bytes < adfp_tsdf_bricks_bytes(tsdf->Z, tsdf->Y, tsdf->X))) return ADFP_E_ARG;
    CastArgs a;
    a.t = make_tsdf(*tsdf); a.nt = make_norm(tsdf_bnds);
    const int size[3] = {tsdf->X, tsdf->Y, tsdf->Z};
    for (int k = 0; k < 3; ++k) { a.lo[k] = tsdf_bnds[k][0]; a.hi[k] = tsdf_bnds[k][1]; a.s1[k] = (double)(size[k] - 1); }
    a.bricks = (const unsigned*)bricks; a.nby = nb[1]; a.nbz = nb[2];
    a.c2w = c2w; a.H = H; a.W = W; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.near = near; a.far = far; a.step = step;
    a.depth = depth; a.lookups = lookups;
    const dim3 grid((unsigned)((W + ADFP_CAST_TILE - 1) / ADFP_CAST_TILE), (unsigned)((H + ADFP_CAST_TILE - 1) / ADFP_CAST_TILE), (unsigned)V);
    const dim3 block(ADFP_CAST_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (skip) {
        if (lookups) hipLaunchKernelGGL((k_tsdf_raycast<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_tsdf_raycast<true, false>), grid, block, 0, st, a);
    } else {
        if (lookups) hipLaunchKernelGGL((k_tsdf_raycast<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_tsdf_raycast<false, false>), grid, block, 0, st, a);
    }
    ADFP_CHECK_LAUNCH();
    return 0;
}
