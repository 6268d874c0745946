// adfp_meshshade.h -- what a mesh view shows beyond depth, from the hit render's face and barycentric images (adfp_raycast.h's
// k_render_hits): area-weighted vertex normals, and a per-pixel shading pass (camera-facing normals, vertex colours, a headlight).
// Contracts: include/adfp.h, "mesh views"; tests/hits_ref.py restates them in numpy.
//
//   vertex normals   n_f = (v1 - v0) x (v2 - v0) per face (f64); the 3 F corners keyed by their vertex and ordered by one stable
//                    radix sort (adfp_sort.h), so a vertex's corners lie together in ascending face index; each vertex finds the
//                    start of its run by bisection and sums it in that order: no float atomics, the same bits every run
//   shading          one lane per pixel: weights from the f32 barycentrics, the geometric or the interpolated normal to camera
//                    space, normalised and turned toward the camera, the intensity of a light at the camera, bytes
#pragma once
#include "adfp_device.h"

#define ADFP_SHADE_THREADS 256

ADFP_DEV bool shade_face_ok(const int* f, long long i, int nv, int* id) {
    id[0] = f[3 * i]; id[1] = f[3 * i + 1]; id[2] = f[3 * i + 2];
    return (unsigned)id[0] < (unsigned)nv && (unsigned)id[1] < (unsigned)nv && (unsigned)id[2] < (unsigned)nv;
}

// g = (v1 - v0) x (v2 - v0), every difference and product rounded on its own
ADFP_DEV void shade_face_normal(const double* v, const int* id, double* g) {
    double e1[3], e2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e1[k] = v[3 * (long long)id[1] + k] - v[3 * (long long)id[0] + k];
        e2[k] = v[3 * (long long)id[2] + k] - v[3 * (long long)id[0] + k];
    }
    g[0] = e1[1] * e2[2] - e1[2] * e2[1];
    g[1] = e1[2] * e2[0] - e1[0] * e2[2];
    g[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// face i: fn[3 i ..] = its normal (zeros for a face with an index outside [0, nv)); corner e = 3 i + c: key[e] = its vertex (nv for
// such a face: sorted last, in no vertex's run), val[e] = e
__global__ __launch_bounds__(ADFP_SHADE_THREADS) void k_vn_faces(const double* __restrict__ v, int nv, const int* __restrict__ f, int nf,
                                                                   double* __restrict__ fn, int* __restrict__ key, int* __restrict__ val) {
    const long long i = (long long)blockIdx.x * ADFP_SHADE_THREADS + threadIdx.x;
    if (i >= nf) return;
    int id[3];
    const bool ok = shade_face_ok(f, i, nv, id);
    double g[3] = {0.0, 0.0, 0.0};
    if (ok) shade_face_normal(v, id, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        fn[3 * i + c] = g[c];
        key[3 * i + c] = ok ? id[c] : nv;
        val[3 * i + c] = (int)(3 * i + c);
    }
}

// vertex i: the first e with key[e] >= i by bisection, then s += fn[val[e] / 3] while key[e] == i (ascending corners: ascending
// faces); out = s / sqrt((sx sx + sy sy) + sz sz), zeros when that length is 0 or not finite
__global__ __launch_bounds__(ADFP_SHADE_THREADS) void k_vn_sum(const int* __restrict__ key, const int* __restrict__ val, long long ne,
                                                                 const double* __restrict__ fn, int nv, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ADFP_SHADE_THREADS + threadIdx.x;
    if (i >= nv) return;
    long long lo = 0, hi = ne;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < (int)i) lo = mid + 1; else hi = mid;
    }
    double s[3] = {0.0, 0.0, 0.0};
    for (long long e = lo; e < ne && key[e] == (int)i; ++e) {
        const double* g = fn + 3 * (long long)(val[e] / 3);
        s[0] += g[0]; s[1] += g[1]; s[2] += g[2];
    }
    const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * i + c] = ok ? s[c] / len : 0.0;
}

struct ShadeArgs {
    const int* face; const float* bary;                       // [views][H][W], [views][H][W][2]: k_render_hits's
    long long npix; int H, W;                                 // npix = views x H x W
    const double* v; int nv; const int* f; int nf;
    const double* c2w; double fx, fy, cx, cy;                 // [views][12]
    const double* vn; const unsigned char* vc;                // [nv][3] each, or NULL: flat shading / the albedo
    double albedo[3], ambient; unsigned char bg[3]; int mode;
    float* normal; unsigned char* rgb;                        // [views][H][W][3] each, or NULL
};

ADFP_DEV unsigned char shade_byte(double x) {
    x = x > 0.0 ? x : 0.0;                                    // NaN goes to 0
    x = x < 1.0 ? x : 1.0;
    return (unsigned char)floor(x * 255.0 + 0.5);
}

// One lane, one pixel; the contract is include/adfp.h's, operation for operation
__global__ __launch_bounds__(ADFP_SHADE_THREADS) void k_shade_hits(ShadeArgs a) {
    const long long px = (long long)blockIdx.x * ADFP_SHADE_THREADS + threadIdx.x;
    if (px >= a.npix) return;
    const long long hw = (long long)a.H * a.W, p = px / hw, rem = px - p * hw;
    const int row = (int)(rem / a.W), col = (int)(rem - (long long)row * a.W);
    const int fi = a.face[px];
    int id[3];
    const bool hit = (unsigned)fi < (unsigned)a.nf && shade_face_ok(a.f, fi, a.nv, id);
    if (!hit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.normal) a.normal[3 * px + c] = 0.f;
            if (a.rgb) a.rgb[3 * px + c] = a.bg[c];
        }
        return;
    }
    const double b1 = (double)a.bary[2 * px], b2 = (double)a.bary[2 * px + 1], b0 = (1.0 - b1) - b2;
    double g[3], n[3];
    shade_face_normal(a.v, id, g);
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = g[c];
    if (a.vn) {
        double s[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            s[c] = (b0 * a.vn[3 * (long long)id[0] + c] + b1 * a.vn[3 * (long long)id[1] + c]) + b2 * a.vn[3 * (long long)id[2] + c];
        if (!(s[0] == 0.0 && s[1] == 0.0 && s[2] == 0.0)) { n[0] = s[0]; n[1] = s[1]; n[2] = s[2]; }
    }
    const double* m = a.c2w + 12 * p;
    double nc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nc[c] = (m[c] * n[0] + m[4 + c] * n[1]) + m[8 + c] * n[2];
    const double len = sqrt((nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2]);
    const bool ok = len > 0.0 && isfinite(len);
#pragma unroll
    for (int c = 0; c < 3; ++c) nc[c] = ok ? nc[c] / len : 0.0;
    const double dx = ((double)col - a.cx) / a.fx, dy = ((double)row - a.cy) / a.fy;
    double dot = (nc[0] * dx + nc[1] * dy) + nc[2];
    if (dot > 0.0) { nc[0] = -nc[0]; nc[1] = -nc[1]; nc[2] = -nc[2]; dot = -dot; }
    if (a.normal) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normal[3 * px + c] = (float)nc[c];
    }
    if (!a.rgb) return;
    double x[3];
    if (a.mode == ADFP_SHADE_NORMAL) {
        x[0] = (nc[0] + 1.0) / 2.0; x[1] = (-nc[1] + 1.0) / 2.0; x[2] = (-nc[2] + 1.0) / 2.0;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            x[c] = a.vc ? ((b0 * (double)a.vc[3 * (long long)id[0] + c] + b1 * (double)a.vc[3 * (long long)id[1] + c]) +
                           b2 * (double)a.vc[3 * (long long)id[2] + c]) / 255.0
                        : a.albedo[c];
        if (a.mode == ADFP_SHADE_SHADED) {
            const double I = a.ambient + (1.0 - a.ambient) * (-dot / sqrt((dx * dx + dy * dy) + 1.0));
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = x[c] * I;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.rgb[3 * px + c] = shade_byte(x[c]);
}

// ---- host side: the launchers ----
#define SHADE_MAX_PIXELS (1ll << 38)                    // the grid's x stays below 2^31
static unsigned shade_blocks(long long n) { return (unsigned)ceil_div(n, ADFP_SHADE_THREADS); }

extern "C" {

// face normals [F][3] doubles; key, val, key_tmp, val_tmp [3 F] ints (the corners by vertex); the sort's
struct VnWork { double* fn; int* key; int* val; int* key_tmp; int* val_tmp; void* sort_ws; };
static VnWork vn_layout(Arena& A, long long nf) {
    VnWork w;
    const size_t ne = 3 * (size_t)nf;
    w.fn = A.take<double>(ne);
    w.key = A.take<int>(ne); w.val = A.take<int>(ne); w.key_tmp = A.take<int>(ne); w.val_tmp = A.take<int>(ne);
    w.sort_ws = A.take<char>(adfp_sort_workspace_bytes((long long)ne));
    return w;
}
size_t adfp_vertex_normals_workspace_bytes(long long n_faces) {
    return n_faces <= 0 || n_faces > RECON_MAX_N / 3 ? 0 : layout_bytes(vn_layout, n_faces);
}

int adfp_vertex_normals(const double* verts, long long n_verts, const int* faces, long long n_faces, void* workspace,
                        size_t workspace_bytes, double* normals, void* stream) {
    if (n_verts < 0 || n_faces < 0) return ADFP_E_ARG;
    if (n_verts == 0) return 0;
    if (!verts || !normals || (n_faces > 0 && (!faces || !workspace))) return ADFP_E_ARG;
    if (mcl_mesh_too_large(n_verts, n_faces)) return ADFP_E_UNSUPPORTED;
    if (n_faces > 0 && workspace_bytes < adfp_vertex_normals_workspace_bytes(n_faces)) return ADFP_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n_faces == 0) {
        hipError_t e = hipMemsetAsync(normals, 0, (size_t)n_verts * 24, st);
        return e == hipSuccess ? 0 : (int)e;
    }
    const long long ne = 3 * n_faces;
    Arena A(workspace);
    const VnWork w = vn_layout(A, n_faces);
    hipLaunchKernelGGL(k_vn_faces, dim3(shade_blocks(n_faces)), dim3(ADFP_SHADE_THREADS), 0, st, verts, (int)n_verts, faces, (int)n_faces,
                       w.fn, w.key, w.val);
    ADFP_CHECK_LAUNCH();
    int rc = adfp_sort_pairs(w.key, w.val, w.key_tmp, w.val_tmp, ne, mcl_bits(n_verts), w.sort_ws, adfp_sort_workspace_bytes(ne), stream);   // keys in [0, n_verts]
    if (rc) return rc;
    hipLaunchKernelGGL(k_vn_sum, dim3(shade_blocks(n_verts)), dim3(ADFP_SHADE_THREADS), 0, st, w.key, w.val, ne, w.fn, (int)n_verts, normals);
    ADFP_CHECK_LAUNCH();
    return 0;
}

int adfp_shade_hits(const int* face, const float* bary, long long n_views, int H, int W, const double* verts, long long n_verts,
                    const int* faces, long long n_faces, const double* c2w, double fx, double fy, double cx, double cy,
                    const double* vertex_normals, const unsigned char* vertex_colors, const float albedo[3], double ambient,
                    const unsigned char background[3], int mode, float* normal, unsigned char* rgb, void* stream) {
    if (n_views < 0 || n_verts < 0 || n_faces < 0 || H <= 0 || W <= 0) return ADFP_E_ARG;
    if (mode != ADFP_SHADE_COLOR && mode != ADFP_SHADE_SHADED && mode != ADFP_SHADE_NORMAL) return ADFP_E_ARG;
    if (!(ambient >= 0.0) || !(ambient <= 1.0)) return ADFP_E_ARG;
    if (!(fx != 0.0) || !(fy != 0.0) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy)) return ADFP_E_ARG;
    if (!background || (!vertex_colors && !albedo)) return ADFP_E_ARG;
    if (n_views == 0 || (!normal && !rgb)) return 0;
    if (!face || !bary || !c2w || (n_faces > 0 && (!faces || (n_verts > 0 && !verts)))) return ADFP_E_ARG;
    if (n_verts > RECON_MAX_N || n_faces > RECON_MAX_N || H > RT_MAX_SIDE || W > RT_MAX_SIDE || n_views > RECON_MAX_N) return ADFP_E_UNSUPPORTED;
    const long long npix = n_views * H * W;
    if (npix > SHADE_MAX_PIXELS) return ADFP_E_UNSUPPORTED;
    ShadeArgs a;
    a.face = face; a.bary = bary; a.npix = npix; a.H = H; a.W = W;
    a.v = verts; a.nv = (int)n_verts; a.f = faces; a.nf = (int)n_faces;
    a.c2w = c2w; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.vn = vertex_normals; a.vc = vertex_colors;
    for (int c = 0; c < 3; ++c) { a.albedo[c] = albedo ? (double)albedo[c] : 0.0; a.bg[c] = background[c]; }
    a.ambient = ambient; a.mode = mode; a.normal = normal; a.rgb = rgb;
    hipLaunchKernelGGL(k_shade_hits, dim3(shade_blocks(npix)), dim3(ADFP_SHADE_THREADS), 0, (hipStream_t)stream, a);
    ADFP_CHECK_LAUNCH();
    return 0;
}

}   // extern "C"
