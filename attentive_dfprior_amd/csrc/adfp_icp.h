// adfp_icp.h -- frame-to-model point-to-plane ICP over the whole depth image (KinectFusion's tracker): the sensor depth against the
// raycast of the TSDF prior (adfp_tsdfcast.h), to seed the Tracker's pose or to stand in for it.  The contract is stated in
// include/adfp.h ("Depth ICP") and, in numpy, in tests/icp_ref.py.
//
//   k_depth_normals  one lane per pixel, a row of the image per blockIdx.y: the three depths a lane reads are its own, its right
//                    neighbour's (the next lane's) and the one below (the next row's same column), so every load is a coalesced
//                    row piece.  Arithmetic in f64 from f32 loads, one rounding to f32 at the store.
//   k_icp_step       256-thread workgroups, a grid-stride loop over the strided pixels, the grid sized to the compute units and not
//                    to the image: a lane keeps the 29 sums of the normal equations in registers (58 VGPRs), the wave adds them
//                    with DPP row steps and four readlanes (wave_sum), the four waves meet in 4 x 29 doubles of LDS, and the
//                    workgroup leaves ONE row of 29 doubles in the caller's workspace.  No atomics.
//                    The pair itself (association, gates, r and J: icp_geo_pair), the accumulation (icp_add_pair) and the
//                    workgroup's reduction (icp_block_sums) are functions that k_rgbd_step (adfp_rgbd.h) calls too.
//   k_icp_solve<NS>  one wave: lane l adds the rows l, l + 64, ... of the workspace in that order, wave_sum adds the lanes, lane 0
//                    solves the 6 x 6 system by LDL^T, applies the twist and writes the stats row.  The order of every addition
//                    is fixed by the launch geometry alone, so two calls on the same inputs give the same bytes.
//   k_icp_begin / k_icp_end   one lane each: T = guess; the gate on the result, c2w_out, cam_out.
//
// The solve runs in a second launch and not in the last workgroup to arrive: a step is two nodes of a captured graph either way,
// the second launch costs a few microseconds against a step's tens, and nothing has to be handed over between workgroups inside a
// launch (no ticket word to zero, no release / acquire pair to get right).
//
// Everything is decided on the device: a step reads the status the step before it left in the state block and does nothing
// when that is not OK, so a whole refinement is one fixed sequence of launches with no read-back.
#pragma once
#include "adfp_device.h"

#define ADFP_ICP_THREADS 256
#define ADFP_ICP_MAX_BLOCKS 1024
#define ADFP_ICP_MAX_DIM 32768

struct IcpState {
    double T[16];          // the current estimate, camera to world, row-major
    double guess[16];      // what adfp_icp_begin was given (f32 values)
    double status;         // ADFP_ICP_OK ...
    double pad;
};
static_assert(sizeof(IcpState) == ADFP_ICP_STATE_BYTES, "include/adfp.h states the size of the state block");

ADFP_DEV bool icp_depth_ok(float d) { return d > 0.f && d <= 3.4028234663852886e38f; }      // NaN and +inf fail

// the camera point of pixel (u, v) at depth d: ((u - cx) / fx d, -(v - cy) / fy d, -d)
ADFP_DEV void icp_vertex(int u, int v, double d, double fx, double fy, double cx, double cy, double p[3]) {
    p[0] = (((double)u - cx) / fx) * d;
    p[1] = (-((double)v - cy) / fy) * d;
    p[2] = -d;
}

// grid (ceil(W / 256), H, V)
__global__ __launch_bounds__(256) void k_depth_normals(const float* __restrict__ depth, int H, int W, float fxf, float fyf, float cxf, float cyf,
                                                       float max_jump, float* __restrict__ out) {
    const int u = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
    if (u >= W) return;
    const long long base = ((long long)blockIdx.z * H + v) * W + u;
    float n[3] = {0.f, 0.f, 0.f};
    if (u + 1 < W && v + 1 < H) {
        const float d0 = depth[base], dr = depth[base + 1], dd = depth[base + W];
        bool ok = icp_depth_ok(d0) && icp_depth_ok(dr) && icp_depth_ok(dd);
        if (ok && max_jump > 0.f)
            ok = fabs((double)dr - (double)d0) <= (double)max_jump && fabs((double)dd - (double)d0) <= (double)max_jump;
        if (ok) {
            const double fx = fxf, fy = fyf, cx = cxf, cy = cyf;
            double p[3], pr[3], pd[3];
            icp_vertex(u, v, d0, fx, fy, cx, cy, p);
            icp_vertex(u + 1, v, dr, fx, fy, cx, cy, pr);
            icp_vertex(u, v + 1, dd, fx, fy, cx, cy, pd);
            const double a[3] = {pr[0] - p[0], pr[1] - p[1], pr[2] - p[2]};
            const double b[3] = {pd[0] - p[0], pd[1] - p[1], pd[2] - p[2]};
            double c[3] = {b[1] * a[2] - b[2] * a[1], b[2] * a[0] - b[0] * a[2], b[0] * a[1] - b[1] * a[0]};
            const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            if (len > 0.0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) c[k] = c[k] / len;
                const bool flip = ((c[0] * p[0] + c[1] * p[1]) + c[2] * p[2]) > 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = (float)(flip ? -c[k] : c[k]);
            }
        }
    }
    out[3 * base + 0] = n[0]; out[3 * base + 1] = n[1]; out[3 * base + 2] = n[2];
}

struct IcpStepArgs {
    const float* ds; const float* ns; const float* dm; const float* nm; const float* pref;
    const IcpState* state;
    int H, W, stride, wn;                  // wn: strided pixels per row
    long long n;                           // strided pixels
    double fx, fy, cx, cy, dist_tol, cos_tol;
    double* part;                          // [gridDim.x][ADFP_ICP_SUMS]
};

// x = T V(u, v, d): the sensor pixel's point in the world
ADFP_DEV void icp_sensor_point(const IcpStepArgs& a, const double T[12], int us, int vs, double d, double x[3]) {
    double Vs[3];
    icp_vertex(us, vs, d, a.fx, a.fy, a.cx, a.cy, Vs);
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = ((T[4 * k] * Vs[0] + T[4 * k + 1] * Vs[1]) + T[4 * k + 2] * Vs[2]) + T[4 * k + 3];
}

// The geometric pair of the sensor point x with the sensor normal Ns (camera frame, not zero): projective association into the model
// image, the gates, then r and J.  false: no pair.  k_icp_step and k_rgbd_step (adfp_rgbd.h) both call this, so that the joint step
// without a photometric term adds the same numbers in the same order.
ADFP_DEV bool icp_geo_pair(const IcpStepArgs& a, const double T[12], const double P[12], const double x[3], const double Ns[3], double J[6],
                           double& r) {
    double nsw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nsw[k] = (T[4 * k] * Ns[0] + T[4 * k + 1] * Ns[1]) + T[4 * k + 2] * Ns[2];
    const double e[3] = {x[0] - P[3], x[1] - P[7], x[2] - P[11]};
    double xc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xc[k] = (P[k] * e[0] + P[4 + k] * e[1]) + P[8 + k] * e[2];
    const double z = -xc[2];
    if (!(z > 0.0)) return false;
    const double pu = floor((((a.fx * xc[0]) / z) + a.cx) + 0.5), pv = floor((((-a.fy * xc[1]) / z) + a.cy) + 0.5);
    if (!(pu >= 0.0 && pu <= (double)(a.W - 1) && pv >= 0.0 && pv <= (double)(a.H - 1))) return false;
    const int um = (int)pu, vm = (int)pv;
    const long long mi = (long long)vm * a.W + um;
    const double Nm[3] = {(double)a.nm[3 * mi], (double)a.nm[3 * mi + 1], (double)a.nm[3 * mi + 2]};
    if (Nm[0] == 0.0 && Nm[1] == 0.0 && Nm[2] == 0.0) return false;
    double Vm[3];
    icp_vertex(um, vm, (double)a.dm[mi], a.fx, a.fy, a.cx, a.cy, Vm);
    double m[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m[k] = ((P[4 * k] * Vm[0] + P[4 * k + 1] * Vm[1]) + P[4 * k + 2] * Vm[2]) + P[4 * k + 3];
        n[k] = (P[4 * k] * Nm[0] + P[4 * k + 1] * Nm[1]) + P[4 * k + 2] * Nm[2];
    }
    const double g[3] = {m[0] - x[0], m[1] - x[1], m[2] - x[2]};
    const double dist = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (!(dist <= a.dist_tol)) return false;
    const double cs = (nsw[0] * n[0] + nsw[1] * n[1]) + nsw[2] * n[2];
    if (!(cs >= a.cos_tol)) return false;
    r = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
    J[0] = x[1] * n[2] - x[2] * n[1]; J[1] = x[2] * n[0] - x[0] * n[2]; J[2] = x[0] * n[1] - x[1] * n[0];
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    return true;
}

// one pair into a lane's sums: acc[0..20] += w J J^T (upper, row by row), acc[21..26] += w J r, acc[tail] += r^2, acc[tail + 1] += 1.
// WEIGHTED false adds the products themselves (w is not read).
template <bool WEIGHTED>
ADFP_DEV void icp_add_pair(double* acc, const double J[6], double r, double w, int tail) {
    int q = 0;
#pragma unroll
    for (int i2 = 0; i2 < 6; ++i2)
#pragma unroll
        for (int j2 = i2; j2 < 6; ++j2) { acc[q] += WEIGHTED ? w * (J[i2] * J[j2]) : J[i2] * J[j2]; ++q; }
#pragma unroll
    for (int i2 = 0; i2 < 6; ++i2) acc[21 + i2] += WEIGHTED ? w * (J[i2] * r) : J[i2] * r;
    acc[tail] += r * r;
    acc[tail + 1] += 1.0;
}

// the lanes' sums -> one row of NS doubles per workgroup: DPP within the wave, the four waves through LDS
template <int NS>
ADFP_DEV void icp_block_sums(double* acc, double (*s_part)[NS], double* __restrict__ part) {
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NS; ++k) s_part[threadIdx.x >> 6][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < NS) {
        const int k = threadIdx.x;
        part[(long long)blockIdx.x * NS + k] = (s_part[0][k] + s_part[1][k]) + (s_part[2][k] + s_part[3][k]);
    }
}

__global__ __launch_bounds__(ADFP_ICP_THREADS) void k_icp_step(IcpStepArgs a) {
    __shared__ double s_part[4][ADFP_ICP_SUMS];
    if (a.state->status != (double)ADFP_ICP_OK) return;          // kernel-uniform: k_icp_solve returns on the same word
    double T[12], P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T[k] = a.state->T[k]; P[k] = (double)a.pref[k]; }
    double acc[ADFP_ICP_SUMS];
#pragma unroll
    for (int k = 0; k < ADFP_ICP_SUMS; ++k) acc[k] = 0.0;
    const long long step = (long long)gridDim.x * ADFP_ICP_THREADS;
    for (long long i = (long long)blockIdx.x * ADFP_ICP_THREADS + threadIdx.x; i < a.n; i += step) {
        const int vs = (int)(i / a.wn) * a.stride, us = (int)(i % a.wn) * a.stride;
        const long long si = (long long)vs * a.W + us;
        const double Ns[3] = {(double)a.ns[3 * si], (double)a.ns[3 * si + 1], (double)a.ns[3 * si + 2]};
        if (Ns[0] == 0.0 && Ns[1] == 0.0 && Ns[2] == 0.0) continue;
        double x[3], J[6], r;
        icp_sensor_point(a, T, us, vs, (double)a.ds[si], x);
        if (!icp_geo_pair(a, T, P, x, Ns, J, r)) continue;
        icp_add_pair<false>(acc, J, r, 1.0, 27);
    }
    icp_block_sums<ADFP_ICP_SUMS>(acc, s_part, a.part);
}

// Exp of the twist (w, t): rotation E[0..8] row-major and translation E[9..11] = V t
ADFP_DEV void icp_exp(const double w[3], const double t[3], double th, double E[12]) {
    double A, B, Cc;
    if (th < 1e-12) { A = 1.0; B = 0.5; Cc = 0.0; }               // the series: R = I + K, V = I + K / 2
    else { A = sin(th) / th; B = (1.0 - cos(th)) / (th * th); Cc = (1.0 - A) / (th * th); }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double K2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
    const bool series = th < 1e-12;
    double Vm[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double id = (i % 4 == 0) ? 1.0 : 0.0;
        E[i] = series ? id + K[i] : (id + A * K[i]) + B * K2[i];
        Vm[i] = series ? id + 0.5 * K[i] : (id + B * K[i]) + Cc * K2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) E[9 + i] = (Vm[3 * i] * t[0] + Vm[3 * i + 1] * t[1]) + Vm[3 * i + 2] * t[2];
}

// one wave.  NS = ADFP_ICP_SUMS: the depth ICP's 29 sums.  NS = ADFP_RGBD_SUMS: two more, the photometric sum of squares and pair
// count; the larger of the two pair counts is held against min_pairs, and rgb_row receives (photometric pairs, photometric rmse).
template <int NS>
__global__ __launch_bounds__(64) void k_icp_solve(const double* __restrict__ part, int rows, IcpState* state, double min_pivot, double min_pairs,
                                                  double* __restrict__ stats_row, double* __restrict__ rgb_row, double* __restrict__ sums_out) {
    const int lane = threadIdx.x;
    const double st_in = state->status;
    if (st_in != (double)ADFP_ICP_OK) {                           // a step after a failed one: the row says so, nothing moves
        if (lane < ADFP_ICP_STATS) stats_row[lane] = lane == ADFP_ICP_STATS - 1 ? st_in : 0.0;
        if (NS > ADFP_ICP_SUMS && lane < 2) rgb_row[lane] = 0.0;
        if (sums_out && lane < NS) sums_out[lane] = 0.0;
        return;
    }
    double S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = 0.0;
    for (int r = lane; r < rows; r += 64)
#pragma unroll
        for (int k = 0; k < NS; ++k) S[k] += part[(long long)r * NS + k];
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = wave_sum(S[k]);
    if (lane != 0) return;
    if (sums_out)
#pragma unroll
        for (int k = 0; k < NS; ++k) sums_out[k] = S[k];
    const double pairs = S[28];
    const double rmse = pairs > 0.0 ? sqrt(S[27] / pairs) : 0.0;
    double most = pairs;                                           // what min_pairs is held against
    if (NS > ADFP_ICP_SUMS) {
        const double pp = S[NS - 1];
        rgb_row[0] = pp; rgb_row[1] = pp > 0.0 ? sqrt(S[NS - 2] / pp) : 0.0;
        most = pp > pairs ? pp : pairs;
    }
    double A[6][6], b[6];
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { A[i][j] = S[q]; A[j][i] = S[q]; ++q; }
#pragma unroll
        for (int i = 0; i < 6; ++i) b[i] = S[21 + i];
    }
    double status = (double)ADFP_ICP_OK, ratio = 0.0, wn = 0.0, tn = 0.0;
    if (most < min_pairs) status = (double)ADFP_ICP_FEW_PAIRS;
    else {
        double dmax = A[0][0];
#pragma unroll
        for (int i = 1; i < 6; ++i) dmax = A[i][i] > dmax ? A[i][i] : dmax;
        // LDL^T without pivoting: A is a sum of J^T J, positive semi-definite; a pivot at or below min_pivot max diag(A) is the
        // direction the pairs do not constrain
        double L[6][6], D[6];
        bool bad = !(dmax > 0.0);
        double rmin = __builtin_inf();
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (bad) break;
            double d = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= (L[j][k] * L[j][k]) * D[k];
            const double rt = d / dmax;
            rmin = rt < rmin ? rt : rmin;
            if (!(d > min_pivot * dmax)) { bad = true; break; }
            D[j] = d;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= (L[i][k] * L[j][k]) * D[k];
                L[i][j] = s / d;
            }
        }
        ratio = dmax > 0.0 ? rmin : 0.0;
        if (bad) status = (double)ADFP_ICP_DEGENERATE;
        else {
            double y[6], xi[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double s = b[i];
#pragma unroll
                for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
                y[i] = s;
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double s = y[i] / D[i];
#pragma unroll
                for (int k = i + 1; k < 6; ++k) s -= L[k][i] * xi[k];
                xi[i] = s;
            }
            const double w[3] = {xi[0], xi[1], xi[2]}, t[3] = {xi[3], xi[4], xi[5]};
            wn = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
            tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
            double E[12], Tn[12];
            icp_exp(w, t, wn, E);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    double s = (E[3 * i] * state->T[j] + E[3 * i + 1] * state->T[4 + j]) + E[3 * i + 2] * state->T[8 + j];
                    if (j == 3) s += E[9 + i];
                    Tn[4 * i + j] = s;
                }
#pragma unroll
            for (int k = 0; k < 12; ++k) state->T[k] = Tn[k];
        }
    }
    state->status = status;
    stats_row[0] = pairs; stats_row[1] = rmse; stats_row[2] = ratio; stats_row[3] = wn; stats_row[4] = tn; stats_row[5] = status;
}

__global__ __launch_bounds__(64) void k_icp_begin(const float* __restrict__ guess, IcpState* state) {
    const int k = threadIdx.x;
    if (k < 16) { const double g = (double)guess[k]; state->T[k] = g; state->guess[k] = g; }
    if (k == 16) { state->status = (double)ADFP_ICP_OK; state->pad = 0.0; }
}

// common.get_tensor_from_camera in f64 on the f32 matrix M (row-major [4][4]): q = (r, i, j, k), then the translation
ADFP_DEV void icp_camera_tensor(const float* M, float cam[7]) {
    double R[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {                                  // unit-length axis vectors (columns); a zero one stays
        const double c0 = (double)M[j], c1 = (double)M[4 + j], c2 = (double)M[8 + j];
        const double nrm = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        const double dv = nrm > 0.0 ? nrm : 1.0;
        R[0][j] = c0 / dv; R[1][j] = c1 / dv; R[2][j] = c2 / dv;
    }
    const double det = (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]))
                       + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0.0)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = -R[i][j];
    double q[4];
    const double tr = (R[0][0] + R[1][1]) + R[2][2];
    if (tr > 0.0) {
        const double s = 2.0 * sqrt(1.0 + tr);
        q[0] = 0.25 * s; q[1] = (R[2][1] - R[1][2]) / s; q[2] = (R[0][2] - R[2][0]) / s; q[3] = (R[1][0] - R[0][1]) / s;
    } else {
        int k = 0;
        if (R[1][1] > R[k][k]) k = 1;
        if (R[2][2] > R[k][k]) k = 2;
        const int ia = (k + 1) % 3, ib = (k + 2) % 3;
        const double s = 2.0 * sqrt(((1.0 + R[k][k]) - R[ia][ia]) - R[ib][ib]);
        q[1 + k] = 0.25 * s; q[1 + ia] = (R[ia][k] + R[k][ia]) / s; q[1 + ib] = (R[ib][k] + R[k][ib]) / s;
        q[0] = (R[ib][ia] - R[ia][ib]) / s;
    }
    const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const double sg = (q[0] / qn) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) cam[i] = (float)(sg * (q[i] / qn));
    cam[4] = M[3]; cam[5] = M[7]; cam[6] = M[11];
}

__global__ __launch_bounds__(64) void k_icp_end(IcpState* state, double max_shift, double max_angle, float* __restrict__ c2w_out,
                                                float* __restrict__ cam_out, double* __restrict__ stats_row) {
    if (threadIdx.x != 0) return;
    double status = state->status, shift = 0.0, angle = 0.0;
    const double* T = state->T;
    const double* G = state->guess;
    if (status == (double)ADFP_ICP_OK) {
        const double e[3] = {T[3] - G[3], T[7] - G[7], T[11] - G[11]};
        shift = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
        double D[3][3];                                             // R_T R_guess^T
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) D[i][j] = (T[4 * i] * G[4 * j] + T[4 * i + 1] * G[4 * j + 1]) + T[4 * i + 2] * G[4 * j + 2];
        const double c = (((D[0][0] + D[1][1]) + D[2][2]) - 1.0) * 0.5;
        const double v[3] = {D[2][1] - D[1][2], D[0][2] - D[2][0], D[1][0] - D[0][1]};
        const double s = 0.5 * sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        angle = atan2(s, c);
        if (!(shift <= max_shift) || !(angle <= max_angle)) status = (double)ADFP_ICP_REJECTED;
    }
    const bool keep = status == (double)ADFP_ICP_OK;
    float M[16];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = (float)(keep ? T[k] : G[k]);
    if (keep) { M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f; }
    else
#pragma unroll
        for (int k = 12; k < 16; ++k) M[k] = (float)G[k];
    float cam[7];
    icp_camera_tensor(M, cam);
#pragma unroll
    for (int k = 0; k < 16; ++k) c2w_out[k] = M[k];
#pragma unroll
    for (int k = 0; k < 7; ++k) cam_out[k] = cam[k];
    state->status = status;
    if (stats_row) { stats_row[0] = 0.0; stats_row[1] = 0.0; stats_row[2] = 0.0; stats_row[3] = angle; stats_row[4] = shift; stats_row[5] = status; }
}

// ---- the C ABI -------------------------------------------------------------------------------------------------------------------
static long long icp_blocks_max(int H, int W) {
    if (H < 1 || W < 1 || H > ADFP_ICP_MAX_DIM || W > ADFP_ICP_MAX_DIM) return 0;
    const long long b = ((long long)H * W + ADFP_ICP_THREADS - 1) / ADFP_ICP_THREADS;
    return b < ADFP_ICP_MAX_BLOCKS ? b : ADFP_ICP_MAX_BLOCKS;
}

extern "C" size_t adfp_icp_workspace_bytes(int H, int W) {
    return (size_t)icp_blocks_max(H, W) * ADFP_ICP_SUMS * sizeof(double);
}

extern "C" int adfp_depth_normals(const float* depth, int V, int H, int W, float fx, float fy, float cx, float cy, float max_jump, float* normals,
                                  void* stream) {
    if (!depth || !normals || V < 1 || H < 1 || W < 1) return ADFP_E_ARG;
    if (!(fx == fx) || !(fy == fy) || fx == 0.f || fy == 0.f || !(cx == cx) || !(cy == cy) || !(max_jump == max_jump)) return ADFP_E_ARG;
    if (H > ADFP_ICP_MAX_DIM || W > ADFP_ICP_MAX_DIM || V > 65535) return ADFP_E_UNSUPPORTED;
    const dim3 grid((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)V);
    hipLaunchKernelGGL(k_depth_normals, grid, dim3(256), 0, (hipStream_t)stream, depth, H, W, fx, fy, cx, cy, max_jump, normals);
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_icp_begin(const float* guess, void* state, void* stream) {
    if (!guess || !state || (((unsigned long long)state) & 7ull)) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_icp_begin, dim3(1), dim3(64), 0, (hipStream_t)stream, guess, (IcpState*)state);
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_icp_step(const float* depth_s, const float* normals_s, const float* depth_m, const float* normals_m, const float* p_ref, int H,
                             int W, float fx, float fy, float cx, float cy, int stride, double dist_tol, double cos_tol, double min_pivot,
                             double min_pairs, void* state, double* stats, int stats_rows, int row, double* sums, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (!depth_s || !normals_s || !depth_m || !normals_m || !p_ref || !state || !stats || !workspace) return ADFP_E_ARG;
    if (H < 1 || W < 1 || stride < 1 || stats_rows < 1 || row < 0 || row >= stats_rows) return ADFP_E_ARG;
    if (!(dist_tol == dist_tol) || !(cos_tol == cos_tol) || !(min_pivot == min_pivot) || !(min_pairs == min_pairs)) return ADFP_E_ARG;
    if (!(fx == fx) || !(fy == fy) || fx == 0.f || fy == 0.f || !(cx == cx) || !(cy == cy)) return ADFP_E_ARG;
    if ((((unsigned long long)state) & 7ull) || (((unsigned long long)workspace) & 7ull) || (((unsigned long long)stats) & 7ull)) return ADFP_E_ARG;
    if (H > ADFP_ICP_MAX_DIM || W > ADFP_ICP_MAX_DIM) return ADFP_E_UNSUPPORTED;
    const size_t need = adfp_icp_workspace_bytes(H, W);
    if (need == 0 || workspace_bytes < need) return ADFP_E_ARG;
    IcpStepArgs a;
    a.ds = depth_s; a.ns = normals_s; a.dm = depth_m; a.nm = normals_m; a.pref = p_ref; a.state = (const IcpState*)state;
    a.H = H; a.W = W; a.stride = stride;
    a.wn = (W + stride - 1) / stride;
    a.n = (long long)a.wn * ((H + stride - 1) / stride);
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.dist_tol = dist_tol; a.cos_tol = cos_tol;
    a.part = (double*)workspace;
    long long blocks = (a.n + ADFP_ICP_THREADS - 1) / ADFP_ICP_THREADS;        // <= icp_blocks_max(H, W): the workspace holds them
    const long long cap = 2ll * num_cu();                                        // two workgroups a compute unit: one hides the other's loads
    if (blocks > cap) blocks = cap;
    if (blocks > ADFP_ICP_MAX_BLOCKS) blocks = ADFP_ICP_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_icp_step, dim3((unsigned)blocks), dim3(ADFP_ICP_THREADS), 0, st, a);
    ADFP_CHECK_LAUNCH();
    hipLaunchKernelGGL((k_icp_solve<ADFP_ICP_SUMS>), dim3(1), dim3(64), 0, st, (const double*)workspace, (int)blocks, (IcpState*)state, min_pivot,
                       min_pairs, stats + (long long)row * ADFP_ICP_STATS, (double*)nullptr, sums);
    ADFP_CHECK_LAUNCH();
    return 0;
}

extern "C" int adfp_icp_end(void* state, double max_shift, double max_angle, float* c2w_out, float* cam_out, double* stats, int stats_rows, int row,
                            void* stream) {
    if (!state || !c2w_out || !cam_out || (((unsigned long long)state) & 7ull)) return ADFP_E_ARG;
    if (!(max_shift == max_shift) || !(max_angle == max_angle)) return ADFP_E_ARG;
    if (stats && (stats_rows < 1 || row < 0 || row >= stats_rows || (((unsigned long long)stats) & 7ull))) return ADFP_E_ARG;
    hipLaunchKernelGGL(k_icp_end, dim3(1), dim3(64), 0, (hipStream_t)stream, (IcpState*)state, max_shift, max_angle, c2w_out, cam_out,
                       stats ? stats + (long long)row * ADFP_ICP_STATS : nullptr);
    ADFP_CHECK_LAUNCH();
    return 0;
}
