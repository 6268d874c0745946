"""The RGB-D ICP (include/adfp.h "RGB-D ICP", csrc/adfp_rgbd.h) restated with numpy on the CPU: the frame map, the photometric pairs
of a step, the 31 joint sums and a whole refinement.  The geometric part, the solve and the gate are icp_ref's.  `dtype` is the
precision of ALL the arithmetic, as in icp_ref: float64 is the rule the kernels implement, float32 the yardstick that says how far
single precision moves the results.  Maps are stored as float32 in both, as the kernel stores them."""
import math

import numpy as np

import icp_ref as R

SUMS, STATS = 31, 2

# ---- float32 against float64, measured by tests/test_rgbd_icp_host.py on the mini scene (it asserts they stay below these constants);
# the kernels' bars against the float64 restatement are 8 x these, the project's margin for a kernel that loads float32 and computes
# in float64.  When this was written the measured values were: map 7.1e-8 (I, gx, gy per component), sums 3.08e-6 (each of the 31 sums
# over the sum of its terms' magnitudes, strides 1 and 2, the nine scene cases with the keyframe at CASE_KEY_SCALE; no pair count
# differed), pose 3.1e-8 m and 1.04e-7 rad after the default levels on the degenerate view's three guesses.
F32_VS_F64_MAP = 9.0e-8
F32_VS_F64_SUMS = 4.0e-6
F32_VS_F64_POSE_M = 4.0e-8
F32_VS_F64_POSE_RAD = 1.3e-7
KERNEL_TOL_MAP = 8 * F32_VS_F64_MAP
KERNEL_TOL_SUMS = 8 * F32_VS_F64_SUMS
KERNEL_TOL_POSE_M = 8 * F32_VS_F64_POSE_M
KERNEL_TOL_POSE_RAD = 8 * F32_VS_F64_POSE_RAD

KEY_TWIST = (0.01, -0.02, 0.015, 0.03, -0.02, 0.01)      # the keyframe of the tests: Exp(KEY_TWIST) P, 36 mm / 27 mrad from P


def frame_map(color, depth, dtype=np.float64):
    """color [H,W,3], depth [H,W] float32 -> [H,W,4] float32 = (I, gx, gy, d)"""
    color, depth = np.asarray(color, dtype=np.float32), np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    c = color.astype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        I = (dtype(0.299) * c[..., 0] + dtype(0.587) * c[..., 1]) + dtype(0.114) * c[..., 2]
        out = np.zeros((H, W, 4), dtype=np.float32)
        out[..., 0] = I.astype(np.float32)
        if W >= 3:
            out[:, 1:-1, 1] = ((I[:, 2:] - I[:, :-2]) / dtype(2)).astype(np.float32)
        if H >= 3:
            out[1:-1, :, 2] = ((I[2:] - I[:-2]) / dtype(2)).astype(np.float32)
    out[..., 3] = depth
    return out


def photo_pairs(cur_map, key_map, p_key, T, fx, fy, cx, cy, stride=1, dist_tol=0.1, rgb_tol=0.25, dtype=np.float64):
    """The photometric pairs of a step -> (pixel index v W + u [n], r [n], J [n,6])"""
    fxd, fyd, cxd, cyd = R.intrinsics(fx, fy, cx, cy, dtype)
    cur, key = np.asarray(cur_map, dtype=np.float32), np.asarray(key_map, dtype=np.float32)
    H, W = cur.shape[:2]
    T = np.asarray(T).astype(dtype)
    K = np.asarray(p_key, dtype=np.float32).astype(dtype)
    vs, us = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    vs, us = vs.reshape(-1), us.reshape(-1)
    keep = R.depth_ok(cur[vs, us, 3]) & np.isfinite(cur[vs, us, 0])
    vs, us = vs[keep], us[keep]
    Is = cur[vs, us, 0].astype(dtype)
    Vs = R.vertices(np.where(R.depth_ok(cur[..., 3]), cur[..., 3], np.float32(0)), fx, fy, cx, cy, dtype)[vs, us]
    x = ((T[:3, 0] * Vs[:, 0:1] + T[:3, 1] * Vs[:, 1:2]) + T[:3, 2] * Vs[:, 2:3]) + T[:3, 3]
    e = x - K[:3, 3]
    y = (K[0, :3] * e[:, 0:1] + K[1, :3] * e[:, 1:2]) + K[2, :3] * e[:, 2:3]
    z = -y[:, 2]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        a = ((fxd * y[:, 0]) / z) + cxd
        b = ((-fyd * y[:, 1]) / z) + cyd
        u0, v0 = np.floor(a), np.floor(b)
        keep = (z > 0) & (u0 >= 1) & (u0 <= W - 3) & (v0 >= 1) & (v0 <= H - 3)
    vs, us, Is, x, y, z, a, b, u0, v0 = (q[keep] for q in (vs, us, Is, x, y, z, a, b, u0, v0))
    s, t = a - u0, b - v0
    u0, v0 = u0.astype(np.int64), v0.astype(np.int64)
    M = [key[v0 + j, u0 + i] for j, i in ((0, 0), (0, 1), (1, 0), (1, 1))]
    ok = np.ones(len(z), dtype=bool)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in M:
            ok &= R.depth_ok(m[:, 3]) & (np.abs(m[:, 3].astype(dtype) - z) <= dtype(dist_tol))
        one = dtype(1)
        w = [(one - s) * (one - t), s * (one - t), (one - s) * t, s * t]
        val = [(w[0] * M[0][:, c].astype(dtype) + w[1] * M[1][:, c].astype(dtype)) + (w[2] * M[2][:, c].astype(dtype) + w[3] * M[3][:, c].astype(dtype))
               for c in range(3)]
        r = Is - val[0]
        ok &= np.abs(r) <= dtype(rgb_tol)
    vs, us, x, y, z, r, gx, gy = (q[ok] for q in (vs, us, x, y, z, r, val[1], val[2]))
    gfx, gfy = gx * fxd, gy * fyd
    c = np.stack([gfx / z, -gfy / z, (gfx * y[:, 0] - gfy * y[:, 1]) / (z * z)], -1)
    n = (K[:3, 0] * c[:, 0:1] + K[:3, 1] * c[:, 1:2]) + K[:3, 2] * c[:, 2:3]
    J = np.concatenate([np.stack([x[:, 1] * n[:, 2] - x[:, 2] * n[:, 1], x[:, 2] * n[:, 0] - x[:, 0] * n[:, 2],
                                  x[:, 0] * n[:, 1] - x[:, 1] * n[:, 0]], -1), n], -1)
    return vs * W + us, r, J


def step_sums(cur_map, normals_s, depth_m, normals_m, p_ref, key_map, p_key, T, fx, fy, cx, cy, stride=1, dist_tol=0.1, cos_tol=0.8,
              rgb_weight=1.0, rgb_tol=0.25, dtype=np.float64):
    """-> (sums [31], scale [31]): the joint sums of one step in adfp.h's order and, per sum, the sum of its terms' magnitudes.
    key_map None or rgb_weight 0: no photometric pair, sums 29 and 30 are 0."""
    cur = np.asarray(cur_map, dtype=np.float32)
    g, gs = R.step_sums(cur[..., 3], normals_s, depth_m, normals_m, p_ref, T, fx, fy, cx, cy, stride, dist_tol, cos_tol, dtype)
    sums, scale = np.zeros(SUMS, dtype=dtype), np.zeros(SUMS, dtype=dtype)
    sums[:29], scale[:29] = g, gs
    if key_map is not None and rgb_weight > 0:
        _, r, J = photo_pairs(cur, key_map, p_key, T, fx, fy, cx, cy, stride, dist_tol, rgb_tol, dtype)
        lam = dtype(rgb_weight)
        terms = [lam * (J[:, i] * J[:, j]) for i in range(6) for j in range(i, 6)] + [lam * (J[:, i] * r) for i in range(6)]
        for q, t in enumerate(terms):
            sums[q] += t.sum(dtype=dtype)
            scale[q] += np.abs(t).sum(dtype=dtype)
        sums[29] = scale[29] = (r * r).sum(dtype=dtype)
        sums[30] = scale[30] = dtype(len(r))
    return sums, scale


def solve(sums, T, min_pivot=1e-6, min_pairs=0.0, dtype=np.float64):
    """-> (T after the step, stats row [6], rgb stats row [photometric pairs, photometric rmse])"""
    S = np.asarray(sums, dtype=dtype)
    pg, pp = float(S[28]), float(S[30])
    rgb = np.array([pp, math.sqrt(float(S[29]) / pp) if pp > 0 else 0.0])
    if max(pg, pp) < min_pairs:
        rmse = math.sqrt(float(S[27]) / pg) if pg > 0 else 0.0
        return np.asarray(T).astype(dtype), np.array([pg, rmse, 0.0, 0.0, 0.0, R.FEW_PAIRS]), rgb
    Tn, row = R.solve(S[:29], T, min_pivot, 0.0, dtype)
    return Tn, row, rgb


def refine(cur_map, depth_m, key_map, p_key, guess, fx, fy, cx, cy, strides=(4, 2, 1), iters=(4, 3, 3), dist_tol=0.1, cos_tol=0.8,
           rgb_weight=1.0, rgb_tol=0.25, min_pivot=1e-6, min_pairs=0.05, max_jump=0.0, max_shift=0.5, max_angle=0.5, dtype=np.float64):
    """The whole refinement on the current frame's map, the model's raycast from `guess` and the keyframe (None: the depth rule):
    -> (c2w_out, cam_out, status, stats rows, rgb stats rows)."""
    guess = np.asarray(guess, dtype=np.float32)
    cur = np.asarray(cur_map, dtype=np.float32)
    H, W = cur.shape[:2]
    ns = R.normals(cur[..., 3], fx, fy, cx, cy, max_jump, dtype)
    nm = R.normals(depth_m, fx, fy, cx, cy, max_jump, dtype)
    T, status, rows, rgb_rows = guess.astype(dtype), R.OK, [], []
    for stride, n in zip(strides, iters):
        need = float(math.ceil(min_pairs * (-(-H // stride)) * (-(-W // stride))))
        for _ in range(n):
            if status != R.OK:
                rows.append(np.array([0.0, 0.0, 0.0, 0.0, 0.0, status]))
                rgb_rows.append(np.zeros(2))
                continue
            sums, _ = step_sums(cur, ns, depth_m, nm, guess, key_map, p_key, T, fx, fy, cx, cy, stride, dist_tol, cos_tol, rgb_weight, rgb_tol, dtype)
            T, row, rgb = solve(sums, T, min_pivot, need, dtype)
            status = int(row[5])
            rows.append(row)
            rgb_rows.append(rgb)
    out, cam, status, shift, angle = R.finish(T.astype(np.float64), guess, status, max_shift, max_angle)
    rows.append(np.array([0.0, 0.0, 0.0, angle, shift, status]))
    rgb_rows.append(np.zeros(2))
    return out, cam, status, np.stack(rows), np.stack(rgb_rows)


# ---- the test scene ---------------------------------------------------------------------------------------------------------------
def texture(X):
    """tests/test_gpu_slam_run.py's colour rule at world points [..., 3] -> [..., 3] float32"""
    return (0.5 + 0.4 * np.sin(np.asarray(X, dtype=np.float64) * np.array([1.3, 1.7, 2.1]) + np.array([0.0, 1.0, 2.0]))).astype(np.float32)


def color_of(depth, c2w, fx, fy, cx, cy):
    """The colour image that goes with a depth image seen from c2w: the texture at every valid pixel's world point, 0 elsewhere."""
    depth = np.asarray(depth, dtype=np.float32)
    ok = R.depth_ok(depth)
    V = R.vertices(np.where(ok, depth, np.float32(0)), fx, fy, cx, cy, np.float64)
    c2w = np.asarray(c2w, dtype=np.float64)
    X = V @ c2w[:3, :3].T + c2w[:3, 3]
    return np.where(ok[..., None], texture(X), np.float32(0))


def key_pose(P, scale=1.0):
    """The tests' keyframe pose for a frame at P: Exp(scale KEY_TWIST) P, float32.  The degenerate view's keyframe is at scale 1; the
    nine corner-facing cases use CASE_KEY_SCALE, 18 mm / 13 mrad away, where at least 0.82 of the strided pixels form a photometric
    pair (at scale 1 two of the stride-2 cases form 0.79)."""
    return (R.exp_se3(np.asarray(KEY_TWIST) * scale) @ np.asarray(P, dtype=np.float64)).astype(np.float32)


CASE_KEY_SCALE = 0.5
