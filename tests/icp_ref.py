"""The depth ICP (include/adfp.h "Depth ICP", csrc/adfp_icp.h) restated with numpy on the CPU.  `dtype` is the precision of ALL the
arithmetic: float64 is the rule the kernels implement (float32 loads promoted to float64), float32 is the yardstick that says how
far single precision moves the normal map, one step's sums and a refinement's pose.  Intrinsics are float32 values in both, and the
normal map is stored as float32 in both, as the kernels store it."""
import math

import numpy as np
import torch

OK, FEW_PAIRS, DEGENERATE, REJECTED = 0, 1, 2, 3

# ---- float32 against float64, measured by tests/test_icp_host.py on the mini scene's nine cases (it asserts they stay below these
# constants); the kernels' bars against the float64 restatement are 8 x these, the project's margin for a kernel that loads float32
# and computes in float64.  When this was written the measured values were: normals 4.2e-6 (per component, pixels valid in
# both; no pixel was valid on one side only), sums 1.85e-6 (each of the 29 sums over the sum of its terms' magnitudes, strides 1 and
# 2), pose 9.4e-8 m and 7.1e-8 rad after five stride-1 steps.
F32_VS_F64_NORMAL = 5.0e-6
F32_VS_F64_SUMS = 2.5e-6
F32_VS_F64_POSE_M = 1.2e-7
F32_VS_F64_POSE_RAD = 1.0e-7
KERNEL_TOL_NORMAL = 8 * F32_VS_F64_NORMAL
KERNEL_TOL_SUMS = 8 * F32_VS_F64_SUMS
KERNEL_TOL_POSE_M = 8 * F32_VS_F64_POSE_M
KERNEL_TOL_POSE_RAD = 8 * F32_VS_F64_POSE_RAD

# ---- the issue's test scene: three corner-facing poses of the mini scene, three guesses each
POSES = (((0.2, 0.2, 0.2), 0.75, -0.6), ((-0.2, 0.25, 0.2), -0.8, -0.65), ((0.0, 0.0, 0.0), 0.78, -0.62))
TWIST = (0.02, -0.015, 0.01, 0.015, -0.01, 0.02)
SCALES = (1.0, 0.5, -1.0)


def intrinsics(fx, fy, cx, cy, dtype):
    return tuple(dtype(np.float32(x)) for x in (fx, fy, cx, cy))


def depth_ok(d):
    return np.isfinite(d) & (d > 0)


def vertices(depth, fx, fy, cx, cy, dtype):
    """[H,W] -> [H,W,3]: ((u - cx) / fx d, -(v - cy) / fy d, -d)"""
    fx, fy, cx, cy = intrinsics(fx, fy, cx, cy, dtype)
    H, W = depth.shape
    d = depth.astype(dtype)
    u = np.arange(W, dtype=dtype)[None, :]
    v = np.arange(H, dtype=dtype)[:, None]
    return np.stack([((u - cx) / fx) * d, (-(v - cy) / fy) * d, -d], -1)


def normals(depth, fx, fy, cx, cy, max_jump=0.0, dtype=np.float64):
    """depth [H,W] float32 -> [H,W,3] float32, 0 where invalid"""
    depth = np.asarray(depth, dtype=np.float32)
    H, W = depth.shape
    out = np.zeros((H, W, 3), dtype=np.float32)
    if H < 2 or W < 2:
        return out
    ok = depth_ok(depth)
    d = np.where(ok, depth, np.float32(0)).astype(dtype)
    V = vertices(d, fx, fy, cx, cy, dtype)
    p, pr, pd = V[:-1, :-1], V[:-1, 1:], V[1:, :-1]
    good = ok[:-1, :-1] & ok[:-1, 1:] & ok[1:, :-1]
    if max_jump > 0:
        mj = dtype(np.float32(max_jump))
        good &= (np.abs(d[:-1, 1:] - d[:-1, :-1]) <= mj) & (np.abs(d[1:, :-1] - d[:-1, :-1]) <= mj)
    a, b = pr - p, pd - p
    c = np.stack([b[..., 1] * a[..., 2] - b[..., 2] * a[..., 1], b[..., 2] * a[..., 0] - b[..., 0] * a[..., 2],
                  b[..., 0] * a[..., 1] - b[..., 1] * a[..., 0]], -1)
    ln = np.sqrt((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2])
    good &= ln > 0
    c = c / np.where(ln > 0, ln, dtype(1))[..., None]
    flip = ((c[..., 0] * p[..., 0] + c[..., 1] * p[..., 1]) + c[..., 2] * p[..., 2]) > 0
    c = np.where(flip[..., None], -c, c)
    out[:-1, :-1] = np.where(good[..., None], c, dtype(0)).astype(np.float32)
    return out


def step_sums(depth_s, normals_s, depth_m, normals_m, p_ref, T, fx, fy, cx, cy, stride=1, dist_tol=0.1, cos_tol=0.8, dtype=np.float64):
    """-> (sums [29], scale [29]): the sums of one step in adfp.h's order and, per sum, the sum of its terms' magnitudes."""
    fxd, fyd, cxd, cyd = intrinsics(fx, fy, cx, cy, dtype)
    H, W = depth_s.shape
    T = np.asarray(T).astype(dtype)
    P = np.asarray(p_ref, dtype=np.float32).astype(dtype)
    vs, us = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    vs, us = vs.reshape(-1), us.reshape(-1)
    Ns = np.asarray(normals_s, dtype=np.float32)[vs, us].astype(dtype)
    keep = (Ns != 0).any(-1)
    vs, us, Ns = vs[keep], us[keep], Ns[keep]
    Vs = vertices(np.asarray(depth_s, dtype=np.float32), fx, fy, cx, cy, dtype)[vs, us]
    x = ((T[:3, 0] * Vs[:, 0:1] + T[:3, 1] * Vs[:, 1:2]) + T[:3, 2] * Vs[:, 2:3]) + T[:3, 3]
    nsw = (T[:3, 0] * Ns[:, 0:1] + T[:3, 1] * Ns[:, 1:2]) + T[:3, 2] * Ns[:, 2:3]
    e = x - P[:3, 3]
    xc = (P[0, :3] * e[:, 0:1] + P[1, :3] * e[:, 1:2]) + P[2, :3] * e[:, 2:3]
    z = -xc[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        pu = np.floor((((fxd * xc[:, 0]) / z) + cxd) + dtype(0.5))
        pv = np.floor((((-fyd * xc[:, 1]) / z) + cyd) + dtype(0.5))
    keep = (z > 0) & (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1)
    x, nsw, pu, pv = x[keep], nsw[keep], pu[keep].astype(np.int64), pv[keep].astype(np.int64)
    Nm = np.asarray(normals_m, dtype=np.float32)[pv, pu].astype(dtype)
    keep = (Nm != 0).any(-1)
    x, nsw, pu, pv, Nm = x[keep], nsw[keep], pu[keep], pv[keep], Nm[keep]
    Vm = vertices(np.asarray(depth_m, dtype=np.float32), fx, fy, cx, cy, dtype)[pv, pu]
    m = ((P[:3, 0] * Vm[:, 0:1] + P[:3, 1] * Vm[:, 1:2]) + P[:3, 2] * Vm[:, 2:3]) + P[:3, 3]
    n = (P[:3, 0] * Nm[:, 0:1] + P[:3, 1] * Nm[:, 1:2]) + P[:3, 2] * Nm[:, 2:3]
    g = m - x
    dist = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    cs = (nsw[:, 0] * n[:, 0] + nsw[:, 1] * n[:, 1]) + nsw[:, 2] * n[:, 2]
    keep = (dist <= dtype(dist_tol)) & (cs >= dtype(cos_tol))
    x, n, g = x[keep], n[keep], g[keep]
    r = (n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]
    J = np.concatenate([np.stack([x[:, 1] * n[:, 2] - x[:, 2] * n[:, 1], x[:, 2] * n[:, 0] - x[:, 0] * n[:, 2],
                                  x[:, 0] * n[:, 1] - x[:, 1] * n[:, 0]], -1), n], -1)
    terms = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [J[:, i] * r for i in range(6)] + [r * r, np.ones_like(r)]
    sums = np.array([t.sum(dtype=dtype) for t in terms], dtype=dtype)
    scale = np.array([np.abs(t).sum(dtype=dtype) for t in terms], dtype=dtype)
    return sums, scale


def exp_se3(xi, dtype=np.float64):
    """Exp of the twist (w, t) -> [4,4]"""
    w, t = np.asarray(xi[:3], dtype=dtype), np.asarray(xi[3:], dtype=dtype)
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=dtype)
    I = np.eye(3, dtype=dtype)
    if th < 1e-12:
        R, V = I + K, I + dtype(0.5) * K
    else:
        A = np.sin(th) / th
        B = (dtype(1) - np.cos(th)) / (th * th)
        Cc = (dtype(1) - A) / (th * th)
        R, V = (I + A * K) + B * (K @ K), (I + B * K) + Cc * (K @ K)
    E = np.eye(4, dtype=dtype)
    E[:3, :3], E[:3, 3] = R, V @ t
    return E


def solve(sums, T, min_pivot=1e-6, min_pairs=0.0, dtype=np.float64):
    """-> (T after the step, stats row [pairs, rmse, pivot ratio, |w|, |t|, status])"""
    S = np.asarray(sums, dtype=dtype)
    T = np.asarray(T).astype(dtype)
    pairs = float(S[28])
    rmse = math.sqrt(float(S[27]) / pairs) if pairs > 0 else 0.0
    if pairs < min_pairs:
        return T, np.array([pairs, rmse, 0.0, 0.0, 0.0, FEW_PAIRS])
    A = np.zeros((6, 6), dtype=dtype)
    q = 0
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = S[q]
            q += 1
    b = S[21:27]
    dmax = A.diagonal().max()
    if not dmax > 0:
        return T, np.array([pairs, rmse, 0.0, 0.0, 0.0, DEGENERATE])
    L, D = np.zeros((6, 6), dtype=dtype), np.zeros(6, dtype=dtype)
    rmin = math.inf
    for j in range(6):
        d = A[j, j]
        for k in range(j):
            d = d - (L[j, k] * L[j, k]) * D[k]
        rmin = min(rmin, float(d / dmax))
        if not d > dtype(min_pivot) * dmax:
            return T, np.array([pairs, rmse, rmin, 0.0, 0.0, DEGENERATE])
        D[j] = d
        for i in range(j + 1, 6):
            s = A[i, j]
            for k in range(j):
                s = s - (L[i, k] * L[j, k]) * D[k]
            L[i, j] = s / d
    y, xi = np.zeros(6, dtype=dtype), np.zeros(6, dtype=dtype)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i] / D[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * xi[k]
        xi[i] = s
    wn, tn = float(np.sqrt((xi[:3] * xi[:3]).sum())), float(np.sqrt((xi[3:] * xi[3:]).sum()))
    Tn = exp_se3(xi, dtype) @ T
    Tn[3] = T[3]
    return Tn, np.array([pairs, rmse, rmin, wn, tn, OK])


def camera_tensor(M):
    """common.get_tensor_from_camera on a float32 [4,4] in float64 -> [7] float32 (restated, not imported: the kernel's yardstick)"""
    M = np.asarray(M, dtype=np.float32).astype(np.float64)
    R, t = M[:3, :3].copy(), M[:3, 3]
    nr = np.linalg.norm(R, axis=0)
    R = R / np.where(nr > 0, nr, 1.0)
    if np.linalg.det(R) < 0:
        R = -R
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(1.0 + tr)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        k = int(np.argmax(np.diag(R)))
        a, b = (k + 1) % 3, (k + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[k, k] - R[a, a] - R[b, b])
        v = [0.0, 0.0, 0.0]
        v[k], v[a], v[b] = 0.25 * s, (R[a, k] + R[k, a]) / s, (R[b, k] + R[k, b]) / s
        q = [(R[b, a] - R[a, b]) / s] + v
    q = np.asarray(q)
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    return np.concatenate([q, t]).astype(np.float32)


def pose_error(A, B):
    """(metres, radians) between two camera-to-world matrices"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    D = A[:3, :3] @ B[:3, :3].T
    c = (np.trace(D) - 1.0) * 0.5
    v = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(math.atan2(0.5 * np.linalg.norm(v), c))


def finish(T, guess, status, max_shift=0.5, max_angle=0.5):
    """The gate: -> (c2w_out [4,4] float32, cam_out [7] float32, final status, shift, angle)"""
    guess = np.asarray(guess, dtype=np.float32)
    shift = angle = 0.0
    if status == OK:
        shift, angle = pose_error(T, guess.astype(np.float64))
        if not shift <= max_shift or not angle <= max_angle:
            status = REJECTED
    if status == OK:
        out = np.asarray(T).astype(np.float32)
        out[3] = (0, 0, 0, 1)
    else:
        out = guess.copy()
    return out, camera_tensor(out), status, shift, angle


def refine(depth_s, depth_m, guess, fx, fy, cx, cy, strides=(4, 2, 1), iters=(4, 3, 3), dist_tol=0.1, cos_tol=0.8, min_pivot=1e-6,
           min_pairs=0.05, max_jump=0.0, max_shift=0.5, max_angle=0.5, dtype=np.float64):
    """The whole refinement on the two depth images (the model's raycast from `guess`): -> (c2w_out, cam_out, status, stats rows)."""
    guess = np.asarray(guess, dtype=np.float32)
    H, W = depth_s.shape
    ns = normals(depth_s, fx, fy, cx, cy, max_jump, dtype)
    nm = normals(depth_m, fx, fy, cx, cy, max_jump, dtype)
    T, status, rows = guess.astype(dtype), OK, []
    for stride, n in zip(strides, iters):
        need = float(math.ceil(min_pairs * (-(-H // stride)) * (-(-W // stride))))
        for _ in range(n):
            if status != OK:
                rows.append(np.array([0.0, 0.0, 0.0, 0.0, 0.0, status]))
                continue
            sums, _ = step_sums(depth_s, ns, depth_m, nm, guess, T, fx, fy, cx, cy, stride, dist_tol, cos_tol, dtype)
            T, row = solve(sums, T, min_pivot, need, dtype)
            status = int(row[5])
            rows.append(row)
    out, cam, status, shift, angle = finish(T.astype(np.float64), guess, status, max_shift, max_angle)
    rows.append(np.array([0.0, 0.0, 0.0, angle, shift, status]))
    return out, cam, status, np.stack(rows)


# ---- the test scene ---------------------------------------------------------------------------------------------------------------
def scene_cases(sc):
    """[(true pose [4,4] float32, guess [4,4] float32)] x 9: Exp(s TWIST) P for the three poses and three scales"""
    out = []
    for offset, yaw, pitch in POSES:
        P = sc.default_c2w(offset=offset, yaw=yaw, pitch=pitch).numpy().astype(np.float64)
        for s in SCALES:
            G = exp_se3(np.asarray(TWIST) * s) @ P
            out.append((P.astype(np.float32), G.astype(np.float32)))
    return out


def cpu_raycast(sc, c2w):
    """The TSDF raycast at a pose with the CPU restatement (tests/tsdfcast_ref.py) -> [H,W] float32 numpy"""
    import tsdfcast_ref
    d = tsdfcast_ref.raycast(sc.tsdf_volume, sc.tsdf_bnds, torch.as_tensor(np.asarray(c2w, dtype=np.float32)), sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy)
    return d.numpy()
