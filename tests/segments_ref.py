"""numpy f64 restatement of adfp_draw_segments (include/adfp.h, "mesh views"): a brute force over all pixels and all listed
segments, one correctly rounded f64 operation at a time in the order of the header.  numpy's elementwise ufuncs round each
operation on its own, as the kernels built without contraction do, so the two sides are compared exactly."""
import numpy as np


def listed(ranges, n_seg):
    """The set of segments a view's ranges [R,2] hold, ascending: clamped to [0, n_seg), empty and inverted ranges hold nothing, a
    segment held twice counts once.  ranges None: all."""
    if ranges is None:
        return list(range(n_seg))
    held = set()
    for b, e in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
        held.update(range(max(int(b), 0), min(int(e), n_seg)))
    return sorted(held)


def n_listed(ranges, n_seg):
    """The largest sum over a view's ranges [P,R,2] of their clamped lengths."""
    r = np.asarray(ranges, dtype=np.int64)
    return int(np.clip(np.minimum(r[..., 1], n_seg) - np.maximum(r[..., 0], 0), 0, None).sum(-1).max())


def to_camera(m, P):
    """m: f64 [12] = the top three rows of c2w; P [3]: e = P - o, cam_c = ((R0c e0 + R1c e1) + R2c e2)."""
    e0, e1, e2 = P[0] - m[3], P[1] - m[7], P[2] - m[11]
    return np.array([(m[c] * e0 + m[4 + c] * e1) + m[8 + c] * e2 for c in range(3)], dtype=np.float64)


def project(m, seg, fx, fy, cx, cy, near_clip):
    """One segment [2,3] in one view: (u0, v0, w0, u1, v1, w1) or None when it draws nothing."""
    seg = np.asarray(seg, dtype=np.float64)
    if not np.isfinite(seg).all():
        return None
    with np.errstate(all='ignore'):
        A, B = to_camera(m, seg[0]), to_camera(m, seg[1])
        if A[2] < near_clip and B[2] < near_clip:
            return None
        if A[2] < near_clip:
            t = (near_clip - A[2]) / (B[2] - A[2])
            A = np.array([A[0] + t * (B[0] - A[0]), A[1] + t * (B[1] - A[1]), near_clip])
        elif B[2] < near_clip:
            t = (near_clip - B[2]) / (A[2] - B[2])
            B = np.array([B[0] + t * (A[0] - B[0]), B[1] + t * (A[1] - B[1]), near_clip])
        out = []
        for E in (A, B):
            out += [fx * (E[0] / E[2]) + cx, fy * (E[1] / E[2]) + cy, 1.0 / E[2]]
    out = np.array(out, dtype=np.float64)
    return out if np.isfinite(out).all() else None


def cover(rec, H, W, half_width):
    """(covered bool [M,H,W], z f64 [M,H,W]) of projected records [M,6] (or one record [6]: [H,W] each) over all pixels."""
    rec = np.asarray(rec, dtype=np.float64)
    single = rec.ndim == 1
    r = rec.reshape(-1, 6)
    u0, v0, w0, u1, v1, w1 = (r[:, c][:, None, None] for c in range(6))
    j = np.arange(W, dtype=np.float64)[None, None, :]
    i = np.arange(H, dtype=np.float64)[None, :, None]
    half_width = np.float64(half_width)
    with np.errstate(all='ignore'):
        ax, ay, dw = u1 - u0, v1 - v0, w1 - w0
        L = ax * ax + ay * ay
        px, py = j - u0, i - v0
        s = np.where(L == 0.0, 0.0, (px * ax + py * ay) / L)
        s = np.where(s > 0.0, s, 0.0)
        s = np.where(s > 1.0, 1.0, s)
        qx, qy = px - s * ax, py - s * ay
        covered = qx * qx + qy * qy <= half_width * half_width
        z = 1.0 / (w0 + s * dw)
    covered, z = np.broadcast_to(covered, (len(r), H, W)), np.broadcast_to(z, (len(r), H, W))
    return (covered[0], z[0]) if single else (covered, z)


def winners(c2w, H, W, fx, fy, cx, cy, segments, ranges=None, half_width=1.0, near_clip=1e-3):
    """(seg int32 [P,H,W], z f64 [P,H,W]): per pixel the listed covering segment of least z, the smallest index among equal z; -1
    and inf where there is none or the view's pose is not finite."""
    c2w = np.asarray(c2w, dtype=np.float64).reshape(-1, 4, 4)
    segments = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 3)
    P, N = len(c2w), len(segments)
    fx, fy, cx, cy, near_clip = (np.float64(x) for x in (fx, fy, cx, cy, near_clip))
    seg = np.full((P, H, W), -1, dtype=np.int32)
    zz = np.full((P, H, W), np.inf)
    for p in range(P):
        m = c2w[p, :3, :].reshape(12)
        if not np.isfinite(m).all():
            continue
        ks, recs = [], []
        for k in listed(None if ranges is None else ranges[p], N):           # ascending
            rec = project(m, segments[k], fx, fy, cx, cy, near_clip)
            if rec is not None:
                ks.append(k)
                recs.append(rec)
        if not ks:
            continue
        covered, z = cover(np.array(recs), H, W, half_width)
        zc = np.where(covered, z, np.inf)
        best = zc.min(0)
        first = (covered & (z == best[None])).argmax(0)                      # the first of the ascending list: the smallest index
        won = covered.any(0)
        seg[p] = np.where(won, np.array(ks)[first], -1)
        zz[p] = np.where(won, best, np.inf)
    return seg, zz


def paint(rgb, depth, seg, z, colors, bias_rel=0.0, bias_abs=0.0, hidden_alpha=0.0):
    """The painted copy of rgb uint8 [P,H,W,3] for winners (seg, z); depth f32 [P,H,W] or None."""
    rgb = np.array(rgb, dtype=np.uint8, copy=True)
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    won = seg >= 0
    if not won.any():
        return rgb
    if depth is None:
        visible = won
    else:
        D = np.asarray(depth, dtype=np.float32).astype(np.float64)
        with np.errstate(all='ignore'):
            visible = won & ((D == 0.0) | (z <= D * (1.0 + np.float64(bias_rel)) + np.float64(bias_abs)))
    hidden = won & ~visible
    col = colors[np.where(won, seg, 0)]
    a = np.float64(hidden_alpha)
    blend = np.floor((a * col.astype(np.float64) + (1.0 - a) * rgb.astype(np.float64)) + 0.5).astype(np.uint8)
    out = np.where(visible[..., None], col, rgb)
    if a > 0.0:
        out = np.where(hidden[..., None], blend, out)
    return out


def draw_segments(rgb, depth, c2w, fx, fy, cx, cy, segments, colors, ranges=None, half_width=1.0, near_clip=1e-3, bias_rel=0.0,
                  bias_abs=0.0, hidden_alpha=0.0):
    """rgb uint8 [P,H,W,3] (not modified), depth f32 [P,H,W] or None, c2w [P,4,4], segments [N,2,3], colors uint8 [N,3], ranges
    [P,R,2] or None -> (the painted copy of rgb, seg int32 [P,H,W])."""
    P, H, W = np.asarray(rgb).shape[:3]
    seg, z = winners(np.asarray(c2w, dtype=np.float64).reshape(P, 4, 4), H, W, fx, fy, cx, cy, segments, ranges, half_width, near_clip)
    return paint(rgb, depth, seg, z, colors, bias_rel, bias_abs, hidden_alpha), seg
