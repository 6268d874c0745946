"""CPU oracle of mesh depth rendering and calc_2d_metric (numpy on the host), restating include/adfp.h's "mesh depth rendering"
contract and what the reference's src/tools/eval_recon.py:139-219 computes through open3d and trimesh:

  * render_depth: the watertight ray/triangle test in f64, per pixel and brute force over all faces, in the kernel's order of
    operations (chunked over faces and pixels);
  * check_proj: eval_recon.py:70-96's test in f32 numpy, in k_cull_seen's order of operations;
  * volume_rectangular: trimesh.sample.volume_rectangular as recon_eval restates it (the golden stub uses this one too);
  * sample_views: the reference's sequential rejection loop over the same streams;
  * depth_l1: the per-view sums of |a - b| and the printed number.
"""
import random

import numpy as np

UP = [0, 0, -1]


def render_depth(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far, face_chunk=512, pix_chunk=8192):
    """f32 [H,W]: the least camera z of a hit with near <= z <= far, 0 where there is none.  c2w: 4x4 or 3x4 (OpenCV axes)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = np.asarray(c2w, np.float64)
    R, o = m[:3, :3], m[:3, 3]
    nv = len(v)
    ok = ((f >= 0) & (f < nv)).all(1)
    f = f[ok]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dxa = ((jj - cx) / fx).reshape(-1)
    dya = ((ii - cy) / fy).reshape(-1)
    out = np.zeros(H * W, np.float64)
    # camera-space vertices: e = v - o, cam_c = ((R0c e0 + R1c e1) + R2c e2), once per vertex (the kernel's per-lane arithmetic)
    e = v - o
    cam = np.stack([(R[0, c] * e[:, 0] + R[1, c] * e[:, 1]) + R[2, c] * e[:, 2] for c in range(3)], 1)
    for p0 in range(0, H * W, pix_chunk):
        dx, dy = dxa[p0:p0 + pix_chunk, None], dya[p0:p0 + pix_chunk, None]
        best = np.full(dx.shape[0], far, np.float64)
        found = np.zeros(dx.shape[0], bool)
        for f0 in range(0, len(f), face_chunk):
            ff = f[f0:f0 + face_chunk]
            A, B, C = cam[ff[:, 0]], cam[ff[:, 1]], cam[ff[:, 2]]
            Ax, Ay = A[:, 0] - dx * A[:, 2], A[:, 1] - dy * A[:, 2]
            Bx, By = B[:, 0] - dx * B[:, 2], B[:, 1] - dy * B[:, 2]
            Cx, Cy = C[:, 0] - dx * C[:, 2], C[:, 1] - dy * C[:, 2]
            U = Cx * By - Cy * Bx
            V = Ax * Cy - Ay * Cx
            Wf = Bx * Ay - By * Ax
            mixed = ((U < 0) | (V < 0) | (Wf < 0)) & ((U > 0) | (V > 0) | (Wf > 0))
            det = (U + V) + Wf
            hit = ~mixed & (det != 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                z = ((U * A[:, 2] + V * B[:, 2]) + Wf * C[:, 2]) / det
            z = np.where(hit & (z >= near) & (z <= far), z, np.inf)
            zm = z.min(1)
            better = zm <= best
            found |= better
            best = np.where(better, zm, best)
        out[p0:p0 + pix_chunk] = np.where(found, best, 0.0)
    return out.astype(np.float32).reshape(H, W)


def check_proj(points, W, H, fx, fy, cx, cy, c2w):
    """eval_recon.py:70-96 in f32: the top rows of inv(c2w') (c2w' = c2w with columns 1, 2 negated; inverted in f64, rounded to
    f32), each point rounded to f32, then k_cull_seen's arithmetic.  True iff some point lands in the image."""
    m = np.array(c2w, np.float64, copy=True)
    m[:3, 1] *= -1.0
    m[:3, 2] *= -1.0
    w = np.linalg.inv(m)[:3, :4].astype(np.float32).reshape(-1)
    p = np.asarray(points, np.float64).reshape(-1, 3).astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    f32 = np.float32
    X = -(((w[0] * x + w[1] * y) + w[2] * z) + w[3])
    Y = ((w[4] * x + w[5] * y) + w[6] * z) + w[7]
    Z = ((w[8] * x + w[9] * y) + w[10] * z) + w[11]
    zz = Z + f32(1e-5)
    u = (f32(fx) * X + f32(cx) * Z) / zz
    v = (f32(fy) * Y + f32(cy) * Z) / zz
    mask = (f32(0) <= -zz) & (u < f32(W)) & (u > f32(0)) & (v < f32(H)) & (v > f32(0))
    return bool(mask.any())


def apply_transform(pts, T):
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def volume_rectangular(extents, count, transform=None):
    """(np.random.random((count, 3)) - 0.5) * extents, moved by transform as ((T00 x + T01 y) + T02 z) + T03."""
    s = (np.random.random((count, 3)) - 0.5) * np.asarray(extents, np.float64)
    return s if transform is None else apply_transform(s, np.asarray(transform, np.float64))


def viewmatrix(z, up, pos):
    zz = z / np.linalg.norm(z)
    xx = np.cross(up, zz)
    xx = xx / np.linalg.norm(xx)
    yy = np.cross(zz, xx)
    yy = yy / np.linalg.norm(yy)
    return np.stack([xx, yy, zz, pos], 1)


def sample_views(pc_unseen, extents, transform, n_imgs, H=500, W=500, fx=300.0, fy=300.0, cx=249.5, cy=249.5):
    """The reference's sequential loop (eval_recon.py:167-186): per candidate one volume_rectangular draw, three
    round(random.uniform(-1e4, 1e4), 2), viewmatrix, check_proj; a degenerate viewmatrix is rejected.  (c2w list, candidates)."""
    out, n = [], 0
    while len(out) < n_imgs:
        n += 1
        origin = volume_rectangular(extents, 1, transform).reshape(-1)
        target = np.array([round(random.uniform(-10000, +10000), 2) for _ in range(3)]) - np.array(origin)
        with np.errstate(all='ignore'):
            c2w = np.eye(4)
            c2w[:3, :] = viewmatrix(target, UP, origin)
        if np.isfinite(c2w).all() and not check_proj(pc_unseen, W, H, fx, fy, cx, cy, c2w):
            out.append(c2w)
    return out, n


def depth_l1_sums(a, b):
    """Per view: the sum of (f64) |a - b| (the f32 difference) over the image."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a - b).reshape(a.shape[0], -1).astype(np.float64).sum(1)


def depth_l1_cm(per_view_sums, n_pixels):
    return float(np.mean(np.asarray(per_view_sums) / n_pixels) * 100)


def near_of(verts, fraction=0.01):
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    return fraction * float((v.max(0) - v.min(0)).max())


def box_room(lo=(-2.0, -1.5, -1.2), hi=(2.0, 1.5, 1.3), inner=None):
    """(verts, faces): the 12 triangles of an axis-aligned box (walls, floor, ceiling), and optionally a second, smaller box
    `inner` = (lo, hi) standing in it."""
    def box(a, b, base):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        v = np.array([[(a, b)[(k >> 0) & 1][0], (a, b)[(k >> 1) & 1][1], (a, b)[(k >> 2) & 1][2]] for k in range(8)])
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        f = []
        for q in quads:
            f.append((q[0], q[1], q[2]))
            f.append((q[0], q[2], q[3]))
        return v, np.array(f, np.int64) + base
    v, f = box(lo, hi, 0)
    if inner is not None:
        v2, f2 = box(inner[0], inner[1], len(v))
        v, f = np.concatenate([v, v2]), np.concatenate([f, f2])
    return v, f
