"""CPU oracle of the mesh views (numpy on the host), restating include/adfp.h's "mesh views" contracts brute force:

  * render_hits: depth_ref.render_depth's watertight test over all faces, keeping the nearest hit's original face index (the
    smallest among hits whose f64 z are equal) and (V / det, W / det), for the three cull modes in one pass;
  * vertex_normals: unnormalised face normals summed per vertex over its face corners in ascending face index, then normalised;
  * shade: the shading pass, operation for operation, and the mask of channels whose value before rounding lies within 1e-6 of a
    half-integer.

Every operation is a single correctly rounded f64 operation of numpy's (+, -, *, /, sqrt), in the order the header writes them.
"""
import functools

import numpy as np

CULLS = ('none', 'back', 'front')
MODES = ('color', 'shaded', 'normal')


def render_hits(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far, face_chunk=512, pix_chunk=4096):
    """{cull: (depth f32 [H,W], face int32 [H,W], bary f32 [H,W,2])} for cull in CULLS.  c2w: 4x4 or 3x4 (OpenCV axes)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = np.asarray(c2w, np.float64)
    R, o = m[:3, :3], m[:3, 3]
    rows = np.flatnonzero(((f >= 0) & (f < len(v))).all(1))          # ascending: the first of equal minima is the smallest index
    f = f[rows]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dxa = ((jj - cx) / fx).reshape(-1)
    dya = ((ii - cy) / fy).reshape(-1)
    n = H * W
    best = {c: np.full(n, np.inf) for c in CULLS}
    face = {c: np.full(n, -1, np.int64) for c in CULLS}
    bary = {c: np.zeros((n, 2)) for c in CULLS}
    with np.errstate(all='ignore'):
        e = v - o
        cam = np.stack([(R[0, c] * e[:, 0] + R[1, c] * e[:, 1]) + R[2, c] * e[:, 2] for c in range(3)], 1)
        for p0 in range(0, n, pix_chunk):
            sl = slice(p0, p0 + pix_chunk)
            dx, dy = dxa[sl, None], dya[sl, None]
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
                z = ((U * A[:, 2] + V * B[:, 2]) + Wf * C[:, 2]) / det
                hit = ~mixed & (det != 0) & (z >= near) & (z <= far)
                for c in CULLS:
                    h = hit if c == 'none' else hit & ((det > 0) if c == 'back' else (det < 0))
                    zc = np.where(h, z, np.inf)
                    arg = zc.argmin(1)[:, None]
                    zm = np.take_along_axis(zc, arg, 1)[:, 0]
                    better = zm < best[c][sl]                         # strictly: an equal z in a later chunk has a larger index
                    if not better.any():
                        continue
                    d = np.take_along_axis(det, arg, 1)[:, 0]
                    b = np.stack([np.take_along_axis(V, arg, 1)[:, 0] / d, np.take_along_axis(Wf, arg, 1)[:, 0] / d], 1)
                    best[c][sl] = np.where(better, zm, best[c][sl])
                    face[c][sl] = np.where(better, rows[f0 + arg[:, 0]], face[c][sl])
                    bary[c][sl] = np.where(better[:, None], b, bary[c][sl])
    out = {}
    for c in CULLS:
        found = face[c] >= 0
        if c != 'none' and not np.isfinite(m[:3, :4]).all():         # the culled modes: no view through a non-finite pose
            found = np.zeros(n, bool)
        out[c] = (np.where(found, best[c], 0.0).astype(np.float32).reshape(H, W),
                  np.where(found, face[c], -1).astype(np.int32).reshape(H, W),
                  np.where(found[:, None], bary[c], 0.0).astype(np.float32).reshape(H, W, 2))
    return out


def face_normals(verts, faces):
    """(g f64 [F,3], ok bool [F]): (v1 - v0) x (v2 - v0) per face, zeros for a face with an index outside [0, V)."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1) if len(v) else np.zeros(len(f), bool)
    fs = np.where(ok[:, None], f, 0)
    g = np.zeros((len(f), 3))
    if len(v) and len(f):
        with np.errstate(all='ignore'):
            e1, e2 = v[fs[:, 1]] - v[fs[:, 0]], v[fs[:, 2]] - v[fs[:, 0]]
            g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        g[~ok] = 0.0
    return g, ok


def vertex_normals(verts, faces):
    """f64 [V,3]: per vertex the sum of its incident corners' face normals in ascending face index, over its length; zeros where
    the length is 0 or not finite."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    g, ok = face_normals(v, f)
    s = np.zeros((len(v), 3))
    with np.errstate(all='ignore'):
        for i in np.flatnonzero(ok):                                # a Python loop: the order of the additions is the contract
            for c in range(3):
                s[f[i, c]] += g[i]
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        good = (ln > 0) & np.isfinite(ln)
        return np.where(good[:, None], s / np.where(good, ln, 1.0)[:, None], 0.0)


def shade(face, bary, verts, faces, c2w, fx, fy, cx, cy, normals=None, colors=None, mode='shaded', ambient=0.3,
          albedo=(0.8, 0.8, 0.8), background=(255, 255, 255)):
    """(normal f32 [H,W,3], rgb u8 [H,W,3], unsure bool [H,W,3]) of one view: face int [H,W], bary f32 [H,W,2].  unsure: a hit
    pixel's channel whose clamped value times 255 lies within 1e-6 of a half-integer."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    m = np.asarray(c2w, np.float64)
    R = m[:3, :3]
    fi = np.asarray(face, np.int64)
    H, W = fi.shape
    g_all, ok = face_normals(v, f)
    safe = np.where((fi >= 0) & (fi < len(f)), fi, 0)
    hit = (fi >= 0) & (fi < len(f)) & (ok[safe] if len(f) else False)
    safe = np.where(hit, safe, 0)
    ids = f[safe] if len(f) else np.zeros((H, W, 3), np.int64)
    ids = np.where(hit[..., None], ids, 0)
    b = np.asarray(bary, np.float32).astype(np.float64)
    b1, b2 = b[..., 0], b[..., 1]
    b0 = (1.0 - b1) - b2
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dx, dy = (jj - cx) / fx, (ii - cy) / fy
    with np.errstate(all='ignore'):
        n = g_all[safe] if len(f) else np.zeros((H, W, 3))
        if normals is not None and len(v):
            vn = np.asarray(normals, np.float64).reshape(-1, 3)
            s = (b0[..., None] * vn[ids[..., 0]] + b1[..., None] * vn[ids[..., 1]]) + b2[..., None] * vn[ids[..., 2]]
            n = np.where((s == 0).all(-1)[..., None], n, s)
        mc = np.stack([(R[0, c] * n[..., 0] + R[1, c] * n[..., 1]) + R[2, c] * n[..., 2] for c in range(3)], -1)
        ln = np.sqrt((mc[..., 0] * mc[..., 0] + mc[..., 1] * mc[..., 1]) + mc[..., 2] * mc[..., 2])
        good = (ln > 0) & np.isfinite(ln)
        mc = np.where(good[..., None], mc / np.where(good, ln, 1.0)[..., None], 0.0)
        t = (mc[..., 0] * dx + mc[..., 1] * dy) + mc[..., 2]
        flip = t > 0
        mc = np.where(flip[..., None], -mc, mc)
        t = np.where(flip, -t, t)
        normal = np.where(hit[..., None], mc, 0.0).astype(np.float32)
        if mode == 'normal':
            x = np.stack([(mc[..., 0] + 1.0) / 2.0, (-mc[..., 1] + 1.0) / 2.0, (-mc[..., 2] + 1.0) / 2.0], -1)
        else:
            if colors is not None and len(v):
                vc = np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.float64)
                x = ((b0[..., None] * vc[ids[..., 0]] + b1[..., None] * vc[ids[..., 1]]) + b2[..., None] * vc[ids[..., 2]]) / 255.0
            else:
                x = np.broadcast_to(np.asarray(albedo, np.float32).astype(np.float64), (H, W, 3))
            if mode == 'shaded':
                inten = ambient + (1.0 - ambient) * (-t / np.sqrt((dx * dx + dy * dy) + 1.0))
                x = x * inten[..., None]
        y = np.where(x > 0, x, 0.0)
        y = np.where(y < 1, y, 1.0)
        y255 = y * 255.0
        rgb = np.floor(y255 + 0.5).astype(np.uint8)
    rgb = np.where(hit[..., None], rgb, np.asarray(background, np.uint8))
    frac = y255 - np.floor(y255)
    unsure = hit[..., None] & (np.abs(frac - 0.5) <= 1e-6)
    return normal, rgb.astype(np.uint8), unsure


@functools.lru_cache(maxsize=None)
def soup_hits(name, v):
    """render_hits of soup `name` from View v of tests/soup_meshes.py, computed once per process, read-only."""
    import soup_meshes as S
    verts, faces = S.mesh(name)
    out = render_hits(verts, faces, S.c2w_of(v), *S.camera(v))
    return {c: tuple(S.frozen(a) for a in t) for c, t in out.items()}
