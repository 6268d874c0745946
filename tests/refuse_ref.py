"""CPU oracle of ScanNet mesh evaluation (numpy on the host), restating include/adfp.h's "ScanNet mesh evaluation" contracts and the
culled depth render:

  * render_depth_cull: depth_ref's brute-force watertight test with a cull mode (det > 0: front face);
  * touch: the unit touch marks of every stride-th pixel, in f64;
  * integrate: the unit-gated f32 integration, view by view, over every voxel of the box;
  * extract: open3d-style extraction -- its own loop over the cubes whose 8 corners are all observed (weight > 0), a vertex on each
    crossed edge (tsdf < 0 at exactly one end), Bourke-style; positions in the marching-cubes kernel's f32 arithmetic;
  * voxel_down_sample: open3d's voxel_down_sample as we read it, in ascending key order, sums in input order;
  * refuse / evaluate: the pipeline of evaluate_scannet.py on top of these, with scipy's cKDTree for the distances.
"""
import numpy as np

import depth_ref

f32 = np.float32
UNIT = 16
CULL = {'none': 0, 'back': 1, 'front': 2}


def render_depth_cull(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far, cull='none', face_chunk=512, pix_chunk=8192):
    """f32 [H,W]: depth_ref.render_depth keeping only front (det > 0, cull='back') or back (det < 0, cull='front') hits; a pose
    with a non-finite entry renders zeros in the culled modes."""
    m = np.asarray(c2w, np.float64)
    if cull == 'none':
        return depth_ref.render_depth(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far, face_chunk, pix_chunk)
    if not np.isfinite(m[:3, :4]).all():
        return np.zeros((H, W), np.float32)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    R, o = m[:3, :3], m[:3, 3]
    f = f[((f >= 0) & (f < len(v))).all(1)]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dxa = ((jj - cx) / fx).reshape(-1)
    dya = ((ii - cy) / fy).reshape(-1)
    out = np.zeros(H * W, np.float64)
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
            hit = ~mixed & (det != 0) & ((det > 0) if cull == 'back' else (det < 0))
            with np.errstate(divide='ignore', invalid='ignore'):
                z = ((U * A[:, 2] + V * B[:, 2]) + Wf * C[:, 2]) / det
            z = np.where(hit & (z >= near) & (z <= far), z, np.inf)
            zm = z.min(1)
            better = zm <= best
            found |= better
            best = np.where(better, zm, best)
        out[p0:p0 + pix_chunk] = np.where(found, best, 0.0)
    return out.astype(np.float32).reshape(H, W)


def touch(depth, c2w_rows, fx, fy, cx, cy, stride, depth_trunc, sdf_trunc, unit_length, lo, dim):
    """(touched uint8 [P, units], outside count): adfp_refuse_touch."""
    depth = np.asarray(depth, np.float32)
    P, H, W = depth.shape
    lo, dim = np.asarray(lo, np.int64), np.asarray(dim, np.int64)
    out = np.zeros((P, int(np.prod(dim))), np.uint8)
    outside = 0
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    for p in range(P):
        d32 = depth[p][vv, uu]
        ok = (d32 > 0) & (d32 <= f32(depth_trunc))
        d = d32[ok].astype(np.float64)
        u, v = uu[ok].astype(np.float64), vv[ok].astype(np.float64)
        x = ((u - cx) * d) / fx
        y = ((v - cy) * d) / fy
        m = np.asarray(c2w_rows[p], np.float64).reshape(3, 4)
        with np.errstate(all='ignore'):
            q = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * d) + m[r, 3] for r in range(3)], 1)
            f0 = np.floor((q - sdf_trunc) / unit_length)
            f1 = np.floor((q + sdf_trunc) / unit_length)
        fin = np.isfinite(f0).all(1) & np.isfinite(f1).all(1)
        f0, f1 = f0[fin], f1[fin]
        hi = lo + dim - 1
        outside += int(((f0 < lo) | (f1 > hi)).any(1).sum())
        a0 = np.clip(f0, lo, hi + 1).astype(np.int64) - lo
        a1 = np.clip(f1, lo - 1, hi).astype(np.int64) - lo
        for k in range(len(a0)):
            for ix in range(a0[k, 0], a1[k, 0] + 1):
                for iy in range(a0[k, 1], a1[k, 1] + 1):
                    for iz in range(a0[k, 2], a1[k, 2] + 1):
                        out[p, (ix * dim[1] + iy) * dim[2] + iz] = 1
    return out, outside


def voxel_centres(lo, dim, voxel):
    """f32 coordinate axes of the box's voxel centres: (k + 0.5) voxel in f64, rounded."""
    return [((np.arange(UNIT * dim[c], dtype=np.int64) + UNIT * lo[c]).astype(np.float64) + 0.5) * voxel for c in range(3)]


def integrate(tsdf, weight, lo, dim, voxel, depth, w2c, touched, fx, fy, cx, cy, sdf_trunc, depth_trunc):
    """In place on f32 [nx,ny,nz] tsdf and weight: adfp_refuse_integrate over every unit, views in order."""
    depth = np.asarray(depth, np.float32)
    P, H, W = depth.shape
    ax = [a.astype(np.float32) for a in voxel_centres(lo, dim, voxel)]
    X, Y, Z = np.meshgrid(ax[0], ax[1], ax[2], indexing='ij')
    nx, ny, nz = (UNIT * d for d in dim)
    ux = (np.arange(nx) // UNIT)[:, None, None]
    uy = (np.arange(ny) // UNIT)[None, :, None]
    uz = (np.arange(nz) // UNIT)[None, None, :]
    unit_id = (ux * dim[1] + uy) * dim[2] + uz
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    trunc, inv = f32(sdf_trunc), f32(1) / f32(sdf_trunc)
    dt = f32(depth_trunc)
    sw, sh = f32(W) - f32(0.0001), f32(H) - f32(0.0001)
    for k in range(P):
        m = np.asarray(w2c[k], np.float32).reshape(12)
        gate = touched[k][unit_id] != 0
        with np.errstate(all='ignore'):
            cz = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            cxx = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            cyy = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            uf = ((cxx * fx) / cz + cx) + f32(0.5)
            vf = ((cyy * fy) / cz + cy) + f32(0.5)
            ok = gate & (cz > 0) & (uf >= f32(0.0001)) & (uf < sw) & (vf >= f32(0.0001)) & (vf < sh)
        u = np.where(ok, uf, 0).astype(np.int64)
        v = np.where(ok, vf, 0).astype(np.int64)
        d = depth[k][v, u]
        ok &= (d > 0) & (d <= dt)
        du = (u.astype(np.float32) - cx) / fx
        dv = (v.astype(np.float32) - cy) / fy
        with np.errstate(all='ignore'):
            sdf = (d - cz) * np.sqrt((du * du + dv * dv) + f32(1))
        ok &= sdf > -trunc
        t = np.minimum(f32(1), sdf * inv)
        w = weight[ok]
        tsdf[ok] = (tsdf[ok] * w + t[ok]) / (w + f32(1))
        weight[ok] = w + f32(1)


# the 12 cube edges as (corner offset (di, dj, dk), axis)
EDGES = [((0, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0), ((0, 1, 1), 0),
         ((0, 0, 0), 1), ((1, 0, 0), 1), ((0, 0, 1), 1), ((1, 0, 1), 1),
         ((0, 0, 0), 2), ((1, 0, 0), 2), ((0, 1, 0), 2), ((1, 1, 0), 2)]


def extract_vertices(tsdf, weight, lo, voxel):
    """f32 [V,3]: one vertex per lattice edge that is crossed (tsdf < 0 at exactly one end) and belongs to some cube whose 8
    corners all have weight > 0; at t = tsdf0 / (tsdf0 - tsdf1) from the lower end, org + (i + t) spacing in f32, org = the first
    voxel's centre.  Sorted by edge key (3 p + axis, p the lower end's linear index)."""
    nx, ny, nz = tsdf.shape
    obs = weight > 0
    cube = obs[:-1, :-1, :-1].copy()
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                cube &= obs[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]
    inside = tsdf < 0
    keys = set()
    ci, cj, ck = np.nonzero(cube)
    for (o, a) in EDGES:
        i, j, k = ci + o[0], cj + o[1], ck + o[2]
        i1, j1, k1 = i + (a == 0), j + (a == 1), k + (a == 2)
        crossed = inside[i, j, k] != inside[i1, j1, k1]
        p = (i[crossed] * ny + j[crossed]) * nz + k[crossed]
        keys.update((3 * p + a).tolist())
    keys = np.array(sorted(keys), np.int64)
    a = keys % 3
    p = keys // 3
    ijk = np.stack([p // (ny * nz), (p // nz) % ny, p % nz], 1)
    step = np.array([ny * nz, nz, 1])[a]
    v0 = -tsdf.reshape(-1)[p]
    v1 = -tsdf.reshape(-1)[p + step]
    t = (f32(0) - v0) / (v1 - v0)
    org = np.array([(UNIT * lo[c] + 0.5) * voxel for c in range(3)], np.float32)
    sp = f32(voxel)
    out = np.empty((len(keys), 3), np.float32)
    for b in range(3):
        x = np.where(a == b, ijk[:, b].astype(np.float32) + t, ijk[:, b].astype(np.float32))
        out[:, b] = org[b] + x * sp
    return out


def voxel_down_sample(points, vs):
    """(means f64 [M,3], counts [M]) in ascending cell-key order; each cell's f64 sum in input order over its count."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    vmin = p.min(0) - vs * 0.5
    dims = np.floor((p.max(0) - vmin) / vs).astype(np.int64) + 1
    idx = np.floor((p - vmin) / vs).astype(np.int64)
    key = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    order = np.argsort(key, kind='stable')
    ks = key[order]
    head = np.ones(len(ks), bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.nonzero(head)[0]
    cnt = np.diff(np.append(start, len(ks)))
    s = np.zeros((len(start), 3))
    for j in range(int(cnt.max())):
        live = cnt > j
        s[live] += p[order[start[live] + j]]
    return s / cnt[:, None].astype(np.float64), cnt


def w2c_rows(poses):
    out = np.empty((len(poses), 12), np.float32)
    for k, m in enumerate(poses):
        with np.errstate(all='ignore'):
            try:
                inv = np.linalg.inv(np.asarray(m, np.float32).astype(np.float64))
            except np.linalg.LinAlgError:
                inv = np.full((4, 4), np.nan)
        out[k] = inv[:3, :4].astype(np.float32).reshape(-1)
    return out


def backproject_rows(w2c):
    out = np.empty((len(w2c), 12))
    for k, r in enumerate(w2c):
        m = np.eye(4)
        m[:3, :4] = np.asarray(r, np.float64).reshape(3, 4)
        with np.errstate(all='ignore'):
            try:
                inv = np.linalg.inv(m) if np.isfinite(m).all() else np.full((4, 4), np.nan)
            except np.linalg.LinAlgError:
                inv = np.full((4, 4), np.nan)
        out[k] = inv[:3, :4].reshape(-1)
    return out


def unit_box(verts, voxel, sdf_trunc):
    v = np.asarray(verts, np.float64)
    L = voxel * UNIT
    lo = np.floor((v.min(0) - sdf_trunc) / L).astype(np.int64) - 1
    hi = np.floor((v.max(0) + sdf_trunc) / L).astype(np.int64) + 1
    return lo, hi - lo + 1


def refuse_tsdf(verts, faces, poses, K, H, W, fx, fy, cx, cy, voxel=0.01, sdf_trunc=0.03, depth_trunc=5.0, stride=4, near=0.05,
                shift=0.5):
    """The fused volume of evaluate_scannet.refuse (faces already inverted): (tsdf, weight, lo, dim, depths)."""
    lo, dim = unit_box(verts, voxel, sdf_trunc)
    shape = tuple(UNIT * d for d in dim)
    tsdf, weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    w2c = w2c_rows(poses)
    bp = backproject_rows(w2c)
    depths = np.stack([render_depth_cull(verts, faces, np.asarray(p, np.float64), H, W, K[0][0], K[1][1], K[0][2] - shift,
                                         K[1][2] - shift, near, depth_trunc, 'back') for p in poses])
    touched, outside = touch(depths, bp, fx, fy, cx, cy, stride, depth_trunc, sdf_trunc, voxel * UNIT, lo, dim)
    assert outside == 0
    integrate(tsdf, weight, lo, dim, voxel, depths, w2c, touched, fx, fy, cx, cy, sdf_trunc, depth_trunc)
    return tsdf, weight, lo, dim, depths


def evaluate(pred, trgt, threshold=.05, down_sample=.02):
    """The reference's metrics with cKDTree distances over the (downsampled) vertex sets."""
    from scipy.spatial import cKDTree
    if down_sample:
        pred, _ = voxel_down_sample(pred, down_sample)
        trgt, _ = voxel_down_sample(trgt, down_sample)
    dist1 = cKDTree(pred).query(trgt)[0]
    dist2 = cKDTree(trgt).query(pred)[0]
    precision = np.mean((dist2 < threshold).astype('float'))
    recal = np.mean((dist1 < threshold).astype('float'))
    return {'Acc': np.mean(dist2), 'Comp': np.mean(dist1), 'Chamfer': (np.mean(dist1) + np.mean(dist2)) / 2, 'Prec': precision,
            'Recal': recal, 'F-score': 2 * precision * recal / (precision + recal)}


# ---- synthetic ScanNet-like scenes ----
def grid_box(lo, hi, step, toward_inside):
    """(verts, faces) of an axis-aligned box surface split into a grid of about `step` per cell, two triangles per cell.  Every
    face's normal (v1 - v0) x (v2 - v0) points into the box when toward_inside, else out of it."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre = (lo + hi) / 2
    V, F = [], []
    base = 0
    for axis in range(3):
        a, b = [c for c in range(3) if c != axis]
        na = max(1, int(round((hi[a] - lo[a]) / step)))
        nb = max(1, int(round((hi[b] - lo[b]) / step)))
        sa = np.linspace(lo[a], hi[a], na + 1)
        sb = np.linspace(lo[b], hi[b], nb + 1)
        for side in (lo[axis], hi[axis]):
            A, B = np.meshgrid(sa, sb, indexing='ij')
            pts = np.zeros((A.size, 3))
            pts[:, axis], pts[:, a], pts[:, b] = side, A.reshape(-1), B.reshape(-1)
            idx = np.arange(A.size).reshape(na + 1, nb + 1) + base
            q0, q1, q2, q3 = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
            f = np.concatenate([np.stack([q0, q1, q2], 1), np.stack([q0, q2, q3], 1)])
            n = np.cross(pts[f[:, 1] - base] - pts[f[:, 0] - base], pts[f[:, 2] - base] - pts[f[:, 0] - base])
            out = (side - centre[axis]) * n[:, axis] > 0
            flip = out if toward_inside else ~out
            f[flip] = f[flip][:, ::-1]
            V.append(pts)
            F.append(f)
            base += len(pts)
    return np.concatenate(V), np.concatenate(F)


def scene(step=0.05, shift=(0.0, 0.0, 0.0), size=(1.6, 1.2, 1.0), crate=((0.25, -0.45, -0.5), (0.65, -0.05, -0.1))):
    """(verts, faces): a room of `size` centred at the origin with a crate on its floor, wound as the reference's predicted meshes
    are before mesh.invert(): every normal points away from the free space the cameras stand in.  `shift` moves the walls' lower
    corner and the crate (a prediction a few cm off)."""
    s = np.asarray(size) / 2
    sh = np.asarray(shift, np.float64)
    rv, rf = grid_box(-s + sh, s, step, toward_inside=False)
    cv, cf = grid_box(np.asarray(crate[0]) + sh, np.asarray(crate[1]) + sh, step, toward_inside=True)
    return np.concatenate([rv, cv]), np.concatenate([rf, cf + len(rv)])


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4x4 OpenCV camera-to-world (x right, y down, z forward) at eye looking at target."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def orbit_poses(n, radius=0.35, height=0.1, seed=0):
    """n cameras on a ring inside the room, looking outward at the walls and down toward the floor, slightly jittered."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n + rng.uniform(-0.1, 0.1)
        eye = np.array([radius * np.cos(a), radius * np.sin(a), height + rng.uniform(-0.05, 0.05)])
        tgt = eye + np.array([np.cos(a + 0.4), np.sin(a + 0.4), rng.uniform(-0.6, 0.1)])
        out.append(look_at(eye, tgt))
    return out
