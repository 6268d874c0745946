"""The numpy statement of adfp_mesh_project_colors' rule (include/adfp.h, "mesh colours from the keyframes"), in f32 -- every
product and sum rounded on its own, as the kernel forms them -- and in f64, the ambiguity mask that says where two evaluations of
the rule may legitimately decide differently, and the analytic scene the tests share.  No GPU, no package import: a helper
module, not a test file."""
import numpy as np

BLENDS = ('weighted', 'best')


def invert_poses(c2w):
    """(w2c [K,12] f32, center [K,3] f32) of c2w [K,4,4] as Mesher.seen_mask forms them: np.linalg.inv in the pose's own dtype, the
    top three rows, then f32; the centre is c2w[:3, 3]."""
    c2w = np.asarray(c2w)
    K = c2w.shape[0]
    if K == 0:
        return np.zeros((0, 12), np.float32), np.zeros((0, 3), np.float32)
    w2c = np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :]).astype(np.float32).reshape(K, 12)
    return w2c, np.ascontiguousarray(c2w[:, :3, 3]).astype(np.float32)


def _project(T, verts, w, fx, fy, cx, cy):
    """Rule 1 in dtype T: (u, v, Z, zz) of all vertices under one keyframe's w2c (12 values)."""
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    X = -(((w[0] * x + w[1] * y) + w[2] * z) + w[3])
    Y = ((w[4] * x + w[5] * y) + w[6] * z) + w[7]
    Z = ((w[8] * x + w[9] * y) + w[10] * z) + w[11]
    zz = Z + T(1e-8)
    u = (fx * X + cx * Z) / zz
    v = (fy * Y + cy * Z) / zz
    return u, v, Z, zz


def _views(T, verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border):
    """Rules 1-6 for every keyframe in dtype T.  Yields per keyframe a dict of per-vertex arrays: u, v, zz (all vertices), inframe,
    and for the in-frame vertices `idx`: corner depths d [n,4], z, the colour c [n,3], the weight w and contributes."""
    K, H, W = depth.shape
    verts = verts.astype(T)
    normals = None if normals is None else normals.astype(T)
    fx, fy, cx, cy, tol = (T(np.float32(a)) for a in (fx, fy, cx, cy, depth_tol))       # the kernel takes them as f32
    lo, uhi, vhi = T(border), T(W - 1 - border), T(H - 1 - border)
    one, tiny = T(1), T(np.float32(1e-12))
    for k in range(K):
        w = w2c[k].astype(T)
        ctr = center[k].astype(T)
        dk = depth[k].astype(T)
        ck = color[k].astype(T)
        with np.errstate(all='ignore'):
            u, v, Z, zz = _project(T, verts, w, fx, fy, cx, cy)
            inframe = (zz < 0) & (u >= lo) & (u <= uhi) & (v >= lo) & (v <= vhi)          # NaN compares false
        idx = np.nonzero(inframe)[0]
        ui, vi = u[idx], v[idx]
        x0 = np.minimum(np.floor(ui).astype(np.int64), W - 2)
        y0 = np.minimum(np.floor(vi).astype(np.int64), H - 2)
        ax, ay, zc = ui - x0.astype(T), vi - y0.astype(T), -Z[idx]
        d = np.stack([dk[y0, x0], dk[y0, x0 + 1], dk[y0 + 1, x0], dk[y0 + 1, x0 + 1]], 1).reshape(-1, 4)
        vis = ((d > 0) & (np.abs(d - zc[:, None]) <= tol)).all(1)
        w00, w01, w10, w11 = (one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay
        c = ((w00[:, None] * ck[y0, x0] + w01[:, None] * ck[y0, x0 + 1]) + w10[:, None] * ck[y0 + 1, x0]) + w11[:, None] * ck[y0 + 1, x0 + 1]
        to = ctr[None, :] - verts[idx]
        with np.errstate(all='ignore'):
            if normals is None:
                cosv = np.ones(len(idx), T)
            else:
                n = normals[idx]
                dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2])
                cosv = np.abs((to[:, 0] * n[:, 0] + to[:, 1] * n[:, 1]) + to[:, 2] * n[:, 2]) / np.fmax(dist, tiny)
            wt = cosv / np.fmax(zc * zc, tiny)
            contributes = vis & (wt > 0)                                                  # a NaN weight compares false
        yield dict(k=k, u=u, v=v, zz=zz, inframe=inframe, idx=idx, d=d, z=zc, c=c.reshape(-1, 3), w=wt, contributes=contributes)


def project_colors_ref(verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border=0, blend='weighted',
                       dtype=np.float32):
    """(rgb [V,3], wsum [V], count int32 [V], best int32 [V]) by the rule, all arithmetic in `dtype` (np.float32: the kernel's
    operations; np.float64: the same operations on the same f32 inputs, without their roundings).  verts [V,3], normals [V,3] or
    None, w2c [K,12], center [K,3], depth [K,H,W], color [K,H,W,3]: f32 arrays (see invert_poses)."""
    assert blend in BLENDS
    T = dtype
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    depth = np.asarray(depth, np.float32)
    color = np.asarray(color, np.float32)
    V = verts.shape[0]
    acc = np.zeros((V, 3), T)
    wsum = np.zeros(V, T)
    count = np.zeros(V, np.int32)
    best = np.full(V, -1, np.int32)
    for s in _views(T, verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border):
        on = s['contributes']
        i, w, c = s['idx'][on], s['w'][on], s['c'][on]
        count[i] += 1
        if blend == 'weighted':
            acc[i] += w[:, None] * c
            wsum[i] += w
        else:
            better = (best[i] < 0) | (w > wsum[i])
            acc[i[better]] = c[better]
            wsum[i[better]] = w[better]
            best[i[better]] = s['k']
    if blend == 'weighted':
        # best: the largest weight, the smallest index among equals -- a second walk, as the sums above do not keep it
        wbest = np.zeros(V, T)
        for s in _views(T, verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border):
            on = s['contributes']
            i, w = s['idx'][on], s['w'][on]
            better = (best[i] < 0) | (w > wbest[i])
            best[i[better]] = s['k']
            wbest[i[better]] = w[better]
        got = count > 0
        with np.errstate(all='ignore'):
            acc[got] = acc[got] / wsum[got][:, None]
    return acc, wsum, count, best


def ambiguity_mask(verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border=0, blend='weighted'):
    """bool [V]: the vertices at which an f32 evaluation of the rule may decide differently from the f64 one.  In the f64 statement:
    some keyframe has the vertex (not behind it: zz < 1e-6) within 1e-3 px of a frame bound, or within 1e-6 of zz = 0, or in frame
    with a corner depth whose | |d - z| - tol | < 1e-4; for 'best', its two largest weights lie within 1e-5 relative."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    depth = np.asarray(depth, np.float32)
    color = np.asarray(color, np.float32)
    V = verts.shape[0]
    K, H, W = depth.shape
    amb = np.zeros(V, bool)
    tol = float(np.float32(depth_tol))
    top = np.zeros((V, 2))                                   # the two largest weights
    for s in _views(np.float64, verts, normals, w2c, center, depth, color, fx, fy, cx, cy, depth_tol, border):
        u, v, zz = s['u'], s['v'], s['zz']
        with np.errstate(all='ignore'):
            near = np.minimum(np.minimum(np.abs(u - border), np.abs(u - (W - 1 - border))),
                              np.minimum(np.abs(v - border), np.abs(v - (H - 1 - border)))) < 1e-3
            amb |= near & (zz < 1e-6)
            amb |= np.abs(zz) < 1e-6
        edge = (np.abs(np.abs(s['d'] - s['z'][:, None]) - tol) < 1e-4).any(1)
        amb[s['idx'][edge]] = True
        on = s['contributes']
        i, w = s['idx'][on], s['w'][on]
        first = w > top[i, 0]
        second = ~first & (w > top[i, 1])
        top[i[first], 1] = top[i[first], 0]
        top[i[first], 0] = w[first]
        top[i[second], 1] = w[second]
    if blend == 'best':
        amb |= (top[:, 1] > 0) & (top[:, 0] - top[:, 1] <= 1e-5 * top[:, 0])
    return amb


# ---- the scene: the inside of the cube [-1, 1]^3 -----------------------------------------------------------------------------
SCENE_H, SCENE_W, SCENE_F = 48, 64, 40.0
SCENE_CX, SCENE_CY = (SCENE_W - 1) / 2.0, (SCENE_H - 1) / 2.0
WALL_N = 24


def texture(p):
    """A smooth colour in (0, 1) at world points p [...,3] (f64)."""
    p = np.asarray(p, np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([0.5 + 0.3 * np.sin(1.1 * x + 0.6 * y - 0.4 * z + 0.3),
                     0.5 + 0.3 * np.sin(-0.5 * x + 1.0 * y + 0.7 * z + 1.1),
                     0.5 + 0.3 * np.cos(0.8 * x - 0.3 * y + 0.9 * z - 0.5)], -1)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [4,4] f64 of this package's camera (x right, y up, looking along -z) at `eye` looking at `target`."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    x = np.cross(f, up)
    x /= np.linalg.norm(x)
    y = np.cross(x, f)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, -f, eye
    return m


def cube_walls():
    """(verts f32 [3456,3], normals f32 [3456,3]): 24 x 24 vertices per wall of the cube at -1 + 2 (j + 0.37) / 24, inward normals."""
    t = -1.0 + 2.0 * (np.arange(WALL_N) + 0.37) / WALL_N
    a, b = (g.reshape(-1) for g in np.meshgrid(t, t, indexing='ij'))
    verts, normals = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = np.empty((a.size, 3))
            p[:, axis] = side
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = a, b
            n = np.zeros((a.size, 3))
            n[:, axis] = -side
            verts.append(p)
            normals.append(n)
    return np.concatenate(verts).astype(np.float32), np.concatenate(normals).astype(np.float32)


def render_cube(c2w, H, W, fx, fy, cx, cy):
    """Analytic (depth f32 [H,W], color f32 [H,W,3]) of the cube's inside seen from c2w (inside the cube): the depth along the
    camera's axis of each pixel centre's hit, the texture at the hit."""
    c2w = np.asarray(c2w, np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = np.stack([(u - cx) / fx, -(v - cy) / fy, -np.ones_like(u)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(all='ignore'):
        t = np.where(d != 0, (np.sign(d) - o) / d, np.inf).min(-1)          # the exit through the wall each component heads for
    hit = o + t[..., None] * d
    return t.astype(np.float32), texture(hit).astype(np.float32)


SCENE_CAMERAS = (((0.15, -0.20, 0.10), (1.0, 0.35, -0.15)),
                 ((-0.25, 0.10, -0.05), (-0.3, 1.0, 0.25)),
                 ((0.10, 0.25, 0.20), (-1.0, -0.4, 0.1)),
                 ((-0.40, -0.30, 0.20), (1.0, 0.5, -0.1)))          # overlaps the first: a few hundred vertices have two views
SCENE_HOLE = (2, 20, 30)            # (keyframe, row, column) of the 10 x 10 block of zero depth


def many_cameras(K, seed=0):
    """K distinct cameras inside the cube, as (eye, target) pairs: seeded eyes in [-0.4, 0.4]^3 looking at seeded wall points."""
    rng = np.random.RandomState(seed)
    cams = []
    for _ in range(K):
        eye = rng.uniform(-0.4, 0.4, 3)
        target = rng.uniform(-0.6, 0.6, 3)
        target[rng.randint(2)] = rng.choice([-1.0, 1.0])          # a point on a wall x = +-1 or y = +-1: never straight up
        cams.append((tuple(eye), tuple(target)))
    return tuple(cams)


def cube_scene(cameras=None):
    """dict(verts, normals, c2w f32 [K,4,4], w2c, center, depth [K,48,64], color [K,48,64,3], fx, fy, cx, cy, H, W): cameras inside
    the cube (default: the four of SCENE_CAMERAS) with analytic depth and texture; one image has a 10 x 10 block of zero depth."""
    verts, normals = cube_walls()
    cameras = SCENE_CAMERAS if cameras is None else cameras
    ups = ((0.0, 0.0, 1.0), (0.1, 0.0, 1.0), (0.0, 0.15, 1.0), (0.0, 0.1, 1.0))
    c2w = np.stack([look_at(e, t, ups[k % 4]) for k, (e, t) in enumerate(cameras)]).astype(np.float32)
    imgs = [render_cube(m, SCENE_H, SCENE_W, SCENE_F, SCENE_F, SCENE_CX, SCENE_CY) for m in c2w]
    depth = np.stack([i[0] for i in imgs])
    color = np.stack([i[1] for i in imgs])
    k, r, c = SCENE_HOLE
    if k < len(cameras):
        depth[k, r:r + 10, c:c + 10] = 0.0
    w2c, center = invert_poses(c2w)
    return dict(verts=verts, normals=normals, c2w=c2w, w2c=w2c, center=center, depth=depth, color=color, fx=SCENE_F, fy=SCENE_F,
                cx=SCENE_CX, cy=SCENE_CY, H=SCENE_H, W=SCENE_W)


def with_keyframes(s, K):
    """The scene with its first K keyframes only."""
    return dict(s, c2w=s['c2w'][:K], w2c=s['w2c'][:K], center=s['center'][:K], depth=s['depth'][:K], color=s['color'][:K])


def scene_args(s, verts=None, normals='scene'):
    """The positional arguments of project_colors_ref / ambiguity_mask up to cy, from a cube_scene() dict."""
    return (s['verts'] if verts is None else verts, s['normals'] if isinstance(normals, str) else normals, s['w2c'], s['center'],
            s['depth'], s['color'], s['fx'], s['fy'], s['cx'], s['cy'])


# ---- cases by construction: one camera at the origin with the identity pose, looking down -z at a wall at z = -2 -----------------
# fx = fy = 8 and the wall at depth 2 make u = 7.5 + 4 x and v = 5.5 - 4 y exact in f32 for the coordinates below.
CASE_H, CASE_W, CASE_F = 12, 16, 8.0
CASE_TOL = 0.1
# (vertex, normal, contributing views with border 0, with border 2, what it is); normals = None turns the two bad normals into 1, 1
CASES = (((0.0, 0.0, 2.0), (0, 0, 1), 0, 0, 'behind the camera'),
         ((-1.875, 0.0, -2.0), (0, 0, 1), 1, 0, 'u = 0: on the bound'),
         ((1.875, 0.0, -2.0), (0, 0, 1), 1, 0, 'u = W - 1: on the bound, x0 clamps to W - 2'),
         ((0.0, 1.375, -2.0), (0, 0, 1), 1, 0, 'v = 0: on the bound'),
         ((0.0, -1.375, -2.0), (0, 0, 1), 1, 0, 'v = H - 1: on the bound, y0 clamps to H - 2'),
         ((-1.375, 0.0, -2.0), (0, 0, 1), 1, 1, 'u = 2: on the bound of border 2'),
         ((1.375, 0.0, -2.0), (0, 0, 1), 1, 1, 'u = W - 3: on the bound of border 2'),
         ((0.0, 0.875, -2.0), (0, 0, 1), 1, 1, 'v = 2: on the bound of border 2'),
         ((0.0, -0.875, -2.0), (0, 0, 1), 1, 1, 'v = H - 3: on the bound of border 2'),
         ((-1.376, 0.0, -2.0), (0, 0, 1), 1, 0, 'u just below 2'),
         ((1.876, 0.0, -2.0), (0, 0, 1), 0, 0, 'u just above W - 1'),
         ((0.0, 1.376, -2.0), (0, 0, 1), 0, 0, 'v just below 0'),
         ((0.0, 0.0, -2.0), (0, 0, 1), 0, 0, 'a zero-depth corner in the footprint'),
         ((0.5, 0.0, -2.0), (0, 0, 1), 1, 1, 'two pixels beside the hole'),
         ((0.75, 0.0, -2.0), (0, 0, 1), 0, 0, 'the edge of the far wall inside the footprint: a far corner'),
         ((1.5, 0.0, -3.0), (0, 0, 1), 1, 1, 'on the far wall'),
         ((0.5, 0.5, -2.0), (0, 0, 0), 0, 0, 'a zero normal'),
         ((0.5, -0.5, -2.0), (float('nan'), 0, 1), 0, 0, 'a NaN normal'),
         ((float('nan'), 0.0, -2.0), (0, 0, 1), 0, 0, 'a NaN vertex'))
CASE_BAD_NORMALS = (16, 17)


def constructed_scene(copies=1):
    """A cube_scene()-shaped dict of the cases above: the wall at depth 2 with colour (x / 16, y / 12, 0.25) at pixel (y, x), one
    zero-depth pixel at (5, 7), a far wall (depth 3) over rows 4..7, columns 11..12; `copies` identical keyframes."""
    H, W = CASE_H, CASE_W
    depth = np.full((H, W), 2.0, np.float32)
    depth[5, 7] = 0.0
    depth[4:8, 11:13] = 3.0
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    color = np.stack([x / 16.0, y / 12.0, np.full((H, W), 0.25)], -1).astype(np.float32)
    c2w = np.tile(np.eye(4, dtype=np.float32), (copies, 1, 1))
    w2c, center = invert_poses(c2w)
    return dict(verts=np.array([c[0] for c in CASES], np.float32), normals=np.array([c[1] for c in CASES], np.float32), c2w=c2w, w2c=w2c,
                center=center, depth=np.tile(depth, (copies, 1, 1)), color=np.tile(color, (copies, 1, 1, 1)), fx=CASE_F, fy=CASE_F,
                cx=(W - 1) / 2.0, cy=(H - 1) / 2.0, H=H, W=W)


def case_counts(border, normals=True):
    """The contributing views per case for one keyframe."""
    n = np.array([c[3] if border else c[2] for c in CASES], np.int32)
    if not normals:
        n[list(CASE_BAD_NORMALS)] = 1
    return n


# ---- the clamp at W - 2, H - 2 on a 13 x 9 image: the identity camera at the cube's centre, looking at the wall z = -1 --------------
CLAMP_H, CLAMP_W, CLAMP_F = 9, 13, 8.0


def clamp_scene():
    """A cube_scene()-shaped dict: 25 x 17 vertices on the wall z = -1 at multiples of 1 / 16, which project to u = 6 + 8 x and
    v = 4 - 8 y exactly in f32: every half pixel of the 13 x 9 image, its last column u = 12 and last row v = 8 included."""
    x, y = (g.reshape(-1) for g in np.meshgrid(-0.75 + np.arange(25) / 16.0, -0.5 + np.arange(17) / 16.0, indexing='ij'))
    verts = np.stack([x, y, np.full_like(x, -1.0)], 1).astype(np.float32)
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (len(verts), 1))
    c2w = np.eye(4, dtype=np.float32)[None]
    depth, color = render_cube(c2w[0], CLAMP_H, CLAMP_W, CLAMP_F, CLAMP_F, (CLAMP_W - 1) / 2.0, (CLAMP_H - 1) / 2.0)
    w2c, center = invert_poses(c2w)
    return dict(verts=verts, normals=normals, c2w=c2w, w2c=w2c, center=center, depth=depth[None], color=color[None], fx=CLAMP_F,
                fy=CLAMP_F, cx=(CLAMP_W - 1) / 2.0, cy=(CLAMP_H - 1) / 2.0, H=CLAMP_H, W=CLAMP_W)


def clamp_counts(s, border):
    """The contributing views (0 or 1) of clamp_scene()'s vertices."""
    u, v = 6.0 + 8.0 * s['verts'][:, 0].astype(np.float64), 4.0 - 8.0 * s['verts'][:, 1].astype(np.float64)
    return ((u >= border) & (u <= CLAMP_W - 1 - border) & (v >= border) & (v <= CLAMP_H - 1 - border)).astype(np.int32)
