"""The seeded triangle soups of the BVH-walk tests (test_soup_host.py, test_gpu_bvh_soup.py), built by numpy on the CPU so that both
suites see the same bits.  Unlike the room meshes of the other tests these have triangles of every size, leaf boxes that overlap
heavily, many surfaces along a ray and centroids that pile up in a few Morton cells:

  uniform          3 000 triangles, centroids uniform in [-2, 2]^3, edge scale log-uniform 0.01 .. 2, with 10 out-of-range and 10
                   degenerate faces sprinkled in
  giants_and_dust  8 triangles that span the whole box and 4 000 of edge 0.005 .. 0.02 in five Gaussian blobs
  sheets           64 parallel sheets 0.05 apart, each a 4 x 4 grid of quads split on alternating diagonals, every third
                   one wound the other way
  coincident       200 distinct triangles, each 1 .. 40 times (some copies rotated or reversed), shuffled
  far_offset       uniform and its cameras moved by (3000, -2000, 1000)
  counts:n         the first n in-range faces of uniform

mesh(name) -> (verts f64 [V,3], faces int64 [F,3]); views(name) -> a tuple of View (4x4 c2w in OpenCV axes, its own image, camera
and clip planes).  reference(name, view, cull) is the brute-force oracle's image, computed once per process and read-only;
visible_reference likewise for the visibility oracle, and mt_of for an independent f64 Moeller-Trumbore renderer."""
import collections
import functools

import numpy as np
import torch

import depth_ref as D
import refuse_ref as RF
import visible_ref as V

NAMES = ('uniform', 'giants_and_dust', 'sheets', 'coincident', 'far_offset')
COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
OFFSET = np.array([3000.0, -2000.0, 1000.0])
SHEETS, SHEET_STEP = 64, 0.05

View = collections.namedtuple('View', 'kind c2w H W fx fy cx cy near far')
CAM = dict(H=48, W=64, fx=40.0, fy=40.0, cx=31.5, cy=23.5, near=0.05, far=20.0)
ODD = dict(CAM, H=47, W=61, cx=30.2, cy=22.7)                  # the 16 x 16 workgroup tile is partial in both axes
WHOLE = dict(CAM, cx=32.0, cy=24.0)                            # a row and a column of rays with d.x or d.y exactly 0
SMALL = dict(H=24, W=32, fx=20.0, fy=20.0, cx=15.5, cy=11.5, near=0.05, far=20.0)
ALONG_X = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))   # camera z -> world x, camera x -> world y, camera y -> world z
ALONG_Z = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
AGAINST_Z = ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0))


def frozen(a):
    a.setflags(write=False)
    return a


def view(kind, c2w, cam=CAM, **kw):
    c = dict(cam, **kw)
    return View(kind, tuple(map(tuple, np.asarray(c2w, np.float64).tolist())), c['H'], c['W'], c['fx'], c['fy'], c['cx'], c['cy'],
                c['near'], c['far'])


def pose(R3, o):
    m = np.eye(4)
    m[:3, :3] = R3
    m[:3, 3] = o
    return m


def look(direction, o, up=D.UP):
    m = np.eye(4)
    m[:3, :] = D.viewmatrix(np.asarray(direction, np.float64), list(up), np.asarray(o, np.float64))
    return m


def c2w_of(v):
    return np.array(v.c2w, np.float64)


def camera(v):
    """(H, W, fx, fy, cx, cy, near, far): the trailing arguments of MeshBVH.render_depth and of the oracles."""
    return v.H, v.W, v.fx, v.fy, v.cx, v.cy, v.near, v.far


# ---- the soups ----
def random_triangles(rng, centres, scale):
    """[n,3,3]: three vertices around each centre, each coordinate uniform within +- scale / 2 of it."""
    return centres[:, None, :] + scale[:, None, None] * rng.uniform(-0.5, 0.5, (len(centres), 3, 3))


def uniform():
    rng = np.random.default_rng(20250301)
    n = 3000
    scale = np.exp(rng.uniform(np.log(0.01), np.log(2.0), n))
    tri = random_triangles(rng, rng.uniform(-2.0, 2.0, (n, 3)), scale)
    verts = tri.reshape(-1, 3)
    faces = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    # ten collinear or repeated-index faces on vertices of their own, ten faces with an index outside [0, V)
    a, b = rng.uniform(-2.0, 2.0, (5, 3)), rng.uniform(-1.0, 1.0, (5, 3))
    line = np.stack([a, a + 0.5 * b, a + 2.0 * b], 1).reshape(-1, 3)          # collinear up to rounding
    base = len(verts)
    verts = np.concatenate([verts, line])
    nv = len(verts)
    flat = [[base + 3 * k, base + 3 * k + 1, base + 3 * k + 2] for k in range(5)]
    pick = rng.integers(0, 3 * n, (5, 2))
    flat += [[p, p, q] if k % 2 else [p, q, q] for k, (p, q) in enumerate(pick.tolist())]
    out = rng.integers(0, 3 * n, (10, 3))
    out[np.arange(10), rng.integers(0, 3, 10)] = [-1, nv, nv + 7, 2 ** 30, -2 ** 31, 2 ** 31 - 1, -5, nv, 3 * nv, -1]
    extra = np.concatenate([np.array(flat, np.int64), out.astype(np.int64)])
    where = np.sort(rng.integers(0, n + 1, len(extra)))
    faces = np.insert(faces, where, extra[rng.permutation(len(extra))], axis=0)
    return verts, faces


def giants_and_dust():
    rng = np.random.default_rng(20250302)
    tris = []
    for _ in range(8):                                    # edge 3.5 sqrt(3), about 6, in planes fanned about the x axis
        ang, tilt = rng.uniform(0, np.pi), rng.normal(0, 0.15, 2)
        n = np.array([tilt[0], np.cos(ang), np.sin(ang)])
        ex = np.cross(n, [tilt[1], -np.sin(ang), np.cos(ang)])
        ex /= np.linalg.norm(ex)
        ey = np.cross(n, ex) / np.linalg.norm(n)
        c = rng.uniform(-0.8, 0.8, 3)
        turn = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.0, 4.0]) * np.pi / 3
        tris.append(c + 3.5 * (np.cos(turn)[:, None] * ex + np.sin(turn)[:, None] * ey))
    blobs = rng.uniform(-1.5, 1.5, (5, 3))
    centres = (blobs[:, None, :] + 0.15 * rng.normal(size=(5, 800, 3))).reshape(-1, 3)
    scale = np.exp(rng.uniform(np.log(0.005), np.log(0.02), len(centres)))
    tri = np.concatenate([np.array(tris), random_triangles(rng, centres, 1.5 * scale)])
    tri = tri[rng.permutation(len(tri))]
    return tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.int64).reshape(-1, 3)


def sheet_z(k):
    return (k - SHEETS // 2) * SHEET_STEP


def sheets():
    xs = np.linspace(-1.0, 1.0, 5)
    X, Y = np.meshgrid(xs, xs, indexing='ij')
    verts, faces = [], []
    for k in range(SHEETS):
        base = 25 * k
        verts.append(np.stack([X.ravel(), Y.ravel(), np.full(25, sheet_z(k))], 1))
        for i in range(4):
            for j in range(4):
                a, b, c, d = base + 5 * i + j, base + 5 * (i + 1) + j, base + 5 * (i + 1) + j + 1, base + 5 * i + j + 1
                quad = [(a, b, c), (a, c, d)] if (i + j + k) % 2 else [(a, b, d), (b, c, d)]
                faces += [q[::-1] for q in quad] if k % 3 == 1 else quad               # every third sheet faces the other way
    return np.concatenate(verts), np.array(faces, np.int64)


def coincident():
    rng = np.random.default_rng(20250304)
    n = 200
    tri = random_triangles(rng, rng.uniform(-2.0, 2.0, (n, 3)), rng.uniform(0.3, 1.8, n))
    copies = rng.integers(1, 41, n)
    copies[:3] = (40, 17, 1)
    faces = []
    for k in range(n):
        for _ in range(copies[k]):
            f = [3 * k, 3 * k + 1, 3 * k + 2]
            r = rng.random()
            f = f if r < 0.6 else (f[1:] + f[:1] if r < 0.8 else f[::-1])     # the same triangle: as is, rotated or reversed
            faces.append(f)
    faces = np.array(faces, np.int64)[rng.permutation(len(faces))]
    return tri.reshape(-1, 3), faces


def in_range(verts, faces):
    return ((faces >= 0) & (faces < len(verts))).all(1)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(verts f64 [V,3], faces int64 [F,3]) of a soup, read-only."""
    if name == 'far_offset':
        v, f = mesh('uniform')
        v, f = v + OFFSET, f.copy()
    elif name.startswith('counts:'):
        v, f = mesh('uniform')
        v, f = v.copy(), f[in_range(v, f)][:int(name.split(':')[1])].copy()
    else:
        v, f = {'uniform': uniform, 'giants_and_dust': giants_and_dust, 'sheets': sheets, 'coincident': coincident}[name]()
    return frozen(np.ascontiguousarray(v, np.float64)), frozen(np.ascontiguousarray(f, np.int64))


def extent(name):
    """The longest side of the box of the vertices that some in-range face uses (counts:n keeps all of uniform's vertices)."""
    v, f = mesh(name)
    return float(np.ptp(v[np.unique(f[in_range(v, f)])], 0).max())


# ---- the views ----
def box_views(shift=(0.0, 0.0, 0.0), inside=(0.2, -1.0, 0.1), clipped=(-0.5, 1.0, -0.3)):
    """Five cameras about a soup in [-2, 2]^3 + shift; the directions do not depend on the shift."""
    s = np.asarray(shift, np.float64)
    eye, out = np.array([-0.5, 0.5, 0.3]), np.array([5.5, 1.0, 0.8])
    return (view('inside', look(inside, eye + s)),
            view('outside_in', look(-out, out + s), ODD),
            view('away', look(out + (0.0, 0.4, 0.1), out + s)),
            view('axis', pose(ALONG_X, np.array([-0.3, 0.2, 0.1]) + s), WHOLE),
            view('clipped', look(clipped, eye + s), near=1.0, far=2.5))


def sheet_views():
    return (view('normal_above', pose(AGAINST_Z, (0.13, -0.07, 3.0))),
            view('normal_below', pose(ALONG_Z, (-0.11, 0.06, -3.0)), ODD),
            view('oblique', look((-1.0, -0.6, -0.8), (2.0, 1.3, 1.2)), near=1.0, far=2.5),
            view('in_plane', pose(ALONG_X, (-0.53, 0.11, sheet_z(20))), WHOLE),   # inside the soup, in sheet 20's plane
            view('away', look((0.3, 0.2, 1.0), (0.0, 0.0, 3.0))))


def count_views():
    """Two cameras on the first face of `uniform` (from along its normal and from the side of the box's centre) and one looking away, 24 x 32."""
    v, f = mesh('counts:1')
    a, b, c = v[f[0]]
    centre = (a + b + c) / 3
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    size = max(np.linalg.norm(b - a), np.linalg.norm(c - b), np.linalg.norm(a - c))
    eye = centre + 1.5 * size * n
    side = n - 0.7 * centre / np.linalg.norm(centre)
    inner = centre + 2.0 * size * side / np.linalg.norm(side)                  # obliquely, from the side of the box's centre
    return (view('facing', look(centre - eye, eye), SMALL),
            view('inside', look(centre - inner, inner), SMALL),
            view('away', look((1.0, 0.2, 0.1), (5.5, 1.0, 0.8)), SMALL))


@functools.lru_cache(maxsize=None)
def views(name):
    if name == 'sheets':
        return sheet_views()
    if name == 'far_offset':
        return box_views(OFFSET)
    if name.startswith('counts:'):
        return count_views()
    if name == 'giants_and_dust':
        # inside: along the giants' fan, not across it; clipped: at giants and two blobs that lie between near and far
        return box_views(inside=(1.0, 0.3, 0.1), clipped=(0.3, -1.0, 1.0))
    return box_views()


@functools.lru_cache(maxsize=None)
def reference(name, v, cull='none'):
    """f32 [H,W], read-only: the brute-force oracle's render of soup `name` from View v (depth_ref.render_depth for 'none',
    refuse_ref.render_depth_cull for 'back' / 'front')."""
    verts, faces = mesh(name)
    if cull == 'none':
        return frozen(D.render_depth(verts, faces, c2w_of(v), *camera(v)))
    return frozen(RF.render_depth_cull(verts, faces, c2w_of(v), *camera(v), cull=cull))


# ---- an independent statement of the render ----
BARY_TOL = 1e-9                                        # a barycentric coordinate this close to 0: the two statements may differ


def mt_render(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far, tol, pix_chunk=256):
    """Moeller-Trumbore in world space, f64, brute force.  With the ray o + t R (dx, dy, 1) the parameter t is the camera z.
    Returns (z [H,W] of the nearest hit with near <= t <= far, inf where none; hits [H,W], their number; face [H,W], the nearest
    hit's row in `faces`, -1 where none; unsure [H,W]: the nearest hit, or a candidate no more than tol behind it, has a
    barycentric coordinate within BARY_TOL of 0 or lies within tol of a clip plane)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    rows = np.flatnonzero(((f >= 0) & (f < len(v))).all(1))
    f = f[rows]
    m = np.asarray(c2w, np.float64)
    R, o = m[:3, :3], m[:3, 3]
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(jj.ravel() - cx) / fx, (ii.ravel() - cy) / fy, np.ones(H * W)], 1) @ R.T
    v0, e1, e2 = v[f[:, 0]], v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    tvec = o - v0
    qvec = np.cross(tvec, e1)
    tnum = (e2 * qvec).sum(1)
    z = np.full(H * W, np.inf)
    hits = np.zeros(H * W, np.int64)
    face = np.full(H * W, -1, np.int64)
    unsure = np.zeros(H * W, bool)
    for p0 in range(0, H * W, pix_chunk):
        dd = d[p0:p0 + pix_chunk, None, :]
        pvec = np.cross(dd, e2[None])
        with np.errstate(all='ignore'):
            det = (e1[None] * pvec).sum(2)
            u = (tvec[None] * pvec).sum(2) / det
            w = (dd * qvec[None]).sum(2) / det
            t = tnum[None] / det
            low = np.minimum(np.minimum(u, w), 1.0 - u - w)
            ok = (det != 0) & np.isfinite(low) & np.isfinite(t)
            hit = ok & (low >= 0) & (t >= near) & (t <= far)
            cand = ok & (low >= -BARY_TOL) & (t >= near - tol) & (t <= far + tol)
            shaky = cand & ((low <= BARY_TOL) | (np.abs(t - near) <= tol) | (np.abs(t - far) <= tol))
        th = np.where(hit, t, np.inf)
        if th.shape[1]:
            tmin = th.min(1)
            arg = th.argmin(1)
            z[p0:p0 + pix_chunk] = tmin
            hits[p0:p0 + pix_chunk] = hit.sum(1)
            face[p0:p0 + pix_chunk] = np.where(np.isfinite(tmin), rows[arg], -1)
            unsure[p0:p0 + pix_chunk] = (shaky & (t <= (tmin + tol)[:, None])).any(1)
    return tuple(frozen(a.reshape(H, W)) for a in (z, hits, face, unsure))


@functools.lru_cache(maxsize=None)
def mt_of(name, v):
    """mt_render of soup `name` from View v with tol = 1e-9 x extent, computed once per process."""
    verts, faces = mesh(name)
    return mt_render(verts, faces, c2w_of(v), *camera(v), tol=1e-9 * extent(name))


# ---- visibility: points and poses ----
VIS_CAM = (CAM['H'], CAM['W'], CAM['fx'], CAM['fy'], CAM['cx'], CAM['cy'])


def vis_pose(c2w):
    """A 4x4 OpenCV c2w in visible_ref.look_at's convention: a float32 tensor with columns 1 and 2 negated."""
    m = np.array(c2w, np.float64, copy=True)
    m[:3, 1] *= -1
    m[:3, 2] *= -1
    return torch.from_numpy(m).float()


@functools.lru_cache(maxsize=None)
def vis_poses(name):
    """The soup's views as poses, then the same list reversed."""
    ps = [vis_pose(c2w_of(v)) for v in views(name)]
    return tuple(ps + ps[::-1])


@functools.lru_cache(maxsize=None)
def vis_points(name):
    """f64 [600 + 2 per view, 3], read-only: 200 soup vertices, 200 area-weighted surface samples, 200 uniform in the soup's box,
    each camera's centre and a point 0.5 behind each camera."""
    verts, faces = mesh(name)
    rng = np.random.default_rng(20250310)
    good = faces[in_range(verts, faces)]
    a, b, c = verts[good[:, 0]], verts[good[:, 1]], verts[good[:, 2]]
    good = good[np.linalg.norm(np.cross(b - a, c - a), axis=1) > 0]
    used = np.unique(good)
    ms = V.opencv_rows(vis_poses(name)[:len(views(name))])
    return frozen(np.concatenate([verts[rng.choice(used, 200, replace=False)], V.surface_samples(verts, good, 200, rng),
                                  rng.uniform(verts[used].min(0), verts[used].max(0), (200, 3)),
                                  ms[:, :, 3], ms[:, :, 3] - 0.5 * ms[:, :, 2]]))


def per_pose_in_frustum(verts, faces, points, poses, eps, near):
    """visible_ref.per_pose with the shadow rays cast only for the pairs that pass the frustum test (the others never count):
    (frustum [P,n], clear [P,n], margin [P,n]); clear is False and margin inf outside the frustum."""
    from attentive_dfprior_amd import recon
    w = recon.w2c_rows(list(poses))
    ms = V.opencv_rows(poses)
    n = len(points)
    fr = np.zeros((len(poses), n), bool)
    cl = np.zeros((len(poses), n), bool)
    mg = np.full((len(poses), n), np.inf)
    for k in range(len(poses)):
        fr[k] = V.in_frustum(points, w[k], *VIS_CAM)
        if fr[k].any():
            cl[k, fr[k]], mg[k, fr[k]] = V.unoccluded(verts, faces, points[fr[k]], ms[k], near, eps)
    return fr, cl, mg


@functools.lru_cache(maxsize=None)
def visible_reference(name, eps, near):
    """per_pose_in_frustum of the soup's points and poses (vis_points, vis_poses), read-only."""
    verts, faces = mesh(name)
    half = per_pose_in_frustum(verts, faces, vis_points(name), vis_poses(name)[:len(views(name))], eps, near)
    return tuple(frozen(np.concatenate([a, a[::-1]])) for a in half)         # the reversed half: the same poses again
