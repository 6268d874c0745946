"""GPU: the Mesher's clean-up on the device (mesh.face_components / clean_components / merge_coincident, Mesher.seen_mask and
the device routing of Mesher.get_mesh) against the host statements of the same steps, which the parent commit ran and which
remain in mesher.py: Mesher.point_masks (torch), Mesher.clean (scipy) and mesher.merge_coincident (numpy)."""
import numpy as np
import pytest
import torch

import mesh_ref as R
import attentive_dfprior_amd as A
from attentive_dfprior_amd import mesh as M
from attentive_dfprior_amd import synthetic
from attentive_dfprior_amd.keyframes import KeyframeStore
from attentive_dfprior_amd.mesher import Mesher, merge_coincident
from oracle import adfp_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def tetra(center, size):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * size + np.asarray(center, np.float32)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def join(*parts):
    vs, fs, n = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f + n)
        n += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def two_tetrahedra():
    """tests/test_mesher_clean.py: a small and a big tetrahedron."""
    return join(tetra((3, 0, 0), 0.1), tetra((0, 0, 0), 0.5))


def shared_edge():
    """tests/test_mesher_clean.py::test_four_face_edge_does_not_join_components: two tetrahedra sharing ONE edge."""
    a = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0.5, 1, 0.5]], np.float32)
    b = np.array([[0, 0, 0], [0, 0, 1], [-1.3, 0, 0], [-0.5, -1.5, 0.5]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    v = np.concatenate([a, b[2:]])
    fb = f.copy()
    fb[fb >= 2] += 2
    fb = fb[:, ::-1]
    return v, np.concatenate([f, fb])


def degenerate():
    """A tetrahedron; a face with a repeated vertex (area 0); three faces around one edge, which with the repeated vertex's two
    half-edges is a run of five and joins nothing; the same face twice, whose three edges have two half-edges each."""
    v, f = tetra((0, 0, 0), 0.5)
    v = np.concatenate([v, np.array([[2, 0, 0], [2, 1, 0], [2, 0, 1], [3, 0, 0.5], [2.5, 0, 2]], np.float32)])
    extra = np.array([[4, 4, 5], [4, 5, 6], [4, 5, 7], [4, 5, 8], [6, 7, 8], [6, 7, 8]], np.int32)
    return v, np.concatenate([f, extra])


_noise = {}


def noise_mesh(n=48, seed=5, offset=-0.4):
    """Marching cubes (the device one) of a seeded noise lattice: hundreds of components, four-face edges.  offset 0 (half the
    corners inside) gives one component of most of the faces beside the small ones."""
    if (n, seed, offset) not in _noise:
        rng = np.random.default_rng(seed)
        z = torch.from_numpy((rng.standard_normal((n, n, n)) + offset).astype(np.float32)).to(DEV)
        v, f, _ = M.marching_cubes(z, level=0.0, spacing=(0.05, 0.05, 0.05), origin=(-1.0, -1.0, -1.0))
        _noise[(n, seed, offset)] = (v.cpu().numpy(), f.cpu().numpy())
    return _noise[(n, seed, offset)]


def noise_mesh_dense():
    return noise_mesh(offset=0.0)


def single_face():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32)


def empty_faces():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.zeros((0, 3), np.int32)


MESHES = {'two_tetrahedra': two_tetrahedra, 'shared_edge': shared_edge, 'degenerate': degenerate, 'noise48': noise_mesh, 'noise48_dense': noise_mesh_dense,
          'single_face': single_face, 'empty': empty_faces}


# ---- the host statements --------------------------------------------------------------------------------------------------
def host_labels(faces, n_verts):
    """The component labels exactly as Mesher.clean derives them (mesher.py, the lines between the unseen-face filter and the
    areas)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    nf = len(faces)
    if nf == 0:
        return np.zeros(0, np.int64), 0
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, 1)
    fid = np.tile(np.arange(nf), 3)
    key = e[:, 0].astype(np.int64) * (n_verts + 1) + e[:, 1]
    order = np.argsort(key, kind='stable')
    ks, fs = key[order], fid[order]
    _, start, count = np.unique(ks, return_index=True, return_counts=True)
    two = start[count == 2]
    adj = coo_matrix((np.ones(len(two)), (fs[two], fs[two + 1])), shape=(nf, nf))
    ncomp, label = connected_components(adj, directed=False)
    return label, (count == 4).sum()


def host_component_areas(v, f, seen):
    f = f[~(~seen)[f].all(axis=1)]
    if len(f) == 0:
        return np.zeros(0)
    label, _ = host_labels(f, len(v))
    v = v.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    return np.bincount(label, weights=area)


def cleaner(threshold, largest, scale):
    m = Mesher.__new__(Mesher)
    m.remove_small_geometry_threshold, m.get_largest_components, m.scale = threshold, largest, scale
    return m


# ---- 1. labels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(MESHES))
def test_labels_equal_scipy_partition(name):
    v, f = MESHES[name]()
    ref, four = host_labels(f, len(v))
    got = M.face_components(torch.from_numpy(f).to(DEV), len(v))
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(f),)
    got = got.cpu().numpy()
    if len(f) == 0:
        return
    if name.startswith('noise48'):
        assert len(np.unique(ref)) >= 100 and four > 0, (len(np.unique(ref)), four)
    if name == 'shared_edge':
        assert len(np.unique(ref)) == 2
    # each label is the smallest face index of its class ...
    first = np.full(ref.max() + 1, len(f), np.int64)
    np.minimum.at(first, ref, np.arange(len(f)))
    assert np.array_equal(got, first[ref])
    # ... which makes the two partitions equal
    assert len(np.unique(got)) == len(np.unique(ref))


def test_labels_reject_indices_out_of_range():
    f = torch.tensor([[0, 1, 2], [1, 2, 7]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        M.face_components(f, 4)
    with pytest.raises(ValueError):
        M.face_components(-f - 1, 4)


# ---- 2. clean -------------------------------------------------------------------------------------------------------------
def seen_masks(nv, rng):
    return {'all': np.ones(nv, bool), 'none': np.zeros(nv, bool), 'half': rng.random(nv) < 0.5, 'sparse': rng.random(nv) < 0.03,
            'dense': rng.random(nv) < 0.97}


def midpoints(areas, rel=1e-6, want=(0.1, 0.5, 0.9)):
    """Thresholds between neighbouring sorted component areas that differ by more than `rel`, near the wanted quantiles."""
    a = np.unique(areas)
    out = []
    for q in want:
        for i in range(int(q * (len(a) - 1)), len(a) - 1):
            if a[i + 1] - a[i] > rel * a[i + 1]:
                out.append(0.5 * (a[i] + a[i + 1]))
                break
    return sorted(set(out))


@pytest.mark.parametrize('name', list(MESHES))
def test_clean_components_equal_host_clean(name):
    v, f = MESHES[name]()
    rng = np.random.default_rng(11)
    vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    ran = 0
    for sname, seen in seen_masks(len(v), rng).items():
        areas = host_component_areas(v, f, seen)
        sd = torch.from_numpy(seen).to(DEV)
        cases = [(0.0, False)] + [(t, False) for t in midpoints(areas)] + [(0.0, True)]
        for thr, largest in cases:
            # the condition on the inputs: no component within 1e-9 (relative) of the threshold / of the runner-up, by the host areas
            if largest:
                if len(areas) > 1:
                    top = np.sort(areas)[-2:]
                    assert top[1] - top[0] > 1e-9 * top[1], (name, sname, top)
            elif len(areas):
                # an area of exactly 0 (degenerate faces only) is 0 in any summation order: it cannot cross thr = 0
                far_enough = np.abs(areas - thr) > 1e-9 * np.maximum(areas, thr)
                assert (far_enough | ((areas == 0.0) & (thr == 0.0))).all(), (name, sname, thr)
            for scale in (1, 2):
                host = cleaner(thr / (scale * scale), largest, scale)
                assert host.remove_small_geometry_threshold * scale * scale == thr
                rv, rf = host.clean(v, f, seen)
                gv, gf = M.clean_components(vd, fd, sd, min_area=host.remove_small_geometry_threshold * scale * scale, largest=largest)
                assert gv.dtype == torch.float32 and gf.dtype == torch.int32
                assert np.array_equal(gf.cpu().numpy(), rf.reshape(-1, 3)), (name, sname, thr, largest, scale)
                assert np.array_equal(gv.cpu().numpy(), rv), (name, sname, thr, largest, scale)
                ran += 1
    assert ran >= 20


# ---- 3. merge -------------------------------------------------------------------------------------------------------------
def check_merge(v, f, c):
    rv, rf, rc = merge_coincident(v, f, c)
    gv, gf, gc = M.merge_coincident(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV),
                                    torch.from_numpy(c).to(DEV) if c is not None else None)
    assert np.array_equal(gv.cpu().numpy().view(np.int32), np.ascontiguousarray(rv).view(np.int32))       # bits: -0.0 stays -0.0
    assert np.array_equal(gf.cpu().numpy(), rf)
    assert (gc is None) == (rc is None)
    if rc is not None:
        assert np.array_equal(gc.cpu().numpy(), rc)
    return len(rv)


def test_merge_coincident_equals_host():
    rng = np.random.default_rng(3)
    v, f = noise_mesh()
    n = len(v)
    c = rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
    assert check_merge(v, f, c) == n                                       # marching cubes welds: nothing coincides, inputs returned
    assert check_merge(v, f, None) == n
    v2 = v.copy()
    dup = rng.choice(n, size=n // 10, replace=False)                       # planted exact duplicates, some in chains of three
    src = rng.choice(n, size=n // 10, replace=True)
    v2[dup] = v2[src]
    left = check_merge(v2, f, c)
    assert n - len(dup) <= left < n
    check_merge(v2, f, None)
    z = np.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [5.0, -0.0, 1.0], [5.0, 0.0, 1.0], [5.0, -0.0, 1.0]], np.float32)
    zf = np.array([[0, 1, 2], [3, 4, 5], [2, 5, 1]], np.int32)
    assert check_merge(z, zf, np.arange(18, dtype=np.uint8).reshape(6, 3)) == 4      # -0.0 and +0.0 differ in bits: not merged
    same = np.tile(np.array([[1.5, -2.0, 3.0]], np.float32), (5000, 1))
    assert check_merge(same, zf, None) == 1
    assert check_merge(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), None) == 0


def test_compaction_scans_more_tiles_than_one_round():
    """k_tile_scan's one workgroup takes 256 x 8 = 2048 tile counts a round and carries the sum into the next round; a tile is 2048
    flags, so 2048 * 2048 + 1 vertices are the smallest mesh whose vertex scan has a second round (2049 tiles: the carry, and a last
    round of one tile).  adfp_mesh_compact_plan / _emit raw, against numpy: integers and copies, so equality."""
    rng = np.random.default_rng(11)
    nv, nf = 2048 * 2048 + 1, 1_400_000
    faces = rng.integers(0, nv, size=(nf, 3), dtype=np.int32)
    keep = rng.random(nf) < 0.5
    faces[-1] = (nv - 1, 0, nv - 2)
    keep[-1] = True                                                        # the vertex of the last tile is used
    verts = rng.standard_normal((nv, 3)).astype(np.float32)
    used = np.zeros(nv, bool)
    used[faces[keep]] = True
    v, f, k = (torch.from_numpy(a).to(DEV) for a in (verts, faces, keep.astype(np.uint8)))
    with M._lib.on(v.device) as L:
        nbytes = M.lib().adfp_mesh_compact_workspace_bytes(nv, nf)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        totals = torch.empty(2, dtype=torch.int64, device=DEV)
        L.adfp_mesh_compact_plan(f, nf, nv, k, ws, nbytes, totals)
        assert tuple(totals.tolist()) == (int(used.sum()), int(keep.sum()))
        vo = torch.empty((int(used.sum()), 3), dtype=torch.float32, device=DEV)
        fo = torch.empty((int(keep.sum()), 3), dtype=torch.int32, device=DEV)
        L.adfp_mesh_compact_emit(v, nv, f, nf, ws, nbytes, vo, vo.shape[0], fo, fo.shape[0])
    assert np.array_equal(vo.cpu().numpy().view(np.int32), verts[used].view(np.int32))
    assert np.array_equal(fo.cpu().numpy(), (np.cumsum(used) - used)[faces[keep]])


def test_color_bytes_equals_numpy():
    rng = np.random.default_rng(4)
    raw = (rng.standard_normal((70001, 4)) * 0.7 + 0.5).astype(np.float32)
    raw[:8, :3] = np.array([0.0, 1.0, -0.0, 1.0 - 2 ** -24, 2 ** -9, 0.999, 255 / 256, 0.5], np.float32)[:, None]
    ref = (np.clip(raw[:, :3], 0, 1) * 255).astype(np.uint8)
    got = M.color_bytes(torch.from_numpy(raw).to(DEV))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(M.color_bytes(torch.from_numpy(raw[:, :3].copy()).to(DEV)).cpu().numpy(), ref)


# ---- 4. seen mask ---------------------------------------------------------------------------------------------------------
class Slam(object):
    pass


def setup(resolution=48, depth_test=False, largest=False, level_set=0.0, n_kf=3):
    sc = synthetic.mini_scene(device=DEV)
    sd = O.random_state_dict(seed=3)
    dec = A.DF()
    dec.load_state_dict(sd)
    dec.bound = sc.bound
    dec = dec.to(DEV)
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
           'scale': 1, 'occupancy': True,
           'meshing': {'resolution': resolution, 'level_set': level_set, 'clean_mesh_bound_scale': 1.02,
                       'remove_small_geometry_threshold': 0.0002, 'color_mesh_extraction_method': 'direct_point_query',
                       'get_largest_components': largest, 'depth_test': depth_test},
           'mapping': {'marching_cubes_bound': sc.bound.tolist()}}
    slam = Slam()
    slam.bound = sc.bound
    slam.vol_bnds = slam.tsdf_bnds = sc.tsdf_bnds.to(DEV)
    slam.verbose = False
    slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
    slam.renderer = A.Renderer(cfg, None, slam)
    kfs = []
    for k in range(n_kf):
        c2w = sc.default_c2w(offset=(0.05 * (k % 4), -0.04 * (k % 3), 0.02), yaw=0.9 * k, pitch=0.1 * (k % 5) - 0.1)
        kfs.append({'est_c2w': c2w.cpu(), 'depth': sc.depth_image(c2w, zero_band=0.08).cpu(),
                    'color': torch.zeros(sc.H, sc.W, 3), 'idx': k})
    est = torch.stack([kf['est_c2w'] for kf in kfs])
    c = {k: v.to(DEV) for k, v in sc.c.items()}
    return sc, sd, dec, cfg, slam, kfs, est, c


def edge_points(pts, poses, depths, rule, m):
    """The points where two correct f32 evaluations of the seen test may disagree, by an f64 restatement of the projection (in the
    manner of keyframes.overlap_ambiguity): for some pose, u or v within 1e-3 px of 0 / W / H, |z| < 1e-6, or -- inside or on the
    edge of the frustum -- a depth comparison whose two sides agree to 1e-5 relative."""
    x = np.asarray(pts, np.float64)
    H, W = m.H, m.W
    amb = np.zeros(len(x), bool)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for k, c2w in enumerate(poses):
            w = np.linalg.inv(np.asarray(c2w, np.float64))[:3]
            cam = x @ w[:, :3].T + w[:, 3]
            X, Y, Z = -cam[:, 0], cam[:, 1], cam[:, 2]
            zz = Z + 1e-8
            u, v = (m.fx * X + m.cx * Z) / zz, (m.fy * Y + m.cy * Z) / zz
            e = np.abs(zz) < 1e-6
            for val, bound in ((u, 0.0), (u, float(W)), (v, 0.0), (v, float(H))):
                e |= np.abs(val - bound) < 1e-3
            inside = (u < W) & (u > 0) & (v < H) & (v > 0) & (zz < 0)
            near = inside | e

            def close(a, b):
                return np.abs(a - b) <= 1e-5 * np.maximum(np.abs(a), np.abs(b))
            if rule == 'max_depth':
                far = np.float64(np.float32(depths[k].max()) * np.float32(1.1))
                e |= near & close(-Z, far)
            elif rule == 'depth_test':
                d = np.asarray(depths[k], np.float64)
                ix = ((u / (W - 1) * 2.0 - 1.0) + 1.0) / 2.0 * (W - 1)
                iy = ((v / (H - 1) * 2.0 - 1.0) + 1.0) / 2.0 * (H - 1)
                ok = near & np.isfinite(ix) & np.isfinite(iy)
                ix, iy = np.where(ok, ix, 0.0), np.where(ok, iy, 0.0)
                x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
                s = np.zeros(len(x))
                for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    xi, yi = x0 + dx, y0 + dy
                    wgt = (1.0 - np.abs(ix - xi)) * (1.0 - np.abs(iy - yi))
                    valid = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
                    s += np.where(valid, d[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)] * wgt, 0.0)
                e |= ok & (close(-Z, s + 2.4) | close(s - 2.4, -Z))
            amb |= e
    return amb


def mask_inputs(m, sc, n_random=24000, seed=0):
    rng = np.random.default_rng(seed)
    b = sc.bound.cpu().numpy().astype(np.float64)
    pts = (b[:, 0] + rng.random((n_random, 3)) * (b[:, 1] - b[:, 0])).astype(np.float32)
    mv, _ = noise_mesh()
    mv = (mv.astype(np.float64) * 0.55 * (b[:, 1] - b[:, 0]).max() / 2 + b.mean(1)).astype(np.float32)    # a real mesh's vertices, in the room
    return np.concatenate([pts, mv[:20000]])


@pytest.mark.parametrize('n_kf', [1, 3, 8])
@pytest.mark.parametrize('rule', ['frustum', 'max_depth', 'depth_test'])
def test_seen_mask_equals_point_masks(rule, n_kf):
    sc, sd, dec, cfg, slam, kfs, est, c = setup(depth_test=rule == 'depth_test', n_kf=n_kf)
    m = Mesher(cfg, None, slam)
    pts = mask_inputs(m, sc, seed=n_kf)
    assert len(pts) >= 20000
    all_frames = rule == 'frustum'
    poses = [kf['est_c2w'].numpy() for kf in kfs]
    amb = edge_points(pts, poses, [kf['depth'].numpy() for kf in kfs], rule, m)
    share = amb.mean()
    print(f'seen mask {rule} K={n_kf}: {amb.sum()} edge points of {len(pts)} ({share:.2e})')
    assert share <= 0.01, share                                            # the cap, from the f64 restatement alone
    ref = m.point_masks(torch.from_numpy(pts), kfs, est, n_kf - 1, DEV, get_mask_use_all_frames=all_frames)[0]
    got = m.seen_mask(torch.from_numpy(pts).to(DEV), kfs, est, n_kf - 1, DEV, get_mask_use_all_frames=all_frames)
    assert got.dtype == torch.bool and got.is_cuda
    got = got.cpu().numpy()
    assert 0 < ref.sum() < len(ref)
    diff = got != ref
    print(f'seen mask {rule} K={n_kf}: {diff.sum()} differ, {(diff & ~amb).sum()} of them outside the edge set')
    assert not (diff & ~amb).any()


@pytest.mark.parametrize('rule', ['max_depth', 'depth_test'])
def test_seen_mask_depth_rules_decide(rule):
    """The mini room is smaller than the 2.4 m band and than 1.1 max(depth), so there the depth rules never reject a point inside
    the frustum.  Here they do: points out to 6 m from the cameras, smooth depth images between 0.5 and 3 m (slope below 0.1 m
    per pixel, so that the f32 rounding of the sample position stays far inside the edge set's 1e-5)."""
    sc, sd, dec, cfg, slam, kfs, est, c = setup(depth_test=rule == 'depth_test', n_kf=4)
    m = Mesher(cfg, None, slam)
    yy, xx = np.meshgrid(np.arange(sc.H), np.arange(sc.W), indexing='ij')
    for k, kf in enumerate(kfs):
        kf['depth'] = torch.from_numpy((1.75 + 1.25 * np.sin(0.07 * xx + 0.05 * yy + k)).astype(np.float32))
    rng = np.random.default_rng(21)
    pts = ((rng.random((40000, 3)) - 0.5) * 12.0 + np.asarray(sc.center)).astype(np.float32)
    amb = edge_points(pts, [kf['est_c2w'].numpy() for kf in kfs], [kf['depth'].numpy() for kf in kfs], rule, m)
    assert amb.mean() <= 0.01, amb.mean()
    ref = m.point_masks(torch.from_numpy(pts), kfs, est, 3, DEV)[0]
    frustum = m.point_masks(torch.from_numpy(pts), kfs, est, 3, DEV, get_mask_use_all_frames=True)[0]
    assert 0 < ref.sum() < 0.8 * frustum.sum()                               # the depth rule rejected a good part of the frustum
    got = m.seen_mask(torch.from_numpy(pts).to(DEV), kfs, est, 3, DEV).cpu().numpy()
    diff = got != ref
    print(f'seen mask {rule}, far points: {amb.sum()} edge points, {diff.sum()} differ, {(diff & ~amb).sum()} outside the edge set')
    assert not (diff & ~amb).any()


def test_seen_mask_all_frames_many_poses_one_launch():
    """get_mask_use_all_frames with 200 poses: equal to the torch path off the edge set, and ONE kernel launch for the mask -- by
    construction of the binding: Mesher.seen_mask makes exactly one call into the library (counted here), adfp_mesh_seen_mask, and
    that export launches k_cull_seen once whatever the pose count (the poses pass through LDS inside the kernel)."""
    sc, sd, dec, cfg, slam, kfs, est, c = setup()
    m = Mesher(cfg, None, slam)
    n = 200
    est = torch.stack([sc.default_c2w(offset=(0.1 * np.sin(0.3 * k), 0.1 * np.cos(0.2 * k), 0.03 * np.sin(0.11 * k)), yaw=0.21 * k,
                                      pitch=0.3 * np.sin(0.17 * k)).cpu() for k in range(n)])
    pts = mask_inputs(m, sc, n_random=24000, seed=9)[:26000]         # 200 poses: ~0.8 % edge points by the f64 restatement
    amb = edge_points(pts, est.numpy(), None, 'frustum', m)
    assert amb.mean() <= 0.01, amb.mean()
    ref = m.point_masks(torch.from_numpy(pts), kfs, est.to(DEV), n - 1, DEV, get_mask_use_all_frames=True)[0]
    L = M.lib()
    calls = []
    real = L.adfp_mesh_seen_mask

    def counted(*a):
        calls.append(a[3])
        return real(*a)
    L.adfp_mesh_seen_mask = counted
    try:
        got = m.seen_mask(torch.from_numpy(pts).to(DEV), kfs, est.to(DEV), n - 1, DEV, get_mask_use_all_frames=True).cpu().numpy()
    finally:
        L.adfp_mesh_seen_mask = real
    assert calls == [n]
    diff = got != ref
    print(f'seen mask, {n} poses: {amb.sum()} edge points, {diff.sum()} differ, {(diff & ~amb).sum()} outside the edge set')
    assert not (diff & ~amb).any()
    assert 0.02 < ref.mean()


@pytest.mark.parametrize('depth_test', [False, True])
def test_seen_mask_reads_a_keyframe_store(depth_test):
    sc, sd, dec, cfg, slam, kfs, est, c = setup(depth_test=depth_test, n_kf=5)
    m = Mesher(cfg, None, slam)
    pts = torch.from_numpy(mask_inputs(m, sc, seed=2)).to(DEV)
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV, capacity=2)
    assert tuple(store.depths().shape) == (5, sc.H, sc.W) and tuple(store.depths(2).shape) == (2, sc.H, sc.W)
    a = m.seen_mask(pts, kfs, est, 4, DEV)
    b = m.seen_mask(pts, kfs, est, 4, DEV, keyframe_store=store)
    assert a.any() and torch.equal(a, b)


# ---- 5. get_mesh ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resolution', [24, 40])
@pytest.mark.parametrize('clean,depth_test,largest', [(False, False, False), (True, False, False), (True, True, False),
                                                      (True, False, True), (True, True, True)])
def test_get_mesh_equals_host_tail(tmp_path, resolution, clean, depth_test, largest):
    sc, sd, dec, cfg, slam, kfs, est, c = setup(resolution=resolution, depth_test=depth_test, largest=largest)
    m = Mesher(cfg, None, slam)
    out = tmp_path / 'mesh.ply'
    tsdf = sc.tsdf_volume.to(DEV)
    z = m.get_mesh(str(out), c, dec, kfs, est, 2, tsdf, DEV, color=True, clean_mesh=clean)
    assert z is not None and z.shape == (resolution,) * 3
    rec, faces = R.read_ply(str(out))
    # the host tail, from the returned lattice: what the parent commit's get_mesh did after marching cubes
    xyz = m.get_grid_uniform(resolution)['xyz']
    spacing, origin = m.marching_cubes_geometry(xyz)
    verts, f, _ = M.marching_cubes(torch.from_numpy(z).to(DEV), level=0.0, spacing=spacing, origin=origin, outward='lower')
    rv, rf = verts.cpu().numpy(), f.cpu().numpy()
    if clean:
        seen, _, _ = m.point_masks(verts, kfs, est, 2, device=DEV)
        rv, rf = m.clean(rv, rf, seen)
        assert 0 < len(rf) <= len(f)
    with torch.no_grad():
        raw = m.eval_points(torch.from_numpy(rv).to(DEV).float(), dec, tsdf, m.tsdf_bnds, c, 'color', DEV)[..., :3]
    col = (np.clip(raw.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
    rv, rf, col = merge_coincident(rv, rf, col)
    rv = rv / np.float32(m.scale)
    assert len(rf) > 0
    assert np.array_equal(faces, rf)
    assert np.array_equal(np.stack([rec['x'], rec['y'], rec['z']], 1), rv)
    assert np.array_equal(np.stack([rec['red'], rec['green'], rec['blue']], 1), col)


def test_get_mesh_without_a_surface_returns_none(tmp_path, capsys):
    sc, sd, dec, cfg, slam, kfs, est, c = setup(resolution=24, level_set=1e9)
    m = Mesher(cfg, None, slam)
    out = tmp_path / 'none.ply'
    assert m.get_mesh(str(out), c, dec, kfs, est, 2, sc.tsdf_volume.to(DEV), DEV) is None
    assert 'marching_cubes error' in capsys.readouterr().out
    assert not out.exists()


def test_get_mesh_takes_a_keyframe_store(tmp_path):
    sc, sd, dec, cfg, slam, kfs, est, c = setup(resolution=24, depth_test=True)
    m = Mesher(cfg, None, slam)
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    tsdf = sc.tsdf_volume.to(DEV)
    a, b = tmp_path / 'a.ply', tmp_path / 'b.ply'
    m.get_mesh(str(a), c, dec, kfs, est, 2, tsdf, DEV)
    m.get_mesh(str(b), c, dec, kfs, est, 2, tsdf, DEV, keyframe_store=store)
    assert a.read_bytes() == b.read_bytes()


def test_empty_inputs():
    """No vertices, no faces, no rows: empty tensors of the documented shape and dtype."""
    v0 = torch.zeros((0, 3), dtype=torch.float32, device=DEV)
    f0 = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    gv, gf = M.clean_components(v0, f0, torch.zeros(0, dtype=torch.bool, device=DEV), min_area=0.0)
    assert gv.shape == (0, 3) and gv.dtype == torch.float32 and gf.shape == (0, 3) and gf.dtype == torch.int32
    gv, gf = M.clean_components(v0, f0, torch.zeros(0, dtype=torch.uint8, device=DEV), largest=True)
    assert gv.shape == (0, 3) and gf.shape == (0, 3)
    assert M.face_components(f0, 0).shape == (0,)
    # coincident vertices that no face uses: merged all the same, the (empty) faces follow
    dup = np.array([[1, 2, 3], [4, 5, 6], [1, 2, 3]], np.float32)
    col = np.arange(9, dtype=np.uint8).reshape(3, 3)
    assert check_merge(dup, np.zeros((0, 3), np.int32), col) == 2
    out = M.color_bytes(torch.zeros((0, 4), dtype=torch.float32, device=DEV))
    assert out.shape == (0, 3) and out.dtype == torch.uint8


def test_seen_mask_without_keyframes_or_points():
    m = Mesher.__new__(Mesher)
    m.H, m.W, m.fx, m.fy, m.cx, m.cy, m.depth_test = 8, 8, 8.0, 8.0, 3.5, 3.5, False
    pts = torch.rand((5, 3), device=DEV)
    none = m.seen_mask(pts, [], torch.eye(4)[None], 0, DEV)
    assert none.shape == (5,) and none.dtype == torch.bool and not none.any()
    kf = [{'est_c2w': torch.eye(4), 'depth': torch.ones((8, 8))}]
    none = m.seen_mask(pts[:0], kf, torch.eye(4)[None], 0, DEV)
    assert none.shape == (0,) and none.dtype == torch.bool
