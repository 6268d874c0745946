"""GPU: occlusion-aware visibility on the MI355X (adfp_points_visible, visibility.py) against the brute-force numpy oracle
tests/visible_ref.py, byte for byte: each pose alone at every leaf size, all poses together, more poses than one LDS stage, no
faces, out-of-range faces, a large eps, degenerate poses and points; cull_mesh(..., occlusion=True); unseen_points and its command
line; the 2D metric on the points it makes.  The fixture and its (non-marginal) classification: tests/test_visible_host.py."""
import inspect
import random

import numpy as np
import pytest
import torch

import depth_ref as D
import visible_ref as V
from attentive_dfprior_amd import _lib, cull_mesh, mesh, raycast, recon, recon_eval, visibility

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAM = (V.H, V.W, V.FX, V.FY, V.CX, V.CY)
CULL_CHUNK = 256                                       # ADFP_CULL_CHUNK (csrc/adfp_recon.h): poses per LDS stage


@pytest.fixture(scope='module')
def bvhs():
    v, f, _, _ = V.fixture()
    return {leaf: raycast.MeshBVH(v, f, DEV, leaf=leaf) for leaf in _lib.TRI_LEAVES}


def gpu(bvh, pts, poses, **kw):
    return visibility.points_visible(bvh, pts, poses, *CAM, **kw).cpu().numpy()


def differing(got, want):
    bad = np.flatnonzero(got != want)
    return len(bad), bad[:8], got[bad[:8]], want[bad[:8]]


@pytest.mark.parametrize('leaf', _lib.TRI_LEAVES)
@pytest.mark.parametrize('k', range(6))
def test_each_pose_alone(bvhs, leaf, k):
    _, _, pts, poses = V.fixture()
    fr, cl, _ = V.fixture_per_pose()
    want = (fr[k] & cl[k]).astype(np.uint8)
    got = gpu(bvhs[leaf], pts, [poses[k]])
    assert got.dtype == np.uint8 and got.shape == (516,)
    assert np.array_equal(got, want), differing(got, want)


@pytest.mark.parametrize('leaf', _lib.TRI_LEAVES)
def test_all_poses_together_are_the_or_of_each(bvhs, leaf):
    _, _, pts, poses = V.fixture()
    fr, cl, _ = V.fixture_per_pose()
    got = gpu(bvhs[leaf], pts, poses)
    single = np.stack([gpu(bvhs[leaf], pts, [p]) for p in poses])
    assert np.array_equal(got, single.any(0).astype(np.uint8)), differing(got, single.any(0).astype(np.uint8))
    assert np.array_equal(got, (fr & cl).any(0).astype(np.uint8))
    assert np.array_equal(gpu(bvhs[leaf], pts, poses[::-1]), got)          # the order of the poses does not matter


def perturbed(poses, n, rng):
    """n poses: `poses` themselves, then copies of them moved by up to 5 cm per axis."""
    out = list(poses)
    while len(out) < n:
        p = poses[len(out) % len(poses)].clone()
        p[:3, 3] += torch.from_numpy(rng.uniform(-0.05, 0.05, 3)).float()
        out.append(p)
    return out[:n]


def test_more_poses_than_one_lds_stage(bvhs):
    v, f, pts, poses = V.fixture()
    rng = np.random.default_rng(7)
    many = perturbed(poses, CULL_CHUNK + 44, rng)
    fr, cl, mg = V.per_pose(v, f, pts, many, *CAM)
    assert mg[fr].min() >= 1e-6
    want = (fr & cl).any(0).astype(np.uint8)
    got = gpu(bvhs[4], pts, many)
    assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(gpu(bvhs[4], pts, many), got)                    # two runs, the same bytes
    tail = gpu(bvhs[4], pts, many[CULL_CHUNK - 3:])                        # the stage boundary at another place
    assert np.array_equal(tail, (fr & cl)[CULL_CHUNK - 3:].any(0).astype(np.uint8))
    # a first stage of three poses' copies only: some points are seen from the second stage alone
    split = perturbed(poses[:3], CULL_CHUNK, rng) + perturbed(poses[3:], 44, rng)
    fr, cl, mg = V.per_pose(v, f, pts, split, *CAM)
    assert mg[fr].min() >= 1e-6
    first, both = (fr & cl)[:CULL_CHUNK].any(0), (fr & cl).any(0)
    assert (both & ~first).sum() >= 20
    got = gpu(bvhs[16], pts, split)
    assert np.array_equal(got, both.astype(np.uint8)), differing(got, both.astype(np.uint8))


def test_no_faces_is_frustum_seen():
    _, _, pts, poses = V.fixture()
    empty = raycast.MeshBVH(np.zeros((0, 3)), np.zeros((0, 3), np.int64), DEV)
    got = visibility.points_visible(empty, pts, poses, *CAM)
    want = recon.frustum_seen(pts, poses, *CAM, device=DEV)
    fr, _, _ = V.fixture_per_pose()
    assert torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), fr.any(0).astype(np.uint8))
    assert torch.equal(visibility.points_visible(empty, pts, [], *CAM), torch.zeros(516, dtype=torch.uint8, device=DEV))


def test_no_poses_and_no_points(bvhs):
    _, _, pts, poses = V.fixture()
    assert torch.equal(visibility.points_visible(bvhs[4], pts, [], *CAM), torch.zeros(516, dtype=torch.uint8, device=DEV))
    out = visibility.points_visible(bvhs[4], np.zeros((0, 3)), poses, *CAM)
    assert out.shape == (0,) and out.dtype == torch.uint8


def test_out_of_range_faces_never_occlude():
    v, f, pts, poses = V.fixture()
    fbad = np.concatenate([[[0, 5, 16]], f[:7], [[-1, 2, 3], [3, 2 ** 31 - 1, 1]], f[7:]])
    want = V.points_visible(v, f, pts, poses, *CAM)
    for leaf in _lib.TRI_LEAVES:
        got = gpu(raycast.MeshBVH(v, fbad, DEV, leaf=leaf), pts, poses)
        assert np.array_equal(got, want), (leaf,) + differing(got, want)


def test_large_eps_is_frustum_seen(bvhs):
    _, _, pts, poses = V.fixture()
    fr, cl, _ = V.fixture_per_pose()
    got = visibility.points_visible(bvhs[8], pts, poses, *CAM, eps=10.0)
    assert torch.equal(got, recon.frustum_seen(pts, poses, *CAM, device=DEV))
    assert np.array_equal(got.cpu().numpy(), fr.any(0).astype(np.uint8))
    assert not got.cpu().numpy()[~fr.any(0)].any()                         # outside every frustum: never seen, whatever eps


def test_near_clips_the_occluders(bvhs):
    """Hits nearer than `near` do not occlude: with near beyond the room nothing does."""
    v, f, pts, poses = V.fixture()
    fr, cl, _ = V.fixture_per_pose()
    want = V.points_visible(v, f, pts, poses, *CAM, near=1.5)
    got = gpu(bvhs[4], pts, poses, near=1.5)
    assert np.array_equal(got, want), differing(got, want)
    assert (want != (fr & cl).any(0)).any()                                # and that changes the answer
    assert np.array_equal(gpu(bvhs[4], pts, poses, near=100.0), fr.any(0).astype(np.uint8))


def raw(bvh, pts, w2c, c2w, eps=V.EPS, near=V.NEAR):
    """adfp_points_visible on explicit pose rows (w2c f32 [P,12], c2w f64 [P,12])."""
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).to(DEV)
    w = torch.from_numpy(np.ascontiguousarray(w2c, np.float32)).to(DEV)
    m = torch.from_numpy(np.ascontiguousarray(c2w, np.float64)).to(DEV)
    seen = torch.full((p.shape[0],), 7, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().adfp_points_visible(_lib.ptr(bvh.bvh), bvh.bvh.numel(), bvh.n_faces, bvh.leaf, _lib.ptr(p), p.shape[0],
                                              _lib.ptr(w), _lib.ptr(m), w.shape[0], V.FX, V.FY, V.CX, V.CY, V.W, V.H, near, eps,
                                              _lib.ptr(seen), _lib.current_stream(torch.device(DEV))), 'adfp_points_visible')
    return seen.cpu().numpy()


def test_pose_with_a_nan_sees_nothing(bvhs):
    _, _, pts, poses = V.fixture()
    fr, cl, _ = V.fixture_per_pose()
    w2c, c2w = recon.w2c_rows(poses), visibility.opencv_rows(poses)
    assert np.array_equal(raw(bvhs[4], pts, w2c, c2w), (fr & cl).any(0).astype(np.uint8))
    for e in (0, 7, 11):
        bad = c2w.copy()
        bad[2, e] = np.nan                                                 # pose 2 keeps its frustum rows: only the ray's pose is bad
        others = [k for k in range(6) if k != 2]
        want = (fr & cl)[others].any(0).astype(np.uint8)
        got = raw(bvhs[4], pts, w2c, bad)
        assert np.array_equal(got, want), (e,) + differing(got, want)
    bad = c2w.copy()
    bad[2, 3] = np.inf
    assert np.array_equal(raw(bvhs[4], pts, w2c[2:3], bad[2:3]), np.zeros(516, np.uint8))
    assert (fr[2] & cl[2]).any()


def test_point_at_and_behind_a_camera_centre(bvhs):
    v, f, _, poses = V.fixture()
    ms = V.opencv_rows(poses)
    o, zaxis = ms[0][:, 3], ms[0][:, 2]
    pts = np.stack([o, o - 0.5 * zaxis, o + 1e-3 * zaxis, o + 0.4 * zaxis, [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]])
    want = V.points_visible(v, f, pts, poses[:1], *CAM)
    got = gpu(bvhs[4], pts, poses[:1])
    assert np.array_equal(got, want), differing(got, want)
    assert want[0] == 0 and want[1] == 0 and want[3] == 1 and not want[4:].any()
    # the frustum rows of a pose that sees the point, the ray rows of a camera standing AT the point: z_p = 0, not visible
    w2c = recon.w2c_rows(poses[:1])
    at = visibility.opencv_rows(poses[:1])
    at[0, 3::4] = pts[3]
    assert raw(bvhs[4], pts[3:4], w2c, visibility.opencv_rows(poses[:1]))[0] == 1
    assert raw(bvhs[4], pts[3:4], w2c, at)[0] == 0


def grid_room(n=8):
    """The fixture's room and inner box with every quad cut into n x n cells, so that faces can lie wholly in the box's shadow."""
    v0, f0 = D.box_room(inner=V.INNER)
    vs, fs = [], []
    for q in range(0, len(f0), 2):                                         # box_room emits each quad as (a, b, c), (a, c, d)
        a, b, c = v0[f0[q]]
        d = v0[f0[q + 1][2]]
        s, t = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing='ij')
        g = a + s[..., None] * (b - a) + t[..., None] * (d - a)
        base = sum(len(x) for x in vs)
        vs.append(g.reshape(-1, 3))
        idx = base + np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
        for i in range(n):
            for j in range(n):
                fs.append((idx[i, j], idx[i + 1, j], idx[i + 1, j + 1]))
                fs.append((idx[i, j], idx[i + 1, j + 1], idx[i, j + 1]))
    return np.concatenate(vs), np.array(fs, np.int64)


def test_cull_mesh_with_occlusion():
    v, f = grid_room()
    poses = [V.look_at((1.5, 0.2, -0.6), (-1.0, -0.1, -0.6))]              # level with the box, the far wall behind it
    cam = dict(H=V.H, W=V.W, fx=V.FX, fy=V.FY, cx=V.CX, cy=V.CY)
    fr, cl, mg = V.per_pose(v, f, v, poses, *CAM)
    assert mg[fr].min() >= 1e-6
    want_occ = V.faces_kept((fr & cl).any(0), f)
    want_fru = V.faces_kept(fr.any(0), f)
    keep_occ = cull_mesh.cull_mesh(v, f, poses, occlusion=True, **cam)
    keep_fru = cull_mesh.cull_mesh(v, f, poses, occlusion=False, **cam)
    keep_def = cull_mesh.cull_mesh(v, f, poses, *CAM)
    assert keep_occ.dtype == bool and np.array_equal(keep_occ, want_occ)
    assert np.array_equal(keep_fru, want_fru) and np.array_equal(keep_def, want_fru)
    seen = recon.frustum_seen(v, poses, *CAM, device=DEV)                  # the parent's path, spelled out
    assert np.array_equal(keep_def, recon.faces_kept(seen, f).cpu().numpy().astype(bool))
    assert not (keep_occ & ~keep_fru).any()                                # occlusion only removes
    hidden = keep_fru & ~keep_occ
    wall = np.isclose(v[f][:, :, 0], -2.0).all(1)                          # the wall x = -2, beyond the box as the camera looks
    assert (hidden & wall).sum() >= 8, int((hidden & wall).sum())          # its faces in the box's shadow go
    assert (keep_occ & wall).any()                                         # the wall beside the shadow stays
    # a larger eps keeps more, and eps travels through cull_mesh
    assert np.array_equal(cull_mesh.cull_mesh(v, f, poses, occlusion=True, eps=10.0, **cam), want_fru)


def write_traj(path, poses):
    """traj.txt rows from which cull_mesh.load_poses returns `poses` (it negates columns 1 and 2)."""
    with open(path, 'w') as out:
        for p in poses:
            m = p.numpy().astype(np.float64)
            m[:3, 1] *= -1
            m[:3, 2] *= -1
            out.write(' '.join(repr(float(x)) for x in m.reshape(-1)) + '\n')


def test_unseen_points_and_command_line(tmp_path):
    v, f, _, poses = V.fixture()
    count, seed = 2000, 11
    cam = dict(H=V.H, W=V.W, fx=V.FX, fy=V.FY, cx=V.CX, cy=V.CY)
    got = visibility.unseen_points(v, f, poses, count=count, generator=torch.Generator().manual_seed(seed), **cam)
    pts, _ = recon.sample_surface(v, f, count, generator=torch.Generator().manual_seed(seed), device=DEV)
    pts = pts.cpu().numpy()
    fr, cl, mg = V.per_pose(v, f, pts, poses, *CAM)
    assert mg[fr].min() >= 1e-6                                            # no marginal decision among these samples either
    want = pts[~(fr & cl).any(0)]
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want)
    assert 100 < len(got) < count - 100

    # the command line: Replica's camera, the mesh as the PLY holds it (f32 vertices), the poses as load_poses reads them
    gt, traj, out = str(tmp_path / 'gt.ply'), str(tmp_path / 'traj.txt'), recon_eval.pc_unseen_file(str(tmp_path / 'gt_culled.ply'))
    mesh.write_ply(gt, v, f)
    write_traj(traj, poses)
    assert out.endswith('gt_culled_pc_unseen.npy')
    ret = visibility.main(['--input_mesh', gt, '--traj', traj, '--unseen_points', out, '--count', str(count), '--seed', str(seed)])
    m = mesh.read_ply(gt)
    read = cull_mesh.load_poses(traj)
    assert all(torch.equal(a, b) for a, b in zip(read, poses))
    api = visibility.unseen_points(m.verts, m.faces, read, count=count, generator=torch.Generator().manual_seed(seed))
    pts, _ = recon.sample_surface(m.verts, m.faces, count, generator=torch.Generator().manual_seed(seed), device=DEV)
    pts = pts.cpu().numpy()
    fr, cl, mg = V.per_pose(m.verts, m.faces, pts, read, cull_mesh.H, cull_mesh.W, cull_mesh.FX, cull_mesh.FY, cull_mesh.CX,
                            cull_mesh.CY, eps=visibility.OCCLUSION_EPS)
    assert mg[fr].min() >= 1e-6
    loaded = np.load(out)
    assert loaded.dtype == np.float64 and np.array_equal(loaded, api) and np.array_equal(loaded, ret)
    assert np.array_equal(loaded, pts[~(fr & cl).any(0)])
    assert np.array_equal(recon_eval.load_pc_unseen(str(tmp_path / 'gt_culled.ply')), loaded)


def test_metric_2d_runs_on_the_points(tmp_path):
    v, f, _, poses = V.fixture()
    pc = visibility.unseen_points(v, f, poses, count=2000, generator=torch.Generator().manual_seed(3), H=V.H, W=V.W, fx=V.FX,
                                  fy=V.FY, cx=V.CX, cy=V.CY)
    gt, rec = str(tmp_path / 'gt.ply'), str(tmp_path / 'rec.ply')
    mesh.write_ply(gt, v, f)
    mesh.write_ply(rec, v + np.array([0.01, 0.0, -0.01]), f)
    random.seed(5)
    np.random.seed(5)
    l1, views = recon_eval.metric_2d(rec, gt, align=False, pc_unseen=pc, n_imgs=4, chunk=2, device=DEV)
    assert len(views) == 4 and np.isfinite(l1) and l1 >= 0.0


def test_load_pc_unseen_is_untouched():
    src = inspect.getsource(recon_eval.load_pc_unseen)
    assert 'it is not built by cull_mesh.' in src and 'NICE-SLAM' in src
