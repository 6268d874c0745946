"""GPU: reconstruction evaluation on the MI355X against scipy's cKDTree, the reference's golden values
(tests/golden/mini_recon.npz) and the CPU oracle tests/recon_ref.py: the exact nearest-neighbour index and query, the three
metrics, area-weighted sampling, ICP, calc_3d_metric end to end, the frustum cull and both command lines; every kernel run twice
gives the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as R
from attentive_dfprior_amd import cull_mesh, mesh, recon, recon_eval
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_recon_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'mini_recon.npz'))
    return {k: z[k] for k in z.files}


def extent(*clouds):
    a = np.concatenate([np.asarray(c).reshape(-1, 3) for c in clouds], 0)
    return float(np.ptp(a, 0).max()) if len(a) else 1.0


def d_to(ref, query, idx):
    """f64 distance of each query to ref[idx], in the kernel's order: sqrt((dx*dx + dy*dy) + dz*dz)."""
    r = ref[idx]
    dx, dy, dz = r[:, 0] - query[:, 0], r[:, 1] - query[:, 1], r[:, 2] - query[:, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def check_nn(ref, query, radius=np.inf, sort_queries=True):
    ext = extent(ref, query)
    index = recon.NNIndex(torch.from_numpy(ref).to(DEV))
    d, i = index.query(torch.from_numpy(query).to(DEV), radius=radius, sort_queries=sort_queries)
    d2, i2 = index.query(torch.from_numpy(query).to(DEV), radius=radius, sort_queries=sort_queries)
    assert torch.equal(d, d2) and torch.equal(i, i2)                       # bitwise deterministic
    d, i = d.cpu().numpy(), i.cpu().numpy().astype(np.int64)
    rd, ri = R.nn(ref, query, radius)
    found, rfound = i >= 0, np.isfinite(rd)
    near_r = np.isfinite(radius) & (np.abs(np.where(rfound, rd, radius) - radius) <= 1e-12 * ext)
    if np.isfinite(radius):
        assert not ((found != rfound) & ~near_r).any()                        # -1 exactly where cKDTree finds nothing below r
    both = found & rfound
    assert np.abs(d[both] - rd[both]).max(initial=0) <= 1e-12 * ext
    # cKDTree computes sqrt((dx*dx + dy*dy) + dz*dz) as the kernel does, and both return the exact minimum of those values:
    # the distances agree to the last bit, not only to 1e-12 (ties may pick different indices)
    assert np.array_equal(d[both], rd[both])
    assert np.array_equal(d[found], d_to(ref, query[found], i[found]))      # the distance of the returned point, to the bit
    assert np.isinf(d[~found]).all()
    return d, i, rd


@pytest.mark.parametrize('sort_queries', [True, False])
def test_nn_uniform_200k(sort_queries):
    rng = np.random.default_rng(0)
    check_nn(rng.random((200000, 3)) * 4 - 2, rng.random((200000, 3)) * 4 - 2, sort_queries=sort_queries)


@pytest.mark.parametrize('case', ['room', 'offset', 'lattice'])
def test_nn_golden_clouds(case):
    gt, rec = G.clouds()[case]
    check_nn(gt, rec)
    check_nn(rec, gt)


def test_nn_small_and_empty():
    rng = np.random.default_rng(1)
    check_nn(rng.random((1, 3)), rng.random((1000, 3)))
    check_nn(rng.random((17, 3)), rng.random((333, 3)))
    index = recon.NNIndex(torch.from_numpy(rng.random((50, 3))).to(DEV))
    d, i = index.query(torch.zeros((0, 3), dtype=torch.float64, device=DEV))
    assert d.shape == (0,) and i.shape == (0,)


@pytest.mark.parametrize('radius', [0.01, 0.05, 0.3])
def test_nn_radius(radius):
    gt, rec = G.clouds()['room']
    _, i, _ = check_nn(gt, rec, radius=radius)
    assert (i >= 0).any() and (i < 0).any() or radius == 0.3


def adversarial_cloud(case):
    """(ref, query), about 20 000 each: clouds on which the Morton order says little about where a point's neighbours are."""
    rng = np.random.default_rng(31)
    n = 20000
    if case == 'duplicates':                                                 # 5 000 copies of one point: many leaves hold nothing else
        p = np.array([0.25, -0.5, 0.75])
        ref = np.concatenate([np.repeat(p[None], 5000, 0), rng.uniform(-2, 2, (15000, 3))])[rng.permutation(n)]
        return ref, np.concatenate([np.repeat(p[None], 10, 0), ref[:1990], rng.uniform(-2, 2, (n - 2000, 3))])
    if case == 'cluster':                                                    # 15 000 points in one cell of the 1024^3 lattice
        c = np.array([0.3, 0.3, 0.3])
        ref = np.concatenate([c + rng.uniform(-1e-6, 1e-6, (15000, 3)), rng.uniform(-1000, 1000, (5000, 3))])[rng.permutation(n)]
        lo, side = ref.min(0), np.ptp(ref, 0)                                # k_nn_morton's lattice over the box of the references
        cell = np.floor(np.clip((ref - lo) * (1024.0 / side), 0.0, 1023.0))
        assert len(np.unique(cell[np.abs(ref - c).max(1) <= 1e-6], axis=0)) == 1 and len(np.unique(cell, axis=0)) > 4000
        # half of the queries near the cluster (inside it and about it, a ten-thousandth of a cell away), half uniform
        near = np.concatenate([c + rng.uniform(-2e-6, 2e-6, (n // 4, 3)), c + rng.normal(0, 2e-4, (n // 4, 3))])
        return ref, np.concatenate([near, rng.uniform(-1000, 1000, (n // 2, 3))])
    if case == 'line':                                                       # leaf boxes are thin diagonal slivers
        t = rng.uniform(-2, 2, n)
        ref = np.array([0.1, -0.2, 0.3]) + t[:, None] * np.array([1.0, 0.5, -0.25])
        return ref, rng.uniform(-2, 2, (n, 3))
    if case == 'plane':                                                      # z = const exactly: leaf boxes of zero thickness
        ref = np.concatenate([rng.uniform(-2, 2, (n, 2)), np.full((n, 1), 0.375)], 1)
        q = rng.uniform(-2, 2, (n, 3))
        q[np.abs(q[:, 2] - 0.375) < 1e-3, 2] += 0.01                         # every query off the plane
        return ref, q
    raise KeyError(case)


@pytest.mark.parametrize('sort_queries', [True, False])
@pytest.mark.parametrize('case', ['duplicates', 'cluster', 'line', 'plane'])
def test_nn_adversarial_clouds(case, sort_queries):
    ref, q = adversarial_cloud(case)
    d, i, rd = check_nn(ref, q, sort_queries=sort_queries)
    if case == 'duplicates':
        assert (d[:2000] == 0).all() and (ref[i[:10]] == q[:10]).all()       # the point itself; any of its copies will do
    if case == 'line':
        assert (d > 0).all()
    if case == 'plane':
        assert (d >= 1e-3).all()


@pytest.mark.parametrize('sort_queries', [True, False])
def test_nn_cluster_radius(sort_queries):
    ref, q = adversarial_cloud('cluster')
    _, i, _ = check_nn(ref, q, radius=50.0, sort_queries=sort_queries)
    assert (i[:10000] >= 0).all() and (i[10000:] >= 0).any() and (i[10000:] < 0).any()


@pytest.mark.parametrize('n', [1, 15, 16, 17, 31, 32, 33, 16 * 1024 + 1])
def test_nn_reference_counts(n):
    """Around one and two leaves of ADFP_NN_LEAF = 16 points, and one point more than a full last level of 1024 leaves."""
    rng = np.random.default_rng(100 + n)
    ref, q = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1.2, 1.2, (1000, 3))
    for sort_queries in (True, False):
        check_nn(ref, q, sort_queries=sort_queries)


def test_nn_transform_on_the_fly():
    rng = np.random.default_rng(2)
    ref, q = rng.random((5000, 3)), rng.random((4000, 3))
    T = np.eye(4)
    c, s = np.cos(0.1), np.sin(0.1)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [0.05, -0.02, 0.01]
    index = recon.NNIndex(torch.from_numpy(ref).to(DEV))
    d, i = index.query(torch.from_numpy(q).to(DEV), transform=T)
    qt = R.apply_transform(q, T)
    rd, _ = R.nn(ref, qt)
    assert np.abs(d.cpu().numpy() - rd).max() <= 1e-12
    assert np.array_equal(d.cpu().numpy(), d_to(ref, qt, i.cpu().numpy().astype(np.int64)))


@pytest.mark.parametrize('case', ['room', 'offset', 'lattice'])
def test_metrics_equal_reference(golden, case):
    gt, rec = G.clouds()[case]
    for fn, key in ((recon_eval.accuracy, 'accuracy'), (recon_eval.completion, 'completion')):
        got = fn(gt, rec)
        assert isinstance(got, float)
        assert abs(got - golden[f'metric.{case}.{key}']) <= 1e-12 * abs(golden[f'metric.{case}.{key}'])
    rd = R.nn(rec, gt)[0]
    ext = extent(gt, rec)
    for th, key in ((0.05, 'ratio05'), (0.02, 'ratio02')):
        got = recon_eval.completion_ratio(torch.from_numpy(gt).to(DEV), torch.from_numpy(rec).to(DEV), th)
        slack = int((np.abs(rd - th) <= 1e-12 * ext).sum())               # points whose distance is within rounding of dist_th
        assert abs(got * len(gt) - golden[f'metric.{case}.{key}'] * len(gt)) <= slack + 1e-6


def test_metric_sums_deterministic():
    d = torch.rand(1234567, dtype=torch.float64, device=DEV)
    a, b = recon.metric_sums(d, 0.3), recon.metric_sums(d, 0.3)
    assert a == b
    assert abs(a[0] - float(d.sum())) <= 1e-9 * a[0] and a[1] == float((d < 0.3).sum())


def test_sampling_equals_oracle():
    v, f = R.room_mesh()
    rng = np.random.default_rng(7)
    uf, ub = rng.random(200000), rng.random((200000, 2))
    uf[:5] = [0.0, 1e-300, 0.5, 1 - 1e-16, 0.999]
    pts, fi = recon.sample_surface(v, f, u_face=torch.from_numpy(uf).to(DEV), u_bary=torch.from_numpy(ub).to(DEV))
    pts2, fi2 = recon.sample_surface(v, f, u_face=torch.from_numpy(uf).to(DEV), u_bary=torch.from_numpy(ub).to(DEV))
    assert torch.equal(pts, pts2) and torch.equal(fi, fi2)
    rp, rf, cum = R.sample_surface(v, f, uf, ub)
    fi, pts = fi.cpu().numpy(), pts.cpu().numpy()
    u = uf * cum[-1]
    edge = np.abs(cum[np.clip(rf, 0, len(cum) - 1)] - u) <= 1e-12 * cum[-1]     # draws within rounding of a cumulative boundary
    edge |= np.abs(cum[np.clip(rf - 1, 0, len(cum) - 1)] - u) <= 1e-12 * cum[-1]
    diff = fi != rf
    assert not (diff & ~edge).any(), np.nonzero(diff & ~edge)[0][:10]
    assert diff.sum() <= 20
    same = ~diff
    assert np.abs(pts[same] - rp[same]).max() <= 1e-12 * extent(v)


def test_sampling_never_picks_a_zero_area_face():
    """searchsorted(side='left') on a non-decreasing cumulative sum never returns a face of zero area for a draw above 0: every
    other face here is degenerate, over many scan tiles, so a cumulative sum that stepped down at a thread or tile boundary
    would show."""
    v, f = R.room_mesh()
    deg = np.stack([f[:, 0], f[:, 0], f[:, 1]], 1)                      # zero area
    ff = np.stack([f, deg], 1).reshape(-1, 3)
    rng = np.random.default_rng(11)
    uf = rng.random(400000)
    _, _, cum = R.sample_surface(v, ff, uf[:1], np.zeros((1, 2)))
    uf[:len(cum) // 2] = cum[1::2][:len(cum) // 2] / cum[-1]              # draws on the cumulative boundaries themselves
    uf = np.clip(uf, 1e-300, None)
    _, fi = recon.sample_surface(v, ff, u_face=torch.from_numpy(uf).to(DEV), u_bary=torch.from_numpy(rng.random((400000, 2))).to(DEV))
    fi = fi.cpu().numpy()
    assert (R.areas(v, ff)[fi] > 0).all()


def room_pair():
    """(src, tgt): the room meshed on the GPU at 4 cm, moved by ~3 degrees and ~5 cm, onto the oracle's room at 5 cm."""
    from attentive_dfprior_amd import synthetic
    b = torch.tensor([[-2.0, 2.0], [-1.5, 1.5], [-1.2, 1.3]], dtype=torch.float64)
    tv, bn, _ = synthetic.make_box_room_tsdf(b, voxel=0.04, inset=0.4)
    vol = tv[0, 0].permute(2, 1, 0).contiguous().to(DEV)
    v, f, _ = mesh.marching_cubes(vol, 0.0, (0.04,) * 3, tuple(bn[:, 0].tolist()))
    a = np.deg2rad(3.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [0.03, 0.02, -0.035]
    src = R.apply_transform(v.double().cpu().numpy(), T)
    tgt, tf = R.room_mesh()
    return src, f.cpu().numpy(), tgt, tf


def test_icp_equals_oracle():
    src, _, tgt, _ = room_pair()
    r = recon_eval.registration_icp(src, tgt)
    r2 = recon_eval.registration_icp(torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV))
    assert np.array_equal(r.transformation, r2.transformation)
    T, fit, rmse, it = R.icp(src, tgt)
    assert r.iterations == it
    assert np.abs(r.transformation - T).max() <= 1e-9
    assert abs(r.fitness - fit) <= 1e-9 and abs(r.inlier_rmse - rmse) <= 1e-9


def write_pair(tmp_path):
    src, sf, tgt, tf = room_pair()
    rec_p, gt_p = str(tmp_path / 'rec.ply'), str(tmp_path / 'gt.ply')
    mesh.write_ply(rec_p, src, sf)
    mesh.write_ply(gt_p, tgt, tf)
    return rec_p, gt_p


@pytest.mark.parametrize('align', [False, True])
def test_calc_3d_metric_end_to_end(tmp_path, align):
    rec_p, gt_p = write_pair(tmp_path)
    got = recon_eval.metric_3d(rec_p, gt_p, align, generator=torch.Generator().manual_seed(5), count=200000)
    again = recon_eval.metric_3d(rec_p, gt_p, align, generator=torch.Generator().manual_seed(5), count=200000)
    assert got == again
    g = torch.Generator().manual_seed(5)
    draws = [(torch.rand(200000, dtype=torch.float64, generator=g).numpy(),
              torch.rand((200000, 2), dtype=torch.float64, generator=g).numpy()) for _ in range(2)]
    rec, gt = mesh.read_ply(rec_p), mesh.read_ply(gt_p)
    T = R.icp(rec.verts, gt.verts)[0] if align else None
    want = R.metric_3d(rec.verts, rec.faces, gt.verts, gt.faces, draws[0], draws[1], T)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9 * abs(want[k]), (k, got[k], want[k])
    if align:
        assert got['accuracy'] < 1.0 and got['completion_ratio'] > 90.0


def test_cull_equals_reference(golden, tmp_path):
    v, f, traj = G.cull_inputs()
    p = tmp_path / 'traj.txt'
    p.write_text(traj)
    poses = cull_mesh.load_poses(str(p))
    keep = cull_mesh.cull_mesh(v, f, poses)
    assert np.array_equal(keep, cull_mesh.cull_mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), poses))
    seen = recon.frustum_seen(v, poses, 680, 1200, 600., 600., 599.5, 339.5)
    assert torch.equal(seen, recon.frustum_seen(v, poses, 680, 1200, 600., 600., 599.5, 339.5))
    near = R.near_border(v, [c.numpy() for c in poses])
    bad = keep != golden['cull.keep']
    listed = near[f].any(1)
    assert not (bad & ~listed).any(), np.nonzero(bad & ~listed)[0][:10]
    _, rseen = R.cull_mask(v, f, [c.numpy() for c in poses])
    sbad = seen.cpu().numpy().astype(bool) != rseen
    assert not (sbad & ~near).any()


def test_cull_many_poses_staged():
    v, f, _ = G.cull_inputs()
    rng = np.random.default_rng(4)
    poses = []
    for _ in range(600):                                           # more than one LDS chunk of poses
        a = rng.uniform(-np.pi, np.pi)
        c2w = np.eye(4)
        c2w[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        c2w[:3, 3] = rng.uniform(-1, 1, 3)
        poses.append(torch.from_numpy(c2w).float())
    keep = cull_mesh.cull_mesh(v, f, poses)
    rkeep, _ = R.cull_mask(v, f, [c.numpy() for c in poses])
    near = R.near_border(v, [c.numpy() for c in poses])
    assert not ((keep != rkeep) & ~near[f].any(1)).any()


def check_culled_file(inp, outp, poses):
    """The cull command line's output: every input vertex with its properties, and exactly the faces of the in-process device
    mask, which equals the oracle's except for faces touching a vertex listed as within rounding of a frustum border."""
    m_in, m_out = mesh.read_ply(inp), mesh.read_ply(outp)
    assert np.array_equal(m_out.vertex, m_in.vertex)                      # every vertex kept, properties included
    keep = cull_mesh.cull_mesh(m_in.verts, m_in.faces, poses)
    assert keep.any() and (~keep).any()
    assert np.array_equal(m_out.faces, m_in.faces[keep])
    rkeep, _ = R.cull_mask(m_in.verts, m_in.faces, [c.numpy() for c in poses])
    listed = R.near_border(m_in.verts, [c.numpy() for c in poses])[m_in.faces].any(1)
    assert not ((keep != rkeep) & ~listed).any()


def test_command_lines(tmp_path):
    rec_p, gt_p = write_pair(tmp_path)
    v, f, traj = G.cull_inputs()
    (tmp_path / 'traj.txt').write_text(traj)
    inp, outp, gtc = str(tmp_path / 'in.ply'), str(tmp_path / 'out.ply'), str(tmp_path / 'gt_culled.ply')
    mesh.write_ply(inp, v, f)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    run = [sys.executable, '-m', 'attentive_dfprior_amd.cull_mesh', '--input_mesh', inp, '--traj', str(tmp_path / 'traj.txt'),
           '--output_mesh', outp]
    subprocess.run(run, check=True, cwd=str(tmp_path), env=env, timeout=300)
    poses = cull_mesh.load_poses(str(tmp_path / 'traj.txt'))
    check_culled_file(inp, outp, poses)
    # score the GPU room against a culled ground truth, through the reference's command line
    subprocess.run(run[:4] + [gt_p, '--traj', str(tmp_path / 'traj.txt'), '--output_mesh', gtc], check=True, env=env, timeout=300)
    check_culled_file(gt_p, gtc, poses)
    r = subprocess.run([sys.executable, '-m', 'attentive_dfprior_amd.recon_eval', '--rec_mesh', rec_p, '--gt_mesh', gtc, '-3d'],
                       check=True, env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert [ln.split(':')[0] for ln in lines] == ['accuracy', 'completion', 'completion ratio']
    assert all(np.isfinite(float(ln.split(':')[1])) for ln in lines)
    r = subprocess.run([sys.executable, '-m', 'attentive_dfprior_amd.recon_eval', '--rec_mesh', rec_p, '--gt_mesh', gtc, '-2d'],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and 'not built' in r.stderr


def test_empty_inputs():
    """V = 0, F = 0, P = 0 views, M = 0 queries: empty or all-zero tensors of the documented shape and dtype, or the ValueError."""
    none3 = torch.zeros((0, 3), dtype=torch.float64, device=DEV)
    index = recon.NNIndex(none3)
    assert index.n == 0
    d, i = index.query(none3)
    assert d.shape == (0,) and d.dtype == torch.float64 and i.shape == (0,) and i.dtype == torch.int32
    with pytest.raises(ValueError, match='holds no points'):
        index.query(torch.zeros((1, 3), dtype=torch.float64, device=DEV))
    assert recon.metric_sums(torch.zeros(0, dtype=torch.float64, device=DEV), 0.05) == (0.0, 0.0)
    eye = np.eye(4)
    tgt = torch.rand((5, 3), dtype=torch.float64, device=DEV)
    no_idx = torch.zeros(0, dtype=torch.int32, device=DEV)
    for t in (tgt, none3):
        m = recon.icp_moments(none3, eye, (0.0, 0.0, 0.0), t, no_idx)
        assert m.shape == (17,) and m.dtype == np.float64 and (m == 0).all()
    v, f = R.room_mesh(0.2)
    u = torch.zeros(0, dtype=torch.float64, device=DEV)
    pts, fi = recon.sample_surface(v, f, u_face=u, u_bary=u.reshape(0, 2), device=DEV)
    assert pts.shape == (0, 3) and pts.dtype == torch.float64 and fi.shape == (0,) and fi.dtype == torch.int32
    pts, fi = recon.sample_surface(v, f[:0], u_face=u, u_bary=u.reshape(0, 2), device=DEV)      # no draws: the faces are not looked at
    assert pts.shape == (0, 3) and fi.shape == (0,)
    with pytest.raises(ValueError, match='no faces'):
        recon.sample_surface(v, f[:0], 3, device=DEV)
    poses = [torch.eye(4) for _ in range(3)]
    cam = (680, 1200, 600., 600., 599.5, 339.5)
    seen = recon.frustum_seen(np.zeros((0, 3)), poses, *cam, device=DEV)
    assert seen.shape == (0,) and seen.dtype == torch.uint8
    seen = recon.frustum_seen(v, [], *cam, device=DEV)
    assert seen.shape == (len(v),) and seen.dtype == torch.uint8 and (seen == 0).all()
    keep = recon.faces_kept(seen, f[:0])
    assert keep.shape == (0,) and keep.dtype == torch.uint8
    keep = recon.faces_kept(seen[:0].contiguous(), np.zeros((0, 3), np.int64))
    assert keep.shape == (0,)
