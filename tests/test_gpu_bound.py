"""GPU: the mesh bound on the device (mesh.depth_hull, Mesher.bound_planes; csrc/adfp_bound.h) against its numpy statement
(mesh.depth_hull_host), bit for bit and round for round, on the clouds of bound_clouds.py; against Mesher.get_bound_planes within
the rounding of that route's BLAS product; and get_mesh routed through it."""
import numpy as np
import pytest
import torch

import bound_clouds as BC
from attentive_dfprior_amd import mesh
from attentive_dfprior_amd.keyframes import KeyframeStore
from attentive_dfprior_amd.mesher import Mesher

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def on_device(args):
    return (args[0].to(DEV), args[1].to(DEV)) + tuple(args[2:])


def same_rounds(dev_stats, host_stats):
    assert len(dev_stats) == len(host_stats)
    for r, (d, h) in enumerate(zip(dev_stats, host_stats)):
        assert np.array_equal(d[0], h[0]), f'round {r}: vertex ids'
        assert np.array_equal(d[1].view(np.int64), h[1].view(np.int64)), f'round {r}: planes'
        assert d[2] == h[2], f'round {r}: survivors {d[2]} on the device, {h[2]} on the host'
        assert np.array_equal(d[3], h[3]), f'round {r}: farthest ids'


def test_points_equal_the_host_statement_bit_for_bit():
    args = BC.cloud('room0')
    depth, c2w = args[0].clone(), args[1]
    depth[2, 7, 100], depth[2, 8, 101], depth[2, 9, 102], depth[2, 10, 103] = float('nan'), float('inf'), 1000.0, -0.0
    args = (depth, c2w) + tuple(args[2:])
    ids, pts = mesh.depth_points_host(*args)
    b = mesh._DeviceBound(*on_device(args))
    every = np.arange(b.n_ids, dtype=np.int64)
    got = b.points(every)
    assert np.array_equal(got[ids].view(np.int64), pts.view(np.int64))
    rest = np.ones(b.n_ids, bool)
    rest[ids] = False
    assert rest.sum() > 0 and np.isnan(got[rest]).all()
    assert np.isnan(b.points(np.array([-1, b.n_ids, 2 ** 40], np.int64))).all()          # ids out of range are never dereferenced


def test_support_pass_equals_the_host_statement():
    args = BC.cloud('room0_noise')
    host, dev = mesh._HostBound(*args), mesh._DeviceBound(*on_device(args))
    for D in (64, 70, 300):                          # one slice set, a ragged one, two chunks of directions
        dirs = mesh.bound_directions(D)
        hb, hbox, hn, hbad = host.support(dirs)
        db, dbox, dn, dbad = dev.support(dirs)
        assert np.array_equal(hb, db) and (hn, hbad) == (dn, dbad) and hbad == 0
        assert np.array_equal(hbox.view(np.int64), dbox.view(np.int64))
        assert np.array_equal(host.pts[np.searchsorted(host.ids, hb[:6]), [0, 0, 1, 1, 2, 2]], hbox[[3, 0, 4, 1, 5, 2]])   # the AABB falls out


@pytest.mark.parametrize('name', BC.NAMES)
def test_hull_equals_the_host_statement_round_by_round(name):
    args = BC.cloud(name)
    hid, hpts, hstats = mesh.depth_hull_host(*args, return_stats=True)
    did, dpts, dstats = mesh.depth_hull(*on_device(args), return_stats=True)
    print(f'{name}: {len(did)} vertices, survivors {[s[2] for s in dstats]}')
    same_rounds(dstats, hstats)
    assert np.array_equal(did, hid) and np.array_equal(dpts.view(np.int64), hpts.view(np.int64))


@pytest.mark.parametrize('name', ['room0', 'mini_doubled'])
def test_ties_give_the_same_result_twice(name):
    """The noise-free planar room, and a keyframe appended twice so that every point has a duplicate of higher id."""
    if name == 'mini_doubled':
        sc, kfs = BC.cloud_keyframes('mini_noise')
        args = BC.arrays(sc, kfs + [kfs[1]])
    else:
        args = BC.cloud(name)
    a = mesh.depth_hull(*on_device(args), return_stats=True)
    b = mesh.depth_hull(*on_device(args), return_stats=True)
    same_rounds(a[2], b[2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
    h = mesh.depth_hull_host(*args, return_stats=True)
    same_rounds(a[2], h[2])
    assert np.array_equal(a[0], h[0])
    if name == 'mini_doubled':
        hw1 = args[0].shape[1] * args[0].shape[2] + 1
        assert (a[0] < 3 * hw1).all()               # of two equal points the lower id is the vertex


def test_survivor_buffer_overflow_is_rerun_in_full(monkeypatch):
    args = BC.cloud('mini')
    want = mesh.depth_hull(*on_device(args), return_stats=True)
    assert want[2][0][2] > 64
    monkeypatch.setattr(mesh, '_BOUND_CAP_ALL', 64)
    got = mesh.depth_hull(*on_device(args), return_stats=True)
    same_rounds(got[2], want[2])
    assert np.array_equal(got[0], want[0])


def test_error_paths_on_the_device():
    depth, c2w, fx, fy, cx, cy = on_device(BC.cloud('mini'))
    bad = c2w.clone()
    bad[1, 0, 0] = float('nan')
    n_bad = int(((depth[1] > 0) & (depth[1] < 1000)).sum())
    with pytest.raises(ValueError, match=str(n_bad)):
        mesh.depth_hull(depth, bad, fx, fy, cx, cy)
    with pytest.raises(RuntimeError, match='rounds'):
        mesh.depth_hull(depth, c2w, fx, fy, cx, cy, max_rounds=2)
    with pytest.raises(ValueError):
        mesh.depth_hull(depth[:0], c2w[:0], fx, fy, cx, cy)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        mesh.depth_hull(depth.cpu(), c2w, fx, fy, cx, cy)


def test_many_planes_are_taken_in_chunks():
    """More planes than one LDS chunk (512) and than the LDS farthest table (4096): a classify call against the host statement."""
    args = BC.cloud('mini_noise')
    host, dev = mesh._HostBound(*args), mesh._DeviceBound(*on_device(args))
    rng = np.random.default_rng(5)
    n = rng.normal(size=(4500, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    c = host.pts.mean(0)
    planes = np.ascontiguousarray(np.concatenate([n, (-(n @ c) - rng.uniform(0.2, 0.9, 4500))[:, None]], 1))
    hc, hn, hfid, hfd = host.classify(None, planes, 1e-12)
    (dt, dn), dn2, dfid, dfd = dev.classify(None, planes, 1e-12)
    assert hn == dn == dn2 and 0 < hn < len(host.ids)
    assert np.array_equal(dt[:dn].cpu().numpy(), hc)
    assert np.array_equal(dfid, hfid) and np.array_equal(dfd.view(np.int64), hfd.view(np.int64))
    assert (hfid[4096:] >= 0).any() and (hfid[:512] >= 0).any()
    hc2, hn2, hfid2, _ = host.classify(hc, planes[:700], 0.05)              # a later round: an explicit candidate list
    (dt2, _), dn3, dfid2, _ = dev.classify((dt, dn), planes[:700], 0.05)
    assert hn2 == dn3 and np.array_equal(dt2[:dn3].cpu().numpy(), hc2) and np.array_equal(dfid2, hfid2)


def support_function(planes, dirs):
    """h(u) = max over the hull's vertices of u . v, from its facet planes [F,4] (the vertices are recovered with Qhull)."""
    from scipy.optimize import linprog
    from scipy.spatial import HalfspaceIntersection
    cheb = linprog([0, 0, 0, -1], A_ub=np.concatenate([planes[:, :3], np.ones((len(planes), 1))], 1), b_ub=-planes[:, 3],
                   bounds=[(None, None)] * 4)                      # the centre of the largest inscribed ball: strictly inside
    assert cheb.success and cheb.x[3] > 0
    v = HalfspaceIntersection(planes, cheb.x[:3]).intersections
    return (dirs @ v.T).max(1)


@pytest.mark.parametrize('name', ['mini', 'room0_noise'])
def test_bound_planes_against_the_host_route(name):
    sc, kfs = BC.cloud_keyframes(name)
    m = BC.mesher_for(sc)
    host = m.get_bound_planes(kfs, 1)
    from_dict = m.bound_planes(kfs, 1, DEV)
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    from_store = m.bound_planes(kfs, 1, DEV, keyframe_store=store)
    assert np.array_equal(from_dict.view(np.int64), from_store.view(np.int64))
    rng = np.random.default_rng(2)
    dirs = rng.normal(size=(2000, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    _, pts = mesh.depth_points_host(*BC.arrays(sc, kfs))
    extent = float(np.ptp(pts, 0).max())
    diff = np.abs(support_function(host, dirs) - support_function(from_dict, dirs)).max()
    print(f'{name}: support functions differ by {diff:.3e} = {diff / extent:.3e} of the extent')
    assert diff <= 1e-9 * extent


@pytest.mark.parametrize('res', [48, 64])
def test_hull_fill_marks_the_same_lattice_points(res):
    sc, kfs = BC.cloud_keyframes('mini')
    m = BC.mesher_for(sc, resolution=res)
    xyz = m.get_grid_uniform(res)['xyz']
    ax = [torch.from_numpy(a.astype(np.float32)).to(DEV) for a in xyz]
    P = np.stack(np.meshgrid(*[a.astype(np.float32) for a in xyz], indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    marks, near = [], np.zeros(len(P), bool)
    for planes in (m.get_bound_planes(kfs, 1), m.bound_planes(kfs, 1, DEV)):
        z = torch.zeros((res, res, res), dtype=torch.float32, device=DEV)
        mesh.hull_fill(z, ax, planes, 100.)
        marks.append(z.cpu().numpy().reshape(-1) == 100.)
        near |= np.abs((P @ planes[:, :3].T + planes[:, 3]).max(1)) < 1e-9
    print(f'{res}^3: {near.sum()} lattice points within 1e-9 of a bound, {(marks[0] != marks[1]).sum()} marked differently')
    assert marks[0].any() and (~marks[0]).any()
    assert near.mean() <= 1e-3
    assert np.array_equal(marks[0][~near], marks[1][~near])


def test_get_mesh_runs_on_bound_planes_alone(tmp_path, monkeypatch):
    import test_gpu_mesher as T
    sc, sd, dec, cfg, slam, kfs, est, c = T.setup()
    m = Mesher(cfg, None, slam)

    def gone(*a, **k):
        raise AssertionError('get_mesh called the host bound')
    monkeypatch.setattr(Mesher, 'get_bound_planes', gone)
    out = tmp_path / 'mesh.ply'
    tsdf = sc.tsdf_volume.to(DEV)
    z = m.get_mesh(str(out), c, dec, kfs, est, 2, tsdf, DEV, color=True, clean_mesh=True)
    assert out.exists() and len(mesh.read_ply(str(out)).faces) > 0
    want, ax = m.lattice(c, dec, tsdf, m.get_grid_uniform(48)['xyz'], DEV)
    mesh.hull_fill(want, ax, m.bound_planes(kfs, 1, DEV), 100.)
    assert np.array_equal(z, want.cpu().numpy()) and (z == 100.).any()
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    z2 = m.get_mesh(str(tmp_path / 'mesh2.ply'), c, dec, kfs, est, 2, tsdf, DEV, color=True, clean_mesh=True, keyframe_store=store)
    assert np.array_equal(z, z2) and (tmp_path / 'mesh2.ply').read_bytes() == out.read_bytes()


def test_points_of_no_ids():
    b = mesh._DeviceBound(*on_device(BC.cloud('mini')))
    got = b.points(np.zeros(0, np.int64))
    assert got.shape == (0, 3) and got.dtype == np.float64
