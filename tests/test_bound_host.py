"""CPU: the numpy statement of the mesh bound (mesh.depth_points_host, mesh.depth_hull_host) against Qhull over the full cloud and
against Mesher.get_bound_planes' own route, on the five seeded clouds of bound_clouds.py.  The device path is held to these
functions bit for bit in test_gpu_bound.py."""
import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

import bound_clouds as BC
from attentive_dfprior_amd import mesh


def planes_max(planes, p):
    m = np.full(len(p), -np.inf)
    for nx, ny, nz, d in planes:
        m = np.maximum(m, ((nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2]) + d)
    return m


def check_same_hull(ids_a, ids_b, ids, pts, eps, what):
    """Vertex sets agree; an id in one only must lie within 4 eps of the other hull's planes, and such ids are at most 1 %."""
    only_a, only_b = np.setdiff1d(ids_a, ids_b), np.setdiff1d(ids_b, ids_a)
    print(f'{what}: {len(ids_a)} / {len(ids_b)} vertices, {len(only_a)} + {len(only_b)} in one set only')
    for only, other in ((only_a, ids_b), (only_b, ids_a)):
        if len(only):
            planes = ConvexHull(pts[np.searchsorted(ids, other)]).equations
            assert np.abs(planes_max(planes, pts[np.searchsorted(ids, only)])).max() <= 4 * eps, what
    assert len(only_a) + len(only_b) <= 0.01 * len(ids_b), what


@pytest.mark.parametrize('name', ['mini', 'room0_random'])
def test_points_match_the_host_backprojection(name):
    sc, kfs = BC.cloud_keyframes(name)
    d = kfs[0]['depth']
    d[3, 20], d[4, 21], d[5, 22], d[6, 23], d[7, 24], d[8, 25] = float('nan'), float('inf'), -1.0, 1000.0, 999.0, -float('inf')
    ids, pts = mesh.depth_points_host(*BC.arrays(sc, kfs))
    rid, rpts, _ = BC.host_route(BC.mesher_for(sc), kfs)
    assert np.array_equal(ids, rid)                                   # the valid masks, NaN and inf depths included
    assert (np.diff(ids) > 0).all() and ids[0] == 0
    hw1 = sc.H * sc.W + 1
    assert not np.isin(1 + np.array([3 * sc.W + 20, 4 * sc.W + 21, 5 * sc.W + 22, 6 * sc.W + 23, 8 * sc.W + 25]), ids).any()
    assert np.isin(1 + 7 * sc.W + 24, ids) and np.isin(np.arange(len(kfs)) * hw1, ids).all()
    extent = float(np.ptp(rpts, 0).max())
    err = np.abs(pts - rpts).max()
    print(f'{name}: {len(ids)} points, max |difference| {err:.3e} = {err / np.spacing(extent):.2f} ulp of the extent {extent:.3f}')
    assert err <= 4 * np.spacing(extent)


@pytest.mark.parametrize('name', BC.NAMES)
def test_hull_equals_qhull_over_the_full_cloud(name):
    sc, kfs = BC.cloud_keyframes(name)
    args = BC.arrays(sc, kfs)
    ids, pts = mesh.depth_points_host(*args)
    eps = mesh.BOUND_EPS_REL * float(np.ptp(pts, 0).max())
    hid, hpts, stats = mesh.depth_hull_host(*args, return_stats=True)
    print(f'{name}: {len(ids)} points, {len(hid)} vertices, {len(stats)} rounds, survivors {[s[2] for s in stats]}')
    assert (np.diff(hid) > 0).all() and np.array_equal(hpts, pts[np.searchsorted(ids, hid)])
    assert stats[-1][2] == 0 and len(stats) <= mesh.BOUND_MAX_ROUNDS
    full = ids[np.sort(ConvexHull(pts).vertices)]
    check_same_hull(hid, full, ids, pts, eps, f'{name} against Qhull over the full cloud')
    _, _, union = BC.host_route(BC.mesher_for(sc), kfs)
    check_same_hull(hid, union, ids, pts, eps, f'{name} against the per-frame-then-union route')
    worst = planes_max(ConvexHull(hpts).equations, pts).max()           # containment of every point in the final hull
    print(f'{name}: max_f s_f over all points {worst:.3e}, eps {eps:.3e}')
    assert worst <= 4 * eps


def test_more_rounds_than_the_cap_raise():
    args = BC.cloud('mini_noise')
    _, _, stats = mesh.depth_hull_host(*args, return_stats=True)
    assert len(stats) > 2
    with pytest.raises(RuntimeError, match='rounds'):
        mesh.depth_hull_host(*args, max_rounds=2)


def test_non_finite_points_and_no_keyframes_raise():
    depth, c2w, fx, fy, cx, cy = BC.cloud('mini')
    bad = c2w.clone()
    bad[1, 0, 0] = float('nan')
    n_bad = int(((depth[1] > 0) & (depth[1] < 1000)).sum())            # every pixel point of keyframe 1; its centre stays finite
    with pytest.raises(ValueError, match=str(n_bad)):
        mesh.depth_hull_host(depth, bad, fx, fy, cx, cy)
    with pytest.raises(ValueError):
        mesh.depth_hull_host(depth[:0], c2w[:0], fx, fy, cx, cy)
    with pytest.raises(ValueError):
        BC.mesher_for(synthetic_mini()).bound_planes([], 1)


def synthetic_mini():
    from attentive_dfprior_amd import synthetic
    return synthetic.mini_scene()


def test_directions_hold_the_axes():
    d = mesh.bound_directions()
    assert d.shape == (mesh.BOUND_DIRECTIONS, 3) and d.dtype == np.float64
    assert np.array_equal(d[:6], [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-12
    assert np.array_equal(d, mesh.bound_directions())
    with pytest.raises(ValueError):
        mesh.bound_directions(5)
