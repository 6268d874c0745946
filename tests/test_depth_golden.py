"""CPU: the oracle of the 2D metric (tests/depth_ref.py) against the reference's own calc_2d_metric (tests/golden/
make_depth_golden.py: eval_recon.py run under stub open3d / trimesh), the port's helpers against the reference's signatures, and
recon_eval.oriented_bounds on known boxes.  The GPU tests (test_gpu_depth.py) hold the port to this oracle."""
import json
import os
import random
import sys

import numpy as np
import pytest

import depth_ref as D
from attentive_dfprior_amd import recon_eval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
import make_depth_golden as G  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'mini_depth.npz'))
    return {k: z[k] for k in z.files}


def cam_position():
    to_origin, extents = G.cam_box()
    extents = extents * np.array([0.3, 0.7, 0.7])
    transform = np.linalg.inv(to_origin)
    transform[2, 3] += 0.4
    return extents, transform


def seeded(s):
    np.random.seed(s)
    random.seed(s)


@pytest.mark.parametrize('seed', G.SEEDS)
def test_oracle_views_equal_reference(golden, seed):
    seeded(seed)
    views, n = D.sample_views(G.pc_unseen(), *cam_position(), G.N_IMGS)
    assert n == golden[f'calc2d.{seed}.candidates']
    assert np.array_equal(np.stack([np.linalg.inv(c) for c in views]), golden[f'calc2d.{seed}.extrinsics'])


@pytest.mark.parametrize('seed', G.SEEDS)
def test_calc_2d_metric_wiring(golden, seed):
    """The stub renders the oracle's depths at the reference's camera; the port's formula (per-view sums / (H W), f64 mean, x100)
    gives the reference's printed number up to its float32 means."""
    W, H, fx, fy, cx, cy = golden['intrinsics']
    assert (W, H, fx, fy, cx, cy) == (recon_eval.W_2D, recon_eval.H_2D, recon_eval.FOCAL_2D, recon_eval.FOCAL_2D, 249.5, 249.5)
    assert golden['z_far'] == recon_eval.FAR_2D and golden['back_face']
    seeded(seed)
    views, _ = D.sample_views(G.pc_unseen(), *cam_position(), G.N_IMGS)
    m = G.meshes()
    sums = []
    for c2w in views:
        d = [D.render_depth(v, f, c2w, 500, 500, fx, fy, cx, cy, D.near_of(v), 20.0) for v, f in (m['gt.ply'], m['rec.ply'])]
        sums.append(D.depth_l1_sums(d[0][None], d[1][None])[0])
    got = D.depth_l1_cm(sums, 500 * 500)
    assert got > 0.5
    assert abs(got - golden[f'calc2d.{seed}.printed']) <= 1e-5 * got


def test_signatures_equal_reference():
    import inspect
    with open(os.path.join(GOLDEN, 'depth_signatures.json')) as fh:
        sigs = json.load(fh)
    for name, sig in sigs.items():
        assert str(inspect.signature(getattr(recon_eval, name))) == sig, name


def test_volume_rectangular_matches_oracle():
    ext, T = cam_position()
    np.random.seed(3)
    a = recon_eval.volume_rectangular(ext, 7, T)
    np.random.seed(3)
    b = np.concatenate([D.volume_rectangular(ext, 1, T) for _ in range(7)])
    assert np.array_equal(a, b)                          # a batch consumes the stream as single draws do


def test_viewmatrix_is_the_reference_frame():
    m = recon_eval.viewmatrix(np.array([3.0, -1.0, 0.5]), [0, 0, -1], np.array([0.1, 0.2, 0.3]))
    assert np.array_equal(m, D.viewmatrix(np.array([3.0, -1.0, 0.5]), [0, 0, -1], np.array([0.1, 0.2, 0.3])))
    R = m[:, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-15) and np.linalg.det(R) > 0


def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@pytest.mark.parametrize('axis,angle', [((0, 0, 1), 0.0), ((0, 0, 1), 0.4), ((0.3, -0.5, 0.8), 1.1)])
def test_oriented_bounds_recovers_a_box(axis, angle):
    ext = np.array([3.0, 1.2, 2.1])                      # deliberately not ascending
    rng = np.random.default_rng(5)
    corners = np.array([[sx, sy, sz] for sx in (-.5, .5) for sy in (-.5, .5) for sz in (-.5, .5)]) * ext
    inside = (rng.random((400, 3)) - 0.5) * ext * 0.98
    R, t = rot(axis, angle), np.array([0.4, -2.0, 1.3])
    pts = np.concatenate([corners, inside]) @ R.T + t
    to_origin, extents = recon_eval.oriented_bounds(pts)
    assert np.allclose(extents, [1.2, 2.1, 3.0], atol=1e-9)          # ascending
    A = to_origin[:3, :3]
    assert np.allclose(A @ A.T, np.eye(3), atol=1e-12) and np.linalg.det(A) > 0.999   # a rotation: right-handed
    local = pts @ A.T + to_origin[:3, 3]
    assert (np.abs(local) <= extents / 2 + 1e-9).all()                # every vertex inside the box, centred at the origin
    assert np.allclose(np.abs(local).max(0), extents / 2, atol=1e-9)
    # the smallest extent lies along the box's own 1.2 axis
    assert abs(abs(A[0] @ (R @ np.array([0.0, 1.0, 0.0]))) - 1) < 1e-9


def test_get_cam_position_scales_smallest_middle_largest(tmp_path):
    from attentive_dfprior_amd import mesh
    v, f = G.meshes()['gt.ply']
    p = str(tmp_path / 'gt.ply')
    mesh.write_ply(p, v, f)
    extents, transform = recon_eval.get_cam_position(p)
    assert np.allclose(extents, [2.5 * 0.3, 3.0 * 0.7, 4.0 * 0.7], atol=1e-12)
    centre = transform[:3, 3]
    assert np.allclose(centre, [0.0, 0.0, 0.05 + 0.4], atol=1e-12)
    assert np.allclose(np.abs(transform[:3, :3]), np.abs(G.cam_box()[0][:3, :3]).T, atol=1e-12)


def test_missing_pc_unseen_names_the_file(tmp_path):
    with pytest.raises(FileNotFoundError) as e:
        recon_eval.load_pc_unseen(str(tmp_path / 'room0.ply'))
    msg = str(e.value)
    assert 'room0_pc_unseen.npy' in msg and 'unseen-region points' in msg and 'NICE-SLAM' in msg and 'not built by cull_mesh' in msg


def test_oracle_render_basics():
    """The oracle itself: a wall straight ahead at z = 2, the near plane cutting a slanted floor, nothing beyond far."""
    v = np.array([[-5, -5, 2.0], [5, -5, 2.0], [0, 5, 2.0]])
    f = np.array([[0, 1, 2]])
    d = D.render_depth(v, f, np.eye(4), 9, 11, 10.0, 10.0, 5.0, 4.0, 0.1, 20.0)
    assert (d == np.float32(2.0)).all()
    assert (D.render_depth(v, f, np.eye(4), 9, 11, 10.0, 10.0, 5.0, 4.0, 0.1, 1.5) == 0).all()
    assert (D.render_depth(v, f[:, ::-1], np.eye(4), 9, 11, 10.0, 10.0, 5.0, 4.0, 0.1, 20.0) == d).all()   # back faces count
    assert (D.render_depth(v, np.array([[0, 1, 7]]), np.eye(4), 9, 11, 10.0, 10.0, 5.0, 4.0, 0.1, 20.0) == 0).all()
