"""GPU: mesh depth rendering on the MI355X against the numpy oracle tests/depth_ref.py, bit for bit: the synthetic room from inside
(views along a wall: zero-thickness leaf boxes, rays parallel to box faces), a plane whose vertices lie on pixel-centre rays, the
near and far planes, degenerate and out-of-range faces, no faces, odd image sizes, every leaf size, reruns; views_in_sight against
the oracle's check_proj; metric_2d end to end on a seeded stream; the -2d command line."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_ref as D
import recon_ref as R
from attentive_dfprior_amd import _lib, mesh, raycast, recon_eval
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_depth_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def pose(R3, o):
    m = np.eye(4)
    m[:3, :3] = R3
    m[:3, 3] = o
    return m


def look(direction, o, up=(0, 0, -1)):
    m = np.eye(4)
    m[:3, :] = recon_eval.viewmatrix(np.asarray(direction, np.float64), list(up), np.asarray(o, np.float64))
    return m


def check(verts, faces, c2ws, H, W, fx, fy, cx, cy, near, far, leaf=_lib.TRI_LEAF_DEFAULT):
    bvh = raycast.MeshBVH(verts, faces, DEV, leaf=leaf)
    got = bvh.render_depth(np.stack(c2ws), H, W, fx, fy, cx, cy, near, far)
    again = bvh.render_depth(np.stack(c2ws), H, W, fx, fy, cx, cy, near, far)
    assert torch.equal(got, again)                                           # a rerun gives the same bits
    got = got.cpu().numpy()
    nears = np.broadcast_to(np.asarray(near, np.float64), (len(c2ws),))
    for k, c2w in enumerate(c2ws):
        want = D.render_depth(verts, faces, c2w, H, W, fx, fy, cx, cy, nears[k], far)
        bad = got[k] != want
        assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:5], got[k][bad][:5], want[bad][:5])
    return got


def room_views():
    v, f = R.room_mesh(0.2)
    lo, hi = v.min(0), v.max(0)
    wall_x = float(lo[0])                                                    # a wall plane of the mesh (axis-aligned)
    views = [look((1.0, 0.3, 0.1), (-1.0, 0.2, 0.1)),
             look((-0.4, -1.0, 0.5), (0.5, 0.8, -0.3)),
             pose(np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (-1.2, -0.5, 0.0)),   # axis-aligned, along +x
             pose(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]), (wall_x + 0.05, -1.0, 0.2)),  # along a wall
             pose(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]]), (wall_x, 0.0, 0.0))]  # on the wall's plane
    return v, f, views


def test_room_from_inside():
    v, f, views = room_views()
    got = check(v, f, views, 40, 48, 30.0, 30.0, 24.0, 20.0, 0.05, 20.0)     # cx, cy whole: rows / columns with d.x or d.y = 0
    assert (got[:3] > 0).mean() > 0.9                                        # inside the room: nearly every pixel sees a wall


def test_leaf_sizes_agree():
    v, f, views = room_views()
    outs = [check(v, f, views[:3], 33, 37, 30.0, 30.0, 18.0, 16.5, 0.05, 20.0, leaf=b) for b in _lib.TRI_LEAVES]
    assert all(np.array_equal(outs[0], o) for o in outs[1:])


def test_plane_on_pixel_centre_rays():
    """Vertices exactly on pixel-centre rays: rays through shared edges and vertices.  A closed surface shows no background."""
    H, W, fx, fy, cx, cy = 33, 41, 16.0, 16.0, 20.0, 16.0
    z = 2.0
    cols, rows = np.arange(0, W, 4), np.arange(0, H, 4)
    xs, ys = z * ((cols - cx) / fx), z * ((rows - cy) / fy)                   # the kernel's d, times a power of two: exact
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1)
    nc = len(cols)
    f = []
    for r in range(len(rows) - 1):
        for c in range(nc - 1):
            a, b, d, e = r * nc + c, r * nc + c + 1, (r + 1) * nc + c, (r + 1) * nc + c + 1
            f += [(a, b, e), (a, e, d)] if (r + c) % 2 else [(a, b, d), (b, e, d)]     # both diagonals
    f = np.array(f)
    got = check(v, f, [np.eye(4)], H, W, fx, fy, cx, cy, 0.1, 20.0)[0]
    inside = got[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    assert (inside == np.float32(z)).all()                                   # every covered pixel, edges and vertices included


def test_near_plane_far_plane_and_bad_faces():
    # a slanted floor crossing the near plane, a back wall behind it, a wall beyond far, and faces to ignore
    v = np.array([[-4, 1.0, -1.0], [4, 1.0, -1.0], [0, -1.5, 6.0],           # straddles z = near
                  [-30, -30, 5.0], [30, -30, 5.0], [0, 30, 5.0],              # back wall at z = 5
                  [-9, -9, 25.0], [9, -9, 25.0], [0, 9, 25.0],                # beyond far
                  [0, 0, 1.0], [1, 1, 1.0], [2, 2, 1.0]])                     # collinear
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [9, 9, 10], [0, 1, -1], [3, 4, 12], [2, 2 ** 30, 5]])
    views = [np.eye(4), pose(np.eye(3), (0.3, -0.2, 0.4))]
    got = check(v, f, views, 29, 35, 20.0, 20.0, 17.0, 14.0, 0.8, 20.0)
    assert (got > 0).all() and (got <= 5.0).all()                            # the clipped floor shows the back wall; nothing at 25
    assert (got[0] == np.float32(5.0)).any() and (got[0] < 5.0).any()
    only_bad = check(v, f[[4, 5, 6, 7, 2]], views, 29, 35, 20.0, 20.0, 17.0, 14.0, 0.8, 20.0)
    assert (only_bad == 0).all()


def test_no_faces_and_no_views():
    bvh = raycast.MeshBVH(np.zeros((3, 3)), np.zeros((0, 3), np.int64), DEV)
    d = bvh.render_depth(np.stack([np.eye(4)] * 3), 17, 9, 10.0, 10.0, 4.0, 8.0, 0.1, 20.0)
    assert d.shape == (3, 17, 9) and (d == 0).all()
    assert raycast.MeshBVH(*R.room_mesh(0.2), DEV).render_depth(np.zeros((0, 4, 4)), 8, 8, 1.0, 1.0, 4.0, 4.0, 0.1, 20.0).numel() == 0


def test_per_view_near():
    v, f, views = room_views()
    check(v, f, views[:3], 24, 24, 20.0, 20.0, 11.5, 11.5, np.array([0.05, 0.9, 1.7]), 20.0)


def test_views_in_sight_equals_check_proj():
    pts = G.pc_unseen()
    rng = np.random.default_rng(3)
    c2ws = []
    for _ in range(300):                                                     # more than one LDS chunk of poses
        o = rng.uniform([-1.5, -1.0, -0.5], [1.5, 1.0, 1.0])
        c2ws.append(look(rng.normal(size=3), o))
    got = raycast.views_in_sight(torch.from_numpy(pts).to(DEV), c2ws, 500, 500, 300.0, 300.0, 249.5, 249.5).cpu().numpy()
    want = np.array([D.check_proj(pts, 500, 500, 300.0, 300.0, 249.5, 249.5, c) for c in c2ws])
    assert np.array_equal(got, want) and want.any() and (~want).any()
    assert all(bool(recon_eval.check_proj(pts, 500, 500, 300.0, 300.0, 249.5, 249.5, c)) == w for c, w in zip(c2ws[:20], want))
    assert not raycast.views_in_sight(np.zeros((0, 3)), c2ws[:4], 500, 500, 300.0, 300.0, 249.5, 249.5, DEV).any()


def test_depth_l1_sums():
    rng = np.random.default_rng(2)
    a = rng.uniform(0, 5, (3, 37, 29)).astype(np.float32)
    b = np.where(rng.random(a.shape) < 0.3, 0, a + rng.normal(0, 0.05, a.shape)).astype(np.float32)
    got = raycast.depth_l1_sums(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert torch.equal(got, raycast.depth_l1_sums(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)))
    want = D.depth_l1_sums(a, b)
    assert np.allclose(got.cpu().numpy(), want, rtol=1e-13, atol=0)


def write_rooms(tmp_path):
    m = G.meshes()
    gt_p, rec_p = str(tmp_path / 'gt.ply'), str(tmp_path / 'rec.ply')
    mesh.write_ply(gt_p, *m['gt.ply'])
    mesh.write_ply(rec_p, *m['rec.ply'])
    return rec_p, gt_p


def test_metric_2d_equals_oracle(tmp_path):
    rec_p, gt_p = write_rooms(tmp_path)
    pts = G.pc_unseen()
    recon_eval.setup_seed(20)
    l1, views = recon_eval.metric_2d(rec_p, gt_p, align=False, n_imgs=5, pc_unseen=pts, chunk=2, device=DEV)
    extents, transform = recon_eval.get_cam_position(gt_p)
    np.random.seed(20)
    random.seed(20)
    want_views, n = D.sample_views(pts, extents, transform, 5)
    assert n > 5 and len(views) == 5
    assert all(np.array_equal(a, b) for a, b in zip(views, want_views))    # the views the sequential loop accepts
    gt, rec = mesh.read_ply(gt_p), mesh.read_ply(rec_p)
    sums = []
    for c2w in want_views:
        dg = D.render_depth(gt.verts, gt.faces, c2w, 500, 500, 300.0, 300.0, 249.5, 249.5, D.near_of(gt.verts), 20.0)
        dr = D.render_depth(rec.verts, rec.faces, c2w, 500, 500, 300.0, 300.0, 249.5, 249.5, D.near_of(rec.verts), 20.0)
        sums.append(D.depth_l1_sums(dg[None], dr[None])[0])
    want = D.depth_l1_cm(sums, 500 * 500)
    assert want > 0.5 and abs(l1 - want) <= 1e-9 * want


def test_command_line_2d(tmp_path):
    rec_p, gt_p = write_rooms(tmp_path)
    np.save(str(tmp_path / 'gt_pc_unseen.npy'), G.pc_unseen())
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'attentive_dfprior_amd.recon_eval', '--rec_mesh', rec_p, '--gt_mesh', gt_p, '-2d'],
                       check=True, env=env, capture_output=True, text=True, timeout=600)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith('Depth L1:')
    assert np.isfinite(float(lines[0].split(':')[1]))


def test_no_views_and_no_pixels():
    pts = torch.rand((7, 3), dtype=torch.float64, device=DEV)
    none = raycast.views_in_sight(pts, [], 500, 500, 300.0, 300.0, 249.5, 249.5)
    assert none.shape == (0,) and none.dtype == torch.bool
    a = torch.zeros((0, 5, 4), dtype=torch.float32, device=DEV)
    got = raycast.depth_l1_sums(a, a.clone())
    assert got.shape == (0,) and got.dtype == torch.float64
    b = torch.zeros((3, 0), dtype=torch.float32, device=DEV)                 # three views of no pixels
    got = raycast.depth_l1_sums(b, b.clone())
    assert got.shape == (3,) and got.dtype == torch.float64 and (got == 0).all()
