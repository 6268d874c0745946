"""The seeded clouds of the mesh-bound tests (test_bound_host.py, test_gpu_bound.py), built on the CPU from `synthetic` so that
both suites see the same bits: the mini scene's three keyframes of test_gpu_mesher.py and the room0 box room at 480 x 640, without
and with depth noise.  The noise-free clouds are exactly planar walls (ties by construction)."""
import math

import numpy as np
import torch

from attentive_dfprior_amd import synthetic

NAMES = ('mini', 'mini_noise', 'room0', 'room0_noise', 'room0_random')


def room0_scene():
    """synthetic.Scene('room0') without its feature grids and TSDF volume (730 MB): what depth_image reads."""
    sc = synthetic.Scene.__new__(synthetic.Scene)
    sc.name = 'room0'
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = 480, 640, 577.6, 577.6, 319.5, 239.5
    sc.bound = synthetic.scene_bound(synthetic.SCENE_BOUNDS['room0'])
    b = sc.bound.clone().double()
    sc.lo_in, sc.hi_in = (b[:, 0] + 0.6).float().double(), (b[:, 1] - 0.6).float().double()
    sc.device = 'cpu'
    sc.center = ((sc.lo_in + sc.hi_in) / 2).tolist()
    return sc


def mini_poses(sc):
    return [sc.default_c2w(offset=(0.05 * k, -0.04 * k, 0.02), yaw=0.9 * k, pitch=0.1 * k - 0.1) for k in range(3)]


def room0_poses(sc, n=6):
    return [sc.default_c2w(offset=(0.1 * k, -0.05 * k, 0.0), yaw=1.2 * k, pitch=-0.1) for k in range(n)]


def random_poses(sc, n, seed):
    rng = np.random.default_rng(seed)
    return [sc.default_c2w(offset=tuple(rng.uniform(-0.5, 0.5, 3)), yaw=float(rng.uniform(0, 2 * math.pi)),
                           pitch=float(rng.uniform(-0.3, 0.3))) for _ in range(n)]


def keyframes(sc, poses, noise=0.0, seed=0, zero_band=0.08):
    """keyframe dicts as the Mapper keeps them (host tensors); depth noise is multiplicative gaussian."""
    g = torch.Generator().manual_seed(seed)
    kfs = []
    for k, c2w in enumerate(poses):
        d = sc.depth_image(c2w, zero_band=zero_band).cpu()
        if noise:
            d = (d * (1.0 + noise * torch.randn(d.shape, generator=g))).float()
        kfs.append({'est_c2w': c2w.cpu(), 'depth': d, 'color': torch.zeros(sc.H, sc.W, 3), 'idx': k})
    return kfs


def cloud_keyframes(name):
    """(scene, keyframe dicts) of one of NAMES."""
    if name.startswith('mini'):
        sc = synthetic.mini_scene()
        return sc, keyframes(sc, mini_poses(sc), 0.01 if name == 'mini_noise' else 0.0, seed=11)
    sc = room0_scene()
    if name == 'room0':
        return sc, keyframes(sc, room0_poses(sc), 0.0, zero_band=0.05)
    if name == 'room0_noise':
        return sc, keyframes(sc, room0_poses(sc), 0.01, seed=12, zero_band=0.05)
    if name == 'room0_random':
        return sc, keyframes(sc, random_poses(sc, 10, seed=13), 0.02, seed=14, zero_band=0.05)
    raise KeyError(name)


def arrays(sc, kfs):
    """(depth [K,H,W] f32, c2w [K,4,4] f32, fx, fy, cx, cy): the arguments of mesh.depth_hull / depth_hull_host."""
    return (torch.stack([kf['depth'] for kf in kfs]).float(), torch.stack([kf['est_c2w'] for kf in kfs]).float(),
            sc.fx, sc.fy, sc.cx, sc.cy)


def cloud(name):
    return arrays(*cloud_keyframes(name))


class Slam(object):
    pass


def mesher_for(sc, resolution=48, device='cpu'):
    """A mesher.Mesher over the scene's intrinsics; only the bound methods are usable without a renderer."""
    from attentive_dfprior_amd.mesher import Mesher
    cfg = {'scale': 1, 'occupancy': True,
           'meshing': {'resolution': resolution, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02, 'remove_small_geometry_threshold': 0.0002,
                       'color_mesh_extraction_method': 'direct_point_query', 'get_largest_components': False, 'depth_test': False},
           'mapping': {'marching_cubes_bound': sc.bound.tolist()}}
    slam = Slam()
    slam.bound, slam.verbose, slam.renderer, slam.tsdf_bnds = sc.bound, False, None, None
    slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
    return Mesher(cfg, None, slam)


def host_route(m, kfs):
    """get_bound_planes' own back-projection and per-frame-then-union hull, unscaled: (ids, points) of every valid point as it forms
    them (cam @ R.T + t through BLAS), and the ids of the union hull's vertices."""
    from scipy.spatial import ConvexHull
    H, W, fx, fy, cx, cy = m.H, m.W, m.fx, m.fy, m.cx, m.cy
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ids, pts, hid, hpt = [], [], [], []
    for k, keyframe in enumerate(kfs):
        c2w = keyframe['est_c2w'].cpu().numpy().astype(np.float64)
        c2w[:3, 1] *= -1.0
        c2w[:3, 2] *= -1.0
        depth = keyframe['depth'].cpu().numpy().astype(np.float64)
        with np.errstate(invalid='ignore'):
            ok = (depth > 0) & (depth < 1000)
        d = depth[ok]
        cam = np.stack([(u[ok] - cx) / fx * d, (v[ok] - cy) / fy * d, d], 1)
        frame = np.concatenate([c2w[:3, 3][None], cam @ c2w[:3, :3].T + c2w[:3, 3]], 0)
        fid = k * (H * W + 1) + np.concatenate([[0], 1 + np.flatnonzero(ok.reshape(-1))]).astype(np.int64)
        ids.append(fid)
        pts.append(frame)
        keep = np.sort(ConvexHull(frame).vertices)
        hid.append(fid[keep])
        hpt.append(frame[keep])
    hid, hpt = np.concatenate(hid), np.concatenate(hpt)
    return np.concatenate(ids), np.concatenate(pts), hid[np.sort(ConvexHull(hpt).vertices)]
