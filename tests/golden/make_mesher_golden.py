"""
Golden vectors for the Mesher (src/utils/Mesher.py).  The module imports open3d, trimesh and scikit-image at top level and
none of them is installed in the build container, so this script puts STUB modules under those names in sys.modules (and
for src.utils.datasets, whose cv2 import is absent too), imports the reference's own Mesher.py from /root/reference and
EXECUTES its methods on seeded inputs: the stored outputs come from the reference's code.  Nothing is written under the
reference (sys.dont_write_bytecode).  Build container only.

    python tests/golden/make_mesher_golden.py

mini_mesher.npz holds
  * grid.x / grid.y / grid.z      get_grid_uniform(resolution)['xyz'] (float64 axes);
  * masks.<case>.seen / .forecast / .unseen   point_masks on seeded points and keyframes, for depth_test on and off with the
    keyframe branch, and for the get_mask_use_all_frames branch;
  * mc.volume / mc.level / mc.spacing / mc.origin   what get_mesh hands to skimage.measure.marching_cubes (captured by a stub)
    and the origin it adds to the vertices, for the stub decoder `stub_decoder` below and a convex stub hull `HULL_PLANES`
    (`mesh_bound.contains`), with clean_mesh=False and color=False.
The stub decoder, the hull and the inputs are defined here and imported by tests/test_mesher_golden.py, which runs the port
on the same inputs.
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))

H, W, FX, FY, CX, CY = 24, 32, 28.0, 27.0, 15.5, 11.5
RESOLUTION = 20
POINTS_BATCH = 1000
BOUND = np.array([[-0.8, 0.7], [-0.6, 0.8], [-0.5, 0.6]])
MC_BOUND = [[-0.7, 0.6], [-0.5, 0.7], [-0.45, 0.5]]
# a box slightly smaller than the lattice, tilted: n . p + d <= 0 inside
_N = np.array([[1, 0.1, 0], [-1, 0.05, 0], [0, 1, -0.1], [0, -1, 0], [0.1, 0, 1], [0, 0, -1]], dtype=np.float64)
_N /= np.linalg.norm(_N, axis=1, keepdims=True)
HULL_PLANES = np.concatenate([_N, np.array([[-0.55], [-0.6], [-0.6], [-0.45], [-0.4], [-0.42]])], 1)


def cfg(depth_test):
    return {'scale': 1.0, 'occupancy': True,
            'meshing': {'resolution': RESOLUTION, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02,
                        'remove_small_geometry_threshold': 0.2, 'color_mesh_extraction_method': 'direct_point_query',
                        'get_largest_components': False, 'depth_test': depth_test},
            'mapping': {'marching_cubes_bound': MC_BOUND},
            'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0}}


def stub_decoder(p, c_grid=None, tsdf_volume=None, tsdf_bnds=None, stage='color'):
    """DF's call shape (decoder.py:307): p [1,N,3] -> (raw [1,N,4], w [1,N]).  Occupancy: a bumpy ball, from correctly rounded
    element-wise operations only (no transcendental functions, no reductions), so every CPU computes the same bits."""
    q = p[0].float()
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    r = torch.sqrt(x * x + y * y + z * z)
    occ = 0.45 - r + 0.3 * x * y - 0.2 * y * z
    rgb = torch.stack([q[:, 0] + 0.5, q[:, 1] * q[:, 1], 0.3 + 0.0 * q[:, 2]], -1)
    return torch.cat([rgb, occ[:, None]], -1)[None], torch.ones_like(occ)[None]


def keyframes():
    g = torch.Generator().manual_seed(7)
    kfs = []
    for k in range(3):
        yaw, pitch = 0.8 * k - 0.4, 0.15 * k - 0.1
        cy_, sy_, cp_, sp_ = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
        Rx = np.array([[1, 0, 0], [0, cp_, -sp_], [0, sp_, cp_]])
        c2w = np.eye(4)
        c2w[:3, :3] = Ry @ Rx
        c2w[:3, 3] = [0.1 * k, -0.05 * k, 0.9]
        depth = 0.5 + 1.5 * torch.rand(H, W, generator=g)
        depth[:, :3] = 0.0
        kfs.append({'est_c2w': torch.from_numpy(c2w).float(), 'depth': depth, 'color': torch.rand(H, W, 3, generator=g), 'idx': k})
    return kfs


def points():
    g = torch.Generator().manual_seed(11)
    return (torch.rand(2500, 3, generator=g, dtype=torch.float64) * 2.4 - 1.2).float()


def tsdf_inputs():
    g = torch.Generator().manual_seed(3)
    return torch.rand(1, 1, 6, 7, 8, generator=g) * 2 - 1, torch.from_numpy(BOUND.copy())


class Slam(object):
    def __init__(self):
        self.renderer = None
        self.bound = torch.from_numpy(BOUND.copy())
        self.verbose = False
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = H, W, FX, FY, CX, CY
        self.tsdf_bnds = torch.from_numpy(BOUND.copy())


MASK_CASES = {'keyframes_depth_test': (True, False), 'keyframes_no_depth_test': (False, False),
              'all_frames': (False, True)}


def _stub_modules(captured):
    skimage = types.ModuleType('skimage')
    skimage.__version__ = '0.19.3'
    measure = types.ModuleType('skimage.measure')

    def marching_cubes(volume, level, spacing):
        captured['volume'] = np.array(volume, copy=True)
        captured['level'] = level
        captured['spacing'] = np.array(spacing, dtype=np.float64)
        return (np.zeros((1, 3), np.float32), np.zeros((1, 3), np.int64), np.zeros((1, 3), np.float32), np.zeros(1, np.float32))
    measure.marching_cubes = marching_cubes
    skimage.measure = measure

    trimesh = types.ModuleType('trimesh')

    class Trimesh(object):
        def __init__(self, vertices=None, faces=None, vertex_colors=None, process=True):
            captured['vertices'] = np.array(vertices, dtype=np.float64, copy=True)

        def export(self, path):
            pass
    trimesh.Trimesh = Trimesh
    open3d = types.ModuleType('open3d')
    open3d.__version__ = '0.16.0'
    datasets = types.ModuleType('src.utils.datasets')
    datasets.get_dataset = lambda cfg, args, scale, device='cpu': []
    return {'skimage': skimage, 'skimage.measure': measure, 'trimesh': trimesh, 'open3d': open3d, 'src.utils.datasets': datasets}


class StubHull(object):
    def contains(self, pts):
        return (np.asarray(pts, np.float64) @ HULL_PLANES[:, :3].T + HULL_PLANES[:, 3]).max(1) <= 0


def main():
    sys.dont_write_bytecode = True
    import importlib.util
    captured = {}
    sys.modules.update(_stub_modules(captured))
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location('ref_mesher', os.path.join(REF, 'src', 'utils', 'Mesher.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    kfs = keyframes()
    est = torch.stack([kf['est_c2w'] for kf in kfs])
    pts = points()
    for name, (depth_test, all_frames) in MASK_CASES.items():
        m = mod.Mesher(cfg(depth_test), None, Slam(), points_batch_size=POINTS_BATCH)
        seen, fc, unseen = m.point_masks(pts, kfs, est, 2, 'cpu', get_mask_use_all_frames=all_frames)
        out[f'masks.{name}.seen'], out[f'masks.{name}.forecast'], out[f'masks.{name}.unseen'] = seen, fc, unseen
        assert seen.any() and (~seen).any(), name
    m = mod.Mesher(cfg(False), None, Slam(), points_batch_size=POINTS_BATCH)
    xyz = m.get_grid_uniform(RESOLUTION)['xyz']
    for k, a in zip('xyz', xyz):
        out[f'grid.{k}'] = np.asarray(a, dtype=np.float64)
    m.get_bound_from_frames = lambda keyframe_dict, scale: StubHull()
    tv, tb = tsdf_inputs()
    m.tsdf_bnds = tb
    z = m.get_mesh('unused.ply', {}, stub_decoder, kfs, est, 2, tv, device='cpu', color=False, clean_mesh=False)
    assert np.array_equal(z, captured['volume'])
    out['mc.volume'] = captured['volume'].astype(np.float32)
    out['mc.level'] = np.float64(captured['level'])
    out['mc.spacing'] = captured['spacing']
    out['mc.origin'] = captured['vertices'][0] * m.scale                  # vertices = verts (stub: 0) + origin, then / scale
    v = out['mc.volume']
    assert (v == 100).any() and (v > 0).any() and (v < 0).any()
    np.savez_compressed(os.path.join(OUT, 'mini_mesher.npz'), **out)
    print('wrote', os.path.join(OUT, 'mini_mesher.npz'), sorted(out))


if __name__ == '__main__':
    main()
