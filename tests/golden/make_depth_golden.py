"""
Golden vectors for the 2D metric of the reference's src/tools/eval_recon.py (calc_2d_metric, :139-219).  The script imports
open3d and trimesh at module level, and neither is installed in the build container.  This script puts STUB open3d / trimesh
modules into sys.modules (as make_recon_golden.py does), makes torch.Tensor.cuda an identity (check_proj then runs on the CPU),
and EXECUTES the reference's own calc_2d_metric with align=False on two small box rooms, after the reference's own setup_seed:
  * trimesh.bounds.oriented_bounds returns the fixed (to_origin, extents) of `cam_box()`; trimesh.sample.volume_rectangular is
    tests/depth_ref.py's restatement (numpy's global stream);
  * the stub Visualizer records every PinholeCameraParameters it is given, the intrinsics, z_far and mesh_show_back_face, and its
    capture_depth_float_buffer returns depth_ref.render_depth of the geometry last added, at the pose check_proj last screened
    (asserted to be the one whose inverse is the recorded extrinsic), near = 0.01 x that mesh's largest AABB extent, far = z_far.
Nothing is written under the reference (sys.dont_write_bytecode).  Build container only.

    python tests/golden/make_depth_golden.py

mini_depth.npz holds, per seed s in SEEDS: calc2d.<s>.extrinsics [n, 4, 4] (in the order the views were set), calc2d.<s>.candidates
(how many candidates check_proj screened), calc2d.<s>.printed (the printed Depth L1); and intrinsics (W, H, fx, fy, cx, cy),
z_far, back_face.  depth_signatures.json holds inspect.signature of the reference's helpers.
"""
import contextlib
import inspect
import io
import json
import os
import sys
import types

import numpy as np
import scipy.spatial  # noqa: F401  (imported before np.bool is restored below: numpy.ma breaks on it)
import torch

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import depth_ref  # noqa: E402

SEEDS = (20, 7)
N_IMGS = 5


def meshes():
    """{'gt.ply': (verts, faces), 'rec.ply': (verts, faces)}: a box room with a crate in it, and the same room with its walls and
    the crate moved by a few centimetres."""
    gt = depth_ref.box_room(inner=((0.5, -0.8, -1.2), (1.3, 0.2, -0.4)))
    rec = depth_ref.box_room((-2.03, -1.48, -1.2), (2.0, 1.52, 1.27), inner=((0.45, -0.8, -1.2), (1.3, 0.25, -0.35)))
    return {'gt.ply': gt, 'rec.ply': rec}


def pc_unseen():
    """Unseen-region points: a patch of the ceiling above one corner and a column behind the crate."""
    rng = np.random.default_rng(11)
    a = np.stack([rng.uniform(-2.0, -1.2, 300), rng.uniform(0.8, 1.5, 300), np.full(300, 1.3)], 1)
    b = np.stack([np.full(100, 1.35), rng.uniform(-0.7, 0.1, 100), rng.uniform(-1.2, -0.5, 100)], 1)
    return np.concatenate([a, b])


def cam_box():
    """(to_origin, extents) of the ground truth's box as trimesh.bounds.oriented_bounds orders it: extents ascending (z, y, x),
    axes (z, y, -x) right-handed, the box centred at the origin."""
    to_origin = np.eye(4)
    to_origin[:3, :3] = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]
    to_origin[:3, 3] = -(to_origin[:3, :3] @ np.array([0.0, 0.0, 0.05]))
    return to_origin, np.array([2.5, 3.0, 4.0])


class _Mesh(object):
    def __init__(self, name, verts, faces):
        self.name, self.verts, self.faces = name, verts, faces


def _stubs(log):
    trimesh = types.ModuleType('trimesh')
    sample = types.ModuleType('trimesh.sample')
    bounds = types.ModuleType('trimesh.bounds')
    trimesh.load = lambda path, **k: _Mesh(path, *meshes()[path])

    def oriented_bounds(m, *a, **k):
        t, e = cam_box()
        return t.copy(), e.copy()
    bounds.oriented_bounds = oriented_bounds
    sample.volume_rectangular = depth_ref.volume_rectangular
    trimesh.sample, trimesh.bounds = sample, bounds

    open3d = types.ModuleType('open3d')
    open3d.__version__ = '0.16.0'
    o3io = types.SimpleNamespace(read_triangle_mesh=lambda path: _Mesh(path, *meshes()[path]))
    open3d.io = o3io

    class PinholeCameraIntrinsic(object):
        def __init__(self, *a):
            log['intrinsics'].append(tuple(float(x) for x in a))

    class PinholeCameraParameters(object):
        extrinsic = None
        intrinsic = None
    open3d.camera = types.SimpleNamespace(PinholeCameraIntrinsic=PinholeCameraIntrinsic,
                                          PinholeCameraParameters=PinholeCameraParameters)

    class Ctr(object):
        z_far, param = None, None

        def set_constant_z_far(self, z):
            self.z_far = float(z)
            log['z_far'].add(self.z_far)

        def convert_from_pinhole_camera_parameters(self, param):
            self.param = param

    class Visualizer(object):
        def __init__(self):
            self.opt = types.SimpleNamespace(mesh_show_back_face=False)
            self.ctr = Ctr()
            self.geom = None

        def create_window(self, width=None, height=None, **k):
            log['window'] = (width, height)

        def get_render_option(self):
            return self.opt

        def get_view_control(self):
            return self.ctr

        def add_geometry(self, g, reset_bounding_box=True):
            self.geom = g

        def remove_geometry(self, g, reset_bounding_box=True):
            self.geom = None

        def poll_events(self):
            pass

        def update_renderer(self):
            pass

        def capture_depth_float_buffer(self, do_render=False):
            ext = np.array(self.ctr.param.extrinsic, dtype=np.float64)
            c2w = log['last_c2w']
            assert np.array_equal(ext, np.linalg.inv(c2w))
            if self.geom.name == 'gt.ply':                 # each view renders the ground truth first
                log['extrinsics'].append(ext)
            log['back_face'].add(bool(self.opt.mesh_show_back_face))
            W, H, fx, fy, cx, cy = log['intrinsics'][-1]
            g = self.geom
            return depth_ref.render_depth(g.verts, g.faces, c2w, int(H), int(W), fx, fy, cx, cy, depth_ref.near_of(g.verts),
                                          self.ctr.z_far)
    open3d.visualization = types.SimpleNamespace(Visualizer=Visualizer)
    return {'trimesh': trimesh, 'trimesh.sample': sample, 'trimesh.bounds': bounds, 'open3d': open3d}


def main():
    sys.dont_write_bytecode = True
    import importlib.util
    np.float = float
    np.bool = bool
    log = {}
    sys.modules.update(_stubs(log))
    spec = importlib.util.spec_from_file_location('ref_eval_recon', os.path.join(REF, 'src', 'tools', 'eval_recon.py'))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    check_proj = ev.check_proj

    def screened(points, W, H, fx, fy, cx, cy, c2w):
        log['candidates'] += 1
        log['last_c2w'] = np.array(c2w, copy=True)
        return check_proj(points, W, H, fx, fy, cx, cy, c2w)
    ev.check_proj = screened
    np_load = np.load
    cuda = torch.Tensor.cuda
    out = {}
    try:
        torch.Tensor.cuda = lambda self, *a, **k: self
        np.load = lambda path, *a, **k: pc_unseen() if path == 'gt_pc_unseen.npy' else np_load(path, *a, **k)
        for s in SEEDS:
            log.update(intrinsics=[], z_far=set(), back_face=set(), extrinsics=[], candidates=0)
            ev.setup_seed(s)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                ev.calc_2d_metric('rec.ply', 'gt.ply', align=False, n_imgs=N_IMGS)
            line = buf.getvalue().strip()
            assert line.startswith('Depth L1:'), line
            assert len(log['extrinsics']) == N_IMGS and log['candidates'] > N_IMGS, (len(log['extrinsics']), log['candidates'])
            out[f'calc2d.{s}.extrinsics'] = np.stack(log['extrinsics'])
            out[f'calc2d.{s}.candidates'] = np.int64(log['candidates'])
            out[f'calc2d.{s}.printed'] = np.float64(float(line.split(':')[-1]))
    finally:
        torch.Tensor.cuda = cuda
        np.load = np_load
    assert len(set(log['intrinsics'])) == 1 and log['window'] == (500, 500)
    out['intrinsics'] = np.array(log['intrinsics'][0])
    out['z_far'] = np.float64(log['z_far'].pop())
    out['back_face'] = np.bool_(log['back_face'].pop())
    sigs = {name: str(inspect.signature(getattr(ev, name))) for name in ('normalize', 'viewmatrix', 'get_cam_position', 'setup_seed',
                                                                        'calc_2d_metric')}
    sigs['check_proj'] = str(inspect.signature(check_proj))
    np.savez_compressed(os.path.join(OUT, 'mini_depth.npz'), **out)
    with open(os.path.join(OUT, 'depth_signatures.json'), 'w') as fh:
        json.dump(sigs, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', os.path.join(OUT, 'mini_depth.npz'), {k: (v if v.ndim == 0 else v.shape) for k, v in out.items()})


if __name__ == '__main__':
    main()
