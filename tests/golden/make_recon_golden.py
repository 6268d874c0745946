"""
Golden vectors for reconstruction evaluation (src/tools/eval_recon.py, src/tools/cull_mesh.py).  Both scripts import trimesh
(and eval_recon.py open3d) at module level, and neither library is installed in the build container; they also use np.float /
np.bool, which numpy 2 removed.  This script puts STUB open3d / trimesh modules into sys.modules, restores np.float = float and
np.bool = bool, and gives np.linalg.inv numpy 1's result type for a torch tensor (an ndarray: numpy 2 wraps the result through
Tensor.__array_wrap__, which cull_mesh.py:54's torch.from_numpy rejects), and EXECUTES the reference's own code on seeded inputs: the stored outputs come from the reference.  Nothing is
written under the reference (sys.dont_write_bytecode).  Build container only.

    python tests/golden/make_recon_golden.py

mini_recon.npz holds
  * metric.<case>.accuracy / .completion / .ratio05 / .ratio02   eval_recon.accuracy, completion, completion_ratio (dist_th 0.05
    and 0.02) on the clouds `clouds()[case]` below: room-surface samples (20 000 gt x 25 000 rec), the same with the
    reconstruction moved by 3 x the room's extent, and lattice points with exact ties;
  * calc3d.values / calc3d.counts / calc3d.order   calc_3d_metric(..., align=False) with a stub sample_surface returning the
    pre-drawn clouds `calc3d_clouds()`: the three printed numbers, the sample counts it asked for and which mesh was sampled first
    (0 = the reconstruction);
  * cull.keep   the face mask cull_mesh.py hands to update_faces, run through runpy on `cull_inputs()` (torch.Tensor.cuda an
    identity: the loop runs on the CPU).
recon_signatures.json holds inspect.signature of the reference's public functions.
"""
import contextlib
import inspect
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import recon_ref  # noqa: E402


def _room():
    return recon_ref.room_mesh()


def _samples(v, f, n, seed):
    rng = np.random.default_rng(seed)
    return recon_ref.sample_surface(v, f, rng.random(n), rng.random((n, 2)))[0]


def clouds():
    """{case: (gt_points, rec_points)} (float64)."""
    v, f = _room()
    gt = _samples(v, f, 20000, 1)
    rec = _samples(v, f, 25000, 2) + np.random.default_rng(3).normal(0, 0.01, (25000, 3))
    ext = float(np.ptp(v, 0).max())
    g = np.arange(-10, 11) * 0.01
    X, Y, Z = np.meshgrid(g, g, g, indexing='ij')
    lat = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    h = np.arange(-8, 8) * 0.01 + 0.005                  # half-way between lattice planes: every query has tied neighbours
    X, Y, Z = np.meshgrid(h, h, g[::3], indexing='ij')
    lat2 = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1)
    return {'room': (gt, rec), 'offset': (gt, rec + np.array([3 * ext, 0.0, 0.0])), 'lattice': (lat, lat2)}


def calc3d_clouds():
    """(rec_points, gt_points) the stub sample_surface hands out, in that order of meshes."""
    v, f = _room()
    return _samples(v, f, 3000, 4) + 0.003, _samples(v, f, 3500, 5)


def cull_inputs():
    """(verts f64 [V,3], faces [F,3], trajectory text): the room mesh scaled to Replica-like size and 12 seeded poses inside it."""
    v, f = _room()
    v = v * 1.5
    rng = np.random.default_rng(9)
    lines = []
    for k in range(12):
        yaw, pitch = rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4)
        cy_, sy_, cp_, sp_ = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        Rz = np.array([[cy_, -sy_, 0], [sy_, cy_, 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, cp_, -sp_], [0, sp_, cp_]])
        c2w = np.eye(4)
        c2w[:3, :3] = Rz @ Rx
        c2w[:3, 3] = rng.uniform([-1.5, -1.0, -0.6], [1.5, 1.0, 0.6])
        lines.append(' '.join(f'{x:.17g}' for x in c2w.reshape(-1)))
    return v, f, '\n'.join(lines) + '\n'


class _Mesh(object):
    def __init__(self, name, vertices=None, faces=None, log=None):
        self.name, self.vertices, self.faces, self.log = name, vertices, faces, log

    def update_faces(self, mask):
        self.log['update_faces'] = np.array(mask, copy=True)

    def export(self, path):
        self.log['export'] = path


def _stubs(log):
    trimesh = types.ModuleType('trimesh')
    sample = types.ModuleType('trimesh.sample')
    log.setdefault('samples', [])
    log.setdefault('loads', {})

    def load(path, process=True):
        return log['loads'][path]()

    def sample_surface(mesh, count, *a, **k):
        log['samples'].append((mesh.name, int(count)))
        pts = log['clouds'][mesh.name]
        return pts, np.zeros(len(pts), np.int64)

    class PointCloud(object):
        def __init__(self, vertices=None, **k):
            self.vertices = np.asarray(vertices)
    sample.sample_surface = sample_surface
    trimesh.sample = sample
    trimesh.load = load
    trimesh.PointCloud = PointCloud
    trimesh.Trimesh = _Mesh
    open3d = types.ModuleType('open3d')
    open3d.__version__ = '0.16.0'
    return {'trimesh': trimesh, 'trimesh.sample': sample, 'open3d': open3d}


def _sig(fn):
    return str(inspect.signature(fn))


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
    out = {}
    for case, (gt, rec) in clouds().items():
        out[f'metric.{case}.accuracy'] = np.float64(ev.accuracy(gt, rec))
        out[f'metric.{case}.completion'] = np.float64(ev.completion(gt, rec))
        out[f'metric.{case}.ratio05'] = np.float64(ev.completion_ratio(gt, rec))
        out[f'metric.{case}.ratio02'] = np.float64(ev.completion_ratio(gt, rec, dist_th=0.02))

    rec_pts, gt_pts = calc3d_clouds()
    log['clouds'] = {'rec': rec_pts, 'gt': gt_pts}
    log['loads'] = {'rec.ply': lambda: _Mesh('rec'), 'gt.ply': lambda: _Mesh('gt')}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        ev.calc_3d_metric('rec.ply', 'gt.ply', align=False)
    printed = [float(line.split(':')[-1]) for line in buf.getvalue().strip().splitlines()]
    assert len(printed) == 3, buf.getvalue()
    out['calc3d.values'] = np.array(printed)
    out['calc3d.counts'] = np.array([c for _, c in log['samples']])
    out['calc3d.order'] = np.array([0 if m == 'rec' else 1 for m, _ in log['samples']])

    v, f, traj = cull_inputs()
    with tempfile.TemporaryDirectory() as d:
        tp = os.path.join(d, 'traj.txt')
        with open(tp, 'w') as fh:
            fh.write(traj)
        log['loads'] = {'in.ply': lambda: _Mesh('in', v.copy(), f.copy(), log)}
        cuda, inv = torch.Tensor.cuda, np.linalg.inv
        torch.Tensor.cuda = lambda self, *a, **k: self
        np.linalg.inv = lambda a: inv(np.asarray(a))
        argv = sys.argv
        sys.argv = ['cull_mesh.py', '--input_mesh', 'in.ply', '--traj', tp, '--output_mesh', 'out.ply']
        try:
            with contextlib.redirect_stderr(io.StringIO()):
                g = runpy.run_path(os.path.join(REF, 'src', 'tools', 'cull_mesh.py'), run_name='__main__')
        finally:
            sys.argv = argv
            torch.Tensor.cuda, np.linalg.inv = cuda, inv
    keep = log['update_faces']
    assert log['export'] == 'out.ply' and keep.dtype == bool and keep.any() and (~keep).any()
    out['cull.keep'] = keep

    sigs = {name: _sig(getattr(ev, name)) for name in ('accuracy', 'completion', 'completion_ratio', 'get_align_transformation',
                                                       'calc_3d_metric', 'calc_2d_metric')}
    sigs['load_poses'] = _sig(g['load_poses'])
    np.savez_compressed(os.path.join(OUT, 'mini_recon.npz'), **out)
    with open(os.path.join(OUT, 'recon_signatures.json'), 'w') as fh:
        json.dump(sigs, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', os.path.join(OUT, 'mini_recon.npz'), sorted(out), 'kept faces', int(keep.sum()), '/', len(keep))


if __name__ == '__main__':
    main()
