"""CPU: the oracle of reconstruction evaluation (tests/recon_ref.py) against the reference's own code (tests/golden/
make_recon_golden.py: eval_recon.py and cull_mesh.py run under stub trimesh / open3d), and the port's public signatures against
the reference's.  The GPU tests (test_gpu_recon.py) hold the port to this oracle."""
import json
import os

import numpy as np
import pytest
import torch

import recon_ref as R
from attentive_dfprior_amd import cull_mesh, recon_eval

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
import sys  # noqa: E402
sys.path.insert(0, GOLDEN)
import make_recon_golden as G  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'mini_recon.npz'))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize('case', ['room', 'offset', 'lattice'])
def test_oracle_metrics_equal_reference(golden, case):
    gt, rec = G.clouds()[case]
    assert R.accuracy(gt, rec) == golden[f'metric.{case}.accuracy']
    assert R.completion(gt, rec) == golden[f'metric.{case}.completion']
    assert R.completion_ratio(gt, rec) == golden[f'metric.{case}.ratio05']
    assert R.completion_ratio(gt, rec, 0.02) == golden[f'metric.{case}.ratio02']


def test_calc_3d_metric_wiring(golden):
    rec, gt = G.calc3d_clouds()
    assert list(golden['calc3d.counts']) == [recon_eval.SAMPLES, recon_eval.SAMPLES] == [200000, 200000]
    assert list(golden['calc3d.order']) == [0, 1]                       # the reconstruction is sampled first
    want = [R.accuracy(gt, rec) * 100, R.completion(gt, rec) * 100, R.completion_ratio(gt, rec) * 100]
    assert np.array_equal(np.array(want), golden['calc3d.values'])


def test_oracle_cull_equals_reference(golden, tmp_path):
    v, f, traj = G.cull_inputs()
    p = tmp_path / 'traj.txt'
    p.write_text(traj)
    poses = cull_mesh.load_poses(str(p))
    assert len(poses) == 12 and all(c.dtype == torch.float32 for c in poses)
    keep, _ = R.cull_mask(v, f, [c.numpy() for c in poses])
    assert np.array_equal(keep, golden['cull.keep'])


def test_signatures_equal_reference():
    import inspect
    with open(os.path.join(GOLDEN, 'recon_signatures.json')) as fh:
        sigs = json.load(fh)
    for name, sig in sigs.items():
        mod = cull_mesh if name == 'load_poses' else recon_eval
        assert str(inspect.signature(getattr(mod, name))) == sig, name


def test_oracle_icp_recovers_rigid_motion():
    v, _ = R.room_mesh()
    a = np.deg2rad(3.0)
    ax = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = [0.03, -0.02, 0.035]                     # |t| ~ 5 cm
    src = R.apply_transform(v, np.linalg.inv(T))
    Te, fitness, rmse, it = R.icp(src, v)
    assert np.abs(Te - T).max() < 1e-6
    assert fitness == 1.0 and rmse < 1e-6 and 1 < it <= 30


def test_sampling_oracle_follows_trimesh_rules():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 2]], np.float64)
    f = np.array([[0, 1, 2], [0, 1, 3]])
    pts, fi, cum = R.sample_surface(v, f, np.array([0.0, 0.2, 1 / 3, 0.9]), np.array([[0.25, 0.5], [0.75, 0.5], [0.1, 0.1], [0.5, 0.5]]))
    assert np.allclose(cum, [0.5, 1.5])
    assert list(fi) == [0, 0, 0, 1]                    # searchsorted side='left': u * total == cum[0] stays on face 0
    assert np.allclose(pts[0], [0.25, 0.5, 0])
    assert np.allclose(pts[1], [0.25, 0.5, 0])         # a + b > 1: (|0.75 - 1|, |0.5 - 1|)
    assert np.allclose(pts[3], [0.5, 0, 1.0])
