"""The Mesher port (attentive_dfprior_amd.mesher) against the reference's own src/utils/Mesher.py, executed under stub
open3d / trimesh / scikit-image modules by tests/golden/make_mesher_golden.py (fixture tests/golden/mini_mesher.npz):
get_grid_uniform's axes, point_masks in both branches with depth_test on and off (on CPU tensors, bit for bit), and the
volume, level, spacing and origin get_mesh hands to marching cubes.  The hull fill of that volume is a kernel: the last test
runs it on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
sys.path.insert(0, GOLDEN)
import make_mesher_golden as G          # noqa: E402  (its inputs and stubs; the reference is only read by its main())
from attentive_dfprior_amd.mesher import Mesher      # noqa: E402


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN, 'mini_mesher.npz'))
    return {k: z[k] for k in z.files}


class StubRenderer(object):
    """Renderer.eval_points' contract: the decoder's raw output, occupancy 100 outside `bound` (Renderer.py:27-71)."""

    def __init__(self, bound):
        self.bound = bound

    def eval_points(self, p, decoders, tsdf_volume, tsdf_bnds, c=None, stage='color', device='cuda:0'):
        b = self.bound
        mask = ((p[:, 0] < b[0][1]) & (p[:, 0] > b[0][0]) & (p[:, 1] < b[1][1]) & (p[:, 1] > b[1][0]) &
                (p[:, 2] < b[2][1]) & (p[:, 2] > b[2][0]))
        ret, w = decoders(p.unsqueeze(0), c_grid=c, tsdf_volume=tsdf_volume, tsdf_bnds=tsdf_bnds, stage=stage)
        ret = ret.squeeze(0)
        ret[~mask, 3] = 100
        return ret, w.squeeze(0)


def mesher(depth_test=False):
    slam = G.Slam()
    slam.renderer = StubRenderer(slam.bound)
    return Mesher(G.cfg(depth_test), None, slam, points_batch_size=G.POINTS_BATCH)


def test_grid_axes(gold):
    xyz = mesher().get_grid_uniform(G.RESOLUTION)['xyz']
    for k, a in zip('xyz', xyz):
        assert a.dtype == np.float64 and np.array_equal(a, gold[f'grid.{k}'])


@pytest.mark.parametrize('case', sorted(G.MASK_CASES))
def test_point_masks(gold, case):
    depth_test, all_frames = G.MASK_CASES[case]
    kfs = G.keyframes()
    est = torch.stack([kf['est_c2w'] for kf in kfs])
    seen, fc, unseen = mesher(depth_test).point_masks(G.points(), kfs, est, 2, 'cpu', get_mask_use_all_frames=all_frames)
    for name, got in (('seen', seen), ('forecast', fc), ('unseen', unseen)):
        ref = gold[f'masks.{case}.{name}']
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (case, name, int((got != ref).sum()))


def test_volume_level_spacing_origin(gold):
    m = mesher()
    xyz = m.get_grid_uniform(G.RESOLUTION)['xyz']
    tv, _ = G.tsdf_inputs()
    z, ax = m.lattice({}, G.stub_decoder, tv, xyz, 'cpu')
    ref = gold['mc.volume']
    assert z.shape == ref.shape
    P = np.stack(np.meshgrid(*[a.cpu().numpy().astype(np.float64) for a in ax], indexing='ij'), -1).reshape(-1, 3)
    inside = G.StubHull().contains(P).reshape(ref.shape)
    assert inside.any() and (~inside).any()
    assert (ref[~inside] == 100).all()
    assert np.array_equal(z.numpy()[inside], ref[inside])              # order, axes, reshape / transpose, bound rule
    assert m.level_set == float(gold['mc.level'])
    spacing, origin = m.marching_cubes_geometry(xyz)
    assert np.array_equal(np.array(spacing, np.float64), gold['mc.spacing'])
    assert np.array_equal(np.array(origin, np.float64), gold['mc.origin'])


@pytest.mark.gpu
def test_hull_fill_gives_the_reference_volume(gold):
    from attentive_dfprior_amd import mesh
    m = mesher()
    xyz = m.get_grid_uniform(G.RESOLUTION)['xyz']
    tv, _ = G.tsdf_inputs()
    z, ax = m.lattice({}, G.stub_decoder, tv, xyz, 'cpu')
    zd = z.to('cuda:0').contiguous()
    mesh.hull_fill(zd, [a.to('cuda:0') for a in ax], G.HULL_PLANES, 100.)
    got, ref, before = zd.cpu().numpy(), gold['mc.volume'], z.numpy()
    filled = (ref == 100) & (before != 100)                             # what the reference's contains() mask set to 100
    assert filled.any()
    assert (got[filled] == 100).all()
    assert np.array_equal(got[~filled], before[~filled])               # nothing else touched
