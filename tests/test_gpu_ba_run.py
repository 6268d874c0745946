"""GPU: the whole run with mapping.BA on, on test_gpu_slam_run's analytic box-room sequence stretched to 12 frames.

every_frame 2 and keyframe_every 2 give the keyframes 0, 2, 4, 6, 8 by the time frame 10 is mapped, so bundle adjustment is active for
the mapped frames 10 and 11 (more than four keyframes) and for no earlier one.  8 mapping iterations (ratios 0.4 / 0.6: three of them
in stage color, where the poses step), a window of 4 frames, 240 pixels.  The decoders are seed-initialised: no accuracy is claimed,
the trajectory error with and without BA is printed."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_gpu_slam_run as R
from attentive_dfprior_amd import datasets, run, slam as slam_module, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_IMG = 12
MAPPING = {'every_frame': 2, 'keyframe_every': 2, 'ckpt_freq': 6, 'mesh_freq': 100, 'iters': 8, 'mapping_window_size': 4, 'color_refine': False}


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    from PIL import Image
    base = tmp_path_factory.mktemp('ba_run')
    root = str(base / 'box')
    os.makedirs(os.path.join(root, 'results'))
    lines = []
    for k in range(N_IMG):
        c2w = R.pose_cv(k)
        depth, color = R.frame_images(c2w)
        assert 0.5 < depth.min() and depth.max() < 4.0
        Image.fromarray(color).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(np.clip(np.rint(depth * R.PNG), 0, 65535).astype(np.uint16)).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
        lines.append(' '.join(repr(float(x)) for x in c2w.reshape(-1)))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    cfg = R.full_cfg(base, R.scene_cfg(root, str(base / 'unused')), 'world')[0]
    ds = datasets.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device=DEV)
    colors, depths, _ = ds.frames(range(N_IMG))
    gt = torch.stack([ds.pose(k) for k in range(N_IMG)])
    bound = synthetic.scene_bound(R.BOUND, 0.32, 1).numpy()
    tsdf, bnds = R.prior_of(bound, [(colors[k], depths[k], gt[k]) for k in range(N_IMG)]).get_render_volume()
    vol_path, bnds_path = str(base / 'box_tsdf_volume.pt'), str(base / 'box_bounds.pt')
    torch.save(tsdf.cpu(), vol_path)
    torch.save(bnds.numpy(), bnds_path)
    return SimpleNamespace(base=base, root=root, vol=vol_path, bnds=bnds_path)


def go(world, name, monkeypatch, ba):
    """One run; records per optimize_map call the frame, the pose it started from (the Tracker's) and what it returned."""
    calls = []
    orig = slam_module.Mapper.optimize_map

    def recording(self, num_joint_iters, lr_factor, idx, *a, **k):
        before = self.estimate_c2w_list[idx].clone()
        ret = orig(self, num_joint_iters, lr_factor, idx, *a, **k)
        calls.append((int(idx), before, None if ret is None else ret.detach().cpu().clone(), len(self.keyframe_list)))
        return ret
    monkeypatch.setattr(slam_module.Mapper, 'optimize_map', recording)
    out = str(world.base / name)
    mapping = dict(MAPPING, BA=True) if ba else dict(MAPPING)
    cfg, path = R.full_cfg(world.base, R.scene_cfg(world.root, out, mapping=mapping, meshing={'eval_rec': False}), name)
    s = run.main([path, '--default_config', R.DEFAULT, '--seed', '0', '--tsdf_volume', world.vol, '--tsdf_bounds', world.bnds])
    torch.cuda.synchronize()
    return s, out, calls


def test_a_run_with_bundle_adjustment(world, monkeypatch):
    s, out, calls = go(world, 'ba', monkeypatch, True)
    m = s.mapper
    assert m.BA and m.keyframe_list == [0, 2, 4, 6, 8, 10] and m.keyframe_store.ids == m.keyframe_list
    assert [c[0] for c in calls] == [0, 2, 4, 6, 8, 10, 11]
    est = s.estimate_c2w_list
    for idx, tracked, returned, n_kf in calls:
        assert (returned is not None) == (n_kf > 4) == (idx >= 10), idx
        if returned is not None:                               # the mapped frame's pose is the corrected one, not the Tracker's
            assert torch.equal(est[idx], returned) and not torch.equal(returned, tracked), idx
            print(f'frame {idx}: bundle adjustment moved the pose by {(returned - tracked).abs().max().item():.3e}')
        else:
            assert torch.equal(est[idx], tracked), idx
    # keyframe_dict and the resident store hold the same poses, bit for bit; keyframe 5 (frame 10) was appended with its corrected pose
    rows = m.keyframe_store.poses()
    for k, kf in enumerate(m.keyframe_dict):
        assert kf['est_c2w'].view(torch.int32).equal(rows[k].view(torch.int32)), k
    # every rotation block is orthonormal to f32 rounding (the bound of test_gpu_slam_run: a float32 quaternion round trip per frame)
    for name, P in (('estimate_c2w_list', est), ('keyframe store', rows.cpu())):
        Rm = P[:, :3, :3].double()
        err = (Rm.transpose(1, 2) @ Rm - torch.eye(3, dtype=torch.float64)).abs().max().item()
        print(f'orthonormality of {name}: max |R^T R - I| = {err:.3e}')
        assert err <= 1e-5 and torch.equal(P[:, 3, :], torch.tensor([[0., 0., 0., 1.]]).repeat(P.shape[0], 1)), name
    # the checkpoint holds the corrected poses
    assert sorted(os.listdir(os.path.join(out, 'ckpts'))) == ['00006.tar', '00011.tar']
    ck = torch.load(os.path.join(out, 'ckpts', '00011.tar'), map_location='cpu', weights_only=False)
    assert torch.equal(ck['estimate_c2w_list'], est) and ck['keyframe_list'] == m.keyframe_list
    for k, kf in enumerate(ck['keyframe_dict']):
        assert torch.equal(kf['est_c2w'].cpu(), rows[k].cpu()), k
    with open(os.path.join(out, 'eval_ate.json')) as f:
        ate = json.load(f)
    assert ate['compared_pose_pairs'] == N_IMG and np.isfinite(ate['absolute_translational_error.rmse'])
    # an observation, not a claim: the same run without BA
    s0, _, calls0 = go(world, 'no_ba', monkeypatch, False)
    assert all(c[2] is None for c in calls0) and not s0.mapper.BA
    print(f"ATE rmse with BA {ate['absolute_translational_error.rmse']:.5f} m, without {s0.ate['absolute_translational_error.rmse']:.5f} m")
