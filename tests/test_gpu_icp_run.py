"""GPU: the whole run with ``tracking.init: icp`` on test_gpu_slam_run's analytic box-room sequence (8 frames, 48 x 64, the prior fused
from the true poses at 4/64 m voxels).

Asserted: the run completes; one ICP status per tracked frame; with ``tracking.iters: 0`` a frame whose status is OK carries the ICP's
pose and every other frame the constant-speed guess; without the key the trajectory is byte for byte that of ``tracking.init: guess``
and no DepthICP is ever built.  The trajectory error with and without ICP is printed as an observation: this sequence's views were
not checked for conditioning (the camera looks at one or two walls), so statuses other than OK are expected and nothing is claimed
about accuracy."""
import importlib.util

import numpy as np
import pytest
import torch

import test_gpu_slam_run as R
from test_gpu_slam_run import world  # noqa: F401  (the module-scoped dataset and prior)
from attentive_dfprior_amd import common

pytestmark = pytest.mark.gpu
LEAN = dict(mapping={'mesh_freq': 100, 'color_refine': False}, meshing={'eval_rec': False})
HAS_ICP = importlib.util.find_spec('attentive_dfprior_amd.icp') is not None


def go(world, name, tracking):  # noqa: F811
    return R.go(world, name, tracking=tracking, **LEAN)[0]


def test_default_path_is_unchanged_and_builds_no_icp(world, monkeypatch):  # noqa: F811
    """Passes before and after the feature: a config without tracking.init against one that says `guess` (a key the run ignored
    before the feature), tracking.iters 0 so that the poses do not depend on the Mapper's atomics."""
    if HAS_ICP:
        from attentive_dfprior_amd import icp

        def never(self, *a, **k):
            raise AssertionError('DepthICP was constructed on the default path')
        monkeypatch.setattr(icp.DepthICP, '__init__', never)
    a = go(world, 'icp_absent', {'iters': 0})
    b = go(world, 'icp_guess', {'iters': 0, 'init': 'guess'})
    assert a.estimate_c2w_list.numpy().tobytes() == b.estimate_c2w_list.numpy().tobytes()
    ref = [world.gt[0].double(), world.gt[0].double()]
    for k in range(2, R.N_IMG):
        ref.append(ref[k - 1] @ torch.linalg.inv(ref[k - 2]) @ ref[k - 1])
    assert (a.estimate_c2w_list.double() - torch.stack(ref)).abs().max().item() <= 1e-5
    if HAS_ICP:
        assert a.tracker.icp_status == [] and a.tracker._icp is None and a.tracker.init == 'guess'
        c = go(world, 'icp_absent_tracked', {})                       # with the iterations on: still no DepthICP
        assert c.tracker._icp is None and c.tracker._it is not None


def test_icp_alone_is_the_tracker_with_zero_iterations(world, monkeypatch):  # noqa: F811
    from attentive_dfprior_amd import icp
    calls = []
    orig = icp.DepthICP.refine

    def recording(self, guess_c2w, gt_depth):
        cam = orig(self, guess_c2w, gt_depth)
        calls.append((guess_c2w.detach().cpu().clone(), cam.detach().clone(), self.c2w_out.detach().clone()))
        return cam
    monkeypatch.setattr(icp.DepthICP, 'refine', recording)
    # near 0.3 m (the sequence's depths are above 0.5 m): the prior is -1 at the cameras' own voxels, which no frame saw, and the
    # raycast from the camera reports no surface there (test_icp_seeds_the_tracking_iterations runs without it)
    s = go(world, 'icp_iters0', {'iters': 0, 'init': 'icp', 'icp': {'near': 0.3}})
    assert s.tracker.icp.near == 0.3
    t = s.tracker
    assert t._it is None and t._icp is not None and t._icp.raycaster._engine is s.renderer._engine
    assert len(t.icp_status) == len(calls) == R.N_IMG - 1 and all(st in (0, 1, 2, 3) for st in t.icp_status)
    print('tracking.iters 0, tracking.init icp: statuses', t.icp_status)
    est = s.estimate_c2w_list
    for k, (guess, cam, c2w_out) in enumerate(calls):
        idx = k + 1
        pose = common.get_camera_from_tensor(cam).cpu()
        assert torch.equal(est[idx, :3], pose), idx                                   # the returned tensor IS the frame's pose
        if t.icp_status[k] == icp.OK:
            assert (est[idx] - c2w_out.cpu()).abs().max().item() <= 1e-5 and not torch.equal(c2w_out.cpu(), guess), idx
        else:
            assert torch.equal(c2w_out.cpu(), guess) and (est[idx] - guess).abs().max().item() <= 1e-5, idx
    assert torch.isfinite(est).all() and s.ate['compared_pose_pairs'] == R.N_IMG
    print(f"ATE rmse, ICP alone: {s.ate['absolute_translational_error.rmse']:.5f} m")


def test_icp_seeds_the_tracking_iterations(world):  # noqa: F811
    s = go(world, 'icp_tracked', {'init': 'icp'})
    t = s.tracker
    assert t._it is not None and t._icp is not None and len(t.icp_status) == R.N_IMG - 1
    est = s.estimate_c2w_list
    assert torch.isfinite(est).all() and est[0].view(torch.int32).equal(world.gt[0].view(torch.int32))
    Rm = est[:, :3, :3].double()
    assert (Rm.transpose(1, 2) @ Rm - torch.eye(3, dtype=torch.float64)).abs().max().item() <= 1e-5
    assert s.ate['compared_pose_pairs'] == R.N_IMG and np.isfinite(s.ate['absolute_translational_error.rmse'])
    s0 = go(world, 'icp_tracked_off', {})
    print(f"statuses {t.icp_status}; ATE rmse with ICP {s.ate['absolute_translational_error.rmse']:.5f} m, "
          f"without {s0.ate['absolute_translational_error.rmse']:.5f} m (an observation, not a claim)")


def test_online_prior_with_icp(world, monkeypatch):  # noqa: F811
    """--prior online: the volume the ICP raycasts grows during the run, and the raycaster's empty-space bitmap follows its version
    counter: a bitmap per volume version a tracked frame met (frames 0, 2, 4, 6 are mapped before frames 1, 3, 5, 7 are tracked)."""
    from attentive_dfprior_amd import engine
    versions = []
    orig = engine.Engine.tsdf_bricks

    def recording(self, tsdf_volume):
        bricks = orig(self, tsdf_volume)
        versions.append((tsdf_volume._version, bricks.data_ptr(), bricks))
        return bricks
    monkeypatch.setattr(engine.Engine, 'tsdf_bricks', recording)
    slam = R.go(world, 'icp_online', extra=['--prior', 'online', '--prior_voxel_size', str(R.VOXEL), '--tracking_init', 'icp'], **LEAN)[0]
    t = slam.tracker
    assert t.init == 'icp' and len(t.icp_status) == R.N_IMG - 1 and len(versions) >= R.N_IMG - 1
    assert t._icp.raycaster.tsdf_volume is slam.tsdf_volume_shared
    assert len(set(v for v, _, _ in versions)) == 4 == len(set(p for _, p, _ in versions))
    print('--prior online, tracking.init icp: statuses', t.icp_status)
    assert torch.isfinite(slam.estimate_c2w_list).all()
