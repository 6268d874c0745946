"""GPU: the whole run with ``tracking.icp_rgb`` on test_gpu_slam_run's analytic box-room sequence (8 frames, 48 x 64, the prior fused
from the true poses at 4/64 m voxels), as tests/test_gpu_icp_run.py runs it with ``tracking.init: icp`` alone.

Asserted: without the key, or with ``weight: 0``, the ``tracking.iters: 0`` trajectory is byte for byte that of ``init: icp`` alone and
no RgbdICP is ever built; with ``weight: 1`` the run completes, there is one status per tracked frame, set_keyframe is called once
(frame 0) and promote once per tracked frame, the Engine is shared, and a frame whose status is OK carries the ICP's pose.  Statuses
and the trajectory error with and without the term are printed as observations: nothing is claimed about accuracy."""
import pytest
import torch

import test_gpu_slam_run as R
from test_gpu_slam_run import world  # noqa: F401  (the module-scoped dataset and prior)
from attentive_dfprior_amd import common, icp

pytestmark = pytest.mark.gpu
LEAN = dict(mapping={'mesh_freq': 100, 'color_refine': False}, meshing={'eval_rec': False})
ICP = {'iters': 0, 'init': 'icp', 'icp': {'near': 0.3}}


def go(world, name, tracking):  # noqa: F811
    return R.go(world, name, tracking=tracking, **LEAN)[0]


def test_off_is_the_depth_icp_byte_for_byte_and_builds_no_rgbd_icp(world, monkeypatch):  # noqa: F811
    def never(self, *a, **k):
        raise AssertionError('RgbdICP was constructed with the photometric term off')
    monkeypatch.setattr(icp.RgbdICP, '__init__', never)
    a = go(world, 'rgbd_absent', dict(ICP))
    b = go(world, 'rgbd_weight0', dict(ICP, icp_rgb={'weight': 0}))
    c = go(world, 'rgbd_empty', dict(ICP, icp_rgb={}))
    for s in (a, b, c):
        assert type(s.tracker._icp) is icp.DepthICP and not s.tracker.icp_rgb and len(s.tracker.icp_status) == R.N_IMG - 1
    assert a.estimate_c2w_list.numpy().tobytes() == b.estimate_c2w_list.numpy().tobytes() == c.estimate_c2w_list.numpy().tobytes()
    assert a.tracker.icp_status == b.tracker.icp_status == c.tracker.icp_status
    d = go(world, 'rgbd_guess', {'iters': 0})                             # and the default path builds no ICP at all
    assert d.tracker._icp is None and not d.tracker.icp_rgb


def test_a_weight_without_init_icp_is_an_error(world):  # noqa: F811
    with pytest.raises(ValueError, match='tracking.init: icp'):
        go(world, 'rgbd_no_init', {'iters': 0, 'icp_rgb': {'weight': 1.0}})


def test_the_joint_icp_alone_is_the_tracker_with_zero_iterations(world, monkeypatch):  # noqa: F811
    calls, keyframes, promoted = [], [], []
    refine, set_keyframe, promote = icp.RgbdICP.refine, icp.RgbdICP.set_keyframe, icp.RgbdICP.promote

    def rec_refine(self, guess_c2w, gt_depth, gt_color):
        cam = refine(self, guess_c2w, gt_depth, gt_color)
        calls.append((guess_c2w.detach().cpu().clone(), cam.detach().clone(), self.c2w_out.detach().clone(), self.has_keyframe))
        return cam

    def rec_set_keyframe(self, c2w, color, depth):
        keyframes.append(c2w.detach().cpu().clone())
        return set_keyframe(self, c2w, color, depth)

    def rec_promote(self, c2w):
        promoted.append((len(calls), c2w.detach().cpu().clone()))
        return promote(self, c2w)
    monkeypatch.setattr(icp.RgbdICP, 'refine', rec_refine)
    monkeypatch.setattr(icp.RgbdICP, 'set_keyframe', rec_set_keyframe)
    monkeypatch.setattr(icp.RgbdICP, 'promote', rec_promote)
    s = go(world, 'rgbd_iters0', dict(ICP, icp_rgb={'weight': 1.0}))
    t = s.tracker
    assert t.icp_rgb and type(t._icp) is icp.RgbdICP and t._icp.rgb_weight == 1.0 and t._icp.rgb_tol == 0.25 and t._icp.near == 0.3
    assert t._it is None and t._icp.raycaster._engine is s.renderer._engine
    assert len(t.icp_status) == len(calls) == R.N_IMG - 1 and all(st in (0, 1, 2, 3) for st in t.icp_status)
    assert len(keyframes) == 1 and torch.equal(keyframes[0], world.gt[0]) and all(c[3] for c in calls)
    est = s.estimate_c2w_list
    assert [n for n, _ in promoted] == list(range(1, R.N_IMG))              # once per tracked frame, after its refine
    for k, (guess, cam, c2w_out, _) in enumerate(calls):
        idx = k + 1
        pose = common.get_camera_from_tensor(cam).cpu()
        assert torch.equal(est[idx, :3], pose), idx                         # the returned tensor IS the frame's pose
        assert torch.equal(promoted[k][1], est[idx]), idx                   # and the pose the frame was promoted at
        if t.icp_status[k] == icp.OK:
            assert (est[idx] - c2w_out.cpu()).abs().max().item() <= 1e-5 and not torch.equal(c2w_out.cpu(), guess), idx
        else:
            assert torch.equal(c2w_out.cpu(), guess) and (est[idx] - guess).abs().max().item() <= 1e-5, idx
    assert torch.isfinite(est).all() and s.ate['compared_pose_pairs'] == R.N_IMG
    rgb = t._icp.last_rgb_stats()
    assert tuple(rgb.shape) == (11, 2)
    s0 = go(world, 'rgbd_iters0_off', dict(ICP))
    print(f"tracking.iters 0: statuses with the term {t.icp_status}, ATE rmse {s.ate['absolute_translational_error.rmse']:.5f} m; without "
          f"{s0.tracker.icp_status}, ATE rmse {s0.ate['absolute_translational_error.rmse']:.5f} m; last frame's photometric pairs per "
          f'step {rgb[:-1, 0].int().tolist()} (observations, not claims)')
