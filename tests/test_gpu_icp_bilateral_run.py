"""GPU: the whole run with ``tracking.icp.bilateral`` on test_gpu_slam_run's analytic box-room sequence (8 frames, 48 x 64, the prior
fused from the true poses at 4/64 m voxels).

Asserted: with the key (and with the command-line flag) the run completes, the Tracker's ICP carries the filter, there is one status
per tracked frame and every pose is finite; without the key the trajectory is byte for byte the ``tracking.init: icp`` run's.  The
dataset is the clean one: its depth has no noise beyond the 16-bit PNG's steps, so the trajectory errors with and without the filter
are printed as an observation and nothing is claimed about accuracy -- what the filter buys on a noisy sensor is the tally of
tests/test_depth_filter_host.py and tests/test_gpu_icp_bilateral.py."""
import pytest
import torch

import test_gpu_slam_run as R
from test_gpu_slam_run import world  # noqa: F401  (the module-scoped dataset and prior)
from attentive_dfprior_amd import icp

pytestmark = pytest.mark.gpu
LEAN = dict(mapping={'mesh_freq': 100, 'color_refine': False}, meshing={'eval_rec': False})
ICP = {'iters': 0, 'init': 'icp', 'icp': {'near': 0.3}}          # near: see tests/test_gpu_icp_run.py


def go(world, name, tracking, extra=()):  # noqa: F811
    return R.go(world, name, extra=extra, tracking=tracking, **LEAN)[0]


def test_the_run_with_and_without_the_filter(world):  # noqa: F811
    plain = go(world, 'bilateral_absent', ICP)
    on = go(world, 'bilateral_on', dict(ICP, icp={'near': 0.3, 'bilateral': {}}))
    # without the key the run builds the object it built before the keyword existed (bytes: tests/test_gpu_icp_bilateral.py), and a
    # second run that says `bilateral: false` repeats its trajectory byte for byte
    off = go(world, 'bilateral_false', dict(ICP, icp={'near': 0.3, 'bilateral': False}))
    for s in (plain, off):
        assert type(s.tracker._icp) is icp.DepthICP and s.tracker._icp.bilateral is None and s.tracker._icp.depth.shape[0] == 2
    assert plain.estimate_c2w_list.numpy().tobytes() == off.estimate_c2w_list.numpy().tobytes()
    assert plain.tracker.icp_status == off.tracker.icp_status and len(plain.tracker.icp_status) == R.N_IMG - 1
    t = on.tracker
    assert type(t._icp) is icp.DepthICP and t._icp.bilateral == icp.BILATERAL_DEFAULTS and t._icp.near == 0.3
    assert len(t.icp_status) == R.N_IMG - 1 and all(st in (0, 1, 2, 3) for st in t.icp_status)
    est = on.estimate_c2w_list
    assert torch.isfinite(est).all() and on.ate['compared_pose_pairs'] == R.N_IMG
    assert est[0].view(torch.int32).equal(world.gt[0].view(torch.int32))
    print(f"statuses with the filter {t.icp_status}, without {plain.tracker.icp_status}; ATE rmse with "
          f"{on.ate['absolute_translational_error.rmse']:.5f} m, without {plain.ate['absolute_translational_error.rmse']:.5f} m "
          '(clean depth: an observation, not a claim)')


def test_the_command_line_flag(world):  # noqa: F811
    s = go(world, 'bilateral_flag', ICP, extra=['--tracking_icp_bilateral'])
    assert s.tracker._icp.bilateral == icp.BILATERAL_DEFAULTS and s.tracker._icp.near == 0.3
    assert len(s.tracker.icp_status) == R.N_IMG - 1 and torch.isfinite(s.estimate_c2w_list).all()
    with pytest.raises(ValueError, match='tracking.init'):
        go(world, 'bilateral_flag_no_icp', {'iters': 0}, extra=['--tracking_icp_bilateral'])
