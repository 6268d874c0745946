"""The public names of the RGB-D ICP: RgbdICP's constructor and methods, the config keys, the command-line flag and the Tracker's
switch.  No GPU: signatures and argument parsing only."""
import inspect

import pytest

from attentive_dfprior_amd import _lib, config, icp, run, slam

E = inspect.Parameter.empty


def params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_rgbd_icp_signature():
    assert issubclass(icp.RgbdICP, icp.DepthICP)
    p = inspect.signature(icp.RgbdICP.__init__).parameters
    assert [(n, q.default) for n, q in p.items()][:12] == [
        ('self', E), ('tsdf_volume', E), ('tsdf_bnds', E), ('H', E), ('W', E), ('fx', E), ('fy', E), ('cx', E), ('cy', E), ('engine', None),
        ('rgb_weight', 1.0), ('rgb_tol', 0.25)]
    assert list(p)[12:] == ['depth_icp_keywords'] and p['depth_icp_keywords'].kind is inspect.Parameter.VAR_KEYWORD
    assert params(icp.RgbdICP.set_keyframe) == [('self', E), ('c2w', E), ('color', E), ('depth', E)]
    assert params(icp.RgbdICP.refine) == [('self', E), ('guess_c2w', E), ('gt_depth', E), ('gt_color', E)]
    assert params(icp.RgbdICP.promote) == [('self', E), ('c2w', E)]
    assert params(icp.RgbdICP.last_rgb_stats) == [('self', E)]
    assert [n for n, _ in params(icp.RgbdICP.step_system_rgbd)][:7] == ['self', 'c2w', 'cur_map', 'normals_s', 'depth_m', 'normals_m', 'p_ref']
    for name in ('frame_map', 'run_steps', 'set_frame', 'last_stats', 'last_status', 'step_system', 'compute_normals'):
        assert callable(getattr(icp.RgbdICP, name)), name
    assert icp.RGB_STATS_COLUMNS == ('rgb_pairs', 'rgb_rmse') and len(icp.RGB_STATS_COLUMNS) == _lib.RGBD_STATS
    assert (_lib.RGBD_SUMS, _lib.RGBD_STATS) == (31, 2)


def test_the_depth_icp_is_as_it_was():
    assert params(icp.DepthICP.refine) == [('self', E), ('guess_c2w', E), ('gt_depth', E)]
    assert icp.DepthICP.run_steps is not icp.RgbdICP.run_steps and icp.DepthICP.step_system is icp.RgbdICP.step_system
    assert config.TRACKING_INITS == ('guess', 'icp')


def test_config_keys_and_defaults():
    assert config.TRACKING_DEFAULTS['icp_rgb'] == {}
    assert config.tracking_setting({}, 'icp_rgb') == {} and config.tracking_setting({'tracking': {'iters': 3}}, 'icp_rgb') == {}
    assert config.tracking_setting({'tracking': {'icp_rgb': {'weight': 1.0, 'tol': 0.1}}}, 'icp_rgb') == {'weight': 1.0, 'tol': 0.1}


def test_command_line_flag():
    assert run.parse_args(['x.yaml']).tracking_rgb_weight is None
    a = run.parse_args(['x.yaml', '--tracking_init', 'icp', '--tracking_rgb_weight', '0.5'])
    assert a.tracking_rgb_weight == 0.5 and a.tracking_init == 'icp'
    assert run.parse_args(['x.yaml', '--tracking_rgb_weight', '0']).tracking_rgb_weight == 0.0
    with pytest.raises(SystemExit):
        run.parse_args(['x.yaml', '--tracking_rgb_weight', 'much'])


def test_tracker_reads_the_switch():
    src = inspect.getsource(slam.Tracker)
    for word in ('icp_rgb', 'RgbdICP', 'set_keyframe', 'promote', 'last_rgb_stats'):
        assert word in src, word
    assert callable(slam.Tracker._new_icp) and isinstance(slam.Tracker.icp, property)
