"""The public names of the depth ICP: DepthICP's constructor keywords and defaults as the config's tracking.icp section passes them,
its methods, the config keys and the command-line flag.  No GPU: signatures and argument parsing only."""
import inspect

import pytest

from attentive_dfprior_amd import config, icp, run, slam, tsdf_raycast

E = inspect.Parameter.empty


def params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_depth_icp_signature():
    assert params(icp.DepthICP.__init__) == [
        ('self', E), ('tsdf_volume', E), ('tsdf_bnds', E), ('H', E), ('W', E), ('fx', E), ('fy', E), ('cx', E), ('cy', E), ('engine', None),
        ('strides', (4, 2, 1)), ('iters', (4, 3, 3)), ('dist_tol', 0.1), ('cos_tol', 0.8), ('min_pivot', 1e-6), ('min_pairs', 0.05),
        ('max_jump', 0.0), ('max_shift', 0.5), ('max_angle', 0.5), ('near', 0.0)]
    assert params(icp.DepthICP.refine) == [('self', E), ('guess_c2w', E), ('gt_depth', E)]
    assert params(icp.DepthICP.last_stats) == [('self', E)]
    assert [n for n, _ in params(icp.DepthICP.step_system)][:7] == ['self', 'c2w', 'depth_s', 'normals_s', 'depth_m', 'normals_m', 'p_ref']
    for name in ('invalidate_tsdf', 'compute_normals', 'run_steps', 'set_frame', 'last_status'):
        assert callable(getattr(icp.DepthICP, name)), name
    assert (icp.OK, icp.FEW_PAIRS, icp.DEGENERATE, icp.REJECTED) == (0, 1, 2, 3)
    assert icp.STATUS_NAMES == {0: 'ok', 1: 'few_pairs', 2: 'degenerate', 3: 'rejected'}
    assert icp.STATS_COLUMNS == ('pairs', 'rmse', 'pivot_ratio', 'omega', 'shift', 'status')


def test_render_depth_grew_only_a_trailing_keyword():
    p = params(tsdf_raycast.TsdfRaycaster.render_depth)
    assert [n for n, _ in p] == ['self', 'c2w', 'H', 'W', 'fx', 'fy', 'cx', 'cy', 'near', 'far', 'step', 'skip', 'tsdf_blocks', 'count', 'out']
    assert p[-1] == ('out', None)


def test_config_keys_and_defaults():
    assert config.tracking_setting({}, 'init') == 'guess' and config.tracking_setting({'tracking': {'iters': 3}}, 'init') == 'guess'
    assert config.tracking_setting({'tracking': {'init': 'icp'}}, 'init') == 'icp'
    assert config.tracking_setting({'tracking': {}}, 'icp') == {}
    assert config.tracking_setting({'tracking': {'icp': {'dist_tol': 0.05}}}, 'icp') == {'dist_tol': 0.05}
    assert config.TRACKING_INITS == ('guess', 'icp')
    keys = set(n for n, _ in params(icp.DepthICP.__init__)[10:])
    assert keys == {'strides', 'iters', 'dist_tol', 'cos_tol', 'min_pivot', 'min_pairs', 'max_jump', 'max_shift', 'max_angle', 'near'}
    assert callable(slam.Tracker._new_icp) and isinstance(slam.Tracker.icp, property)


def test_command_line_flag():
    assert run.parse_args(['x.yaml']).tracking_init is None
    assert run.parse_args(['x.yaml', '--tracking_init', 'icp']).tracking_init == 'icp'
    assert run.parse_args(['x.yaml', '--tracking_init', 'guess']).tracking_init == 'guess'
    with pytest.raises(SystemExit):
        run.parse_args(['x.yaml', '--tracking_init', 'other'])
