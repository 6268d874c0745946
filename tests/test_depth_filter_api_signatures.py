"""The public names of the depth bilateral filter: icp.depth_bilateral, DepthICP's `bilateral` keyword and its dict, the command-line
flag, synthetic.sensor_depth.  No GPU: signatures, argument parsing and the keyword's validation only."""
import inspect

import pytest

from attentive_dfprior_amd import icp, run, slam, synthetic

E = inspect.Parameter.empty


def params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_depth_bilateral_signature():
    assert params(icp.depth_bilateral) == [('depth', E), ('radius', 2), ('sigma_space', 1.5), ('sigma_depth', 0.05), ('sigma_depth_z2', 0.0),
                                           ('out', None)]
    assert 'mini scene' in icp.depth_bilateral.__doc__


def test_the_bilateral_keyword():
    assert icp.DepthICP.__init__.__kwdefaults__ == {'bilateral': None}                     # DepthICP(..., bilateral=None)
    assert 'bilateral' not in inspect.signature(icp.RgbdICP.__init__).parameters          # through **depth_icp_keywords
    with pytest.raises(ValueError, match='unknown keys'):                                 # validated before anything else is touched
        icp.DepthICP(None, None, 48, 64, 50.0, 50.0, 31.5, 23.5, bilateral={'sigma': 1.0})
    with pytest.raises(ValueError, match='radius'):
        icp.RgbdICP(None, None, 48, 64, 50.0, 50.0, 31.5, 23.5, bilateral={'radius': 9})
    assert icp.BILATERAL_DEFAULTS == {'radius': 2, 'sigma_space': 1.5, 'sigma_depth': 0.05, 'sigma_depth_z2': 0.0, 'points': True}


def test_the_keyword_is_validated():
    assert icp.bilateral_config(None) is None and icp.bilateral_config(False) is None
    assert icp.bilateral_config({}) == icp.BILATERAL_DEFAULTS
    assert icp.bilateral_config({'radius': 3, 'points': False}) == dict(icp.BILATERAL_DEFAULTS, radius=3, points=False)
    assert icp.bilateral_config({}, points=False)['points'] is False
    for bad in ({'sigma': 1.0}, {'radius': 2, 'Points': True}, {'radius': 0}, {'radius': 9}, {'radius': 2.5}, {'sigma_space': 0.0},
                {'sigma_space': float('nan')}, {'sigma_depth': -0.1}, {'sigma_depth_z2': -1.0}, {'sigma_depth_z2': float('nan')},
                {'points': 1}, 'on', 3, True):
        with pytest.raises(ValueError):
            icp.bilateral_config(bad)


def test_command_line_flag():
    assert run.parse_args(['x.yaml']).tracking_icp_bilateral is False
    a = run.parse_args(['x.yaml', '--tracking_init', 'icp', '--tracking_icp_bilateral'])
    assert a.tracking_icp_bilateral is True and a.tracking_init == 'icp'
    with pytest.raises(SystemExit):
        run.parse_args(['x.yaml', '--tracking_icp_bilateral', '2'])              # a plain flag: no value


def test_the_flag_needs_tracking_init_icp(tmp_path, monkeypatch):
    cfg = tmp_path / 'c.yaml'
    cfg.write_text('tracking:\n  iters: 0\n')
    seen = {}

    class Stop(Exception):
        pass

    def stand_in(cfg_, args):
        seen['tracking'] = cfg_['tracking']
        raise Stop()
    monkeypatch.setattr(run, 'DF_Prior', stand_in)
    none = str(tmp_path / 'no_default.yaml')
    with pytest.raises(ValueError, match='tracking.init'):
        run.main([str(cfg), '--default_config', none, '--tracking_icp_bilateral'])
    assert seen == {}
    with pytest.raises(Stop):
        run.main([str(cfg), '--default_config', none, '--tracking_init', 'icp', '--tracking_icp_bilateral'])
    assert seen['tracking']['init'] == 'icp' and seen['tracking']['icp'] == {'bilateral': {}}
    cfg.write_text('tracking:\n  init: icp\n  icp:\n    near: 0.3\n    bilateral:\n      radius: 3\n')
    with pytest.raises(Stop):
        run.main([str(cfg), '--default_config', none, '--tracking_icp_bilateral'])
    assert seen['tracking']['icp'] == {'near': 0.3, 'bilateral': {'radius': 3}}      # the config's own dict stays


def test_the_config_key_is_documented():
    assert 'tracking.icp.bilateral' in slam.__doc__ and '--tracking_icp_bilateral' in slam.__doc__


def test_sensor_depth_signature():
    assert params(synthetic.sensor_depth) == [('depth', E), ('seed', E), ('a', 0.0012), ('b', 0.0019), ('z0', 0.4), ('scale', 1.0),
                                              ('quantum', 0.0), ('edge_jump', 0.0)]
