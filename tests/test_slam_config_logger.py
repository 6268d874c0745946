"""Host tests of the run's small parts: config.load_config's inherit_from merge against the settings fixture, the checkpoint
Logger.log writes, the CLI's arguments, and the reference's signatures (tests/golden/slam_signatures.json, read from the
reference's source with ast by tests/golden/make_slam_signature_golden.py) under test_api_signatures.py's compatibility rule."""
import inspect
import json
import os
from types import SimpleNamespace

import torch
import yaml

import attentive_dfprior_amd as A
from attentive_dfprior_amd import config, eval_ate, run, slam

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = os.path.join(HERE, 'golden', 'configs', 'df_prior.yaml')
GOLDEN = os.path.join(HERE, 'golden', 'slam_signatures.json')


def test_inherit_from_merge(tmp_path):
    with open(DEFAULT) as f:
        default = yaml.full_load(f)
    family = {'dataset': 'replica', 'meshing': {'eval_rec': True}, 'tracking': {'vis_freq': 50, 'iters': 10},
              'cam': {'H': 680, 'W': 1200, 'crop_edge': 0}}
    scene = {'inherit_from': str(tmp_path / 'family.yaml'), 'mapping': {'bound': [[-1, 1], [-2, 2], [-3, 3]], 'iters': 7},
             'tracking': {'iters': 3}, 'data': {'id': 'room', 'output': 'out/room'}, 'new_section': {'a': {'b': 1}}}
    for name, d in (('family.yaml', family), ('scene.yaml', scene)):
        with open(tmp_path / name, 'w') as f:
            yaml.safe_dump(d, f)
    cfg = config.load_config(str(tmp_path / 'scene.yaml'), DEFAULT)
    assert cfg['dataset'] == 'replica' and cfg['inherit_from'] == scene['inherit_from']
    assert cfg['tracking']['iters'] == 3 and cfg['tracking']['vis_freq'] == 50 and cfg['tracking']['lr'] == default['tracking']['lr']
    assert cfg['mapping']['iters'] == 7 and cfg['mapping']['iters_first'] == default['mapping']['iters_first'] == 1500
    assert cfg['mapping']['stage'] == default['mapping']['stage'] and cfg['mapping']['bound'] == [[-1, 1], [-2, 2], [-3, 3]]
    assert cfg['meshing']['eval_rec'] is True and cfg['meshing']['resolution'] == 256
    assert cfg['data'] == {'dim': 3, 'id': 'room', 'output': 'out/room'} and cfg['new_section'] == {'a': {'b': 1}}
    # without a default path only the chain itself; the sections the default supplied are gone
    bare = config.load_config(str(tmp_path / 'scene.yaml'))
    assert 'rendering' not in bare and bare['tracking'] == {'vis_freq': 50, 'iters': 3}
    # the two older copies of the merge agree
    from attentive_dfprior_amd import get_tsdf
    assert get_tsdf.load_config(str(tmp_path / 'scene.yaml'), DEFAULT) == cfg
    assert config.get_model is A.get_model and isinstance(config.get_model(cfg), A.DF)
    assert config.DEFAULT_CONFIG == 'configs/df_prior.yaml'


def test_logger_checkpoint_has_the_nine_keys(tmp_path):
    dec = A.DF()
    c = {'grid_low': torch.randn(1, 32, 2, 3, 4), 'grid_high': torch.randn(1, 32, 4, 6, 8), 'grid_color': torch.randn(1, 32, 4, 6, 8)}
    vol = torch.randn(5, 6, 7).reshape(1, 1, 5, 6, 7).permute(0, 1, 4, 3, 2)          # the permuted view get_tsdf hands over
    s = SimpleNamespace(verbose=False, ckptsdir=str(tmp_path), shared_c=c, gt_c2w_list=torch.eye(4).repeat(3, 1, 1),
                        shared_decoders=dec, estimate_c2w_list=torch.eye(4).repeat(3, 1, 1) * 2, tsdf_volume_shared=vol)
    kd = [{'gt_c2w': torch.eye(4), 'idx': 0, 'color': torch.zeros(2, 2, 3), 'depth': torch.ones(2, 2), 'est_c2w': torch.eye(4)}]
    slam.Logger(None, None, s).log(2, kd, [0], selected_keyframes=None)
    assert os.listdir(tmp_path) == ['00002.tar']
    ck = torch.load(str(tmp_path / '00002.tar'), map_location='cpu', weights_only=False)
    assert list(ck.keys()) == ['c', 'decoder_state_dict', 'gt_c2w_list', 'estimate_c2w_list', 'keyframe_list', 'keyframe_dict',
                               'selected_keyframes', 'idx', 'tsdf_volume']
    assert ck['idx'] == 2 and ck['keyframe_list'] == [0] and ck['selected_keyframes'] is None and ck['keyframe_dict'][0]['idx'] == 0
    assert all(torch.equal(ck['c'][k], c[k]) for k in c) and torch.equal(ck['tsdf_volume'], vol) and ck['tsdf_volume'].shape == vol.shape
    assert torch.equal(ck['estimate_c2w_list'], s.estimate_c2w_list) and torch.equal(ck['gt_c2w_list'], s.gt_c2w_list)
    sd = dec.state_dict()
    assert list(ck['decoder_state_dict'].keys()) == list(sd.keys()) and all(torch.equal(ck['decoder_state_dict'][k], sd[k]) for k in sd)
    fresh = A.DF()
    fresh.load_state_dict(ck['decoder_state_dict'])


def test_cli_arguments():
    a = run.parse_args(['scene.yaml'])
    assert (a.config, a.input_folder, a.output, a.tsdf_volume, a.tsdf_bounds, a.prior, a.seed, a.last_frame, a.no_prefetch) == \
        ('scene.yaml', None, None, None, None, 'file', None, None, False)
    assert a.prior_voxel_size == 4.0 / 256 and a.default_config == 'configs/df_prior.yaml'
    a = run.parse_args(['s.yaml', '--prior', 'online', '--prior_voxel_size', '0.0625', '--seed', '3', '--last_frame', '40', '--no_prefetch',
                        '--input_folder', 'in', '--output', 'out', '--tsdf_volume', 'v.pt', '--tsdf_bounds', 'b.pt'])
    assert (a.prior, a.prior_voxel_size, a.seed, a.last_frame, a.no_prefetch, a.input_folder, a.output, a.tsdf_volume, a.tsdf_bounds) == \
        ('online', 0.0625, 3, 40, True, 'in', 'out', 'v.pt', 'b.pt')


# ---- tests/test_api_signatures.py's rule, copied ----------------------------------------------------------------------------
def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def _ref_params(entry):
    return [(n, getattr(inspect.Parameter, k), d if has else inspect.Parameter.empty) for n, k, has, d in entry]


def _assert_compatible(mine, ref, what):
    pm, pr = _params(mine), _ref_params(ref)
    assert len(pm) >= len(pr), f'{what}: fewer parameters than the reference: {pm} vs {pr}'
    for (n1, k1, d1), (n2, k2, d2) in zip(pm, pr):
        assert n1 == n2, f'{what}: parameter {n1!r} where the reference has {n2!r}'
        assert k1 == k2, f'{what}: parameter {n1!r} kind differs'
        if isinstance(d2, (list, tuple)):
            assert list(d1) == list(d2), f'{what}: default of {n1!r}'
        else:
            assert d1 == d2 or (d1 is inspect.Parameter.empty) == (d2 is inspect.Parameter.empty) and d1 == d2, \
                f'{what}: default of {n1!r}: {d1!r} vs {d2!r}'
    for n, k, d in pm[len(pr):]:                    # extensions: optional, never positional-required
        assert d is not inspect.Parameter.empty or k in (inspect.Parameter.VAR_KEYWORD, inspect.Parameter.VAR_POSITIONAL), \
            f'{what}: extra required parameter {n!r}'


def test_signatures_match_the_reference():
    with open(GOLDEN) as f:
        ref = json.load(f)['signatures']
    owners = {'DF_Prior': slam.DF_Prior, 'Mapper': slam.Mapper, 'Tracker': slam.Tracker, 'Logger': slam.Logger, 'eval_ate': eval_ate}
    assert sorted(ref) == sorted(
        ['DF_Prior.__init__', 'DF_Prior.run', 'Mapper.__init__', 'Mapper.run', 'Mapper.optimize_map', 'Mapper.keyframe_selection_overlap',
         'Tracker.__init__', 'Tracker.run', 'Tracker.optimize_cam_in_batch', 'Logger.__init__', 'Logger.log', 'eval_ate.associate',
         'eval_ate.align', 'eval_ate.plot_traj', 'eval_ate.evaluate_ate', 'eval_ate.evaluate', 'eval_ate.convert_poses'])
    for name, entry in ref.items():
        owner, attr = name.split('.')
        _assert_compatible(getattr(owners[owner], attr), entry, name)
