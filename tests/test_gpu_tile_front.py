"""GPU: the tile fronts of the persistent inference kernels (k_decode_lc16, k_decode_high_g, k_attention_g: csrc/adfp_decode_g.h).
The fronts were reworked for memory latency only -- the ray-mode loads of a tile issued back to back, the high decoder fetching its
next tile's front one tile ahead -- so every output of the in-band stage must keep the
BITS it had before: tests/golden/tile_front.npz was recorded with the build before the change (tools/gen_tile_front_golden.py), in
both math modes (ADFP_MATH=f16x3: the three kernels above, k_attention_g consuming what the high decoder leaves; f32: the exact kernels, which share load_point), stage colour.  NaNs are
compared as NaNs (one canonical quiet NaN on both sides, as tests/test_gpu_sampler_merge.py does).  Against the oracle: 1e-4.

Cases (tests/tile_front_cases.py):
  r3x24     3 rays x 24 samples: 72 points, a partial last tile
  r130x64   130 rays x 64: with a ray whose direction is NaN and a ray that leaves the bound at once between ordinary ones
  noband    a TSDF entirely outside the band: an empty in-band list, no tile, the one-ahead fetch must read nothing
  band32/33 in-band counts of exactly 32 (one full tile) and 33 (one entry in a second tile)
  many      40 000 rays x 64 (sha256 only): ~20 000 in-band tiles on 2 048 waves -- every wave takes several tiles, so the one-ahead
            claim and fetch really run and end in the middle of a workgroup's share
  points    eval_points and every decoder alone (adfp_decode_single) on 70 explicit f64 / f32 points: the non-ray modes of load_point
"""
import os

import numpy as np
import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import _lib
from oracle import adfp_oracle as O
from conftest import GOLDEN, assert_close
import tile_front_cases as T

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KEYS = ('depth', 'uncertainty', 'color', 'weight', 'raw', 'att_occ')
RAY_CASES = ('r3x24', 'r130x64', 'noband', 'band32', 'band33')


@pytest.fixture(scope='module')
def world():
    sc = T.Scene()
    return dict(sc=sc, cases=T.cases(sc), golden=np.load(os.path.join(GOLDEN, 'tile_front.npz')), oracle={})


def same_bits(got, want, what):
    a, b = T.canon(got), T.canon(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
    print(f'{what}: {len(bad)} of {a.size} elements differ')
    assert len(bad) == 0, (what, bad[:8].tolist(), np.asarray(got).reshape(-1)[bad[:4]].tolist(), np.asarray(want).reshape(-1)[bad[:4]].tolist())


def oracle_rays(world, name):
    if name not in world['oracle']:
        sc, case = world['sc'], world['cases'][name]
        vol = sc.tsdf_volume if case['tsdf'] == 'room' else sc.tsdf_outside
        world['oracle'][name] = O.render_batch_ray(sc.sd, sc.c, case['rd'], case['ro'], vol, sc.tsdf_bnds, sc.bound, 'color', case['gd'],
                                                   case['ns'], case['nf'], return_aux=True, depth_max=case['depth_max'])
    return world['oracle'][name]


@pytest.mark.parametrize('math', ['f16x3', 'f32'])
@pytest.mark.parametrize('name', RAY_CASES)
def test_ray_cases_keep_their_bits(world, name, math, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', math)
    sc, case, gold = world['sc'], world['cases'][name], world['golden']
    sc_dev, dec = T.device_scene(A, sc, DEV)
    r = T.run_rays(A, _lib.lib(), sc_dev, dec, case, DEV)
    S = case['ns'] + case['nf']
    print(f'{math} {name}: {case["ro"].shape[0]} rays x {S}, in-band count {r["count"]}')
    if case['band'] is not None:
        assert r['count'] == case['band']
    assert r['count'] == int(gold[f'{math}.{name}.count'])
    for k in KEYS:
        same_bits(r[k], gold[f'{math}.{name}.{k}'], f'{math} {name} {k}')
    # the oracle: the frame's outputs, the attention weights and raw of every ray whose reference is a number
    od, ou, oc, ow, aux = oracle_rays(world, name)
    assert int(aux['band'].sum()) == r['count']
    bad = torch.isnan(od)
    assert torch.equal(torch.isnan(torch.from_numpy(r['depth'])), bad)
    ok = ~bad
    if name == 'r130x64':
        assert bool(bad[T.I_NAN]) and bool(ok[T.I_OUT]) and int(bad.sum()) == 1
        assert np.isnan(r['raw'].reshape(-1, S, 4)[T.I_NAN, :, :3]).all()                       # nan_point_outputs
        assert (r['raw'].reshape(-1, S, 4)[T.I_OUT, :, 3] == 100.0).all()                       # the out-of-bound rule
    assert_close(torch.from_numpy(r['depth'])[ok], od[ok], 1e-4, f'{math} {name} depth')
    assert_close(torch.from_numpy(r['color'])[ok], oc[ok], 1e-4, f'{math} {name} colour')
    assert_close(torch.from_numpy(r['weight']).reshape(-1, S)[ok], ow.reshape(-1, S)[ok], 1e-4, f'{math} {name} attention weight')
    assert_close(torch.from_numpy(r['raw']).reshape(-1, S, 4)[ok], aux['raw'][ok], 1e-4, f'{math} {name} raw')


@pytest.mark.parametrize('math', ['f16x3', 'f32'])
def test_many_tiles_per_wave(world, math, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', math)
    sc, case, gold = world['sc'], world['cases']['many'], world['golden']
    sc_dev, dec = T.device_scene(A, sc, DEV)
    r = T.run_rays(A, _lib.lib(), sc_dev, dec, case, DEV)
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f'{math} many: in-band count {r["count"]} = {(r["count"] + 31) // 32} tiles on {waves} waves')
    assert (r['count'] + 31) // 32 > 3 * waves
    assert r['count'] == int(gold[f'{math}.many.count'])
    # the 40 000 rays are the 130 rows over and over: whichever wave and tile a point lands in, its row is the row of its first copy
    rep = r['raw'].reshape(T.MANY, -1)[:T.N * (T.MANY // T.N)].reshape(T.MANY // T.N, T.N, -1)
    assert (T.canon(rep) == T.canon(rep[0])[None]).all()
    assert T.digest(*[r[k] for k in KEYS]) == str(gold[f'{math}.many.sha256'])


@pytest.mark.parametrize('math', ['f16x3', 'f32'])
def test_explicit_points_keep_their_bits(world, math, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', math)
    sc, gold = world['sc'], world['golden']
    sc_dev, dec = T.device_scene(A, sc, DEV)
    got = T.run_points(A, sc_dev, dec, DEV)
    for k, v in got.items():
        same_bits(v, gold[f'{math}.points.{k}'], f'{math} points {k}')
    p = T.points70()
    ok = ~torch.isnan(p).any(1)
    for tag, pts in (('f64', p), ('f32', p.float().double())):
        raw, w = O.eval_points(sc.sd, pts[ok], sc.c, sc.tsdf_volume, sc.tsdf_bnds, sc.bound, 'color')
        assert_close(torch.from_numpy(got[f'eval_{tag}_raw'])[ok], raw, 1e-4, f'{math} eval_points {tag} raw')
        assert_close(torch.from_numpy(got[f'eval_{tag}_w'])[ok], w, 1e-4, f'{math} eval_points {tag} w')
        for name in ('low', 'high', 'color'):
            ref = O.mlp_forward(sc.sd, name, pts[ok], sc.c, sc.bound)
            assert_close(torch.from_numpy(got[f'single_{tag}_{name}'])[ok], ref, 1e-4, f'{math} {name} decoder alone, {tag} points')
    assert np.isnan(got['eval_f64_raw'][11, :3]).all() and got['eval_f64_raw'][12, 3] == 100.0
