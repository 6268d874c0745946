"""GPU (MI355X): the kernels over the whole range of the in-band count, from an empty list to every point, against the oracle.

The high decoder and the attention MLP run on the in-band list; its length is a device word (adfp_train_state.counter, the head of
the forward workspace), the host sizes every launch from the upper bound P and the kernels cut their work down by that word:
k_attention_bwd_h, k_decode_bwd_h<64, 1, ROLE_HIGH> and k_outer_h clamp their chunk to it, k_outer_h splits its rows itself
(even_block), the attention weight gradients are written to per-workgroup slots WITHOUT a zero fill and k_reduce_partials_scaled
reads slots_in_use(count) of them -- the writer's and the reader's arithmetic must agree at every count -- and the scratch all of
this lives in is grow-only, one per engine: a call with a small count runs over what a larger call left behind.

The cases are tests/inband_cases.py's (tests/test_inband_cases.py shows on the CPU what they guarantee): counts 0, 1, 2, both sides
of the 16-row and 32-entry tile edges up to 65, both sides of 16 rows a slot at 252 and at 256 slots (the step of even_block with
and without the side lane's reserve: all four run whatever the device, no device constant is read), and every point at P = 984
and P = 2 064.  The criterion is test_gpu_grad.check_tight: conftest.TIGHT_GRAD_TOL on every element along the kernels' own ReLU
decisions, the forced decisions on boundary units only, the loss within 1e-5.

PRIMED: a case whose count is below P runs on a Renderer that has just made a training call on the same rays with the constant
0.25 volume -- every point in the band, so every staging row and every partial-sum slot that call's row split reaches holds a
foreign value (the slot cases: after a second call that reaches the remaining slots)."""
import copy

import pytest
import torch

import attentive_dfprior_amd as A
import inband_cases as IB
import test_gpu_grad as G
import test_gpu_grad_sample_range as SRG
import test_gpu_mapper_iteration as MI
from attentive_dfprior_amd import mapping
from attentive_dfprior_amd.engine import Engine
from oracle import adfp_oracle as O
from conftest import make_cfg, assert_close, assert_adam_trajectory

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = G.MODES
IN_BAND_ONLY = ('high_decoder.', 'mlp.')


@pytest.fixture(scope='module')
def cases(mini):
    return IB.build(mini)


@pytest.fixture(scope='module')
def sd():
    return O.random_state_dict(seed=17)


def primed_renderer(mini, case, sd, stage, then=None):
    """A Renderer whose engine has just trained on the case's rays with every point in the band, and after that on the case `then`
    (of the same P, so that the scratch is carved alike)."""
    rend = A.Renderer(make_cfg(IB.NS, IB.NF), None, mini)
    calls = [(IB.constant_volume(mini, 0.25), case.rays)]
    if then is not None:
        assert then.P == case.P
        calls.append((then.volume, then.rays))
    for volume, rays in calls:
        loss, c, dec = G.run(IB.with_volume(mini, volume), stage, True, sd=sd, n_samples=IB.NS, n_surface=IB.NF, rays=rays, rend=rend)
        assert bool(torch.isfinite(loss))
        assert all(float(p.grad.abs().max()) > 0 for n, p in dec.named_parameters() if n.startswith(IN_BAND_ONLY))
    return rend


def check_case(mini, case, sd, stage, mode, primed, then=None):
    rend = primed_renderer(mini, case, sd, stage, then) if primed else None
    out = {}
    G.check_tight(IB.with_volume(mini, case.volume), stage, True, mode, sd=sd, n_samples=IB.NS, n_surface=IB.NF, rays=case.rays,
                  what=f'in-band count {case.name}{", primed" if primed else ""}, ', out=out, rend=rend)
    saved = out['capture']['saved']
    assert int(Engine.state_tensor(saved, 'counter', torch.int32)[0]) == case.count
    assert int(out['capture']['relu_masks']['band'].sum()) == case.count
    grads = {n: p.grad for n, p in out['dec'].named_parameters() if n.startswith(IN_BAND_ONLY)}
    grads['grid_high'] = out['c']['grid_high'].grad
    assert len(grads) > 20
    if case.count == 0:                     # exactly zero, not small: nothing of a larger call's sums may come through
        for k, g in grads.items():
            assert g is None or float(g.abs().max()) == 0.0, f'{case.name}, {stage}: d/d {k} with an empty list: max {float(g.abs().max()):.3e}'
    else:
        assert float(out['oracle_params']['mlp.pts_linears.0.weight'].abs().max()) > 0 and float(grads['mlp.pts_linears.0.weight'].abs().max()) > 0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', IB.NAMES)
def test_gradients_over_the_in_band_count_range(mini, cases, sd, name, mode, monkeypatch):
    """Stage color with the warm-up term, every case; primed wherever the count is below P.  With every point in the band the
    priming call of a slot case has 32 rows a slot and leaves the last slots alone; slot256's 4 096 rows, 16 a slot, write them all,
    so the other three slot cases run after that call too."""
    monkeypatch.setenv('ADFP_MATH', mode)
    case = cases[name]
    then = cases[IB.SLOT_PRIMER] if name in IB.SLOT_TARGETS and name != IB.SLOT_PRIMER else None
    check_case(mini, case, sd, 'color', mode, primed=case.count < case.P, then=then)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', IB.UNPRIMED)
def test_gradients_on_fresh_scratch(mini, cases, sd, name, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    check_case(mini, cases[name], sd, 'color', mode, primed=False)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', IB.STAGE_HIGH)
def test_stage_high_gradients_over_the_in_band_count_range(mini, cases, sd, name, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    case = cases[name]
    check_case(mini, case, sd, 'high', mode, primed=case.count < case.P)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', IB.TRACKER)
def test_tracker_ray_gradients_over_the_in_band_count_range(mini, name, mode, monkeypatch):
    """The position-gradient kernels on a list (k_attention_bwd_h<false, true>, k_decode_bwd_h_pgrad3): d/d rays_o and d/d rays_d with
    an empty list, a list of one tile and one entry, and every point.  Without the anchor (inband_cases.build_tracker)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    case = IB.build_tracker(mini)[name]
    SRG._tracker_tight(IB.with_volume(mini, case.volume), case.rays, IB.NS, IB.NF, mode, f'tracker, in-band count {name},')


def _rewrite(tsdf, how, voxel):
    """The volume written in place, as TSDF fusion between keyframes writes it."""
    if how == 'every_point':
        tsdf.fill_(0.25)
    elif how in ('nothing', 'one_voxel'):
        tsdf.fill_(1.0)
        if how == 'one_voxel':
            x, y, z = voxel
            tsdf[0, 0, z, y, x] = 0.0
    else:
        assert how == 'room'


@pytest.mark.parametrize('first,then', [('room', 'every_point'), ('every_point', 'nothing'), ('every_point', 'one_voxel')])
def test_fused_iteration_follows_the_in_band_count(mini, cases, first, then):
    """The fused, graph-replayed Mapper iteration, where the side lane holds its reserve and the slot cap is 252, shaped as
    test_gpu_mapper_iteration's test of a rewritten volume: two steps, the volume rewritten in place, two steps.  From the room
    volume to constant 0.25 (every point in the band), and from there -- every slot and staging row of the graph's own workspaces
    filled -- to all 1.0 (an empty list) and to inband_cases' one-voxel volume.  Against the eager, unfused iteration, whose
    engine's scratch is zeroed before every step: a stale slot or row that is read is a foreign value on one side and zero on
    the other.  (Three runs of four steps, not one of eight: assert_adam_trajectory's bound on the outliers is for a few steps.)"""
    sc, dec, rend, rays, masks = MI.setup()
    dec_b = copy.deepcopy(dec)
    tsdf, tb = sc.tsdf_volume.to(DEV).clone(), sc.tsdf_bnds.to(DEV)
    tsdf_b = tsdf.clone()
    assert tuple(tsdf.shape) == tuple(mini.tsdf_volume.shape)
    ga, gb = ({k: v.clone().to(DEV) for k, v in sc.c.items()} for _ in range(2))
    rend_plain = A.Renderer(make_cfg(32, 16), None, sc)
    rend_plain.tsdf_blocks = False
    it_a = mapping.MapperIteration(A.Renderer(make_cfg(32, 16), None, sc), dec, ga, masks, tsdf, tb, MI.STAGE_LR, use_graph=True)
    it_b = mapping.MapperIteration(rend_plain, dec_b, gb, masks, tsdf_b, tb, MI.STAGE_LR, use_graph=False)
    eng_b = rend_plain._engine
    steps = 0
    for how in (first, then):
        for t in (tsdf, tsdf_b):
            _rewrite(t, how, cases['few1'].voxel)
        for k in range(2):
            for scratch in (eng_b._ws, eng_b._bws):
                if scratch is not None:
                    scratch.zero_()
            la, lb = float(it_a.step(*rays, 'color', True)), float(it_b.step(*rays, 'color', True))
            assert abs(la - lb) <= 1e-6 * abs(lb), (how, k, la, lb)
            steps += 1
    for k in ga:
        assert_adam_trajectory(ga[k], gb[k], 0.005, steps, f'{k} after {steps} iterations')
    for (n, p), (_, q) in zip(dec.named_parameters(), dec_b.named_parameters()):
        assert_adam_trajectory(p, q, 0.005, steps, n)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', IB.FORWARD)
def test_inference_forward_against_the_oracle(mini, cases, sd, name, mode, monkeypatch):
    """render_batch_ray under no_grad (k_tsdf's compaction, k_decode_high_g and k_attention_g on 32-entry tiles of the list) and
    eval_points on the same sample points, against the oracle at the parity tolerance; after a forward with every point in the
    band on the same Renderer wherever the count is below P."""
    monkeypatch.setenv('ADFP_MATH', mode)
    case = cases[name]
    ro_c, rd_c, gd_c, _ = case.rays
    dec = A.DF()
    dec.load_state_dict(sd)
    dec.bound = mini.bound
    dec = dec.to(DEV)
    rend = A.Renderer(make_cfg(IB.NS, IB.NF), None, mini)
    c = {k: v.to(DEV) for k, v in mini.c.items()}
    ro, rd, gd, tb = ro_c.to(DEV), rd_c.to(DEV), gd_c.to(DEV), mini.tsdf_bnds.to(DEV)
    vol = case.volume.to(DEV)

    def count():
        return int(rend._engine._ws[:4].view(torch.int32).item())
    with torch.no_grad():
        if case.count < case.P:
            rend.render_batch_ray(c, dec, rd, ro, DEV, IB.constant_volume(mini, 0.25).to(DEV), tb, 'color', gt_depth=gd)
            assert count() == case.P
        d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, vol, tb, 'color', gt_depth=gd)
        assert count() == case.count
    d2, u2, col2, w2, aux = O.render_batch_ray(sd, mini.c, rd_c, ro_c, case.volume, mini.tsdf_bnds, mini.bound, 'color', gd_c, IB.NS, IB.NF,
                                               return_aux=True)
    assert int(aux['band'].sum()) == case.count
    what = f'in-band count {name}: '
    assert_close(d, d2, 1e-4, what + 'depth')
    assert_close(u, u2, 1e-4, what + 'uncertainty')
    assert_close(col, col2, 1e-4, what + 'color')
    assert_close(w, w2, 1e-4, what + 'weight')
    pts = (ro_c[..., None, :] + rd_c[..., None, :] * aux['z_vals'][..., :, None]).reshape(-1, 3)
    with torch.no_grad():
        raw, pw = rend.eval_points(pts.to(DEV), dec, vol, tb, c, 'color', DEV)
    assert count() == case.count
    raw2, inb = aux['raw'].reshape(-1, 4), aux['inbound']
    assert bool((raw2[~inb, 3] == 100).all()) and bool((raw.cpu()[~inb, 3] == 100).all())        # (kept out of the scale of the rest)
    assert_close(raw[inb.to(DEV)], raw2[inb], 1e-4, what + 'eval_points raw')
    assert_close(raw[:, :3], raw2[:, :3], 1e-4, what + 'eval_points colour')
    assert_close(pw, w2.reshape(-1), 1e-4, what + 'eval_points weight')
