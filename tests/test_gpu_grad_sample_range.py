"""GPU (MI355X): the training path over the whole sample-count range the ABI takes, S = 1..256, against the oracle's autograd along
the kernels' own ReLU decisions (test_gpu_grad.check_tight: conftest.TIGHT_GRAD_TOL on every element, the forced decisions on
boundary units only, the loss within 1e-5).

The other gradient tests run at S = 24..64 and so stay inside the first 64-sample chunk of composite_bwd_block; here the chunk 1..3
register slots, the transmittance carried forwards and the suffix sum carried backwards across chunks are compared with something
(tests/sample_range_cases.py: S on both sides of every chunk edge, and at the maximum), a training call without sensor depth is
made, and rays leave the scene bound: occupancy 100, alpha = 1 exactly, f = 1e-10, a transmittance that underflows -- the
occupancy cotangent of such a sample must vanish while its colour cotangent still reaches the border-clamped cells of the
colour grid."""
import pytest
import torch

import attentive_dfprior_amd as A
import sample_range_cases as SR
import test_gpu_grad as G
from attentive_dfprior_amd import synthetic
from oracle import adfp_oracle as O
from conftest import make_cfg, to_dev, assert_grad_tight, ReluCapture, assert_forced_decisions_are_boundary_units

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = G.MODES
N_RAYS = 24


@pytest.fixture(scope='module')
def inputs():
    sc = synthetic.mini_scene()
    return dict(sd=O.random_state_dict(seed=17), plain=SR.plain_rays(sc, N_RAYS), leaving=SR.leaving_rays(sc, N_RAYS))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', SR.S_CASES, ids=SR.case_id)
def test_gradients_over_the_sample_range(mini, inputs, case, mode, monkeypatch):
    """Stage color with the warm-up term -- all four networks, the weight cotangent and the in-band list -- at every S of S_CASES."""
    ns, nf, with_depth = case
    monkeypatch.setenv('ADFP_MATH', mode)
    G.check_tight(mini, 'color', True, mode, sd=inputs['sd'], n_samples=ns, n_surface=nf, rays=inputs['plain'], with_depth=with_depth,
                  what=f'sample range {SR.case_id(case)}, ')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', [(48, 17, True), (224, 32, True)], ids=SR.case_id)
def test_stage_low_gradients_at_65_and_256_samples(mini, inputs, case, mode, monkeypatch):
    ns, nf, with_depth = case
    monkeypatch.setenv('ADFP_MATH', mode)
    G.check_tight(mini, 'low', False, mode, sd=inputs['sd'], n_samples=ns, n_surface=nf, rays=inputs['plain'], with_depth=with_depth,
                  what=f'sample range {SR.case_id(case)}, ')


def _zero(t):
    return t is None or float(t.abs().max()) == 0.0


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ns,nf', [(100, 29), (224, 32)])
def test_gradients_of_rays_that_leave_the_bound(mini, inputs, ns, nf, mode, monkeypatch):
    """sample_range_cases.leaving_rays (tests/test_sample_range_cases.py: 10..60 % of the samples at occupancy 100, rays that leave
    the bound behind the first chunk, rays outside altogether, zero depths), stage color with warm-up: the whole criterion.
    Then the rays that lie outside altogether, alone.  Every sample has occupancy 100, a constant: without the warm-up term (the
    attention weight of a point depends on the decoders wherever the border-clamped TSDF is in its band, inside the bound or
    not) nothing reaches the grids and the low / high decoders at stages low and high -- exactly zero, not small.  At stage color
    the colour of a sample outside the bound is still decoded from the border-clamped colour grid, the first sample of such a ray
    has weight 1, and the colour grid's gradient is there and within the criterion."""
    monkeypatch.setenv('ADFP_MATH', mode)
    sd, rays = inputs['sd'], inputs['leaving']
    G.check_tight(mini, 'color', True, mode, sd=sd, n_samples=ns, n_surface=nf, rays=rays, what=f'leaving rays {ns}+{nf}, ')
    outside = SR.subset(rays, SR.far_shift(N_RAYS))
    assert outside[0].shape[0] == 6 and int((outside[2] > 0).sum()) >= 3
    for stage in ('low', 'high'):
        loss, c, dec = G.run(mini, stage, False, sd=sd, n_samples=ns, n_surface=nf, rays=outside)
        assert bool(torch.isfinite(loss)) and loss.item() > 0
        for k, v in c.items():
            assert _zero(v.grad), f'{stage}: d/d {k} of rays outside the bound: max {float(v.grad.abs().max()):.3e}'
        for name, p in dec.named_parameters():
            if name.startswith(('low_decoder', 'high_decoder')):
                assert _zero(p.grad), f'{stage}: d/d {name} of rays outside the bound: max {float(p.grad.abs().max()):.3e}'
    out = {}
    G.check_tight(mini, 'color', True, mode, sd=sd, n_samples=ns, n_surface=nf, rays=outside, what=f'outside rays {ns}+{nf}, ', out=out)
    g = out['c']['grid_color'].grad
    assert g is not None and float(g.abs().max()) > 0 and float(out['oracle_grids']['grid_color'].abs().max()) > 0
    assert_grad_tight(g, out['oracle_grids']['grid_color'], f'outside rays {ns}+{nf}, color d/d grid_color', mode)


def _tracker_tight(mini, rays, ns, nf, mode, what):
    """test_gpu_grad.test_tracker_ray_gradients_along_the_kernels_relu_decisions' comparison on given rays and sample counts."""
    dec = A.DF()
    dec.load_state_dict(mini.sd)
    dec.bound = mini.bound
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(False)
    rend = A.Renderer(make_cfg(ns, nf), None, mini)
    cap = ReluCapture(rend)
    c = to_dev(mini.c, DEV)
    ro_c, rd_c, gd_c, gc_c = rays
    ro = ro_c.to(DEV).clone().requires_grad_(True)
    rd = rd_c.to(DEV).clone().requires_grad_(True)
    gd, gc = gd_c.to(DEV), gc_c.to(DEV)
    d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), 'color', gt_depth=gd)
    loss = G.tracker_loss(d, u, col, gd, gc)
    loss.backward()
    ro_o, rd_o = ro_c.clone().requires_grad_(True), rd_c.clone().requires_grad_(True)
    O.reset_relu_flips()
    d2, u2, col2, w2 = O.render_batch_ray(mini.sd, mini.c, rd_o, ro_o, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'color', gd_c, ns, nf,
                                          relu_masks=cap.masks('color'))
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    loss2 = O.tracker_loss(d2, u2, col2, gd_c, gc_c)
    loss2.backward()
    assert bool(torch.isfinite(ro_o.grad).all()) and bool(torch.isfinite(rd_o.grad).all()), f'{what}: the oracle\'s ray gradients are not finite'
    assert float(ro_o.grad.abs().max()) > 0 and float(rd_o.grad.abs().max()) > 0
    assert abs(loss.item() - loss2.item()) <= 2e-5 * abs(loss2.item())
    assert_grad_tight(ro.grad, ro_o.grad, f'{what} d/d rays_o', mode)
    assert_grad_tight(rd.grad, rd_o.grad, f'{what} d/d rays_d', mode)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('which', ['plain', 'leaving'])
def test_tracker_ray_gradients_at_129_samples(mini, inputs, which, mode, monkeypatch):
    """d/d rays_o and d/d rays_d (reduced per ray over a row of 129 samples, three chunks) on the plain rays and on the rays of
    leaving_rays that are not outside altogether: a ray without a single sample inside has variance 0, and the loss divides by
    sqrt(variance + 1e-10)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    rays = inputs[which]
    if which == 'leaving':
        rays = SR.subset(rays, ~SR.far_shift(N_RAYS))
        assert rays[0].shape[0] == 18
    _tracker_tight(mini, rays, 100, 29, mode, f'tracker, {which} rays 100+29,')


def test_a_training_call_above_256_samples_is_refused(mini, inputs):
    """autograd.render_with_grad: S = 225 + 32 = 257 raises (test_gradients_over_the_sample_range's S256 case shows that 256 does not);
    without sensor depth the surface count does not count, and 256 + 32 trains."""
    with pytest.raises(NotImplementedError, match='256'):
        G.run(mini, 'color', True, sd=inputs['sd'], n_samples=225, n_surface=32, rays=inputs['plain'])
    with pytest.raises(NotImplementedError, match='256'):
        G.run(mini, 'color', True, sd=inputs['sd'], n_samples=257, n_surface=0, rays=inputs['plain'], with_depth=False)
    loss, c, dec = G.run(mini, 'color', True, sd=inputs['sd'], n_samples=256, n_surface=32, rays=inputs['plain'], with_depth=False)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v.grad).all()) for v in c.values())
