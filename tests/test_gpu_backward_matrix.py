"""GPU (MI355X): every cell of the backward's kernel selection (csrc/adfp_kernels.hip: plan_sorted_scatter, attention_bwd_h /
attention_bwd, decode_bwd_h's selector, launch_decode_bwd, flush_pgrad) and the edges of its staging chunks.  The counterpart of
tests/test_gpu_forward_matrix.py.

  entry    render_batch_ray under autograd (adfp_render_backward); eval_points under autograd (adfp_eval_points_backward)
  math     f16x3 (the f16-split backward wherever its rule allows), ADFP_MATH=f32 (the exact kernels)
  stage    low, high, color
  wanted   grids only (masks, no layer inputs); parameters and grids; parameters only; positions only (the Tracker);
           positions with parameters and grids (bundle adjustment: the exact kernels in both modes)
  options  0, BWD_SCATTER_IN_KERNEL, BWD_STAGED_WGRAD, BWD_FUSED_ONE_WAVE, BWD_GRIDS_PREZEROED, a side lane

Not the product: one case per launcher and per branch of a selector.  Which branch each case reaches:

  RENDER_CELLS (33 rays x 13 samples = 429 points unless it says S = 5; the oracle along the kernels' ReLU decisions,
  conftest.assert_grad_tight on every wanted tensor, no gradient at all on the others)
    f16x3 color grids            k_backward_head with the sort keys, the radix sort, k_attention_bwd_h<false>, k_decode_bwd_h without
                                 staging rows on the sorted scatter (512 threads) x 3, k_scatter_sorted with three jobs
    f16x3 high  grids            the same with two grids; no colour decoder
    f16x3 color grids in_kernel  no scatter plan: k_backward_head without keys, k_max_reduce, k_decode_bwd_h with the in-kernel scatter
    f16x3 color both  S = 5      fewer than 8 samples per ray: k_decode_bwd_fused (one wave) for LOW and COLOR by the rule
    f16x3 color both  one_wave   ... by the option, at S = 13
    f16x3 color both  staged     LOW's and COLOR's staged loop (k_decode_bwd_h with rows + k_outer_h) on the sorted scatter
    f16x3 color both  in_kernel  all three staged loops with the in-kernel scatter (the fused path needs the sorted one)
    f16x3 color both  prezeroed  the head's zero fill without the grids
    f16x3 color both  side lane  the gradient-scale fold on the main stream, the sort on the lane, the whole-CU kernels on fewer CUs
    f16x3 color params           no grid wanted, so no plan: k_decode_bwd_roles without d/d c rows, HIGH staged without a scatter
    f16x3 low   params           stage low: no attention, one decoder
    f32   color grids            k_attention_bwd<false, false>, k_decode_bwd without rows x 3
    f32   color params           k_attention_bwd<true, false> + k_outer_lds, k_decode_bwd with rows and no grid gradient
  f16x3 / f32, every stage, parameters and grids, options 0 (k_attention_bwd_h<true> in one chunk, HIGH staged on the sorted scatter,
  k_decode_bwd_roles; the exact staged loops) is tests/test_gpu_forward_matrix.py::test_backward_cell_per_stage on these 429 points.

  TRACKER_CELLS (the same 429 points; ray gradients, and in the bundle-adjustment cells every grid and parameter gradient, under
  conftest.assert_grad_tight)
    f16x3 low   positions        one deferred job: launch_pgrad_single from flush_pgrad
    f16x3 high  positions        k_attention_bwd_h<false, true>, two deferred jobs: k_decode_bwd_h_pgrad3
    f16x3 color ba               positions with parameters and grids: k_attention_bwd<true, true>, k_decode_bwd<.., PGRAD> with rows
    f32   color ba               the same from the exact forward
    f32   high  positions        k_attention_bwd<false, true>, k_decode_bwd<.., PGRAD> without rows
  Stage color, positions only, both modes (three jobs in k_decode_bwd_h_pgrad3; the exact kernels) is
  tests/test_gpu_grad.py::test_tracker_ray_gradients_along_the_kernels_relu_decisions.

  POINTS_CELLS (eval_points on 429 points, some outside the bound; test_gpu_grad.py's comparison with the oracle's own autograd,
  its tolerances)
    f16x3 color grids + params   k_bin_keys as a launch of its own (no head), the sorted scatter, k_decode_bwd_roles (points are no rays)
    f16x3 color positions        three deferred jobs, one launch_pgrad_single each (no separate buffers in this entry)
  Points, grids and parameters together (the exact kernels) is tests/test_gpu_grad.py::test_eval_points_is_autograd_transparent.

  No rays / no points: zero gradients, nothing launched on the points.

  Every cell above runs on the mini scene's one geometry (high and colour one shape, low the coarser lattice).  The branches that need
  another one -- a third lattice on the in-kernel scatter beside the sorted one (run_decode_bwd_h), no plan for a coarse axis below 2 or
  above 256 cells (plan_sorted_scatter), the refusal of a binned axis above 1 023 cells (scatter_bins) -- are
  tests/test_gpu_grid_lattices.py's, on these 429 points; tests/test_lattice_cases.py shows on the CPU which case reaches which.

Chunk edges (test_chunk_edges): STG_ROWS_MAX = 163 840 staging rows; the second chunk of a loop starts above 163 840 points (exact
attention), 170 393 (exact HIGH), 177 493 (exact LOW and COLOR), 327 680 (f16-split attention) and 473 316 (f16-split staged
decoders).  Reference: with a loss that is a plain sum over rays, the gradient of a batch is the gradient of its first half plus that
of its second half, and neither half crosses a chunk; the ReLU decisions are per point and come from the forward.  Compared: every
grid and parameter gradient, in the f32 case also the ray gradients; bar conftest.TIGHT_GRAD_TOL (5e-5) x the tensor's scale, which
the code before the host refactor stays under.  Measured, worst |whole - (half + half)| / max |half + half| over the tensors of a case,
before / after the refactor (profiles/backward_host_refactor_trace.txt): f32 2 800 rays 7.9e-6 / 5.2e-6; f16x3 5 120 rays 1.7e-6 /
1.6e-6; 5 121 rays 2.4e-6 / 2.6e-6; 7 400 rays 4.9e-6 / 2.6e-6; 7 400 rays staged 5.2e-6 / 5.0e-6.  A dropped, doubled or stale chunk
is off by O(1) x scale."""
import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import synthetic, _lib
from oracle import adfp_oracle as O
from conftest import make_cfg, to_dev, assert_grad_tight, assert_forced_decisions_are_boundary_units, ReluCapture, TIGHT_GRAD_TOL
from test_gpu_grad import run, oracle_grads, tracker_loss, grad_close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_RAYS, NS, NF = 33, 8, 5                   # the forward matrix's 429 points


@pytest.fixture(scope='module')
def rays(mini):
    return tuple(t[:N_RAYS].contiguous() for t in (mini.rays_o, mini.rays_d, mini.gt_depth, mini.gt_color))


def wanting(wanted, prezeroed=False):
    """run()'s `rend` hook: the call's parameters / grids want a gradient as `wanted` says ('grids', 'params', 'both'); prezeroed:
    the backward gets BWD_GRIDS_PREZEROED and finds its channels-last gradient scratch zeroed, as the option promises."""
    def prime(rend):
        eng, render = rend._engine, rend.render_batch_ray

        def call(c, dec, *a, **k):
            for p in dec.parameters():
                p.requires_grad_(wanted in ('params', 'both'))
            for v in c.values():
                v.requires_grad_(wanted in ('grids', 'both'))
            return render(c, dec, *a, **k)
        rend.render_batch_ray = call
        if prezeroed:
            backward = eng.render_backward

            def zeroed(decoders, c, *a, **k):
                need_grid = a[9]
                for name in ('low', 'high', 'color'):
                    if need_grid.get(name):
                        Z, Y, X = c['grid_' + name].shape[2:]
                        eng._cl_scratch(name, (Z, Y, X, 32), c['grid_' + name].device).zero_()
                return backward(decoders, c, *a, **k)
            eng.render_backward = zeroed
    return prime


RENDER_CELLS = [
    # id, math, stage, wanted, samples, surface samples, options, side lane
    ('f16x3-color-grids', 'f16x3', 'color', 'grids', NS, NF, 0, None),
    ('f16x3-high-grids', 'f16x3', 'high', 'grids', NS, NF, 0, None),
    ('f16x3-color-grids-in_kernel', 'f16x3', 'color', 'grids', NS, NF, _lib.BWD_SCATTER_IN_KERNEL, None),
    ('f16x3-color-both-S5', 'f16x3', 'color', 'both', 3, 2, 0, None),
    ('f16x3-color-both-one_wave', 'f16x3', 'color', 'both', NS, NF, _lib.BWD_FUSED_ONE_WAVE, None),
    ('f16x3-color-both-staged', 'f16x3', 'color', 'both', NS, NF, _lib.BWD_STAGED_WGRAD, None),
    ('f16x3-color-both-in_kernel', 'f16x3', 'color', 'both', NS, NF, _lib.BWD_SCATTER_IN_KERNEL, None),
    ('f16x3-color-both-prezeroed', 'f16x3', 'color', 'both', NS, NF, _lib.BWD_GRIDS_PREZEROED, None),
    ('f16x3-color-both-side_lane', 'f16x3', 'color', 'both', NS, NF, 0, True),
    ('f16x3-color-params', 'f16x3', 'color', 'params', NS, NF, 0, None),
    ('f16x3-low-params', 'f16x3', 'low', 'params', NS, NF, 0, None),
    ('f32-color-grids', 'f32', 'color', 'grids', NS, NF, 0, None),
    ('f32-color-params', 'f32', 'color', 'params', NS, NF, 0, None),
]


@pytest.mark.parametrize('cell', RENDER_CELLS, ids=[c[0] for c in RENDER_CELLS])
def test_render_cells(mini, rays, cell, monkeypatch):
    _, mode, stage, wanted, ns, nf, options, lane = cell
    monkeypatch.setenv('ADFP_MATH', mode)
    warm = stage != 'color'
    cap = {}
    loss, c, dec = run(mini, stage, warm, n_samples=ns, n_surface=nf, rays=rays, bwd_options=options, capture=cap, side_lane=lane,
                       rend=wanting(wanted, prezeroed=bool(options & _lib.BWD_GRIDS_PREZEROED)))
    O.reset_relu_flips()
    loss2, g_grids, g_params = oracle_grads(mini, mini.sd, rays, stage, warm, ns, nf, relu_masks=cap['relu_masks'])
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    assert abs(loss.item() - loss2.item()) <= 1e-5 * abs(loss2.item())
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)                       # noqa: E731
    for k, v in c.items():
        if wanted == 'params':
            assert v.grad is None, k
        else:
            assert_grad_tight(zero(v), g_grids[k], f'{cell[0]} d/d {k}', mode)
    for name, p in dec.named_parameters():
        if wanted == 'grids':
            assert p.grad is None, name
        else:
            assert_grad_tight(zero(p), g_params[name], f'{cell[0]} d/d {name}', mode)
    if wanted != 'params':
        assert float(c['grid_low'].grad.abs().max()) > 0


TRACKER_CELLS = [('f16x3', 'low', False), ('f16x3', 'high', False), ('f16x3', 'color', True), ('f32', 'color', True), ('f32', 'high', False)]


@pytest.mark.parametrize('mode,stage,ba', TRACKER_CELLS, ids=['%s-%s-%s' % (m, s, 'ba' if b else 'positions') for m, s, b in TRACKER_CELLS])
def test_tracker_cells(mini, rays, mode, stage, ba, monkeypatch):
    """Ray gradients under the Tracker's loss; ba: the grids and the parameters want theirs too (the Mapper's bundle adjustment)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    dec = A.DF()
    dec.load_state_dict(mini.sd)
    dec.bound = mini.bound
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(ba)
    rend = A.Renderer(make_cfg(NS, NF), None, mini)
    cap = ReluCapture(rend)
    c = {k: v.to(DEV).clone().requires_grad_(ba) for k, v in mini.c.items()}
    ro, rd = rays[0].to(DEV).clone().requires_grad_(True), rays[1].to(DEV).clone().requires_grad_(True)
    gd, gc = rays[2].to(DEV), rays[3].to(DEV)
    d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), stage, gt_depth=gd)
    loss = tracker_loss(d, u, col, gd, gc)
    loss.backward()
    c_o = {k: v.clone().requires_grad_(ba) for k, v in mini.c.items()}
    sd_o = {k: v.clone().requires_grad_(ba) for k, v in mini.sd.items()}
    ro_o, rd_o = rays[0].clone().requires_grad_(True), rays[1].clone().requires_grad_(True)
    O.reset_relu_flips()
    d2, u2, col2, w2 = O.render_batch_ray(sd_o, c_o, rd_o, ro_o, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, stage, rays[2], NS, NF,
                                          relu_masks=cap.masks(stage))
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    loss2 = O.tracker_loss(d2, u2, col2, rays[2], rays[3])
    loss2.backward()
    assert abs(loss.item() - loss2.item()) <= 2e-5 * abs(loss2.item())
    assert_grad_tight(ro.grad, ro_o.grad, f'{stage} d/d rays_o', mode)
    assert_grad_tight(rd.grad, rd_o.grad, f'{stage} d/d rays_d', mode)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)                       # noqa: E731
    if ba:
        for k in c:
            assert_grad_tight(zero(c[k]), zero(c_o[k]), f'{stage} ba d/d {k}', mode)
        for name, p in dec.named_parameters():
            assert_grad_tight(zero(p), zero(sd_o[name]), f'{stage} ba d/d {name}', mode)
        assert float(c['grid_color'].grad.abs().max()) > 0


@pytest.mark.parametrize('wanted', ['grids+params', 'positions'])
def test_eval_points_cells(mini, wanted, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', 'f16x3')
    g = torch.Generator().manual_seed(12)
    lo, hi = mini.bound[:, 0], mini.bound[:, 1]
    pts = lo + (hi - lo) * (torch.rand(429, 3, generator=g, dtype=torch.float64) * 1.1 - 0.05)     # some outside the bound
    wr, ww = torch.randn(429, 4, generator=g), torch.randn(429, generator=g)
    pos = wanted == 'positions'
    c_o = {k: v.clone().requires_grad_(not pos) for k, v in mini.c.items()}
    sd_o = {k: v.clone().requires_grad_(not pos) for k, v in mini.sd.items()}
    p_o = pts.clone().requires_grad_(pos)
    raw_o, w_o = O.eval_points(sd_o, p_o, c_o, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'color')
    ((raw_o * wr).sum() + (w_o * ww).sum()).backward()
    dec = A.DF()
    dec.load_state_dict(mini.sd)
    dec.bound = mini.bound
    dec = dec.to(DEV)
    for prm in dec.parameters():
        prm.requires_grad_(not pos)
    rend = A.Renderer(make_cfg(NS, NF), None, mini)
    c = {k: v.to(DEV).clone().requires_grad_(not pos) for k, v in mini.c.items()}
    p = pts.to(DEV).requires_grad_(pos)
    raw, w = rend.eval_points(p, dec, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), c, 'color', DEV)
    ((raw * wr.to(DEV)).sum() + (w * ww.to(DEV)).sum()).backward()
    if pos:
        grad_close(p.grad, p_o.grad, 'd/d points', 5e-4)
        assert all(v.grad is None for v in c.values()) and all(prm.grad is None for prm in dec.parameters())
        return
    assert p.grad is None
    for k in c:
        grad_close(c[k].grad, c_o[k].grad, k)
    for name, prm in dec.named_parameters():
        grad_close(prm.grad, sd_o[name].grad, name, mode='f16x3')


@pytest.mark.parametrize('mode', ['f16x3', 'f32'])
def test_no_rays_and_no_points(mini, rays, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    empty = tuple(t[:0] for t in rays)
    loss, c, dec = run(mini, 'color', False, n_samples=NS, n_surface=NF, rays=empty)
    assert loss.item() == 0
    for k, v in c.items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().max()) == 0, k
    assert all(p.grad is None or float(p.grad.abs().max()) == 0 for p in dec.parameters())
    rend = A.Renderer(make_cfg(NS, NF), None, mini)
    c = {k: v.to(DEV).clone().requires_grad_(True) for k, v in mini.c.items()}
    p = torch.zeros((0, 3), dtype=torch.float64, device=DEV, requires_grad=True)
    raw, w = rend.eval_points(p, dec, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), c, 'color', DEV)
    assert raw.shape == (0, 4) and w.shape == (0,)
    (raw.sum() + w.sum()).backward()
    assert all(v.grad is None or float(v.grad.abs().max()) == 0 for v in c.values())


# --------------------------------------------------------------------------- chunk edges
CHUNK_S = (48, 16)
CHUNK_CASES = [
    # id, rays, math, options: what it crosses
    ('f32-2800', 2800, 'f32', 0),                                       # 179 200 points: all four exact loops take two chunks
    ('f16x3-5120', 5120, 'f16x3', 0),                                   # 327 680: the f16-split attention's last one-chunk size
    ('f16x3-5121', 5121, 'f16x3', 0),                                   # 327 744: one tile into the attention's second chunk
    ('f16x3-7400', 7400, 'f16x3', 0),                                   # 473 600: HIGH's staged loop
    ('f16x3-7400-staged', 7400, 'f16x3', _lib.BWD_STAGED_WGRAD),        # ... and LOW's and COLOR's
]


def chunk_gradients(mini, dec, rend, batch, cot, with_rays, depth_max):
    """Every grid and parameter gradient (and the ray gradients) of sum(depth * a) + sum(color * b) + sum(weight * c) over `batch`."""
    ro, rd, gd = (t.to(DEV) for t in batch)
    a, b, cw = (t.to(DEV) for t in cot)
    c = {k: v.to(DEV).clone().requires_grad_(True) for k, v in mini.c.items()}
    ro, rd = ro.clone().requires_grad_(with_rays), rd.clone().requires_grad_(with_rays)
    d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), 'color', gt_depth=gd,
                                         depth_max=depth_max)
    loss = (d * a).sum() + (col * b).sum() + (w * cw).sum()
    names = list(c) + [n for n, _ in dec.named_parameters()]
    leaves = list(c.values()) + [p for _, p in dec.named_parameters()]
    if with_rays:
        names += ['rays_o', 'rays_d']
        leaves += [ro, rd]
    grads = torch.autograd.grad(loss, leaves)
    return {n: g.detach().double() for n, g in zip(names, grads)}


@pytest.mark.parametrize('case', CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_chunk_edges(mini, case, monkeypatch):
    tag, n, mode, options = case
    monkeypatch.setenv('ADFP_MATH', mode)
    S = sum(CHUNK_S)
    ro, rd, gd, _ = synthetic.make_ray_batch(synthetic.mini_scene(), n, seed=8, poses=3)
    g = torch.Generator().manual_seed(31)
    cot = (torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, 3, generator=g), torch.randn(n, S, 1, generator=g))
    dec = A.DF()
    dec.load_state_dict(mini.sd)
    dec.bound = mini.bound
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(True)
    rend = A.Renderer(make_cfg(*CHUNK_S), None, mini)
    rend._engine.bwd_options = options
    depth_max = gd.max().reshape(1).to(DEV)                               # the halves clamp `far` like the whole batch does
    with_rays = mode == 'f32'
    h = n // 2
    whole = chunk_gradients(mini, dec, rend, (ro, rd, gd), cot, with_rays, depth_max)
    parts = [chunk_gradients(mini, dec, rend, (ro[s], rd[s], gd[s]), tuple(t[s] for t in cot), with_rays, depth_max)
             for s in (slice(0, h), slice(h, n))]
    worst, where = 0.0, None
    for k in whole:
        ref = torch.cat([parts[0][k], parts[1][k]]) if k.startswith('rays_') else parts[0][k] + parts[1][k]
        err = float((whole[k] - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        assert float(ref.abs().max()) > 0, k
        if err > worst:
            worst, where = err, k
    print(f'chunk edge {tag}: {n * S} points, worst |whole - (half + half)| / scale = {worst:.2e} ({where})')
    assert worst <= TIGHT_GRAD_TOL[mode], f'{tag}: {where} is off by {worst:.2e} x scale'
