"""GPU (MI355X): the decoders, forward and backward, on feature-grid geometries other than the suite's one (tests/lattice_cases.py: three
different lattices, swapped roles, one lattice, non-integer and large cell ratios, a unit axis, axes past the sorted scatter's limits).
Which branch of plan_sorted_scatter / run_decode_bwd_h / scatter_bins each case reaches is asserted on the CPU in
tests/test_lattice_cases.py; here every case runs on the forward and backward matrices' 429 points (33 rays x 13 samples: 14 tiles, not a
multiple of 32, 262 points in the TSDF band, 20 outside the bound) in both math modes, against the oracle at the suite's own bars:

  forward    conftest.assert_close at the forward matrix's 1e-4 -- render_batch_ray at every stage as inference and as a training
             forward, eval_points on the f64 points and their f32 rounding with the `== 100` pattern exact.  The three grids differ in
             every case but one, so a kernel that reads one grid's dims for another shows.
  Mapper     test_gpu_grad.check_tight (the oracle's autograd along the kernels' ReLU decisions, conftest.TIGHT_GRAD_TOL x scale on
             every element of every grid and parameter gradient) at every stage; stage colour also with the grids alone wanted
             (k_decode_bwd_h without staging rows) and, f16x3, with BWD_SCATTER_IN_KERNEL; every grid's gradient is non-zero
  Tracker    d/d rays_o, d/d rays_d under the Tracker's loss, stage colour: three deferred position-gradient jobs with three different
             dims, tri_axis_d on a unit axis; one bundle-adjustment cell (three_lattices, f16x3)
  refusal    axis_1024: the forward has no limit; the f16-split backward raises ADFP_E_UNSUPPORTED (scatter_bins, after the call's head,
             sort and first kernels are queued) and leaves the Renderer usable -- the default lattice then passes check_tight on it, with
             and without the side lane; the exact backward (no sorted scatter) has no such limit and is held to the oracle.

Every test prints its worst error / tolerance ratio per tensor kind; measured on the MI355X: profiles/grid_lattices_grad_stats.txt."""
import os
import re

import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import _lib
from oracle import adfp_oracle as O
from conftest import make_cfg, assert_close, assert_grad_tight, assert_forced_decisions_are_boundary_units, ReluCapture, TIGHT_GRAD_TOL
from test_gpu_parity import build
from test_gpu_grad import run, oracle_grads, check_tight, tracker_loss
from test_gpu_backward_matrix import wanting
import lattice_cases as LC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4                                  # the forward matrix's
MODES = ['f16x3', 'f32']
NS, NF = LC.NS, LC.NF
S = NS + NF


@pytest.fixture(autouse=True)
def measured(request, monkeypatch, tmp_path):
    """The comparisons' own logs (conftest: ADFP_GRAD_STATS, ADFP_PARITY_STATS), read back after the test: the worst error / tolerance
    per tensor kind."""
    logs = {}
    for var in ('ADFP_GRAD_STATS', 'ADFP_PARITY_STATS'):
        path = os.environ.get(var)
        if not path:
            path = str(tmp_path / var.lower())
            monkeypatch.setenv(var, path)
        logs[var] = (path, os.path.getsize(path) if os.path.exists(path) else 0)
    yield
    worst = {}
    for var, (path, start) in logs.items():
        if not os.path.exists(path):
            continue
        with open(path) as f:
            f.seek(start)
            for line in f:
                t = line.split()
                if var == 'ADFP_GRAD_STATS' and t and t[0] == 'tight' and ' d/d ' in line:
                    name = line.split(' d/d ')[1].split()[0]
                    kind = 'grid' if name.startswith('grid_') else 'ray' if name.startswith('rays_') else 'parameter'
                    worst[kind] = max(worst.get(kind, 0.0), float(t[-1]) / TIGHT_GRAD_TOL[t[1]])
                m = re.search(r'\| tol \S+ worst (\S+) of the limit', line) if var == 'ADFP_PARITY_STATS' else None
                if m:
                    worst['forward'] = max(worst.get('forward', 0.0), float(m.group(1)))
    if worst:
        print(f'{request.node.name}: worst error / tolerance ' + ', '.join(f'{k} {v:.3f}' for k, v in sorted(worst.items())))


class Ref(object):
    pass


_REFS = {}


def ref_of(mini, name):
    """The case's scene and the oracle on its 429 points, once per case: per stage the render's outputs and raw; the points (f64) and
    eval_points on them and on their f32 rounding."""
    if name in _REFS:
        return _REFS[name]
    r = Ref()
    r.sc = sc = LC.scene(mini, name)
    r.rays = LC.rays(mini)
    ro, rd, gd, _ = r.rays
    r.render, r.pts_raw = {}, {}
    with torch.no_grad():
        for stage in O.STAGES:
            d, u, c, w, aux = O.render_batch_ray(sc.sd, sc.c, rd, ro, sc.tsdf_volume, sc.tsdf_bnds, sc.bound, stage, gd, NS, NF, return_aux=True)
            r.render[stage] = (d, u, c, w)
        r.pts = (ro[..., None, :] + rd[..., None, :] * aux['z_vals'][..., :, None]).reshape(-1, 3)
        assert r.pts.dtype == torch.float64 and r.pts.shape[0] == 429
        assert 0 < int(aux['band'].sum()) < 429 and int((aux['raw'][..., 3] == 100).sum()) > 0
        for dt in (torch.float64, torch.float32):
            for stage in O.STAGES:
                r.pts_raw[dt, stage] = O.eval_points(sc.sd, r.pts.to(dt), sc.c, sc.tsdf_volume, sc.tsdf_bnds, sc.bound, stage)
    _REFS[name] = r
    return r


def scene_on_gpu(sc, train):
    dec, rend = build(sc, sc.sd, NS, NF)
    for p in dec.parameters():
        p.requires_grad_(train)
    c = {k: v.to(DEV).clone().requires_grad_(train) for k, v in sc.c.items()}
    return dec, rend, c


def forward_against_the_oracle(r, stages, calls, label):
    sc = r.sc
    ro, rd, gd, _ = (t.to(DEV) for t in r.rays)
    tsdf, tb = sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV)
    for train in calls:
        dec, rend, c = scene_on_gpu(sc, train)
        call = 'training' if train else 'inference'
        for stage in stages:
            with torch.set_grad_enabled(train):
                d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, tsdf, tb, stage, gt_depth=gd)
            assert d.requires_grad == train
            od, ou, oc, ow = r.render[stage]
            assert_close(d.detach(), od, TOL, f'{label} {stage} {call} depth')
            assert_close(u.detach(), ou, TOL, f'{label} {stage} {call} uncertainty')
            assert_close(col.detach(), oc, TOL, f'{label} {stage} {call} color')
            assert_close(w.detach(), ow, TOL, f'{label} {stage} {call} weight')
            if train:
                continue
            for dt in (torch.float64, torch.float32):
                with torch.no_grad():
                    raw, pw = rend.eval_points(r.pts.to(dt).to(DEV), dec, tsdf, tb, c, stage, DEV)
                oraw, opw = r.pts_raw[dt, stage]
                assert torch.equal(raw[:, 3].cpu() == 100, oraw[:, 3] == 100), f'{label} {stage} {dt}: the out-of-bound pattern'
                inb = oraw[:, 3] != 100
                assert 0 < int(inb.sum()) < 429
                assert_close(raw, oraw, TOL, f'{label} {stage} points {dt} raw')
                # ... and without the 100s as the tensor's scale, where both sides see the same normalised coordinate: f64 points,
                # rounded to f32 once.  f32 points the oracle normalises in f32, as the reference does, the kernels in f64: an ulp of
                # a coordinate near 1 is 3e-5 cells of a 1 024-cell axis, and the ORACLE moves by 4.4e-5 (axis_257) / 5.7e-5 (axis_1024)
                # of a scale of 4.8 / 4.4 between the two normalisations of the same f32 points (2e-6 on the small grids) -- the
                # kernels' distance from it on f32 points is that figure (measured 4.1e-5 / 5.7e-5), not theirs.
                if dt == torch.float64:
                    assert_close(raw.cpu()[inb], oraw[inb], TOL, f'{label} {stage} points {dt} raw inside the bound')
                assert_close(pw, opw, TOL, f'{label} {stage} points {dt} w')


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', LC.RUNNABLE)
def test_forward(mini, name, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    forward_against_the_oracle(ref_of(mini, name), O.STAGES, (False, True), f'lattice {name}')


def with_options(options):
    """run()'s `rend` hook: the fresh Renderer's backward gets `options`."""
    def prime(rend):
        rend._engine.bwd_options = options
    return prime


def every_grid_has_a_gradient(c, stage, label):
    for k in LC.STAGE_GRIDS[stage]:
        assert c[k].grad is not None and float(c[k].grad.abs().max()) > 0, f'{label}: no gradient in {k}'
    for k in LC.GRIDS:
        if k not in LC.STAGE_GRIDS[stage]:
            assert c[k].grad is None or float(c[k].grad.abs().max()) == 0, f'{label}: stage {stage} wrote a gradient into {k}'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('stage', O.STAGES)
@pytest.mark.parametrize('name', LC.RUNNABLE)
def test_mapper_gradients(mini, name, stage, mode, monkeypatch):
    """Parameters and grids wanted, every stage (the warm-up term where the stage has it in the Mapper's schedule)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    r = ref_of(mini, name)
    out = {}
    check_tight(r.sc, stage, stage != 'color', mode, n_samples=NS, n_surface=NF, rays=r.rays, what=f'lattice {name}, ', out=out)
    every_grid_has_a_gradient(out['c'], stage, f'{name} {stage}')


@pytest.mark.parametrize('name', LC.RUNNABLE)
def test_mapper_gradients_with_the_in_kernel_scatter(mini, name, monkeypatch):
    """BWD_SCATTER_IN_KERNEL on the f16-split backward: held to the oracle like the default, not only to the other option value."""
    monkeypatch.setenv('ADFP_MATH', 'f16x3')
    r = ref_of(mini, name)
    out = {}
    check_tight(r.sc, 'color', False, 'f16x3', n_samples=NS, n_surface=NF, rays=r.rays, what=f'lattice {name} in_kernel, ', out=out,
                rend=with_options(_lib.BWD_SCATTER_IN_KERNEL))
    every_grid_has_a_gradient(out['c'], 'color', f'{name} in_kernel')


def grids_only_cell(sc, rays, mode, label, lane=None, rend=None):
    """Stage colour, the grids alone want a gradient (test_gpu_backward_matrix.test_render_cells' comparison)."""
    cap = {}
    loss, c, dec = run(sc, 'color', False, n_samples=NS, n_surface=NF, rays=rays, capture=cap, side_lane=lane, rend=rend or wanting('grids'))
    O.reset_relu_flips()
    loss2, g_grids, g_params = oracle_grads(sc, sc.sd, rays, 'color', False, NS, NF, relu_masks=cap['relu_masks'])
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    assert abs(loss.item() - loss2.item()) <= 1e-5 * abs(loss2.item())
    for k, v in c.items():
        assert v.grad is not None, k
        assert_grad_tight(v.grad, g_grids[k], f'{label} d/d {k}', mode)
    assert all(p.grad is None for p in dec.parameters())
    every_grid_has_a_gradient(c, 'color', label)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', LC.RUNNABLE)
def test_mapper_gradients_of_the_grids_alone(mini, name, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    r = ref_of(mini, name)
    grids_only_cell(r.sc, r.rays, mode, f'lattice {name} grids only, color')


def tracker_cell(sc, rays, mode, stage, ba, label):
    """test_gpu_backward_matrix.test_tracker_cells' comparison on the scene `sc`."""
    dec = A.DF()
    dec.load_state_dict(sc.sd)
    dec.bound = sc.bound
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(ba)
    rend = A.Renderer(make_cfg(NS, NF), None, sc)
    cap = ReluCapture(rend)
    c = {k: v.to(DEV).clone().requires_grad_(ba) for k, v in sc.c.items()}
    ro, rd = rays[0].to(DEV).clone().requires_grad_(True), rays[1].to(DEV).clone().requires_grad_(True)
    gd, gc = rays[2].to(DEV), rays[3].to(DEV)
    d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV), stage, gt_depth=gd)
    loss = tracker_loss(d, u, col, gd, gc)
    loss.backward()
    c_o = {k: v.clone().requires_grad_(ba) for k, v in sc.c.items()}
    sd_o = {k: v.clone().requires_grad_(ba) for k, v in sc.sd.items()}
    ro_o, rd_o = rays[0].clone().requires_grad_(True), rays[1].clone().requires_grad_(True)
    O.reset_relu_flips()
    d2, u2, col2, w2 = O.render_batch_ray(sd_o, c_o, rd_o, ro_o, sc.tsdf_volume, sc.tsdf_bnds, sc.bound, stage, rays[2], NS, NF,
                                          relu_masks=cap.masks(stage))
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    loss2 = O.tracker_loss(d2, u2, col2, rays[2], rays[3])
    loss2.backward()
    assert abs(loss.item() - loss2.item()) <= 2e-5 * abs(loss2.item())
    assert float(ro_o.grad.abs().max()) > 0 and float(rd_o.grad.abs().max()) > 0
    assert_grad_tight(ro.grad, ro_o.grad, f'{label} d/d rays_o', mode)
    assert_grad_tight(rd.grad, rd_o.grad, f'{label} d/d rays_d', mode)
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)                       # noqa: E731
    if ba:
        for k in c:
            assert_grad_tight(zero(c[k]), zero(c_o[k]), f'{label} d/d {k}', mode)
        for pname, p in dec.named_parameters():
            assert_grad_tight(zero(p), zero(sd_o[pname]), f'{label} d/d {pname}', mode)
        every_grid_has_a_gradient(c, stage, label)
    else:
        assert all(v.grad is None for v in c.values()) and all(p.grad is None for p in dec.parameters())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', LC.RUNNABLE)
def test_tracker_gradients(mini, name, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    r = ref_of(mini, name)
    tracker_cell(r.sc, r.rays, mode, 'color', False, f'lattice {name} tracker, color')


def test_bundle_adjustment_on_three_lattices(mini, monkeypatch):
    """Positions, parameters and grids wanted together."""
    monkeypatch.setenv('ADFP_MATH', 'f16x3')
    r = ref_of(mini, 'three_lattices')
    tracker_cell(r.sc, r.rays, 'f16x3', 'color', True, 'lattice three_lattices ba, color')


# --------------------------------------------------------------------------- axis_1024: the sorted scatter's packed cell coordinates
@pytest.mark.parametrize('mode', MODES)
def test_forward_has_no_axis_limit(mini, mode, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    forward_against_the_oracle(ref_of(mini, 'axis_1024'), ('color',), (False,), 'lattice axis_1024')


@pytest.mark.parametrize('lane', [None, True], ids=['one_stream', 'side_lane'])
def test_a_refused_backward_leaves_the_renderer_usable(mini, lane, monkeypatch):
    """The colour grid is the plan's fine grid and has a 1 024-cell axis: scatter_bins refuses it when the call's head, the sort (on the
    side lane, if there is one) and the other decoders' kernels are already queued.  The binding raises; the same Renderer -- its side
    lane joined, its compute units handed back, its grow-only scratch as the call left it -- then runs the default lattice through
    check_tight, on the same lane setting."""
    monkeypatch.setenv('ADFP_MATH', 'f16x3')
    r = ref_of(mini, 'axis_1024')
    kept = []
    with pytest.raises(RuntimeError, match='ADFP_E_UNSUPPORTED'):
        run(r.sc, 'color', False, n_samples=NS, n_surface=NF, rays=r.rays, side_lane=lane, rend=kept.append)
    assert len(kept) == 1
    torch.cuda.synchronize()
    check_tight(mini, 'color', False, 'f16x3', n_samples=NS, n_surface=NF, rays=r.rays, what='default lattice after a refused call, ', rend=kept[0])


def test_the_exact_backward_has_no_axis_limit(mini, monkeypatch):
    """ADFP_MATH=f32: no sorted scatter in the call, the in-kernel scatter addresses whole voxels."""
    monkeypatch.setenv('ADFP_MATH', 'f32')
    r = ref_of(mini, 'axis_1024')
    out = {}
    check_tight(r.sc, 'color', False, 'f32', n_samples=NS, n_surface=NF, rays=r.rays, what='lattice axis_1024, ', out=out)
    every_grid_has_a_gradient(out['c'], 'color', 'axis_1024 f32')
