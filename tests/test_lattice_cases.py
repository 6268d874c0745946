"""CPU, oracle only: the inputs of tests/lattice_cases.py are what tests/test_gpu_grid_lattices.py relies on -- every case has a live
reference gradient in every grid, points in the TSDF band and outside the bound, and lands in the branch of the backward's scatter
selection that the case table claims.  An edit of the table, or of the rule, that empties a condition fails here, not silently on the
GPU.

The rule restated in lattice_cases.scatter_plan / scatter_branch / fine_offsets is that of csrc/adfp_kernels.hip and
csrc/adfp_backward_h.h (line numbers as of this test's writing):
  plan_sorted_scatter   adfp_kernels.hip:2839-2853   fine / coarse = the candidates of most / fewest voxels (first wins a tie); no plan
                                                     with a coarse axis < 2 cells or above 2^ADFP_BIN_MAXBITS = 256 cells
  run_decode_bwd_h      adfp_kernels.hip:2700-2708   binned = a plan and the grid's dims equal the fine or the coarse dims; else the
                                                     in-kernel scatter
  scatter_bins          adfp_kernels.hip:2533-2534   a binned grid with an axis above 1023 cells: ADFP_E_UNSUPPORTED
  bin_keys_block        adfp_backward_h.h:449-459    offset = fc - floor(cc (Rf - 1) / (Rc - 1) - 1e-3), clamped to 0..3
If one of them changes, this is where the table of lattice_cases.py gets re-derived."""
import pytest
import torch

import lattice_cases as LC
from oracle import adfp_oracle as O

# case: ((fine, coarse) or None, {grid: branch}) at stage colour, every grid wanted
CLAIMS = {
    'three_lattices': (((15, 19, 19), (3, 4, 4)), dict(grid_low='sorted', grid_high='in_kernel', grid_color='sorted')),
    'colour_coarsest': (((15, 19, 19), (3, 4, 4)), dict(grid_low='in_kernel', grid_high='sorted', grid_color='sorted')),
    'one_lattice': (((7, 9, 9), (7, 9, 9)), dict(grid_low='sorted', grid_high='sorted', grid_color='sorted')),
    'incommensurate': (((11, 14, 14), (4, 5, 5)), dict(grid_low='sorted', grid_high='in_kernel', grid_color='sorted')),
    'ratio_12': (((31, 39, 39), (3, 4, 4)), dict(grid_low='sorted', grid_high='in_kernel', grid_color='sorted')),
    'unit_axis_coarse': (None, dict(grid_low='in_kernel', grid_high='in_kernel', grid_color='in_kernel')),
    'unit_axis_fine': (((1, 12, 12), (3, 4, 4)), dict(grid_low='sorted', grid_high='sorted', grid_color='sorted')),
    'axis_257': (None, dict(grid_low='in_kernel', grid_high='in_kernel', grid_color='in_kernel')),
    'axis_1024': (((2, 2, 1024), (3, 4, 4)), dict(grid_low='sorted', grid_high='in_kernel', grid_color='refused')),
    'distinct_axes': (((13, 17, 23), (3, 4, 5)), dict(grid_low='sorted', grid_high='in_kernel', grid_color='sorted')),
}


def test_the_case_list_is_the_one_the_gpu_tests_name():
    assert list(LC.SHAPES) == list(CLAIMS) and len(LC.RUNNABLE) == 9 and LC.REFUSED == ('axis_1024',)
    assert len(set(LC.SEEDS.values())) == len(LC.SHAPES)
    assert LC.N_RAYS * (LC.NS + LC.NF) == 429
    for name in LC.SHAPES:
        c = LC.make_grids(name)
        assert [tuple(c[k].shape) for k in LC.GRIDS] == [(1, 32) + s for s in LC.SHAPES[name]]
        assert sum(v.numel() * 4 for v in c.values()) <= 8 << 20
        for k, v in c.items():
            assert 0.25 <= float(v.std()) <= 0.35, (name, k)                          # the mini scene's statistics
        again = LC.make_grids(name)
        assert all(torch.equal(c[k], again[k]) for k in c)
    # what the other cases with a plan leave open (Y == X in all of them): no two axes of a grid alike, and no two grids alike
    axes = [a for s in LC.SHAPES['distinct_axes'] for a in s]
    assert len(set(axes)) == 9
    assert max(sum(v.numel() * 4 for v in LC.make_grids(n).values()) for n in LC.RUNNABLE) <= 20 << 20


def test_scene_swaps_the_grids_and_nothing_else(mini):
    sc = LC.scene(mini, 'three_lattices')
    assert sc is not mini and sc.c is not mini.c and tuple(mini.c['grid_color'].shape[2:]) == (7, 9, 9)
    for attr in ('bound', 'tsdf_bnds', 'tsdf_volume', 'sd', 'rays_o', 'rays_d', 'gt_depth', 'gt_color', 'vol_bnds'):
        assert getattr(sc, attr) is getattr(mini, attr), attr
    assert (sc.n_samples, sc.n_surface, sc.H, sc.W) == (mini.n_samples, mini.n_surface, mini.H, mini.W)


@pytest.mark.parametrize('name', list(LC.SHAPES))
def test_every_case_lands_in_the_branch_the_table_claims(name):
    shp = LC.shapes(name)
    plan, branches = CLAIMS[name]
    assert LC.scatter_plan(shp) == plan
    assert {k: LC.scatter_branch(shp, k) for k in LC.GRIDS} == branches
    # BWD_SCATTER_IN_KERNEL: no plan at all, whatever the shapes
    assert LC.scatter_plan(shp, in_kernel_option=True) is None
    assert all(LC.scatter_branch(shp, k, in_kernel_option=True) == 'in_kernel' for k in LC.GRIDS)


def test_what_the_other_stages_of_the_cases_reach():
    """Stage low has one candidate (fine == coarse == low), stage high two: the roles move with the stage."""
    assert LC.scatter_plan(LC.shapes('three_lattices'), 'low') == ((3, 4, 4), (3, 4, 4))
    assert LC.scatter_plan(LC.shapes('three_lattices'), 'high') == ((7, 9, 9), (3, 4, 4))                 # high is binned at stage high ...
    assert LC.scatter_branch(LC.shapes('three_lattices'), 'grid_high', 'high') == 'sorted'
    assert LC.scatter_branch(LC.shapes('three_lattices'), 'grid_high', 'color') == 'in_kernel'            # ... and the third lattice at colour
    assert LC.scatter_plan(LC.shapes('colour_coarsest'), 'high') == ((15, 19, 19), (7, 9, 9))
    assert LC.scatter_plan(LC.shapes('unit_axis_coarse'), 'low') is None and LC.scatter_plan(LC.shapes('axis_257'), 'low') is None
    assert LC.scatter_plan(LC.shapes('axis_1024'), 'high') == ((7, 9, 9), (3, 4, 4))                      # the refusal needs the colour grid


@pytest.fixture(scope='module')
def oracle_runs(mini):
    """Stage colour on the 429 points, the oracle alone: per case the loss, the grids' gradients and the forward's aux."""
    out = {}
    ro, rd, gd, gc = LC.rays(mini)
    for name in LC.SHAPES:
        c = {k: v.clone().requires_grad_(True) for k, v in LC.make_grids(name).items()}
        d, u, col, w, aux = O.render_batch_ray(mini.sd, c, rd, ro, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'color', gd, LC.NS, LC.NF, return_aux=True)
        loss = O.mapper_loss(d, col, w, gd, gc, 'color', False)
        loss.backward()
        out[name] = (loss.detach(), {k: v.grad for k, v in c.items()}, aux, (d.detach(), u.detach(), col.detach()))
    return out


@pytest.mark.parametrize('name', list(LC.SHAPES))
def test_a_live_reference_gradient_in_every_grid(oracle_runs, name):
    loss, grads, aux, (d, u, col) = oracle_runs[name]
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(u).all()) and bool(torch.isfinite(col).all())
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), k
        frac = float((g != 0).float().mean())
        print(f'{name} {k} {tuple(g.shape[2:])}: gradient on {100 * frac:.1f} % of the elements, max {float(g.abs().max()):.3e}')
        assert frac > 0, k
    occ = aux['raw'].detach()[..., 3].reshape(-1)
    outside = occ == 100
    assert 0 < int(aux['band'].sum()) < 429 and 0 < int(outside.sum()) < 429
    alpha = torch.sigmoid(10 * occ[~outside])
    print(f'{name}: {int(aux["band"].sum())} points in the band, {int(outside.sum())} outside the bound, alpha {float(alpha.min()):.3f} .. {float(alpha.max()):.3f}')
    assert float(alpha.max()) > 0.05 and float(alpha.min()) < 0.95                  # neither all transparent nor all opaque
    assert bool((u > 0).all())                                                      # the Tracker loss divides by sqrt(u + 1e-10)


def pn_of_the_points(mini, aux):
    ro, rd, _, _ = LC.rays(mini)
    pts = (ro[..., None, :] + rd[..., None, :] * aux['z_vals'][..., :, None]).reshape(-1, 3)
    return O.normalize_3d_coordinate(pts, mini.bound)


def test_fine_cell_offsets_of_the_cases(mini, oracle_runs):
    """What the key arithmetic of bin_keys_block sees on the 429 points: one offset per coarse cell on one lattice (0 in an axis' first
    cell, 1 in the others -- the - 1e-3 puts f0 one cell below -- so the keys order the points by cell alone); 0 on the unit axis; the
    whole 0..3 range at the non-integer ratios; beyond 3 (clamped) at ratio 12."""
    pn = pn_of_the_points(mini, oracle_runs['one_lattice'][2])
    raw, clamped = LC.fine_offsets(LC.shapes('one_lattice'), pn)
    cell = torch.floor(((pn.float() + 1.0) / 2.0 * torch.tensor([8.0, 8.0, 6.0])).clamp_min(0.0).minimum(torch.tensor([8.0, 8.0, 6.0]))).long()
    assert torch.equal(raw, (cell > 0).long()) and int(cell.min()) == 0 and int(cell.max()) == 8
    raw, clamped = LC.fine_offsets(LC.shapes('unit_axis_fine'), pn)
    assert int(raw[:, 2].abs().max()) == 0 and int(raw[:, :2].max()) >= 2            # z: dims_f - 1 == 0
    raw, clamped = LC.fine_offsets(LC.shapes('incommensurate'), pn)
    assert set(clamped.reshape(-1).tolist()) == {0, 1, 2, 3} and int(raw.min()) >= 0
    raw, clamped = LC.fine_offsets(LC.shapes('ratio_12'), pn)
    assert int(raw.max()) >= 9 and float((raw > 3).float().mean()) > 0.3             # most fine cells of a coarse cell share offset 3
    raw, clamped = LC.fine_offsets(LC.shapes('three_lattices'), pn)
    assert int(raw.max()) >= 4                                                        # ratio 14/3 ... 18/3: the clamp works here too


@pytest.mark.parametrize('name', list(LC.UNIT_AXIS))
def test_a_unit_axis_carries_no_position_gradient(mini, name, monkeypatch):
    """d/d rays_o under the Tracker's loss is live, and its z part comes from the other grids (and the TSDF, and sin(p @ B)) only:
    with the unit-axis grids' lookups cut off from the position, z stays bit for bit and x / y change."""
    ro, rd, gd, gc = LC.rays(mini)
    c = LC.make_grids(name)
    unit = [c[k] for k in LC.UNIT_AXIS[name]]
    assert all(v.shape[2] == 1 for v in unit) and all(c[k].shape[2] > 1 for k in LC.GRIDS if k not in LC.UNIT_AXIS[name])

    def grad():
        o, d_ = ro.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        dep, u, col, w = O.render_batch_ray(mini.sd, c, d_, o, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'color', gd, LC.NS, LC.NF)
        O.tracker_loss(dep, u, col, gd, gc).backward()
        return o.grad, d_.grad
    g_o, g_d = grad()
    assert bool(torch.isfinite(g_o).all()) and all(float(g_o[:, k].abs().max()) > 0 for k in range(3))
    trilerp = O.trilerp
    monkeypatch.setattr(O, 'trilerp', lambda vol, p, bound: trilerp(vol, p.detach() if any(vol is v for v in unit) else p, bound))
    cut_o, cut_d = grad()
    assert torch.equal(cut_o[:, 2], g_o[:, 2]) and torch.equal(cut_d[:, 2], g_d[:, 2])
    assert not torch.equal(cut_o[:, :2], g_o[:, :2])
