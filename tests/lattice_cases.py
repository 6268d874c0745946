"""Feature-grid geometries other than the one every scene of the suite has (low at grid_len 0.32, high and colour at 0.16: high and
colour one shape, low the coarser lattice at half the resolution).  Shared by tests/test_lattice_cases.py (CPU, the oracle alone) and
tests/test_gpu_grid_lattices.py / tests/test_gpu_mapper_iteration.py (the kernels).

A case replaces only the three grids of the committed mini scene (conftest.Mini): bound, TSDF, rays, decoder weights and sample counts
stay.  Shapes are explicit (Z, Y, X), not grid_len: the reference's int(extent / grid_len) gives 0 for an axis thinner than a cell.
The grids are seeded normals of the mini scene's statistics (std 0.3 per grid: synthetic.make_grids with std_scale = 30, and the
x 100 on grid_high of synthetic.mini_scene), one fixed seed per case.

What each case reaches in csrc/adfp_kernels.hip (plan_sorted_scatter, run_decode_bwd_h, scatter_bins) -- restated in Python and
asserted in tests/test_lattice_cases.py:

  three_lattices     coarse = low, fine = colour; high is a third lattice: the in-kernel scatter beside two sorted-scatter jobs
  colour_coarsest    the roles swapped: coarse = colour, fine = high, third = low (the LOW decoder's backward scatters in-kernel)
  one_lattice        fine == coarse: three jobs on one key order, one fine-cell offset per coarse cell
  incommensurate     non-integer cell ratios (11/4, 13/4 ...): the f0 rounding and the 0..3 clamp of bin_keys_block
  ratio_12           10-13 fine cells per coarse cell: the offset saturates, many fine cells share a key, fine runs interleave
  unit_axis_coarse   coarse Z < 2: no plan, every scatter in-kernel; tri_axis* with size 1, forward and d/d position
  unit_axis_fine     the plan holds; dims_f - 1 == 0 in the key arithmetic
  axis_257           coarse = low with a 257-cell axis: 9 bits > ADFP_BIN_MAXBITS, no plan
  axis_1024          (refusal only) a plan, colour is the fine grid with an axis above 1023: scatter_bins refuses it
  distinct_axes      three lattices again, Z != Y != X in every grid: every case above with a plan has Y == X, where an exchanged pair of
                     dims in a sorted-scatter job or a deferred position-gradient job would not show"""
import copy

import torch

GRIDS = ('grid_low', 'grid_high', 'grid_color')
STAGE_GRIDS = {'low': GRIDS[:1], 'high': GRIDS[:2], 'color': GRIDS}

# name: (low, high, colour), each (Z, Y, X)
SHAPES = {
    'three_lattices': ((3, 4, 4), (7, 9, 9), (15, 19, 19)),
    'colour_coarsest': ((7, 9, 9), (15, 19, 19), (3, 4, 4)),
    'one_lattice': ((7, 9, 9), (7, 9, 9), (7, 9, 9)),
    'incommensurate': ((4, 5, 5), (9, 12, 12), (11, 14, 14)),
    'ratio_12': ((3, 4, 4), (7, 9, 9), (31, 39, 39)),
    'unit_axis_coarse': ((1, 4, 4), (2, 9, 9), (2, 9, 9)),
    'unit_axis_fine': ((3, 4, 4), (1, 12, 12), (1, 12, 12)),
    'axis_257': ((2, 2, 257), (2, 3, 300), (2, 3, 300)),
    'axis_1024': ((3, 4, 4), (7, 9, 9), (2, 2, 1024)),
    'distinct_axes': ((3, 4, 5), (6, 8, 11), (13, 17, 23)),
}
REFUSED = ('axis_1024',)
RUNNABLE = tuple(k for k in SHAPES if k not in REFUSED)
UNIT_AXIS = {'unit_axis_coarse': ('grid_low',), 'unit_axis_fine': ('grid_high', 'grid_color')}      # the grids with Z == 1
SEEDS = {name: 1000 + k for k, name in enumerate(SHAPES)}

N_RAYS, NS, NF = 33, 8, 5                   # the forward and backward matrices' 429 points
C_DIM = 32
STD = {'grid_low': 0.01 * 30.0, 'grid_high': 0.0001 * 30.0 * 100.0, 'grid_color': 0.01 * 30.0}


def shapes(name):
    return dict(zip(GRIDS, SHAPES[name]))


def make_grids(name):
    g = torch.Generator().manual_seed(SEEDS[name])
    return {key: torch.randn((1, C_DIM) + tuple(zyx), generator=g) * STD[key] for key, zyx in shapes(name).items()}


def scene(mini, name):
    """The mini scene with the case's grids: every attribute of the fixture, `.c` swapped (the fixture itself is left alone)."""
    sc = copy.copy(mini)
    sc.c = make_grids(name)
    return sc


def rays(mini):
    return tuple(t[:N_RAYS].contiguous() for t in (mini.rays_o, mini.rays_d, mini.gt_depth, mini.gt_color))


# ------------------------------------------------------------------- the kernels' selection rule, restated
BIN_MAXBITS = 8            # ADFP_BIN_MAXBITS (csrc/adfp_backward_h.h)
PACKED_AXIS_MAX = 1023     # scatter_bins: x0 | y0 << 10 | z0 << 20


def scatter_plan(case_shapes, stage='color', in_kernel_option=False):
    """plan_sorted_scatter over the grids of `stage` that want a gradient on the f16-split backward: (fine, coarse) as (Z, Y, X), or
    None (no plan: every grid scatters in-kernel).  Ties go to the first candidate, as the strict comparisons there do."""
    cand = [tuple(case_shapes[k]) for k in STAGE_GRIDS[stage]]
    vox = lambda s: s[0] * s[1] * s[2]                                     # noqa: E731
    fine = coarse = None
    for s in cand:
        if fine is None or vox(s) > vox(fine):
            fine = s
        if coarse is None or vox(s) < vox(coarse):
            coarse = s
    if fine is None or in_kernel_option or min(coarse) < 2:
        return None
    bits = 0
    while (1 << bits) < max(coarse):
        bits += 1
    if bits > BIN_MAXBITS:
        return None
    return fine, coarse


def scatter_branch(case_shapes, key, stage='color', in_kernel_option=False):
    """run_decode_bwd_h + scatter_bins for one grid: 'sorted' (a job of the call's k_scatter_sorted), 'in_kernel', or 'refused'."""
    plan = scatter_plan(case_shapes, stage, in_kernel_option)
    if plan is None or tuple(case_shapes[key]) not in plan:
        return 'in_kernel'
    return 'refused' if max(case_shapes[key]) > PACKED_AXIS_MAX else 'sorted'


def fine_offsets(case_shapes, pn, stage='color'):
    """bin_keys_block's per-axis fine-cell offset (before and after the 0..3 clamp) of normalised coordinates pn [P, 3] (x, y, z) in f32
    arithmetic: -> (raw [P, 3], clamped [P, 3]) int64."""
    fine, coarse = scatter_plan(case_shapes, stage)
    raw = []
    for k in range(3):
        nf, nc = fine[2 - k], coarse[2 - k]                                # axis k = x, y, z; shapes are (Z, Y, X)

        def cell(size):
            c = ((pn[:, k].float() + 1.0) / 2.0) * float(size - 1)
            return torch.floor(c.clamp(0.0, float(size - 1))).long()
        cc, fc = cell(nc), cell(nf)
        ratio = torch.tensor(float(nf - 1), dtype=torch.float32) / torch.tensor(float(nc - 1), dtype=torch.float32)
        f0 = torch.floor(cc.float() * ratio - 1e-3).long().clamp_min(0)
        raw.append(fc - f0)
    raw = torch.stack(raw, 1)
    return raw, raw.clamp(0, 3)
