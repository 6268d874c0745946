"""CPU: the float64 statements of tests/mapper_glue_ref.py against what they restate -- the reference's own pre-filter
vectors (tests/golden/mapper_prefilter.npz), torch autograd of oracle.mapper_loss on the compacted batch, and
torch.optim.Adam's bias corrections -- so that tests/test_gpu_mapper_glue.py does not judge the kernels by an unpinned
reference; and two negative controls of that file's loss criteria."""
import math
import os

import numpy as np
import pytest
import torch

import mapper_glue_ref as R
from oracle import adfp_oracle as O
from conftest import GOLDEN


def test_prefilter_statement_reproduces_the_reference_lines():
    g = np.load(os.path.join(GOLDEN, 'mapper_prefilter.npz'))
    names = sorted({k.split('.')[0] for k in g.files if '.' in k})
    assert len(names) == 6
    some_kept = False
    for n in names:
        keep, dmax = R.prefilter(g[f'{n}.rays_o'], g[f'{n}.rays_d'], g[f'{n}.gt_depth'], g[f'{n}.bound'])
        assert np.array_equal(keep, g[f'{n}.inside_mask']), n
        kept = g[f'{n}.kept_gt_depth']
        assert dmax.dtype == np.float32
        assert dmax == (kept.max() if kept.size else -np.inf), n
        some_kept |= kept.size > 0
    assert some_kept


def test_prefilter_statement_with_nothing_kept():
    sc_bound = np.array([[-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0]])
    ro, rd = np.zeros((5, 3), np.float32), np.ones((5, 3), np.float32)
    keep, dmax = R.prefilter(ro, rd, np.full(5, 10.0, np.float32), sc_bound)
    assert not keep.any() and dmax == -np.inf and dmax.dtype == np.float32


def autograd_on_the_compacted_batch(b, stage, warm, w_color):
    """oracle.mapper_loss on x[keep] with float64 leaves; the gradients scattered back into all-zero [N, ...] arrays."""
    N, S = b['weight'].shape
    kept = np.ones(N, dtype=bool) if b['keep'] is None else b['keep'].astype(bool)
    k = torch.from_numpy(kept)
    depth = torch.from_numpy(b['depth'])[k].clone().requires_grad_(True)
    color = torch.from_numpy(b['color'])[k].double().requires_grad_(True)
    weight = torch.from_numpy(b['weight'])[k].double().requires_grad_(True)
    gd, gc = torch.from_numpy(b['gd'])[k], torch.from_numpy(b['gc'])[k]
    loss = O.mapper_loss(depth, color, weight, gd, gc, stage, warm, w_color_loss=float(np.float32(w_color)))
    g_depth, g_color, g_weight = np.zeros(N), np.zeros((N, 3), np.float32), np.zeros((N, S), np.float32)
    if loss.requires_grad:
        loss.backward()
        for leaf, out in ((depth, g_depth), (color, g_color), (weight, g_weight)):
            if leaf.grad is not None:
                out[kept] = leaf.grad.numpy().astype(out.dtype)
    return float(loss.detach()), g_depth, g_color, g_weight


@pytest.mark.parametrize('warm', [False, True])
@pytest.mark.parametrize('stage', R.STAGES)
@pytest.mark.parametrize('N,S,keep_mode', [(300, 7, 'mixed'), (65, 48, 'null'), (40, 3, 'zero')])
def test_loss_statement_equals_autograd_of_the_oracle_on_the_compacted_batch(N, S, keep_mode, stage, warm):
    """Cotangents: bit for bit after the scatter (float64 -> float32 of a sign times float(f32(w)) is exact), the sign of a
    zero included: torch leaves -0.0 at a colour tie (-w * sign(0)), +0.0 at a depth tie (the same -0.0 accumulated into the
    zeros of the boolean index's backward) and +0.0 at a weight tie.  Loss: 1e-12 relative (two float64 summation orders)."""
    b = R.make_loss_batch(N, S, keep_mode)
    ref = autograd_on_the_compacted_batch(b, stage, warm, 0.2)
    got = R.loss_and_cotangents(b['depth'], b['color'], b['weight'], b['gd'], b['gc'], b['keep'], stage, warm, 0.2)
    assert abs(got[0] - ref[0]) <= 1e-12 * abs(ref[0]) and math.isfinite(got[0])
    for name, a, r in zip(('g_depth', 'g_color', 'g_weight'), got[1:], ref[1:]):
        assert a.dtype == r.dtype and a.shape == r.shape, name
        R.assert_bits_equal(a, r, name)
    kept = np.ones(N, dtype=bool) if b['keep'] is None else b['keep'].astype(bool)
    if keep_mode != 'zero':
        # the batch exercises what it is meant to: ties of all three kinds on kept rays, zero depths, and every sign
        assert ((b['gd'] > 0) & kept & (b['gd'].astype(np.float64) == b['depth'])).any()
        assert (kept[:, None] & (b['gc'] == b['color'])).any() and (kept[:, None] & (b['weight'] == 1)).any()
        assert ((b['gd'] == 0) & kept).any()
        assert set(np.unique(got[1])) == {-1.0, 0.0, 1.0}
        if warm:
            assert set(np.unique(got[3])) == {-1.0, 0.0, 1.0}
        if stage == 'color':
            w = np.float32(0.2)
            assert set(np.unique(got[2])) == {-w, np.float32(0), w}
    else:
        assert got[0] == 0.0 and not got[1].any() and not got[2].any() and not got[3].any()
    if not warm:
        assert not got[3].any()
    if stage != 'color':
        assert not got[2].any()
    assert not got[1][~kept].any() and not got[2][~kept].any() and not got[3][~kept].any()


def test_a_wrong_colour_weight_fails_the_gpu_criteria():
    """Negative control: w_color 0.2 -> 0.25 in the statement.  The loss criterion and the cotangent criterion of
    tests/test_gpu_mapper_glue.py must each fail on their own (Adam's normalisation hides such a factor from a trajectory)."""
    b = R.make_loss_batch(5000, 48, 'mixed')
    args = (b['depth'], b['color'], b['weight'], b['gd'], b['gc'], b['keep'], 'color', True)
    good, wrong = R.loss_and_cotangents(*args, 0.2), R.loss_and_cotangents(*args, 0.25)
    R.assert_loss_close(good[0], good[0])
    R.assert_cotangents_equal(good[1:], good[1:])
    with pytest.raises(AssertionError):
        R.assert_loss_close(wrong[0], good[0], 'w_color 0.25')
    with pytest.raises(AssertionError):
        R.assert_cotangents_equal(wrong[1:], good[1:], 'w_color 0.25')
    R.assert_bits_equal(wrong[1], good[1], 'g_depth')                       # the depth and weight terms are not touched by it
    R.assert_bits_equal(wrong[3], good[3], 'g_weight')


@pytest.mark.parametrize('stage,warm', [('low', False), ('color', True)])
def test_one_leaked_dropped_ray_fails_the_gpu_criteria(stage, warm):
    """Negative control: keep ignored for ONE dropped ray of 5 000 (a finite one; a NaN ray would be louder).  Both criteria
    must fail on their own."""
    b = R.make_loss_batch(5000, 48, 'mixed')
    dropped = np.nonzero((b['keep'] == 0) & (b['gd'] > 0) & np.isfinite(b['depth']) & np.isfinite(b['color']).all(1)
                         & np.isfinite(b['weight']).all(1) & (b['gd'].astype(np.float64) != b['depth']))[0]
    assert dropped.size
    leaky = b['keep'].copy()
    leaky[dropped[0]] = 1
    args = (b['depth'], b['color'], b['weight'], b['gd'], b['gc'])
    good, wrong = R.loss_and_cotangents(*args, b['keep'], stage, warm, 0.2), R.loss_and_cotangents(*args, leaky, stage, warm, 0.2)
    with pytest.raises(AssertionError):
        R.assert_loss_close(wrong[0], good[0], 'one leaked ray')
    with pytest.raises(AssertionError):
        R.assert_cotangents_equal(wrong[1:], good[1:], 'one leaked ray')


def test_adam_statement_is_torch_adams_bias_correction():
    """adam_derived against the scalars torch.optim.Adam computes (step_size = lr / (1 - beta1^t), bias_correction2_sqrt =
    sqrt(1 - beta2^t), python floats) once its betas are the floats the C ABI passes; and its three branches."""
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    steps = np.array([0, 1, 9, 999, 99999, 5, 6], np.int32)
    lrs = [0.1, 0.005, 0.0, 0.1, 0.005, -1.0, 0.0]
    before = np.arange(14, dtype=np.float32).reshape(7, 2) + 100
    s2, d = R.adam_derived(steps, lrs, 0.9, 0.999, 0, before)
    assert s2.tolist() == [1, 2, 10, 1000, 100000, 5, 7] and steps[0] == 0          # the caller's array is not modified
    for g in (0, 1, 2, 3, 4, 6):
        t = int(s2[g])
        lr = float(np.float32(lrs[g]))
        assert d[g, 0] == np.float32(lr / (1 - b1 ** t)) and d[g, 1] == np.float32(math.sqrt(1 - b2 ** t))
    assert d[2, 0] == 0 and d[2, 1] > 0                                              # lr == 0 steps: its moments advance
    assert d[4, 0] == np.float32(0.005) and d[4, 1] == 1.0                           # far from step 1 the corrections are gone
    assert np.array_equal(d[5], before[5])                                           # lr < 0: untouched
    s3, d3 = R.adam_derived(steps, lrs, 0.9, 0.999, 1, before)
    assert np.array_equal(s3, steps) and not d3.any()                                # skip: nobody steps, derived zeroed
    # stated on python's 0.9 / 0.999 instead, sqrt(1 - beta2) at t = 1 differs by 6.4e-6 relative: that is NOT the statement
    assert abs(float(d[0, 1]) / math.sqrt(1 - 0.999) - 1) > 1e-6
    # the first torch.optim.Adam step with those betas moves a parameter by the statement's step_size / (|g| / sqrt_bc2 + eps) * m
    p = torch.nn.Parameter(torch.tensor([1.0], dtype=torch.float64))
    lr = float(np.float32(0.1))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=1e-8)
    p.grad = torch.tensor([0.5], dtype=torch.float64)
    opt.step()
    m, v = (1 - b1) * 0.5, (1 - b2) * 0.25
    want = 1.0 - (lr / (1 - b1)) * m / (math.sqrt(v) / math.sqrt(1 - b2) + 1e-8)
    assert abs(float(p.detach()) - want) <= 1e-12
