"""Plain float64 statements of the Mapper iteration's glue kernels (csrc/adfp_mapper_iter.h): the bounding-box pre-filter as
keep flags + the far clamp, the Mapper loss with its three cotangents, and torch.optim.Adam's step counters / bias
corrections -- numpy on the CPU, no project code.  tests/test_mapper_glue_host.py pins these statements against the
reference's own vectors and torch autograd; tests/test_gpu_mapper_glue.py holds the HIP kernels to them.

Also here, because both test files need them: the seeded loss batch with its planted ties and poisoned dropped rays
(make_loss_batch) and the comparison criteria themselves (assert_cotangents_equal, assert_loss_close, assert_within_one_ulp)."""
import math

import numpy as np
import torch

from oracle import adfp_oracle as O

STAGES = ('low', 'high', 'color')


def _np(x, dtype=None):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a if dtype is None else a.astype(dtype, copy=False)


# ----------------------------------------------------------------------------------------------------------- pre-filter
def prefilter(ro, rd, gd, bound):
    """src/Mapper.py:438-449 as a keep flag: (keep bool [N] = oracle.prefilter_mask, dmax float32 = gd[keep].max(), -inf when
    nothing is kept).  A max of float32 values has no rounding."""
    t = lambda x, dt: torch.as_tensor(_np(x)).to(dt)                                   # noqa: E731
    gd32 = t(gd, torch.float32)
    keep = O.prefilter_mask(t(ro, torch.float32), t(rd, torch.float32), gd32, t(bound, torch.float64)).numpy().astype(bool)
    kept = gd32.numpy()[keep]
    return keep, np.float32(kept.max()) if kept.size else np.float32(-np.inf)


# ----------------------------------------------------------------------------------------------------------------- loss
def loss_and_cotangents(depth64, color, weight, gd, gc, keep, stage, warmup, w_color):
    """src/Mapper.py:457-469 restricted to the rays with keep != 0 (keep None: every ray):
        sum_{gd > 0} |gd - depth|  [+ sum |weight - 1| with warm-up]  [+ w_color * sum |gc - color| in stage color]
    in float64, w_color as the C ABI receives it (a float).  Returns (loss f64, g_depth f64 [N], g_color f32 [N,3],
    g_weight f32 [N,S]) with torch.abs's backward (the sign, 0 at 0) in torch's own bits: at a colour tie
    d w|gt - c|/dc = -w sign(0) is -0.0; at a depth tie the same -0.0 is ADDED into the zeros that the backward of the
    boolean index [depth_mask] starts from, which leaves +0.0; at a weight tie sign(w - 1) is +0.0.  Rows of dropped rays, rays
    without a sensor depth, and the cotangents of a term that does not exist in this stage / without warm-up are +0.0.  A
    dropped ray may hold NaN or inf anywhere: it is never read."""
    assert stage in STAGES
    depth64, gd = _np(depth64, np.float64), _np(gd, np.float32)
    color, gc, weight = _np(color, np.float32), _np(gc, np.float32), _np(weight, np.float32)
    N, S = weight.shape
    kept = np.ones(N, dtype=bool) if keep is None else _np(keep).astype(bool)
    w = float(np.float32(w_color))
    g_depth, g_color, g_weight = np.zeros(N, np.float64), np.zeros((N, 3), np.float32), np.zeros((N, S), np.float32)
    sign = lambda d: np.where(d > 0, 1.0, np.where(d < 0, -1.0, 0.0))                  # noqa: E731
    with np.errstate(invalid='ignore'):
        m = kept & (gd > 0)                                                            # depth_mask, on the kept rays
    diff = gd[m].astype(np.float64) - depth64[m]
    loss = float(np.abs(diff).sum())
    g_depth[m] = 0.0 + -sign(diff)                                                     # the index backward's accumulation
    if warmup:
        diff = weight[kept].astype(np.float64) - 1.0
        loss += float(np.abs(diff).sum())
        g_weight[kept] = sign(diff).astype(np.float32)
    if stage == 'color':
        diff = gc[kept].astype(np.float64) - color[kept].astype(np.float64)
        loss += w * float(np.abs(diff).sum())
        g_color[kept] = (-w * sign(diff)).astype(np.float32)
    return loss, g_depth, g_color, g_weight


# ----------------------------------------------------------------------------------------------------------------- Adam
def adam_derived(steps, lrs, beta1, beta2, skip, derived=None):
    """torch.optim.Adam's per-group step counter and bias corrections (adfp_adam_prep): for lr >= 0
        t = step + 1,   derived = (f32(lr / (1 - beta1^t)), f32(sqrt(1 - beta2^t)))
    in python floats on the float values the C ABI receives (float beta1, beta2, lr[]).  lr < 0: the entry is unchanged;
    skip: the steps are unchanged and derived is zero.  `derived`: what the entries held before (default NaN), returned for
    the groups that do not step.  Returns (steps' int32 [n], derived f32 [n,2])."""
    steps = np.array(_np(steps), dtype=np.int32)
    n = steps.shape[0]
    out = np.full((n, 2), np.nan, np.float32) if derived is None else np.array(_np(derived), dtype=np.float32).reshape(n, 2)
    if skip:
        return steps, np.zeros((n, 2), np.float32)
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    for g in range(n):
        lr = float(np.float32(lrs[g]))
        if lr < 0:
            continue
        t = int(steps[g]) + 1
        steps[g] = t
        out[g, 0] = np.float32(lr / (1.0 - b1 ** t))
        out[g, 1] = np.float32(math.sqrt(1.0 - b2 ** t))
    return steps, out


# ------------------------------------------------------------------------------------------------- the seeded loss batch
def make_loss_batch(N, S, keep_mode, seed=0):
    """Renderer outputs and sensor values of N rays as the loss kernel receives them: random f64 depth, f32 colour and weight,
    15 % zero gt_depth, planted ties of all three kinds (depth == gt_depth, colour == gt_colour, weight == 1) and, with
    keep_mode 'mixed' (~20 % dropped) or 'zero' (all dropped), dropped rays that carry NaN and +-inf in depth, colour, weight
    and gt_depth -- a NaN direction is what the pre-filter drops, and the ray is rendered anyway.  keep_mode 'null': keep is None."""
    assert keep_mode in ('null', 'mixed', 'zero')
    r = np.random.default_rng(1000 + 7 * N + S + seed)
    depth = r.uniform(0.2, 4.0, N)
    gd = (depth + r.normal(0.0, 0.1, N)).astype(np.float32)
    gd[r.random(N) < 0.15] = 0.0
    color, gc = r.random((N, 3), dtype=np.float32), r.random((N, 3), dtype=np.float32)
    weight = (r.random((N, S), dtype=np.float32) * np.float32(1.5)).astype(np.float32)
    tie = np.arange(N) % 7 == 3
    depth[tie] = gd[tie].astype(np.float64)                                            # gt_depth - depth == 0
    tie = np.arange(N) % 5 == 0
    color[tie, np.arange(N)[tie] % 3] = gc[tie, np.arange(N)[tie] % 3]                 # gt_color - color == 0
    weight[r.random((N, S)) < 0.1] = 1.0                                               # weight - 1 == 0
    if keep_mode == 'null':
        keep = None
    else:
        keep = (r.random(N) >= 0.2).astype(np.uint8) if keep_mode == 'mixed' else np.zeros(N, np.uint8)
        poison = np.array([np.nan, np.inf, -np.inf])
        for j, i in enumerate(np.nonzero(keep == 0)[0]):
            what = j % 4                                                               # the fourth dropped ray stays finite: a leak of it is small
            if what == 0:
                depth[i] = poison[j // 4 % 3]
                gd[i] = np.float32(np.nan) if j % 8 == 0 else gd[i]
            elif what == 1:
                color[i, j % 3] = np.float32(poison[j // 4 % 3])
            elif what == 2:
                weight[i, j % S] = np.float32(poison[j // 4 % 3])
    return dict(depth=depth, color=color, weight=weight, gd=gd, gc=gc, keep=keep)


# ------------------------------------------------------------------------------------------------------------- criteria
def bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def assert_bits_equal(got, ref, what):
    got, ref = _np(got), _np(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, f'{what}: {got.dtype}{got.shape} vs {ref.dtype}{ref.shape}'
    bad = bits(got) != bits(ref)
    assert not bad.any(), f'{what}: {int(bad.sum())}/{bad.size} elements differ in their bits, first at {np.argwhere(bad)[0].tolist()}'


def assert_cotangents_equal(got, ref, what=''):
    """(g_depth, g_color, g_weight) against the statement's, bit for bit: they are signs times exact constants."""
    for name, a, b in zip(('g_depth', 'g_color', 'g_weight'), got, ref):
        assert_bits_equal(a, b, f'{what} {name}')


LOSS_RTOL = 3.0 * 2.0 ** -24


def assert_loss_close(got, ref, what=''):
    """|loss - ref| <= 3 * 2^-24 * ref, exactly 0 when ref == 0.  Derived: every term is non-negative, and carries at most two
    float32 roundings (the difference, the product with w_color: (1 + 2^-24)^2 - 1 < 3 * 2^-24) before its float64 sum, whose
    own error (N (S + 4) 2^-53 at most) is five orders of magnitude below that at every shape in use."""
    got, ref = float(got), float(ref)
    assert ref >= 0.0 and math.isfinite(ref)
    if ref == 0.0:
        assert got == 0.0, f'{what}: loss {got!r}, statement exactly 0'
    else:
        assert abs(got - ref) <= LOSS_RTOL * ref, f'{what}: loss {got!r} vs {ref!r}: {abs(got - ref) / ref:.3e} relative > {LOSS_RTOL:.3e}'


def assert_within_one_ulp(got, ref, what):
    """float32 arrays: |got - ref| <= the spacing of float32 at ref.  Returns how many elements are not bit-equal."""
    got, ref = _np(got), _np(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = ~(err <= np.spacing(np.abs(ref)).astype(np.float64))
    assert not bad.any(), f'{what}: {got[bad]} vs {ref[bad]}: more than one float32 ulp'
    return int((bits(got) != bits(ref)).sum())
