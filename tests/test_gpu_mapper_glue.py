"""GPU: the kernels between render_forward and render_backward of mapping.MapperIteration and after its backward
(csrc/adfp_mapper_iter.h, csrc/adfp_mapping.h) -- adfp_prefilter_mask, adfp_mapper_loss, adfp_mapper_loss_step, adfp_adam_prep,
adfp_masked_adam_dev, adfp_masked_adam_multi, adfp_adam_step -- called raw through ctypes and held element by element to the
float64 statements of tests/mapper_glue_ref.py (pinned on the CPU by tests/test_mapper_glue_host.py), to torch.optim.Adam, and,
for the fused path's gradients, to the oracle's autograd along the kernels' own ReLU decisions.

Every output buffer carries 64 elements of tail and is pre-filled, tail included, with a sentinel (NaN; 7 for bytes; -77 for
ints): every payload element must have been written, no tail element may have been.

No tolerance here comes from the code under test: cotangents, keep flags, the far clamp and step counters are exact; the loss
bound is derived (mapper_glue_ref.assert_loss_close); 2e-6 with its 1e-3 floor, TIGHT_GRAD_TOL and 1e-5 on the loss are the
project's own.

Two memory-safe mutations of k_mapper_loss, each built from a patched copy of csrc/ into a library of its own and selected
with ADFP_LIB_PATH, this file and tests/test_gpu_mapper_iteration.py run once per build on an MI355X:
  (a) the last workgroup adds up only the partial sums b < 64.  Here: 2 of 54 fail, the two 65-workgroup colour cases of
      test_mapper_loss_entries_against_the_statement, on adfp_mapper_loss_step's loss: [16385-48-color-False-null] 1.2e-4
      relative, [16385-65-color-True-mixed] 1.5e-2, against the bound of 1.8e-7.  (16385 x 1, keep all zero, has an exactly zero
      loss either way.)  test_gpu_mapper_iteration.py: 6 passed -- it has 3 workgroups and does not notice.
  (b) the colour cotangent ignores `kept`.  Here: 5 of 54 fail, every colour case with dropped rays ([255-48-color-False-mixed],
      [256-65-color-True-mixed], [257-48-color-True-zero], [5000-48-color-True-mixed], [16385-65-color-True-mixed]), on g_color
      bit for bit: the dropped rays' rows are +-w_color or NaN instead of +0.0.  test_gpu_mapper_iteration.py: 6 passed -- the
      backward masks the dropped rays once more with ray_keep, so the fused path (and test_fused_gradient_against_the_oracle
      here) is not affected by a leak in this one cotangent; the raw entry is.
With the unmodified kernels all 54 pass, in both ADFP_MATH modes: no test here exposed a defect.
(Since then: three LOSS_CASES with rows of 129 and 256 samples, and a 129-sample case of test_fused_gradient_against_the_oracle,
which now runs on an engine whose backward scratch holds an earlier iteration's cotangents -- HISTORY.md, sample-count range log.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import mapper_glue_ref as R
from attentive_dfprior_amd import _lib, mapping, synthetic
from attentive_dfprior_amd._lib import lib, ptr, check
from oracle import adfp_oracle as O
from conftest import GOLDEN, ReluCapture, assert_grad_tight, assert_forced_decisions_are_boundary_units

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TAIL = 64
SENTINEL = {torch.float32: float('nan'), torch.float64: float('nan'), torch.uint8: 7, torch.int32: -77}
B1, B2, EPS = 0.9, 0.999, 1e-8


def stream():
    return _lib.current_stream(DEV)


class Guarded(object):
    """A device buffer of `shape` followed by TAIL elements, all of it pre-filled with the dtype's sentinel."""

    def __init__(self, shape, dtype, init=None):
        self.shape, self.n, self.dtype = tuple(shape), int(np.prod(shape)), dtype
        self.buf = torch.empty(self.n + TAIL, dtype=dtype, device=DEV)
        self.reset(init)

    def reset(self, init=None):
        self.buf.fill_(SENTINEL[self.dtype])
        if init is not None:
            self.buf[:self.n].copy_(torch.as_tensor(init).reshape(-1))

    @property
    def data(self):
        return self.buf[:self.n].view(self.shape)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def addr(self):
        return self.buf.data_ptr()

    def is_sentinel(self, t):
        return torch.isnan(t) if self.dtype.is_floating_point else t == SENTINEL[self.dtype]

    def check(self, what, written=True):
        """The tail is untouched; with `written`, no payload element still holds the sentinel.  Returns the payload on the CPU."""
        assert bool(self.is_sentinel(self.buf[self.n:]).all()), f'{what}: something wrote behind the buffer'
        if written:
            left = int(self.is_sentinel(self.buf[:self.n]).sum())
            assert left == 0, f'{what}: {left}/{self.n} elements were never written'
        return self.data.cpu().numpy()


# ================================================================================================== adfp_prefilter_mask
def run_prefilter(ro, rd, gd, bound):
    N = ro.shape[0]
    t = lambda x, dt: torch.as_tensor(np.asarray(x)).to(DEV, dt).contiguous()           # noqa: E731
    ro_d, rd_d, gd_d, b_d = t(ro, torch.float32), t(rd, torch.float32), t(gd, torch.float32), t(bound, torch.float64)
    keep, dmax = Guarded((N,), torch.uint8), Guarded((1,), torch.float32)
    check(lib().adfp_prefilter_mask(ptr(ro_d), ptr(rd_d), ptr(gd_d), N, ptr(b_d), keep.ptr, dmax.ptr, stream()), 'adfp_prefilter_mask')
    # the compacting entry on the same batch: its ordered index list is nonzero(keep), its count the number of kept rays
    index, count = Guarded((N,), torch.int32), Guarded((1,), torch.int32)
    check(lib().adfp_prefilter_rays(ptr(ro_d), ptr(rd_d), ptr(gd_d), N, ptr(b_d), index.ptr, count.ptr, stream()), 'adfp_prefilter_rays')
    torch.cuda.synchronize()
    k = keep.check('keep')
    assert k.max() <= 1
    kept = np.nonzero(k)[0]
    assert int(count.check('count')[0]) == kept.size
    got = index.check('index', written=False)
    assert np.array_equal(got[:kept.size], kept), 'adfp_prefilter_rays and adfp_prefilter_mask keep different rays'
    assert (got[kept.size:] == SENTINEL[torch.int32]).all(), 'adfp_prefilter_rays wrote behind its count'
    return k.astype(bool), dmax.check('depth_max')[0]


def assert_prefilter(ro, rd, gd, bound, what):
    keep, dmax = run_prefilter(ro, rd, gd, bound)
    k_ref, d_ref = R.prefilter(ro, rd, gd, bound)
    assert np.array_equal(keep, k_ref), f'{what}: keep differs at {np.nonzero(keep != k_ref)[0][:8].tolist()}'
    assert dmax.dtype == np.float32 and dmax == d_ref, f'{what}: depth_max {dmax!r} vs {d_ref!r}'     # a max has no rounding
    return k_ref, d_ref


def test_prefilter_mask_reproduces_the_reference_lines():
    """The six cases of tests/golden/mapper_prefilter.npz (what src/Mapper.py:438-449 itself computed): keep bit for bit,
    depth_max == max(kept_gt_depth) exactly."""
    g = np.load(os.path.join(GOLDEN, 'mapper_prefilter.npz'))
    names = sorted({k.split('.')[0] for k in g.files if '.' in k})
    assert len(names) == 6
    for n in names:
        keep, dmax = run_prefilter(g[f'{n}.rays_o'], g[f'{n}.rays_d'], g[f'{n}.gt_depth'], g[f'{n}.bound'])
        assert np.array_equal(keep, g[f'{n}.inside_mask']), n
        kept = g[f'{n}.kept_gt_depth']
        assert dmax == (kept.max() if kept.size else -np.inf), n


def mini_rays(n, planted=True):
    scene = synthetic.mini_scene()
    ro, rd, depth, _ = synthetic.make_ray_batch(scene, n, seed=11 + n, zero_frac=0.2)
    depth = depth * (0.5 + 1.5 * torch.rand(depth.shape, generator=torch.Generator().manual_seed(n)))      # some beyond the box: dropped
    depth[n - 1] = 0.4 * depth[n - 1]                          # (the last ray of the stride loop, the only one of n = 1: a kept one)
    bound = scene.bound.float().double()                       # float32-representable planes: an origin can lie ON one
    if planted and n >= 63:                                    # what test_prefilter_rays_vs_oracle plants ...
        rd[3, 0] = 0.0                                         # one zero direction component: +-inf on one axis
        rd[5] = 0.0                                            # all three zero
        depth[3] = depth[5] = 0.05                             # (close enough for the other axes to keep them)
        ro[7, 1] = float(bound[1, 0]); rd[7, 1] = 0.0          # 0/0 on a bound plane
        t = (bound.unsqueeze(0) - ro[9:10].unsqueeze(-1)) / rd[9:10].unsqueeze(-1)
        depth[9] = torch.min(torch.max(t, dim=2)[0], dim=1)[0].float()                 # t == depth after rounding (or just not)
        rd[11, 2] = float('nan')                               # ... and a NaN direction, a NaN depth
        depth[13] = float('nan')
    return bound, ro, rd, depth


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1024, 1025, 5000, 20001])
def test_prefilter_mask_vs_oracle(n):
    """One workgroup of 1 024 threads with a stride loop and a 16-wave max reduction: below one wave, below / at / above one
    workgroup, many strides; degenerate rays planted."""
    bound, ro, rd, depth = mini_rays(n)
    keep, dmax = assert_prefilter(ro, rd, depth, bound, f'{n} rays')
    assert keep[n - 1] and np.isfinite(dmax)
    if n >= 63:
        assert keep[3] and keep[5]                             # +-inf in the slab test: kept
        assert not keep[7] and not keep[11] and not keep[13]   # NaN compares false: dropped
        assert keep.sum() < n
        # the maximum is taken over the KEPT rays only: a larger depth sits on a dropped one
        assert np.nanmax(np.where(keep, -np.inf, depth.numpy())) > dmax


@pytest.mark.parametrize('n', [1, 65, 1025])
def test_prefilter_mask_with_every_ray_dropped(n):
    bound, ro, rd, depth = mini_rays(n, planted=False)
    keep, dmax = assert_prefilter(ro, rd, torch.full_like(depth, 1e6), bound, f'{n} rays, all dropped')
    assert not keep.any() and dmax == -np.inf


# ===================================================================================== adfp_mapper_loss, adfp_mapper_loss_step
LOSS_CASES = [  # N, S, stage, warm-up, keep: every N and S of interest, every stage x warm-up, every kind of keep; 16385 rays = 65 workgroups
    (1, 1, 'low', False, 'null'),
    (63, 48, 'low', True, 'mixed'),
    (64, 65, 'high', False, 'mixed'),
    (65, 1, 'high', True, 'null'),
    (255, 48, 'color', False, 'mixed'),
    (256, 65, 'color', True, 'mixed'),
    (257, 48, 'color', True, 'zero'),
    (5000, 48, 'color', True, 'mixed'),
    (5000, 65, 'low', True, 'null'),
    (16385, 1, 'high', False, 'zero'),
    (16385, 48, 'color', False, 'null'),
    (16385, 65, 'color', True, 'mixed'),
    (64, 129, 'color', True, 'mixed'),           # rows of three and four 64-sample passes, the last one ragged (129) or full (256 = the maximum)
    (65, 256, 'color', True, 'mixed'),
    (5000, 256, 'high', False, 'zero'),
]
PREP_STEPS = [0, 1, 9, 999, 99999]
PREP_LRS = [0.1, 0.005, 0.0, -1.0]


class LossCall(object):
    def __init__(self, b, N, S, stage, warm, w_color=0.2):
        dev = lambda x, dt: None if x is None else torch.as_tensor(x).to(DEV, dt).contiguous()      # noqa: E731
        self.inputs = [dev(b['depth'], torch.float64), dev(b['color'], torch.float32), dev(b['weight'], torch.float32),
                       dev(b['gd'], torch.float32), dev(b['gc'], torch.float32), dev(b['keep'], torch.uint8)]
        self.N, self.S = N, S
        self.loss = Guarded((1,), torch.float64)
        self.g_depth, self.g_color, self.g_weight = Guarded((N,), torch.float64), Guarded((N, 3), torch.float32), Guarded((N, S), torch.float32)
        la = self.la = _lib.AdfpLossArgs()
        la.n_rays, la.S, la.stage, la.warmup, la.w_color_loss = N, S, _lib.STAGE[stage], 1 if warm else 0, w_color
        d, c, w, gd, gc, keep = self.inputs
        la.depth, la.color, la.weight, la.gt_depth, la.gt_color = d.data_ptr(), c.data_ptr(), w.data_ptr(), gd.data_ptr(), gc.data_ptr()
        la.keep = keep.data_ptr() if keep is not None else None
        # the colour and weight buffers are passed in every stage: without their term they must come back all zero
        la.loss, la.g_depth, la.g_color, la.g_weight = self.loss.addr(), self.g_depth.addr(), self.g_color.addr(), self.g_weight.addr()

    def prepare(self, loss_init):
        for g in (self.g_depth, self.g_color, self.g_weight):
            g.reset()
        self.loss.reset(torch.tensor([loss_init], dtype=torch.float64))

    def results(self, what):
        torch.cuda.synchronize()
        return (float(self.loss.check(what + ' loss')[0]), self.g_depth.check(what + ' g_depth'), self.g_color.check(what + ' g_color'),
                self.g_weight.check(what + ' g_weight'))

    def accumulate(self, loss_init, what):
        self.prepare(loss_init)
        check(lib().adfp_mapper_loss(C.byref(self.la), stream()), 'adfp_mapper_loss')
        return self.results(what)


@pytest.mark.parametrize('N,S,stage,warm,keep_mode', LOSS_CASES)
def test_mapper_loss_entries_against_the_statement(N, S, stage, warm, keep_mode):
    """Both entries on one batch (ties of all three kinds, 15 % zero depths, dropped rays carrying NaN / +-inf): cotangents
    bit for bit, the loss within 3 * 2^-24 relative (exactly 0 at 0), the two entries within N (S + 4) 2^-53 of each other."""
    L = lib()
    b = R.make_loss_batch(N, S, keep_mode)
    ref = R.loss_and_cotangents(b['depth'], b['color'], b['weight'], b['gd'], b['gc'], b['keep'], stage, warm, 0.2)
    call = LossCall(b, N, S, stage, warm)
    what = f'{N}x{S} {stage} warm={warm} keep={keep_mode}'

    # ---- adfp_mapper_loss: accumulated onto what the word held
    acc0 = call.accumulate(0.0, what + ' adfp_mapper_loss')
    R.assert_loss_close(acc0[0], ref[0], what + ' adfp_mapper_loss')
    R.assert_cotangents_equal(acc0[1:], ref[1:], what + ' adfp_mapper_loss')
    acc5 = call.accumulate(5.0, what + ' adfp_mapper_loss onto 5.0')
    R.assert_cotangents_equal(acc5[1:], ref[1:], what + ' adfp_mapper_loss onto 5.0')
    if ref[0] == 0.0:
        assert acc5[0] == 5.0
    else:
        # one f64 atomic per wave (4 per workgroup) onto a word that starts at 5.0: each add rounds at most half an ulp of the
        # running value <= 5 + loss, and the order of the adds differs from the first call's by at most the summation bound
        waves = 4 * ((N + 255) // 256)
        assert abs(acc5[0] - (5.0 + acc0[0])) <= (waves + 1) * 2.0 ** -53 * (5.0 + ref[0]) + N * (S + 4) * 2.0 ** -53 * ref[0], (acc5[0], acc0[0])
        assert acc5[0] > 5.0

    # ---- adfp_mapper_loss_step: written through the ticket; the first workgroup does adfp_adam_prep's work on the side
    nblocks = (N + 255) // 256
    assert int(L.adfp_mapper_loss_scratch_bytes(N)) == 8 * (1 + nblocks)
    scratch = Guarded((1 + nblocks,), torch.float64)                       # partial-sum slots: NaN
    scratch.buf[:1].zero_()                                                # the ticket word: zero before the first call
    n_groups = 5
    steps0 = torch.tensor(PREP_STEPS + [4242] * 3, dtype=torch.int32)
    derived0 = torch.arange(16, dtype=torch.float32).reshape(8, 2) + 100.0
    lrs = (C.c_float * n_groups)(0.1, 0.005, 0.0, -1.0, 0.005)
    steps, derived = Guarded((8,), torch.int32, steps0), Guarded((8, 2), torch.float32, derived0)
    got = []
    for k, ng in enumerate((0, n_groups)):                                 # the second call on the same scratch also steps Adam's counters
        call.prepare(float('nan'))                                         # the loss word is overwritten, whatever it held
        check(L.adfp_mapper_loss_step(C.byref(call.la), scratch.ptr, 8 * (1 + nblocks), steps.ptr, derived.ptr, ng, lrs, B1, B2, None,
                                      stream()), 'adfp_mapper_loss_step')
        got.append(call.results(what + f' adfp_mapper_loss_step call {k}'))
        sc = scratch.check(what + ' scratch')                              # every partial-sum slot written, nothing behind them
        assert int(scratch.buf[:1].view(torch.int32)[0]) == 0, 'the ticket is not zero after the call'
        assert np.isfinite(sc[1:]).all()
        if k == 0:
            R.assert_bits_equal(steps.check('steps'), steps0.numpy(), 'steps after n_groups = 0')
            R.assert_bits_equal(derived.check('derived'), derived0.numpy(), 'derived after n_groups = 0')
    R.assert_loss_close(got[0][0], ref[0], what + ' adfp_mapper_loss_step')
    R.assert_cotangents_equal(got[0][1:], ref[1:], what + ' adfp_mapper_loss_step')
    assert got[1][0] == got[0][0] and math.copysign(1.0, got[1][0]) == 1.0, 'a second call on the same scratch gives other bits'
    R.assert_cotangents_equal(got[1][1:], ref[1:], what + ' adfp_mapper_loss_step, second call')
    # the two entries against each other: float64 summation order only
    assert abs(got[0][0] - acc0[0]) <= N * (S + 4) * 2.0 ** -53 * ref[0], (got[0][0], acc0[0])
    # the side job = a separate adfp_adam_prep call, bit for bit; = the statement within one float32 ulp
    steps_b, derived_b = Guarded((8,), torch.int32, steps0), Guarded((8, 2), torch.float32, derived0)
    check(L.adfp_adam_prep(steps_b.ptr, derived_b.ptr, n_groups, lrs, B1, B2, None, stream()), 'adfp_adam_prep')
    torch.cuda.synchronize()
    R.assert_bits_equal(steps.check('steps'), steps_b.check('steps'), 'steps: loss_step vs adam_prep')
    R.assert_bits_equal(derived.check('derived'), derived_b.check('derived'), 'derived: loss_step vs adam_prep')
    s_ref, d_ref = R.adam_derived(steps0.numpy()[:n_groups], list(lrs), B1, B2, 0, derived0.numpy()[:n_groups])
    assert steps.data.cpu().numpy()[:n_groups].tolist() == s_ref.tolist()
    R.assert_within_one_ulp(derived.data.cpu().numpy()[:n_groups], d_ref, 'derived: loss_step vs the statement')
    R.assert_bits_equal(steps.data.cpu().numpy()[n_groups:], steps0.numpy()[n_groups:], 'steps beyond n_groups')
    R.assert_bits_equal(derived.data.cpu().numpy()[n_groups:], derived0.numpy()[n_groups:], 'derived beyond n_groups')


# ======================================================================================================= adfp_adam_prep
@pytest.mark.parametrize('skip', [None, 0, 1])
@pytest.mark.parametrize('n_groups', [1, 5, 8])
def test_adam_prep_against_the_statement(n_groups, skip):
    """Step counters exact; derived within one float32 ulp of python-float arithmetic; groups with lr < 0 and everything beyond
    n_groups untouched bit for bit; a set skip flag: no counter moves and derived is zeroed.  Step counts from 0 to 99 999,
    lr 0 among the learning rates.
    The device's double pow / sqrt need not be correctly rounded, but a double result that is off by a few of ITS ulps changes
    the float32 it rounds to only when it lies within 2^-50 relative of a float32 rounding boundary: one value in 2^27.  So at
    most ONE of a case's values (30 to 320 of them, 1 400 over the nine cases) may differ in its bits, and then by one ulp;
    two would mean a pow / sqrt that is wrong in earnest.  Observed on gfx950: all 1 400 bit-equal."""
    L = lib()
    skip_dev = None if skip is None else torch.tensor([skip], dtype=torch.int32, device=DEV)
    not_bit_equal = checked = 0
    for shift in range(20):
        steps0 = torch.full((8,), 4242, dtype=torch.int32)
        steps0[:n_groups] = torch.tensor([PREP_STEPS[(g + shift) % 5] for g in range(n_groups)], dtype=torch.int32)
        lr_list = [PREP_LRS[(g + shift // 5) % 4] for g in range(n_groups)]
        derived0 = torch.arange(16, dtype=torch.float32).reshape(8, 2) + 100.0
        steps, derived = Guarded((8,), torch.int32, steps0), Guarded((8, 2), torch.float32, derived0)
        check(L.adfp_adam_prep(steps.ptr, derived.ptr, n_groups, (C.c_float * n_groups)(*lr_list), B1, B2, ptr(skip_dev), stream()), 'adfp_adam_prep')
        torch.cuda.synchronize()
        s, d = steps.check('steps'), derived.check('derived')
        s_ref, d_ref = R.adam_derived(steps0.numpy()[:n_groups], lr_list, B1, B2, skip, derived0.numpy()[:n_groups])
        assert s[:n_groups].tolist() == s_ref.tolist(), (shift, s, s_ref)
        stepping = np.array([(lr >= 0) or bool(skip) for lr in lr_list])
        not_bit_equal += R.assert_within_one_ulp(d[:n_groups][stepping], d_ref[stepping], f'derived, shift {shift}')
        checked += 2 * int(stepping.sum())
        R.assert_bits_equal(d[:n_groups][~stepping], derived0.numpy()[:n_groups][~stepping], 'derived of a group with lr < 0')
        R.assert_bits_equal(s[n_groups:], steps0.numpy()[n_groups:], 'steps beyond n_groups')
        R.assert_bits_equal(d[n_groups:], derived0.numpy()[n_groups:], 'derived beyond n_groups')
        if skip:
            assert not d[:n_groups].any()
        else:
            for g, lr in enumerate(lr_list):
                if lr == 0.0:
                    assert s[g] == steps0[g] + 1 and d[g, 0] == 0.0 and d[g, 1] > 0.0     # lr == 0 steps: its moments advance
    assert not_bit_equal <= 1, f'{not_bit_equal} of {checked} derived values are not bit-equal to the statement'


# ============================================================================================== Adam against torch.optim.Adam
LR_SCHEDULE = [0.1, 0.005, 0.0, 0.005]             # the schedule of test_masked_adam_vs_torch_adam
PARAM_TOL = 2e-6                                   # and its criterion: |out - ref| / max(|ref|, 1e-3) <= 2e-6
# Which betas torch.optim.Adam is given.  'abi' is the criterion proper; 'python' is an extra that pins why the two differ.
# The kernels receive `float beta1, beta2` and form 1 - beta in float32 from them.  torch.optim.Adam given the SAME two values
# (the doubles of those floats) agrees in all three tensors to 2e-6.  Given python's 0.9 / 0.999 it multiplies the squared
# gradient by float32(1 - 0.999) where the kernel has 1 - float32(0.999): 1.29e-5 smaller, the whole second moment with it.  The
# parameters do not see that factor -- sqrt(1 - beta2^t) in `derived` is formed from the same float and cancels it -- so they are
# held to 2e-6 against python's betas too, and the second moment to 2e-6 plus that factor, which the number formats give:
BETAS = {'abi': (float(np.float32(B1)), float(np.float32(B2))), 'python': (B1, B2)}
V_FACTOR = (abs((1.0 - float(np.float32(B2))) / float(np.float32(1.0 - B2)) - 1.0)          # the weight of g^2: 1.29e-5
            + len(LR_SCHEDULE) * abs(float(np.float32(B2)) / B2 - 1.0))                        # the decay of the older terms: 4 x 1.3e-8


class Group(object):
    """One parameter group on both sides: torch.optim.Adam on the compact copy p0[mask] (src/Mapper.py:347-378) and the device
    buffers of one of the three layouts -- 'cm' [C][nvox] (adfp_masked_adam_dev / _multi) or 'cl' [nvox][32] with its
    reference-layout twin (adfp_adam_step)."""

    def __init__(self, layout, nvox, C_, masked, gen):
        self.layout, self.nvox, self.C = layout, nvox, C_
        self.p0 = torch.randn(C_, nvox, generator=gen) * 0.01                          # channel-major on the host, always
        self.mask = (torch.rand(nvox, generator=gen) < 0.4) if masked else None
        self.full = torch.ones(C_, nvox, dtype=torch.bool) if self.mask is None else self.mask[None].expand(C_, nvox)
        self.ref = self.p0[self.full].clone().requires_grad_(True)
        dev = (lambda x: x.t().contiguous()) if layout == 'cl' else (lambda x: x)
        self.to_dev, shape = dev, ((nvox, C_) if layout == 'cl' else (C_, nvox))
        self.p = Guarded(shape, torch.float32, dev(self.p0))
        self.m, self.v = Guarded(shape, torch.float32, torch.zeros(shape)), Guarded(shape, torch.float32, torch.zeros(shape))
        self.g = Guarded(shape, torch.float32, torch.zeros(shape))
        self.p_cm = Guarded((C_, nvox), torch.float32, self.p0) if layout == 'cl' else None
        self.mask_dev = None if self.mask is None else self.mask.to(DEV, torch.uint8).contiguous()

    def host(self, buf):
        """A device buffer of this group as a channel-major CPU tensor; tails checked."""
        x = torch.from_numpy(buf.check('adam buffer', written=False))
        return x.t() if self.layout == 'cl' else x

    def state(self):
        return [self.host(b).clone() for b in (self.p, self.m, self.v)]

    def compare(self, opt, what, v_tol=PARAM_TOL):
        p, m, v = self.state()
        full = self.full
        st = opt.state[self.ref]
        for name, got, ref, init in (('param', p, self.ref.detach(), self.p0), ('exp_avg', m, st['exp_avg'], torch.zeros_like(self.p0)),
                                     ('exp_avg_sq', v, st['exp_avg_sq'], torch.zeros_like(self.p0))):
            assert torch.equal(got[~full], init[~full]), f'{what} {name}: touched outside the mask'
            if name == 'param':
                err = ((got[full] - ref).abs() / ref.abs().clamp_min(1e-3)).max()
            else:
                err = (got[full] - ref).abs().max() / ref.abs().max().clamp_min(1e-30)   # relative to the tensor's scale
            tol = v_tol if name == 'exp_avg_sq' else PARAM_TOL
            assert float(err) <= tol, f'{what} {name}: {float(err):.3e} > {tol}'
        if self.p_cm is not None:                                                       # the reference-layout twin, bit for bit
            R.assert_bits_equal(self.p_cm.check('param_cm', written=False), p.contiguous().numpy(), f'{what} param_cm vs param_cl transposed')


def fill_groups(groups, der):
    """(AdfpAdamClGroup[], n, AdfpAdamGroup[], n) of `groups`; der: {group: its row of the derived buffer}."""
    cl, fl = [g for g in groups if g.layout == 'cl'], [g for g in groups if g.layout == 'cm']
    carr, farr = (_lib.AdfpAdamClGroup * max(1, len(cl)))(), (_lib.AdfpAdamGroup * max(1, len(fl)))()
    for a, g in zip(carr, cl):
        a.param_cl, a.param_cm, a.grad_cl, a.exp_avg_cl, a.exp_avg_sq_cl = g.p.addr(), g.p_cm.addr(), g.g.addr(), g.m.addr(), g.v.addr()
        a.mask, a.nvox, a.derived = (g.mask_dev.data_ptr() if g.mask_dev is not None else None), g.nvox, der[g]
    for a, g in zip(farr, fl):
        a.param, a.grad, a.exp_avg, a.exp_avg_sq = g.p.addr(), g.g.addr(), g.m.addr(), g.v.addr()
        a.mask, a.nvox, a.channels, a.derived = (g.mask_dev.data_ptr() if g.mask_dev is not None else None), g.nvox, g.C, der[g]
    return carr, len(cl), farr, len(fl)


def launch(entry, groups, der):
    L = lib()
    carr, ncl, farr, nfl = fill_groups(groups, der)
    if entry == 'dev':
        for g in groups:
            check(L.adfp_masked_adam_dev(g.p.ptr, g.g.ptr, g.m.ptr, g.v.ptr, ptr(g.mask_dev), g.nvox, g.C, B1, B2, EPS, C.c_void_p(der[g]), stream()),
                  'adfp_masked_adam_dev')
    elif entry == 'multi':
        assert ncl == 0
        check(L.adfp_masked_adam_multi(nfl, C.byref(farr), B1, B2, EPS, stream()), 'adfp_masked_adam_multi')
    else:
        check(L.adfp_adam_step(ncl, C.byref(carr), nfl, C.byref(farr), B1, B2, EPS, stream()), 'adfp_adam_step')
    torch.cuda.synchronize()


ADAM_ENTRIES = {'dev': [('cm', 315, 32), ('cm', 27, 32)],      # a grid of 32 channels with a ragged 4-voxel tail; a second one: the group without a gradient
                'multi': [('cm', 1000, 1), ('cm', 37, 1), ('cm', 4097, 1)],
                'step': [('cl', 27, 32), ('cl', 315, 32), ('cl', 64 * 5, 32), ('cm', 1000, 1), ('cm', 37, 1), ('cm', 4097, 1)]}


@pytest.mark.parametrize('betas', ['abi', 'python'])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('entry', ['dev', 'multi', 'step'])
def test_adam_entries_vs_torch_adam(entry, masked, betas):
    """Identical gradients on both sides, the step-dependent scalars from adfp_adam_prep, four steps with the lr schedule
    [0.1, 0.005, 0, 0.005]: parameters within 2e-6 (floor 1e-3), both moments within 2e-6 of their tensor's scale, against
    torch.optim.Adam's param / exp_avg / exp_avg_sq.  'abi' (torch given the betas the C ABI carries) is that criterion as it
    stands, 2e-6 on all three tensors; 'python' (torch given 0.9 / 0.999) is an extra, see BETAS above: the same 2e-6 on the
    parameters and the first moment, 2e-6 + V_FACTOR on the second.
    In the second iteration the last group has lr < 0 (torch: grad = None; here: the group is left out of the launch, its
    counter must not move); after it comes an iteration with the skip flag set, which may change no bit of parameters, moments
    and counters (torch: no step) but still zeroes the channels-last gradients."""
    L = lib()
    gen = torch.Generator().manual_seed(3)
    groups = [Group(layout, nvox, C_, masked, gen) for layout, nvox, C_ in ADAM_ENTRIES[entry]]
    opt = torch.optim.Adam([{'params': [g.ref], 'lr': 0} for g in groups], betas=BETAS[betas], eps=EPS)
    v_tol = PARAM_TOL + (V_FACTOR if betas == 'python' else 0.0)
    n = len(groups)
    steps = Guarded((8,), torch.int32, torch.zeros(8, dtype=torch.int32))
    derived = Guarded((8, 2), torch.float32, torch.zeros(8, 2))
    der = {g: derived.addr() + 8 * k for k, g in enumerate(groups)}
    skip = torch.zeros(1, dtype=torch.int32, device=DEV)
    absent = groups[-1]
    expect_steps = [0] * n

    def iteration(k, lr, skipped=False, without=None):
        active = [g for g in groups if g is not without]
        grads = {g: torch.randn(g.C, g.nvox, generator=gen) * (10.0 ** -k) for g in groups}
        for g in groups:
            g.g.reset(g.to_dev(grads[g]))
        before = {g: g.state() + ([torch.from_numpy(g.p_cm.check('param_cm', written=False)).clone()] if g.p_cm is not None else []) for g in groups}
        skip.fill_(1 if skipped else 0)
        lrs = (C.c_float * n)(*[(-1.0 if g is without else lr) for g in groups])
        check(L.adfp_adam_prep(steps.ptr, derived.ptr, n, lrs, B1, B2, ptr(skip), stream()), 'adfp_adam_prep')
        launch(entry, active, der)
        if not skipped:
            for pg, g in zip(opt.param_groups, groups):
                pg['lr'] = lr
                g.ref.grad = None if g is without else grads[g][g.full].clone()
            opt.step()
            for j, g in enumerate(groups):
                expect_steps[j] += 0 if g is without else 1
        assert steps.check('steps')[:n].tolist() == expect_steps
        for g in active:
            if g.layout == 'cl':
                assert not g.g.check('grad_cl').any(), 'the consumed channels-last gradient is not zeroed'
            else:
                R.assert_bits_equal(g.g.check('grad'), g.to_dev(grads[g]).numpy(), 'a flat gradient is read only')
        return before

    def unchanged(g, before, what):
        now = g.state() + ([torch.from_numpy(g.p_cm.check('param_cm', written=False))] if g.p_cm is not None else [])
        for name, a, b in zip(('param', 'exp_avg', 'exp_avg_sq', 'param_cm'), now, before):
            R.assert_bits_equal(a.contiguous().numpy(), b.contiguous().numpy(), f'{what}: {name}')

    for k, lr in enumerate(LR_SCHEDULE):
        before = iteration(k, lr, without=absent if (k == 1 and n > 1) else None)
        for j, g in enumerate(groups):
            g.compare(opt, f'{entry} group {j} after step {k}', v_tol)
        if k == 1 and n > 1:
            unchanged(absent, before[absent], 'the group without a gradient')
        if k == 2:                                             # lr == 0: the moments move, the parameters do not
            for g in groups:
                now = g.state()
                R.assert_bits_equal(now[0].contiguous().numpy(), before[g][0].contiguous().numpy(), 'param after the lr = 0 step')
                assert not torch.equal(now[1], before[g][1]) and not torch.equal(now[2], before[g][2])
        if k == 1:                                             # an iteration whose gradients are not valid: nobody steps
            before = iteration(k, lr, skipped=True)
            assert not derived.check('derived')[:n].any()
            for g in groups:
                unchanged(g, before[g], 'the skipped iteration')
    assert expect_steps == [4] * (n - 1) + [3 if n > 1 else 4]


# ====================================================================================== the fused path's gradients vs the oracle
MODES = ['f32', 'f16x3']


def rows_of_the_kept_rays(masks, keep, N, S):
    """Engine.relu_masks covers the N x S points of the batch, ray-major; the oracle renders the kept rays only."""
    k = torch.from_numpy(keep)

    def sub(x):
        return x.reshape(N, S, *x.shape[1:])[k].reshape(-1, *x.shape[1:])
    out = {}
    for name, v in masks.items():
        if name == 'att_softmax':
            continue                                           # per in-band point, not per point; the oracle does not take it
        out[name] = [sub(x) for x in v] if isinstance(v, (list, tuple)) else sub(v)
    return out


FUSED_CASES = [('low', True, (32, 16)), ('high', True, (32, 16)), ('color', False, (32, 16)), ('color', True, (32, 16)),
               ('color', True, (100, 29))]      # S = 129: three chunks in composite_bwd_block, the dropped rays' zero fill in steps of 64


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('stage,warm,samples', FUSED_CASES,
                         ids=[f'{st}-{w}' + ('' if smp == (32, 16) else f'-{smp[0]}+{smp[1]}') for st, w, smp in FUSED_CASES])
def test_fused_gradient_against_the_oracle(stage, warm, samples, mode, monkeypatch):
    """The Mapper's counterpart of the Tracker's test of this name: MapperIteration._sequence(adam=False) on
    test_gpu_mapper_iteration.setup()'s batch (700 rays, some dropped, some at zero depth) -- pre-filter job, forward, loss +
    cotangents, backward with ray_keep -- against the oracle's autograd of oracle.mapper_loss over the kept rays, rendered with
    depth_max = the max of the kept depths.  Criterion: conftest.assert_grad_tight (TIGHT_GRAD_TOL of each tensor's scale on
    every element, both math modes) with the kernels' ReLU decisions of the kept rays' points forced on the oracle; the loss
    within 1e-5 relative.  A cotangent off by a constant factor, or a dropped ray that leaks, moves these gradients; Adam's
    normalisation hides both from a parameter trajectory.
    samples: (N_samples, N_surface).  (100, 29): rows of 129 samples -- the dropped rays (ray_keep) are zero-filled in several
    steps of 64, the kept ones carry the transmittance and the suffix sum across three chunks."""
    import test_gpu_mapper_iteration as MI
    monkeypatch.setenv('ADFP_MATH', mode)
    sc, dec, rend, rays, masks = MI.setup(samples)
    for p in dec.high_decoder.parameters():
        p.requires_grad_(True)
    tsdf, tb = sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV)
    grids = {k: v.clone().to(DEV) for k, v in sc.c.items()}
    it = mapping.MapperIteration(rend, dec, grids, None, tsdf, tb, MI.STAGE_LR, train=('high', 'color', 'att'), use_graph=False, distributed=False)
    sd = {k: v.detach().cpu().clone() for k, v in dec.state_dict().items()}
    # The backward's scratch is kept across calls.  An iteration on the same rays with shortened depths (nothing beyond the box:
    # every ray kept) leaves a cotangent in every sample's slot; the dropped rays of the measured call must not inherit them.
    near = [t.float().contiguous() for t in (rays[0], rays[1], rays[2] * 0.3, rays[3])]
    assert R.prefilter(*[t.cpu() for t in near[:3]], sc.bound)[0].sum() > 0.95 * rays[0].shape[0]
    it._sequence(*near, stage, warm, adam=False)               # (adam=False leaves the bucket's grid slots zero for the next call)
    cap = ReluCapture(rend)
    g_grids, g_flats = it._sequence(*[t.float().contiguous() for t in rays], stage, warm, adam=False)
    torch.cuda.synchronize()
    loss = float(it.loss)
    g_grids = {k: v.cpu() for k, v in g_grids.items()}
    g_flats = {k: v.detach().cpu().clone() for k, v in g_flats.items()}
    N, S = rays[0].shape[0], rend.N_samples + rend.N_surface

    ro, rd, gd, gc = [t.cpu() for t in rays]
    keep, dmax = R.prefilter(ro, rd, gd, sc.bound)
    assert 0 < keep.sum() < N and ((gd.numpy() == 0) & keep).any()
    k = torch.from_numpy(keep)
    relu = rows_of_the_kept_rays(cap.masks(stage), keep, N, S)
    c_or = {n: v.clone().requires_grad_(True) for n, v in sc.c.items()}
    sd_or = {n: v.clone().requires_grad_(True) for n, v in sd.items()}
    O.reset_relu_flips()
    d, u, col, w = O.render_batch_ray(sd_or, c_or, rd[k], ro[k], sc.tsdf_volume, sc.tsdf_bnds, sc.bound, stage, gd[k], rend.N_samples, rend.N_surface,
                                      depth_max=torch.tensor(float(dmax)), relu_masks=relu)
    ref = O.mapper_loss(d, col, w, gd[k], gc[k], stage, warm)
    ref.backward()
    assert_forced_decisions_are_boundary_units(dict(O.RELU_FLIPS))
    assert abs(loss - ref.item()) <= 1e-5 * abs(ref.item()), (loss, ref.item())

    tag = f'fused {stage} warm={warm}' + ('' if samples == (32, 16) else f' {samples[0]}+{samples[1]}')
    used = {'low': ('low',), 'high': ('low', 'high'), 'color': ('low', 'high', 'color')}[stage]
    assert sorted(g_grids) == sorted(used)
    for name in used:                                          # grids: returned in the reference layout
        assert_grad_tight(g_grids[name], c_or['grid_' + name].grad, f'{tag} d/d grid_{name}', mode)
    nets = {'high': ('high_decoder', 'high'), 'color': ('color_decoder', 'color'), 'att': ('mlp', 'att')}
    want = {'low': (), 'high': ('high', 'att'), 'color': ('high', 'color', 'att')}[stage]
    assert sorted(g_flats) == sorted(want)
    for net in want:                                           # flat network gradients: split in named_parameters order
        attr, key = nets[net]
        off = 0
        for pname, prm in getattr(dec, attr).named_parameters():
            cnt = prm.numel()
            got = g_flats[key][off:off + cnt].view(prm.shape)
            r = sd_or[f'{attr}.{pname}'].grad
            assert_grad_tight(got, r if r is not None else torch.zeros_like(got), f'{tag} d/d {attr}.{pname}', mode)
            off += cnt
        assert off == g_flats[key].numel()
