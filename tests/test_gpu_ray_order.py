"""GPU: the ray-order machinery of the render path -- adfp_ray_sort_keys and adfp_ray_order_probe (k_ray_sort_keys, morton3,
k_ray_order_probe; csrc/adfp_kernels.hip) called raw through ctypes and held to the numpy statements of tests/ray_order_ref.py
(pinned on the CPU by tests/test_ray_order_host.py); Renderer._batch_is_incoherent, Renderer._coherent_order and the sorted
branch of Renderer.render_batch_ray at a few thousand rays of the mini scene; and the full-frame adfp_get_rays against the
reference's float32 formula, bit for bit.

Keys are exact wherever float32 cannot round a coordinate across a cell face (ray_order_ref: `ambiguous`, at most 3 % of a case's
rays by the host test; there the key must be that of a neighbouring cell).  The probe's counts are exact: every probed pair of
every case keeps a relative distance of 1e-3 from the threshold (host test).  Output buffers carry 64 elements of tail and a
sentinel (-77): every payload element is written, nothing behind it."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import attentive_dfprior_amd as A
import ray_order_ref as R
from attentive_dfprior_amd import _lib, common, synthetic
from attentive_dfprior_amd._lib import lib
from oracle import adfp_oracle as O
from conftest import make_cfg, to_dev

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
E_ARG = -1
TAIL, SENTINEL = 64, -77


def stream():
    return _lib.current_stream(DEV)


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bound_of(b):
    out = _lib.Bound()
    _lib.fill_bound(out, [[float(v) for v in row] for row in np.asarray(b)])
    return out


def run_keys(ro, rd, gd, bnds):
    """adfp_ray_sort_keys on numpy inputs -> (key, val) int32 numpy, tails and coverage checked."""
    n = ro.shape[0]
    ro_d, rd_d, gd_d = dev(ro), dev(rd), dev(gd)
    key = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
    val = torch.full((n + TAIL,), SENTINEL, dtype=torch.int32, device=DEV)
    rc = lib().adfp_ray_sort_keys(_lib.ptr(ro_d), _lib.ptr(rd_d), _lib.ptr(gd_d), n, C.byref(bound_of(bnds)), _lib.ptr(key), _lib.ptr(val), stream())
    assert rc == 0
    torch.cuda.synchronize()
    k, v = key.cpu().numpy(), val.cpu().numpy()
    assert (k[n:] == SENTINEL).all() and (v[n:] == SENTINEL).all(), 'something wrote behind the buffers'
    assert (k[:n] >= 0).all() and (v[:n] >= 0).all(), 'elements never written'
    return k[:n], v[:n]


# ================================================================================================== adfp_ray_sort_keys
@pytest.mark.parametrize('n', R.KEY_SIZES)
def test_sort_keys_against_the_statement(n):
    ro, rd, gd = R.key_case(n)
    for depth in (gd, None):
        key, val = run_keys(ro, rd, depth, R.KEY_BNDS)
        assert np.array_equal(val, np.arange(n))
        ref, amb = R.sort_keys(ro, rd, depth, R.KEY_BNDS)
        wrong = np.nonzero((key != ref) & ~amb)[0]
        assert wrong.size == 0, f'{wrong.size} keys differ, first ray {int(wrong[0])}: {int(key[wrong[0]]):#x} vs {int(ref[wrong[0]]):#x}'
        cand = R.candidate_keys(ro, rd, depth, R.KEY_BNDS)
        assert (cand == key[None, :]).any(axis=0).all(), 'an ambiguous ray has the key of no neighbouring cell'
        assert key.max() < 2 ** R.KEY_BITS


def test_sort_keys_planted_rows():
    ro, rd, gd, co, cs, cs_null, names = R.planted_rows()
    for depth, want in ((gd, cs), (None, cs_null)):
        key, val = run_keys(ro, rd, depth, R.KEY_BNDS)
        ref = R.planted_keys(co, want)
        wrong = [f'{names[i]}: {int(key[i]):#x} vs {int(ref[i]):#x}' for i in np.nonzero(key != ref)[0]]
        assert not wrong, wrong
        assert np.array_equal(val, np.arange(len(names)))


def test_sort_keys_argument_checks():
    L = lib()
    ro, rd, gd = (dev(x) for x in R.key_case(257))
    n = 257
    key = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    val = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    p, b, st = _lib.ptr, C.byref(bound_of(R.KEY_BNDS)), stream()
    assert L.adfp_ray_sort_keys(None, p(rd), p(gd), n, b, p(key), p(val), st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), None, p(gd), n, b, p(key), p(val), st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), n, b, None, p(val), st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), n, b, p(key), None, st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), n, None, p(key), p(val), st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), -1, b, p(key), p(val), st) == E_ARG
    for axis in range(3):
        for hi in ('lo', 'below'):
            flat = R.KEY_BNDS.copy()
            flat[axis, 1] = flat[axis, 0] - (0.0 if hi == 'lo' else 0.5)
            assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), n, C.byref(bound_of(flat)), p(key), p(val), st) == E_ARG
    assert L.adfp_ray_sort_keys(p(ro), p(rd), p(gd), 0, b, p(key), p(val), st) == 0
    torch.cuda.synchronize()
    assert bool((key == SENTINEL).all()) and bool((val == SENTINEL).all())


@pytest.fixture(scope='module')
def world():
    """The mini scene on the device, seeded decoders, and the Renderer-level batch of ray_order_ref.render_batch."""
    sc = synthetic.mini_scene()
    dec = A.DF()
    dec.load_state_dict(O.random_state_dict(seed=3))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    (ro, rd, gd), perm = R.render_batch(sc.center, sc.lo_in.numpy(), sc.hi_in.numpy())
    w = dict(sc=sc, dec=dec, c=to_dev(sc.c, DEV), tsdf=sc.tsdf_volume.to(DEV), tb=sc.tsdf_bnds.to(DEV),
             pixel=(dev(ro), dev(rd), dev(gd)), perm=dev(perm))
    w['shuffled'] = tuple(x.index_select(0, w['perm']).contiguous() for x in w['pixel'])
    return w


def new_renderer(world, **attrs):
    rend = A.Renderer(make_cfg(32, 16), None, world['sc'])
    rend.sort_rays_min = 1024
    for k, v in attrs.items():
        setattr(rend, k, v)
    return rend


def test_coherent_order_is_the_stable_sort_of_the_kernels_keys(world):
    n = 4099
    ro, rd, gd = R.shuffled_key_case(n)
    key, _ = run_keys(ro, rd, gd, R.KEY_BNDS)
    rend = new_renderer(world)
    order = rend._coherent_order(dev(ro), dev(rd), dev(gd), None, torch.from_numpy(R.KEY_BNDS), probe=False)
    assert order.dtype == torch.int64 and order.is_cuda and tuple(order.shape) == (n,)
    o = order.cpu().numpy()
    assert np.array_equal(np.sort(o), np.arange(n))
    sorted_keys = key[o]
    assert (np.diff(sorted_keys) >= 0).all()
    same = np.diff(sorted_keys) == 0
    assert same.sum() > n // 2 and (np.diff(o)[same] > 0).all()                        # equal keys keep the caller's order
    assert np.array_equal(o, torch.sort(torch.from_numpy(key.astype(np.int64)), stable=True).indices.numpy())
    assert np.array_equal(o, np.argsort(key, kind='stable'))


# ================================================================================================== adfp_ray_order_probe
def pinned_verdict(fill=SENTINEL):
    word = torch.full((2,), fill, dtype=torch.int32).pin_memory()
    return word, C.c_void_p(word.data_ptr())


def probe(ro_d, rd_d, gd_d, n, far, wp):
    return lib().adfp_ray_order_probe(_lib.ptr(ro_d), _lib.ptr(rd_d), _lib.ptr(gd_d), n, far, wp, stream())


@pytest.mark.parametrize('name', sorted(R.PROBE_CASES))
def test_order_probe_counts_exactly(name):
    ro, rd, gd = R.probe_case(name)
    n = ro.shape[0]
    far, pairs, margin = R.order_verdict(ro, rd, gd, R.PROBE_FAR)
    assert margin >= 1e-3
    word, wp = pinned_verdict()
    assert probe(dev(ro), dev(rd), dev(gd), n, R.PROBE_FAR, wp) == 0
    torch.cuda.synchronize()
    assert (int(word[0]), int(word[1])) == (far, pairs)


def test_order_probe_replaces_the_previous_verdict():
    word, wp = pinned_verdict()
    for name in ('2049-mixed', '2049-mixed', '4097-alternating', '257-coherent', '100003-mixed-null'):
        ro, rd, gd = R.probe_case(name)
        assert probe(dev(ro), dev(rd), dev(gd), ro.shape[0], R.PROBE_FAR, wp) == 0
        torch.cuda.synchronize()
        assert (int(word[0]), int(word[1])) == R.order_verdict(ro, rd, gd, R.PROBE_FAR)[:2], name


def test_order_probe_small_batches_and_argument_checks():
    ro, rd, gd = (dev(x) for x in R.probe_case('257-alternating'))
    for n in (1, 0):
        word, wp = pinned_verdict()
        assert probe(ro, rd, gd, n, R.PROBE_FAR, wp) == 0
        torch.cuda.synchronize()
        assert (int(word[0]), int(word[1])) == (0, 0), n
    word, wp = pinned_verdict()
    L, p, st = lib(), _lib.ptr, stream()
    assert L.adfp_ray_order_probe(None, p(rd), p(gd), 257, R.PROBE_FAR, wp, st) == E_ARG
    assert L.adfp_ray_order_probe(p(ro), None, p(gd), 257, R.PROBE_FAR, wp, st) == E_ARG
    assert L.adfp_ray_order_probe(p(ro), p(rd), p(gd), 257, R.PROBE_FAR, None, st) == E_ARG
    assert L.adfp_ray_order_probe(p(ro), p(rd), p(gd), -1, R.PROBE_FAR, wp, st) == E_ARG
    for far in (0.0, -0.125, float('nan')):
        assert L.adfp_ray_order_probe(p(ro), p(rd), p(gd), 257, far, wp, st) == E_ARG
    torch.cuda.synchronize()
    assert int(word[0]) == SENTINEL and int(word[1]) == SENTINEL


# ================================================================================================== the Renderer around them
class Spy(object):
    """Records what Engine.render_forward is handed (rays and depth as given, depth_max, tsdf_blocks) and passes the call on."""

    def __init__(self, rend, monkeypatch):
        self.calls = []
        orig = rend._engine.render_forward
        sig = inspect.signature(orig)

        def spy(*a, **k):
            args = sig.bind(*a, **k).arguments
            self.calls.append(dict(ro=args['rays_o'], rd=args['rays_d'], gd=args['gt_depth'], depth_max=args.get('depth_max'),
                                   blocks=args.get('tsdf_blocks', False), train=args.get('train', False)))
            return orig(*a, **k)
        monkeypatch.setattr(rend._engine, 'render_forward', spy)

    def last(self):
        return self.calls[-1]


def render(rend, world, batch, stage='color', **kw):
    ro, rd, gd = batch
    gd = kw.pop('gt_depth', gd)
    return rend.render_batch_ray(world['c'], world['dec'], rd, ro, DEV, world['tsdf'], world['tb'], stage, gt_depth=gd, **kw)


def handed(call, batch, order=None):
    """Did the engine receive `batch` (in `order`)?"""
    want = batch if order is None else tuple(x.index_select(0, order) for x in batch)
    return all(torch.equal(call[k].reshape(want[i].shape), want[i]) for i, k in enumerate(('ro', 'rd', 'gd')))


def test_batch_verdicts_of_the_renderer(world):
    rend = new_renderer(world)
    assert rend._batch_is_incoherent(*world['shuffled'], world['tsdf'], world['tb'], wait=True)
    assert not rend._batch_is_incoherent(*world['pixel'], world['tsdf'], world['tb'], wait=True)
    word, far, pairs, far_distance = rend._order_verdict[R.RENDER_N]
    assert far_distance == pytest.approx(8 * 0.04) and word.is_pinned() and word.dtype == torch.int32 and tuple(word.shape) == (2,)
    ref = R.order_verdict(*(x.cpu().numpy() for x in world['pixel']), far_distance)
    assert (far.value, pairs.value) == ref[:2]
    assert rend._coherent_order(*world['pixel'], world['tsdf'], world['tb'], wait=True) is None
    order = rend._coherent_order(*world['shuffled'], world['tsdf'], world['tb'], wait=True)
    assert order is not None and np.array_equal(np.sort(order.cpu().numpy()), np.arange(R.RENDER_N))


def test_a_calls_verdict_steers_the_next_call_of_the_same_size(world, monkeypatch):
    rend = new_renderer(world, tsdf_blocks=False)
    spy = Spy(rend, monkeypatch)
    shuffled, pixel = world['shuffled'], world['pixel']
    other = tuple(x[:3000].contiguous() for x in pixel)
    order = rend._coherent_order(*shuffled, world['tsdf'], world['tb'], probe=False)
    assert not torch.equal(order, torch.arange(R.RENDER_N, device=DEV))
    with torch.no_grad():
        first = render(rend, world, shuffled)
        assert handed(spy.last(), shuffled)                       # no verdict yet: the caller's order
        torch.cuda.synchronize()
        second = render(rend, world, shuffled)
        assert handed(spy.last(), shuffled, order) and not handed(spy.last(), shuffled)
        assert spy.last()['blocks'] is False
        for _ in range(2):                                        # another size: its own verdict, never the shuffled batch's
            render(rend, world, other)
            assert handed(spy.last(), other)
            torch.cuda.synchronize()
        render(rend, world, pixel)                                # same size: still steered by the shuffled batch's verdict ...
        assert handed(spy.last(), pixel, rend._coherent_order(*pixel, world['tsdf'], world['tb'], probe=False))
        torch.cuda.synchronize()
        render(rend, world, pixel)                                # ... and by its own from then on
        assert handed(spy.last(), pixel)
    assert len(spy.calls) == 6
    for x, y in zip(first, second):
        assert torch.equal(x, y)


@pytest.mark.parametrize('stage', ['high', 'color'])
def test_sorted_and_corner_block_renders_are_bit_for_bit_the_plain_one(world, stage, monkeypatch):
    shuffled = world['shuffled']
    order = None
    results = {}
    for name, attrs, permuted, blocks in (('plain', dict(sort_rays_min=0), False, False),
                                          ('sorted', dict(tsdf_blocks=False), True, False),
                                          ('blocks', dict(tsdf_blocks='auto', sort_incoherent='auto'), False, True),
                                          ('both', dict(tsdf_blocks='auto', sort_incoherent=True), True, True)):
        rend = new_renderer(world, **attrs)
        spy = Spy(rend, monkeypatch)
        if order is None:
            order = rend._coherent_order(*shuffled, world['tsdf'], world['tb'], probe=False)
        with torch.no_grad():
            render(rend, world, shuffled, stage)                   # leaves the verdict the next call acts on
            torch.cuda.synchronize()
            results[name] = render(rend, world, shuffled, stage)
        call = spy.last()
        assert handed(call, shuffled, order if permuted else None), name
        assert bool(call['blocks']) == blocks, name
    d, u, col, w = results['plain']
    assert tuple(d.shape) == (R.RENDER_N,) and tuple(col.shape) == (R.RENDER_N, 3) and tuple(w.shape)[:2] == (R.RENDER_N, 48)
    assert torch.isfinite(d).all() and torch.isfinite(u).all() and torch.isfinite(col).all()
    for name in ('sorted', 'blocks', 'both'):
        for x, y, what in zip(results['plain'], results[name], ('depth', 'uncertainty', 'colour', 'weight')):
            assert torch.equal(x, y), f'{name}: {what}'


def test_the_sorted_branch_is_not_taken_without_its_conditions(world, monkeypatch):
    shuffled = world['shuffled']
    rend = new_renderer(world, tsdf_blocks=False)
    spy = Spy(rend, monkeypatch)
    assert rend._batch_is_incoherent(*shuffled, world['tsdf'], world['tb'], wait=True)          # the verdict every call below finds
    order = rend._coherent_order(*shuffled, world['tsdf'], world['tb'], probe=False)
    with torch.no_grad():
        render(rend, world, shuffled)                                                        # the control: this one is sorted
        assert handed(spy.last(), shuffled, order)
        render(rend, world, shuffled, 'low')
        assert handed(spy.last(), shuffled)
        render(rend, world, shuffled, gt_depth=None)
        assert spy.last()['gd'] is None and torch.equal(spy.last()['ro'], shuffled[0])
        rend.perturb = 0.5
        render(rend, world, shuffled)
        assert handed(spy.last(), shuffled)
        rend.perturb = 0.0
        rend.sort_rays_min = R.RENDER_N + 1
        render(rend, world, shuffled)
        assert handed(spy.last(), shuffled)
        rend.sort_rays_min = 1024
    n = len(spy.calls)
    out = render(rend, world, shuffled)                                                      # gradients are wanted: the training path
    assert out[0].requires_grad
    assert len(spy.calls) == n + 1 and spy.last()['train'] and torch.equal(spy.last()['ro'], shuffled[0])


def test_depth_max_of_the_sorted_branch(world, monkeypatch):
    shuffled = world['shuffled']
    rend = new_renderer(world, tsdf_blocks=False)
    spy = Spy(rend, monkeypatch)
    assert rend._batch_is_incoherent(*shuffled, world['tsdf'], world['tb'], wait=True)
    order = rend._coherent_order(*shuffled, world['tsdf'], world['tb'], probe=False)
    mine = torch.tensor([2.0], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        a = render(rend, world, shuffled, depth_max=mine)
        assert handed(spy.last(), shuffled, order) and spy.last()['depth_max'] is mine
        b = render(rend, world, shuffled)
        got = spy.last()['depth_max']
        assert handed(spy.last(), shuffled, order)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) and torch.equal(got, shuffled[2].max().reshape(1))
        rend.sort_rays_min = 0
        plain = render(rend, world, shuffled, depth_max=mine)
    assert float(shuffled[2].max()) < 1.0 and not torch.equal(a[0], b[0])                    # a whole batch's maximum of 2 m moves the far clamp
    for x, y in zip(a, plain):
        assert torch.equal(x, y)


# ================================================================================================== adfp_get_rays
@pytest.mark.parametrize('H,W', [(1, 1), (3, 5), (17, 257), (68, 120)])
def test_get_rays_is_the_float32_formula_bit_for_bit(H, W):
    """common.get_rays on the device (k_get_rays) against its host path: src/common.py:254-272 of the reference in torch float32 --
    a correctly rounded division, products and left-to-right adds."""
    fx, fy, cx, cy = 57.3, 61.9, W / 2 - 0.37, H / 2 + 0.21
    c2w = torch.from_numpy(R.camera((0.31, -1.7, 2.45), 0.7, -0.35, 0.2))
    assert (c2w[:3, :3].abs() > 0.05).all()                                 # a general rotation
    ro_h, rd_h = common.get_rays(H, W, fx, fy, cx, cy, c2w, 'cpu')
    ro_d, rd_d = common.get_rays(H, W, fx, fy, cx, cy, c2w.to(DEV), DEV)
    assert tuple(ro_d.shape) == tuple(rd_d.shape) == (H, W, 3) and ro_d.dtype == rd_d.dtype == torch.float32
    assert torch.equal(ro_d.cpu(), ro_h.contiguous())
    got, want = rd_d.cpu(), rd_h.contiguous()
    ulp = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs().max()
    assert torch.equal(got, want), f'worst distance {int(ulp)} ulp'
    # and the formula itself, in float64 from the same float32 operands: nothing beyond float32 rounding of three terms
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing='ij')
    f = lambda v: float(np.float32(v))                                      # noqa: E731
    dirs = torch.stack([(i - f(cx)) / f(fx), -(j - f(cy)) / f(fy), -torch.ones_like(i)], -1)
    exact = (dirs[..., None, :] * c2w[:3, :3].double()).sum(-1)
    assert float((got.double() - exact).abs().max()) <= 4 * 2.0 ** -24 * float(exact.abs().max() + dirs.abs().max())
