"""GPU: the two sides of the sharded render's one all-gather -- adfp_gather_pack / adfp_gather_unpack (k_gather_rows<PACK>,
csrc/adfp_kernels.hip) -- called raw through ctypes for a SIMULATED world in one process: one pack per rank into that rank's
`pad`-row slice of one gathered buffer, one unpack out of it, held bit for bit to the concatenation over the ranks
(tests/ray_order_ref.py: gather_ref and the inputs, every 4-byte word distinct; pinned on the CPU by tests/test_ray_order_host.py).
The multi-process tests reach these kernels only with shard_range sizes (never zero, at most one row apart) and pad = max(sizes).

Buffers carry sentinels: the gathered buffer is pre-filled with 0xA5 bytes (pack may write nothing beyond a rank's rows), the outputs
with 0x5A bytes and 64 bytes of tail (unpack must write every word and nothing behind them); no input word has either pattern."""
import ctypes as C

import numpy as np
import pytest
import torch

import ray_order_ref as R
from attentive_dfprior_amd import _lib
from attentive_dfprior_amd import dist as adist
from attentive_dfprior_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
E_ARG = -1
TAIL = 64
PACK_FILL, OUT_FILL = 0xA5, 0x5A


def stream():
    return _lib.current_stream(DEV)


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def words_of(layout):
    return [np.dtype(d).itemsize * e // 4 for d, e in layout]


def to_dev(per_rank):
    """numpy [rows, el] -> device tensors; a rank without rows gets one spare row (torch gives an empty tensor no address, and the
    entry points refuse a null array whatever the row count)."""
    return [[torch.from_numpy(a if a.shape[0] else np.zeros((1,) + a.shape[1:], a.dtype)).to(DEV) for a in rank] for rank in per_rank]


def pack_and_unpack(sizes, layout, pad):
    per_rank = R.gather_inputs(sizes, layout)
    want = R.gather_ref(per_rank)
    dev_in = to_dev(per_rank)
    keep = [[t.clone() for t in rank] for rank in dev_in]
    n, world, total = len(layout), len(sizes), sum(sizes)
    wds = words_of(layout)
    W = sum(wds)
    words = (C.c_int * n)(*wds)
    gathered = torch.full((world * pad * W * 4 + TAIL,), PACK_FILL, dtype=torch.uint8, device=DEV)
    L = lib()
    for r in range(world):
        dst = C.c_void_p(gathered.data_ptr() + r * pad * W * 4)
        assert L.adfp_gather_pack(n, ptrs(dev_in[r]), words, sizes[r], dst, stream()) == 0, f'pack of rank {r}'
    outs = [torch.full((total * w * 4 + TAIL,), OUT_FILL, dtype=torch.uint8, device=DEV) for w in wds]
    per = (C.c_longlong * world)(*sizes)
    assert L.adfp_gather_unpack(n, ptrs(outs), words, world, pad, per, C.c_void_p(gathered.data_ptr()), stream()) == 0
    torch.cuda.synchronize()
    # pack: a rank's rows, interleaved, and nothing beyond them
    g = gathered.cpu().numpy()
    assert (g[world * pad * W * 4:] == PACK_FILL).all(), 'pack wrote behind the gathered buffer'
    slots = g[:world * pad * W * 4].reshape(world, pad, W * 4)
    for r in range(world):
        assert (slots[r, sizes[r]:] == PACK_FILL).all(), f'pack wrote into the padding rows of rank {r}'
        off = 0
        for a, w in enumerate(wds):
            got = slots[r, :sizes[r], off:off + 4 * w]
            assert np.array_equal(got, per_rank[r][a].view(np.uint8).reshape(sizes[r], 4 * w)), f'packed rows of rank {r}, array {a}'
            off += 4 * w
    # unpack: the concatenation over the ranks, every word written, nothing behind them
    for a, (o, w) in enumerate(zip(outs, wds)):
        h = o.cpu().numpy()
        assert (h[total * w * 4:] == OUT_FILL).all(), f'unpack wrote behind array {a}'
        got = h[:total * w * 4].view(np.int32)
        ref = np.ascontiguousarray(want[a]).view(np.int32).reshape(-1)
        assert not (got == np.int32(0x5A5A5A5A)).any(), f'array {a}: words never written'
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, f'array {a}: {bad.size} words differ, first at word {bad[:4].tolist()} (row {int(bad[0]) // w})'
    for rank, kept in zip(dev_in, keep):
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(rank, kept)), 'an input changed'


@pytest.mark.parametrize('extra_pad', [0, 3])
@pytest.mark.parametrize('layout', ['render', 'one-word', 'eight'])
@pytest.mark.parametrize('world', ['w1', 'w3', 'w4', 'w5', 'w64'])
def test_pack_and_unpack_reproduce_the_concatenation(world, layout, extra_pad):
    sizes = R.GATHER_WORLDS[world]
    pack_and_unpack(sizes, R.GATHER_LAYOUTS[layout], max(sizes) + extra_pad)


def test_a_frame_sized_gather():
    sizes = R.GATHER_WORLDS['big']                       # 30 000 rows x 7 words
    pack_and_unpack(sizes, R.GATHER_LAYOUTS['render'], max(sizes))


def test_argument_checks_and_empty_calls():
    L = lib()
    layout = R.GATHER_LAYOUTS['render']
    wds = words_of(layout)
    n, W = len(wds), sum(wds)
    rows, pad, world = 6, 8, 2
    src = [torch.zeros((rows, e), dtype=getattr(torch, d), device=DEV) for d, e in layout]
    send = torch.full((world * pad * W * 4,), PACK_FILL, dtype=torch.uint8, device=DEV)
    dst = [torch.full((2 * rows * w * 4,), OUT_FILL, dtype=torch.uint8, device=DEV) for w in wds]
    words = (C.c_int * n)(*wds)
    sp, dp, buf = ptrs(src), ptrs(dst), C.c_void_p(send.data_ptr())
    per = (C.c_longlong * world)(rows, rows)
    big_words = (C.c_int * 9)(*([1] * 9))
    many = (C.c_void_p * 9)(*([src[0].data_ptr()] * 9))

    def bad_words(k, v):
        w = list(wds)
        w[k] = v
        return (C.c_int * n)(*w)

    def null_at(tensors, k):
        p = ptrs(tensors)
        p[k] = None
        return p
    st = stream()
    for nn, s, w in ((0, sp, words), (9, many, big_words)):
        assert L.adfp_gather_pack(nn, s, w, rows, buf, st) == E_ARG
        assert L.adfp_gather_unpack(nn, s, w, world, pad, per, buf, st) == E_ARG
    for v in (0, -1):
        assert L.adfp_gather_pack(n, sp, bad_words(1, v), rows, buf, st) == E_ARG
        assert L.adfp_gather_unpack(n, dp, bad_words(2, v), world, pad, per, buf, st) == E_ARG
    assert L.adfp_gather_pack(n, null_at(src, 2), words, rows, buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, null_at(dst, 0), words, world, pad, per, buf, st) == E_ARG
    assert L.adfp_gather_pack(n, None, words, rows, buf, st) == E_ARG and L.adfp_gather_pack(n, sp, None, rows, buf, st) == E_ARG
    assert L.adfp_gather_pack(n, sp, words, rows, None, st) == E_ARG
    assert L.adfp_gather_pack(n, sp, words, -1, buf, st) == E_ARG
    for wd in (0, 65, -1):
        assert L.adfp_gather_unpack(n, dp, words, wd, pad, (C.c_longlong * 65)(*([1] * 65)), buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, dp, words, world, pad, (C.c_longlong * world)(rows, pad + 1), buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, dp, words, world, pad, (C.c_longlong * world)(-1, rows), buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, dp, words, world, -1, per, buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, dp, words, world, pad, None, buf, st) == E_ARG
    assert L.adfp_gather_unpack(n, dp, words, world, pad, per, None, st) == E_ARG
    # nothing to move: 0, and nothing is written
    assert L.adfp_gather_pack(n, sp, words, 0, buf, st) == 0
    assert L.adfp_gather_unpack(n, dp, words, world, 0, (C.c_longlong * world)(0, 0), buf, st) == 0
    assert L.adfp_gather_unpack(n, dp, words, world, pad, (C.c_longlong * world)(0, 0), buf, st) == 0       # launches, every thread returns
    torch.cuda.synchronize()
    assert bool((send == PACK_FILL).all()) and all(bool((d == OUT_FILL).all()) for d in dst)


@pytest.mark.parametrize('world', ['w3', 'w5'])
def test_all_gather_packed_device_branch_equals_the_host_composition(world, monkeypatch):
    """dist._all_gather_packed once per simulated rank around a stand-in for all_gather_into_tensor: device tensors (the kernels)
    and host tensors (the torch composition tests/test_dist_gloo.py pins) return the same tensors -- a rank without rows included,
    whose fresh empty outputs have no address at all."""
    sizes = R.GATHER_WORLDS[world]
    layout = R.GATHER_LAYOUTS['render']
    per_rank = R.gather_inputs(sizes, layout)
    want = [torch.from_numpy(np.ascontiguousarray(w)) for w in R.gather_ref(per_rank)]
    want[0], want[1] = want[0].reshape(-1), want[1].reshape(-1)                     # depth, uncertainty: [N]; colour: [N, 3]
    sends = {}
    state = dict(rank=0, record=True)

    def fake_all_gather(gathered, send, group=None):
        if state['record']:
            sends[(send.device.type, state['rank'])] = send.clone()
        else:
            parts = [sends[(send.device.type, r)] for r in range(len(sizes))]
            assert all(p.shape == send.shape for p in parts)
            gathered.copy_(torch.cat(parts, dim=0).reshape(gathered.shape))
    monkeypatch.setattr(torch.distributed, 'all_gather_into_tensor', fake_all_gather)
    results = {}
    for device in (DEV, torch.device('cpu')):
        for record in (True, False):
            state['record'] = record
            for r in range(len(sizes)):
                state['rank'] = r
                outs = []
                for a, arr in enumerate(per_rank[r]):
                    t = torch.from_numpy(arr.copy()).to(device) if arr.shape[0] else torch.empty((0, arr.shape[1]), dtype=getattr(torch, layout[a][0]), device=device)
                    outs.append(t.reshape(-1) if a < 2 else t)
                res = adist._all_gather_packed(tuple(outs), list(sizes), None)
                if not record:
                    results[(device.type, r)] = res
    for r in range(len(sizes)):
        for a in range(3):
            g, h = results[('cuda', r)][a], results[('cpu', r)][a]
            assert g.is_cuda and g.dtype == h.dtype == want[a].dtype and g.shape == h.shape == want[a].shape
            assert torch.equal(g.cpu().view(torch.uint8), h.view(torch.uint8)) and torch.equal(h.view(torch.uint8), want[a].view(torch.uint8)), (r, a)
