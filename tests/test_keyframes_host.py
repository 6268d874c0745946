"""CPU: the Mapper's overlap keyframe selection (attentive_dfprior_amd.keyframes) against mapper_keyframes.npz, which holds the
reference's own Mapper.keyframe_selection_overlap executed on the mini scene (tests/golden/make_keyframe_golden.py): the ranking
step, the host path, and the C entry's argument checks (no device needed for those)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from attentive_dfprior_amd import _lib, keyframes as KF

KS = (0, 3, 8, 1000)


@pytest.fixture(autouse=True)
def _restore_global_rngs():
    """These tests seed torch's and numpy's global streams (the selection draws from them, as the reference does); the suite after
    them sees the streams as they were."""
    np_state = np.random.get_state()
    with torch.random.fork_rng(devices=[]):
        yield
    np.random.set_state(np_state)


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN, 'mapper_keyframes.npz'))
    return {k: z[k] for k in z.files}


def intr(g):
    H, W, fx, fy, cx, cy = g['intrinsics'].tolist()
    return int(H), int(W), fx, fy, cx, cy


def recorded_counts(g, c):
    total = int(g['pixels']) * int(g['n_samples'])
    cnt = np.rint(g[f'{c}.percent'] * total).astype(np.int64)
    assert np.array_equal(cnt / total, g[f'{c}.percent'])
    return cnt, total


def test_fixture_covers_the_cases(gold):
    cases = list(gold['cases'])
    assert set(cases) == {'main', 'zeros', 'random', 'empty'}
    main, _ = recorded_counts(gold, 'main')
    assert main[0] > 0 and (main == 0).sum() >= 3                             # the current pose sees; facing away sees nothing
    assert len(set(main[4:7].tolist())) == 1 and main[4] > 0                  # duplicate poses: a three-way tie
    assert gold['empty.poses'].shape == (0, 4, 4)
    assert (gold['zeros.depth'] == 0).any()


@pytest.mark.parametrize('case', ['main', 'zeros', 'random', 'empty'])
def test_ranking_reproduces_recorded_lists(gold, case):
    cnt, total = recorded_counts(gold, case)
    for s in gold['np_seeds'].tolist():
        for k in KS:
            np.random.seed(s)
            got = KF.select_from_counts(cnt, total, k)
            want = gold[f'{case}.sel.{s}.{k}']
            assert [int(v) for v in got] == want.tolist(), (case, s, k)
            assert all(isinstance(v, np.integer) for v in got)
            # numpy's global stream advanced exactly as the reference's single permutation
            np.random.seed(s)
            np.random.permutation(np.array([i for i in sorted(range(len(cnt)), key=lambda i: cnt[i], reverse=True) if cnt[i] > 0]))
            a = np.random.rand()
            np.random.seed(s)
            KF.select_from_counts(cnt, total, k)
            assert np.random.rand() == a


def test_ranking_is_stable_for_ties():
    np.random.seed(3)
    ref = list(np.random.permutation(np.array([2, 0, 1, 4]))[:10])
    np.random.seed(3)
    assert KF.select_from_counts([5, 5, 9, 0, 5], 10, 10) == ref


@pytest.mark.parametrize('case', ['main', 'zeros', 'random'])
def test_host_path_matches_reference(gold, case):
    H, W, fx, fy, cx, cy = intr(gold)
    n_s = int(gold['n_samples'])
    cnt, total = recorded_counts(gold, case)
    got, pts = KF.keyframe_overlap_counts_host(torch.from_numpy(gold[f'{case}.idx']), torch.from_numpy(gold[f'{case}.depth']),
                                               torch.from_numpy(gold[f'{case}.c2w']), torch.from_numpy(gold[f'{case}.poses']),
                                               n_s, H, W, fx, fy, cx, cy, return_points=True)
    assert np.array_equal(pts.numpy().view(np.uint32), gold[f'{case}.points'].view(np.uint32))
    amb = gold[f'{case}.ambiguous']
    assert (np.abs(got - cnt) <= amb).all(), np.nonzero(np.abs(got - cnt) > amb)
    assert np.array_equal(got[amb == 0], cnt[amb == 0])


@pytest.mark.parametrize('case', ['main', 'random', 'empty'])
def test_host_drop_in_end_to_end(gold, case):
    """The drop-in on the CPU: the reference's draw (same torch seed -> same indices) and the recorded lists wherever the counts agree."""
    H, W, fx, fy, cx, cy = intr(gold)
    seed = int(gold[f'{case}.torch_seed'])
    depth, c2w = torch.from_numpy(gold[f'{case}.depth']), torch.from_numpy(gold[f'{case}.c2w'])
    kd = [{'est_c2w': torch.from_numpy(p)} for p in gold[f'{case}.poses']]
    color = torch.zeros(H, W, 3)
    cnt, _ = recorded_counts(gold, case)
    got_counts = KF.keyframe_overlap_counts_host(torch.from_numpy(gold[f'{case}.idx']), depth, c2w, gold[f'{case}.poses'],
                                                 int(gold['n_samples']), H, W, fx, fy, cx, cy) if kd else cnt
    for s in gold['np_seeds'].tolist():
        for k in KS:
            torch.manual_seed(seed)
            np.random.seed(s)
            sel = KF.keyframe_selection_overlap(color, depth, c2w, kd, k, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, device='cpu')
            after = torch.rand(1)
            torch.manual_seed(seed)
            torch.randint(H * W, (int(gold['pixels']),))
            assert torch.equal(after, torch.rand(1))                 # exactly one draw of the reference's shape
            if np.array_equal(got_counts, cnt):
                assert [int(v) for v in sel] == gold[f'{case}.sel.{s}.{k}'].tolist(), (case, s, k)


def test_entry_rejects_bad_arguments_without_a_device():
    L = _lib.lib()
    f = L.adfp_keyframe_overlap
    p = 16                                       # any non-null address: nothing is dereferenced on an argument error
    ok = dict(idx=p, n=100, depth=p, H=48, W=64, c2w=p, S=16, poses=p, K=4, fx=57.76, fy=57.76, cx=31.5, cy=23.5, edge=20,
              counts=p, pts=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['idx'], a['n'], a['depth'], a['H'], a['W'], a['c2w'], a['S'], a['poses'], a['K'], a['fx'], a['fy'], a['cx'],
                 a['cy'], a['edge'], a['counts'], a['pts'], a['stream'])

    for bad in (dict(K=-1), dict(n=0), dict(n=-3), dict(S=0), dict(H=0), dict(W=-1), dict(idx=None), dict(depth=None),
                dict(c2w=None), dict(counts=None), dict(poses=None), dict(fx=0.0), dict(fy=float('nan')), dict(cx=float('inf'))):
        assert call(**bad) == -1, bad
    assert call(n=1 << 27, S=16) == -2
    assert call(K=0, poses=None) == 0            # valid and launches nothing
