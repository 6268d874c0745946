"""CPU: the statements of tests/ray_order_ref.py and the conditions on its fixed-seed inputs that keep tests/test_gpu_ray_order.py and
tests/test_gpu_gather_rows.py honest -- the Morton code against hand-stated keys, the share of rays whose cell the float32 kernel may
legitimately round the other way (at most 3 % per key case), the distance of every probed pair from the probe's threshold (at least
1e-3 relative, three orders above float32 rounding of a squared distance, so the count can be asserted exactly), and the spread of the
probe cases over the decision."""
import numpy as np
import pytest

import ray_order_ref as R


# ================================================================================================== Morton code, keys
def test_morton_interleave_by_hand():
    assert int(R.morton(1, 0, 0, 8)) == 1 and int(R.morton(0, 1, 0, 8)) == 2 and int(R.morton(0, 0, 1, 8)) == 4
    assert int(R.morton(2, 0, 0, 8)) == 8 and int(R.morton(0, 2, 0, 8)) == 16 and int(R.morton(0, 0, 2, 8)) == 32
    assert int(R.morton(255, 255, 255, 8)) == 2 ** 24 - 1
    assert int(R.morton(255, 0, 0, 8)) == 0b001001001001001001001001
    assert int(R.morton(0b101, 0b011, 0b110, 8)) == 0b101110011                 # bits (z y x) of bit 2, bit 1, bit 0
    k = R.planted_keys(np.array([[3, 3, 3]]), np.array([[0, 0, 0]]))
    assert int(k[0]) == 0b111111 << 24
    k = R.planted_keys(np.array([[3, 3, 3]]), np.array([[255, 255, 255]]))
    assert int(k[0]) == 2 ** 30 - 1 and R.KEY_BITS == 30
    assert int(R.planted_keys(np.array([[1, 0, 0]]), np.array([[0, 0, 1]]))[0]) == (1 << 24) | 4


def test_planted_rows_follow_their_hand_stated_cells():
    ro, rd, gd, co, cs, cs_null, names = R.planted_rows()
    assert np.isinf(gd[names.index('depth 3.5e38 acts as 1')]) and np.isfinite(gd[names.index('depth 3.2e38 acts as 1')])
    for depth, want in ((gd, cs), (None, cs_null)):
        key, amb = R.sort_keys(ro, rd, depth, R.KEY_BNDS)
        assert not amb.any(), [n for n, a in zip(names, amb) if a]
        o_cells, s_cells = R.ray_cells(ro, rd, depth, R.KEY_BNDS)
        for i, n in enumerate(names):
            assert tuple(o_cells[i]) == tuple(co[i]) and tuple(s_cells[i]) == tuple(want[i]), n
        assert np.array_equal(key, R.planted_keys(co, want))
        assert (R.candidate_keys(ro, rd, depth, R.KEY_BNDS) == key).all()
    # the depth matters where it is valid, every axis meets both clamps, and NaN has its rows
    assert tuple(cs[0]) != tuple(cs[1])
    for a in range(3):
        assert {0, 3} <= set(co[:, a].tolist()) and {0, 255} <= set(cs[:, a].tolist())
    assert np.isnan(ro).any() and np.isnan(rd).any()


@pytest.mark.parametrize('n', R.KEY_SIZES + (4099,))
def test_key_cases_stay_under_the_ambiguity_cap(n):
    ro, rd, gd = R.key_case(n) if n != 4099 else R.shuffled_key_case(n)
    assert ro.shape == (n, 3) and ro.dtype == rd.dtype == gd.dtype == np.float32
    key, amb = R.sort_keys(ro, rd, gd, R.KEY_BNDS)
    assert amb.mean() <= 0.03
    assert key.min() >= 0 and key.max() < 2 ** R.KEY_BITS
    hw_o, hw_s = R.rounding_half_width(ro, rd, gd, R.KEY_BNDS)
    assert 0 < hw_o <= R.HW_ORIGIN <= 1e-3 and 0 < hw_s <= R.HW_SURFACE <= 1e-3       # the band covers float32 rounding of the kernel's chain
    cand = R.candidate_keys(ro, rd, gd, R.KEY_BNDS)
    assert (cand[:, ~amb] == key[~amb]).all()                                          # nudging decides nothing outside the band
    assert (cand == key).any(axis=0).all()
    if n >= 255:
        lo, hi = R.KEY_BNDS[:, 0], R.KEY_BNDS[:, 1]
        assert (ro < lo).any() and (ro > hi).any() and ((ro > lo) & (ro < hi)).all(axis=1).any()      # inside and slightly outside
        co, cs = R.ray_cells(ro, rd, gd, R.KEY_BNDS)
        assert set(np.unique(co)) == {0, 1, 2, 3} and len(np.unique(cs)) > 100
    if n == 4099:
        assert len(np.unique(key)) < n // 8                                             # equal keys: stability is visible


def test_key_statement_by_brute_force():
    """sort_keys against a scalar, per-ray evaluation with Python integers."""
    ro, rd, gd = R.key_case(257)
    key, _ = R.sort_keys(ro, rd, gd, R.KEY_BNDS)
    for i in range(0, 257, 8):
        cells = []
        for x, n_cells in ((ro[i].astype(np.float64), 4), (ro[i].astype(np.float64) + rd[i].astype(np.float64) * float(gd[i]), 256)):
            u = (x - R.KEY_BNDS[:, 0]) / (R.KEY_BNDS[:, 1] - R.KEY_BNDS[:, 0])
            cells.append([min(max(int(np.floor(n_cells * v)), 0), n_cells - 1) for v in u])
        k = 0
        for b in range(8):
            for a in range(3):
                k |= ((cells[1][a] >> b) & 1) << (3 * b + a)
                if b < 2:
                    k |= ((cells[0][a] >> b) & 1) << (24 + 3 * b + a)
        assert k == int(key[i]), i


# ================================================================================================== the probe
def test_probe_statement_on_a_hand_made_batch():
    ro = np.zeros((5, 3), np.float32)
    rd = np.array([[1, 0, 0], [1, 0.5, 0], [0, 0, 2], [0, 0, 2.05], [3, 4, 0]], np.float32)
    gd = np.array([1, 2, 0, np.nan, 1], np.float32)          # points (1,0,0) (2,1,0) (0,0,2) (0,0,2.05) (3,4,0)
    far, pairs, margin = R.order_verdict(ro, rd, gd, 1.0)
    assert (far, pairs) == (3, 4) and margin == pytest.approx(2 ** 0.5 - 1, abs=1e-6)   # distances sqrt 2, 3, 0.05, 5.4
    far, pairs, margin = R.order_verdict(ro, rd, None, 0.5)   # points = rd: distances 0.5, 2.29, 0.05, 5.4
    assert (far, pairs) == (2, 4) and margin < 1e-6
    assert R.order_verdict(ro[:1], rd[:1], gd[:1], 1.0)[:2] == (0, 0) and R.order_verdict(ro[:0], rd[:0], gd[:0], 1.0)[:2] == (0, 0)
    n = 6151                                                  # stride 3: only pairs (3k, 3k+1) count
    ro = np.zeros((n, 3), np.float32)
    rd = np.zeros((n, 3), np.float32)
    rd[1::3, 0] = 1.0
    assert R.order_verdict(ro, rd, None, 0.5)[:2] == (2048, 2048)
    rd[:] = 0
    rd[2::3, 0] = 1.0
    assert R.order_verdict(ro, rd, None, 0.5)[:2] == (0, 2048)


@pytest.mark.parametrize('name', sorted(R.PROBE_CASES))
def test_probe_cases_keep_their_distance_from_the_threshold(name):
    ro, rd, gd = R.probe_case(name)
    n = R.PROBE_CASES[name][0]
    assert ro.shape == rd.shape == (n, 3) and ro.dtype == rd.dtype == np.float32 and ro.flags.c_contiguous and rd.flags.c_contiguous
    far, pairs, margin = R.order_verdict(ro, rd, gd, R.PROBE_FAR)
    assert pairs == min(n - 1, 2048) and 0 <= far <= pairs
    assert margin >= 1e-3
    if R.PROBE_CASES[name][2] == 'invalid':
        stride = (n - 1) // pairs
        sampled = np.concatenate([np.arange(pairs) * stride, np.arange(pairs) * stride + 1])
        with np.errstate(invalid='ignore'):
            bad = ~((gd > 0) & (gd < 3e38))
        assert bad[sampled].any() and gd.dtype == np.float32
        assert R.order_verdict(ro, rd, np.where(bad, 1.0, gd).astype(np.float32), R.PROBE_FAR)[:2] == (far, pairs)


def test_probe_cases_span_the_decision():
    sizes = {R.PROBE_CASES[k][0] for k in R.PROBE_CASES}
    assert sizes == set(R.PROBE_SIZES) == {2, 3, 257, 2049, 2050, 4097, 6151, 100003}
    assert {(n - 1) // min(n - 1, 2048) for n in sizes} == {1, 2, 3, 48}
    v = {k: R.order_verdict(*R.probe_case(k), R.PROBE_FAR) for k in R.PROBE_CASES}
    assert any(far == 0 and pairs > 0 for far, pairs, _ in v.values())
    assert any(far == pairs and pairs >= 2048 for far, pairs, _ in v.values())
    assert sum(0.4 * pairs <= far <= 0.6 * pairs and far > 256 for far, pairs, _ in v.values()) >= 5       # beyond one wavefront's / one thread's share
    assert v['257-coherent'][:2] == (0, 256) and v['257-alternating'][:2] == (256, 256) and v['2-jump'][:2] == (1, 1)
    for n in R.PROBE_SIZES:                                    # every size has a verdict with and without gt_depth and with invalid depths
        assert all(f'{n}-mixed{s}' in v for s in ('', '-null', '-invalid'))
    assert any(R.PROBE_CASES[k][2] == 'null' and 0 < v[k][0] < v[k][1] for k in v)


def test_render_batch_is_coherent_in_pixel_order_and_not_when_shuffled():
    """The Renderer-level batch of tests/test_gpu_ray_order.py at the mini scene's voxel (far distance 8 x 0.04 m)."""
    from attentive_dfprior_amd import synthetic
    sc = synthetic.mini_scene()
    X = sc.tsdf_volume.shape[4]
    voxel = float(sc.tsdf_bnds[0, 1] - sc.tsdf_bnds[0, 0]) / X
    assert voxel == pytest.approx(0.04)
    (ro, rd, gd), perm = R.render_batch(sc.center, sc.lo_in.numpy(), sc.hi_in.numpy())
    assert ro.shape == (R.RENDER_N, 3) and sorted(perm.tolist()) == list(range(R.RENDER_N)) and (gd > 0.1).all()
    far, pairs, _ = R.order_verdict(ro, rd, gd, 8 * voxel)
    assert pairs == 2048 and far <= 0.05 * pairs
    far, pairs, _ = R.order_verdict(ro[perm], rd[perm], gd[perm], 8 * voxel)
    assert far >= 0.65 * pairs
    far, pairs, _ = R.order_verdict(ro[:3000], rd[:3000], gd[:3000], 8 * voxel)         # the pixel-order batch of another size
    assert far <= 0.05 * pairs
    lo, hi = sc.bound[:, 0].numpy(), sc.bound[:, 1].numpy()
    p = ro.astype(np.float64) + rd.astype(np.float64) * gd[:, None]
    assert ((p > lo) & (p < hi)).all()                                                   # every ray's surface lies inside the scene bound


# ================================================================================================== the gather
def test_gather_inputs_make_every_word_distinct():
    for wname, sizes in R.GATHER_WORLDS.items():
        assert len(sizes) <= 64
        for lname, layout in R.GATHER_LAYOUTS.items():
            per_rank = R.gather_inputs(sizes, layout)
            assert len(per_rank) == len(sizes) and all(a.shape[0] == s for rank, s in zip(per_rank, sizes) for a in rank)
            out = R.gather_ref(per_rank)
            words = np.concatenate([np.ascontiguousarray(o).view(np.int32).reshape(-1) for o in out])
            assert len(np.unique(words)) == words.size == sum(sizes) * sum(np.dtype(d).itemsize * e // 4 for d, e in layout), (wname, lname)
            assert all(o.dtype == np.dtype(d) and o.shape == (sum(sizes), e) for o, (d, e) in zip(out, layout))
    assert [np.dtype(d).itemsize * e // 4 for d, e in R.GATHER_LAYOUTS['eight']] == [1, 2, 3, 4, 5, 6, 7, 9]
    assert [np.dtype(d).itemsize * e // 4 for d, e in R.GATHER_LAYOUTS['render']] == [2, 2, 3]
    assert R.GATHER_WORLDS['w3'] == (5, 0, 2) and R.GATHER_WORLDS['w4'] == (0, 0, 1, 0) and R.GATHER_WORLDS['w5'] == (257, 256, 255, 1, 300)
    w64 = R.GATHER_WORLDS['w64']
    assert len(w64) == 64 and min(w64) == 0 and max(w64) <= 40 and len(set(w64)) > 20 and 29000 <= sum(R.GATHER_WORLDS['big']) <= 31000
