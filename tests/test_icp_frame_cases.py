"""CPU, restatement only: the inputs of tests/icp_frame_cases.py are what tests/test_gpu_icp_frame_sizes.py relies on -- shapes that
cross the launch edges they claim, nearly every strided pixel a pair, a solvable system, masks that select pixels which do form
pairs, a texture whose gradient is not zero where the frame map's workgroups meet.  An edit of the generator that empties one of
these fails here, not silently on the GPU."""
import numpy as np
import pytest

import icp_frame_cases as F
import icp_ref as R
import rgbd_icp_ref as G

CU = F.DEFAULT_CU
STEP_CASES = tuple(F.shapes())
ONE_SHORT = {'solve': 'solve_b', 'pass2': 'pass2_b', 'pass3': 'pass3_b'}


@pytest.fixture(scope='module')
def flags():
    """(case name, stride) -> pair_flags of the restatement's normal maps, computed once and only read"""
    out = {}
    for name in STEP_CASES:
        c = F.case(name)
        ns, nm = c.ref_normals
        for stride in F.STRIDES:
            out[name, stride] = F.pair_flags(c, ns, nm, stride)
    return out


def test_the_shapes_cross_the_edges_they_claim():
    sh = F.shapes(CU)
    assert sh['solve'] == (129, 128) and sh['pass2'] == (CU + 1, 512) and sh['pass3'] == (2 * CU + 1, 512)
    for a, b in ONE_SHORT.items():
        assert sh[b] == (sh[a][0] + 1, sh[a][1])
    assert F.ROWS_SHAPES == ((3, 513), (4, 256), (4, 257))
    assert [-(-W // 256) for _, W in F.ROWS_SHAPES] == [3, 1, 2]
    # solve: more partial rows than the solve's wave has lanes, lane 0 alone adds two
    for name in ('solve', 'solve_b'):
        blocks = F.expected_blocks(*sh[name], 1, CU)
        assert blocks == 65 > F.SOLVE_LANES and F.passes(*sh[name], 1, CU)[0] == 1
    assert 129 * 128 - 64 * 256 == 128                                     # the last workgroup's live lanes
    # pass2 / pass3: the grid is capped at 2 CU and n > blocks 256
    for name, npass, lanes in (('pass2', 2, 512), ('pass2_b', 2, 1024), ('pass3', 3, 512), ('pass3_b', 3, 1024)):
        H, W = sh[name]
        blocks, n = F.expected_blocks(H, W, 1, CU), F.strided(H, W, 1)[2]
        assert blocks == 2 * CU > 64 and n > blocks * 256 and F.passes(H, W, 1, CU) == (npass, lanes)
        assert 2 * CU < F.MAX_BLOCKS or CU >= 512                           # the 1024 cap cannot bind below 512 compute units
    # pass3 at the coarser strides: 257 workgroups (five ragged passes of the solve's row loop), then 29 241 pixels
    H, W = sh['pass3']
    assert F.expected_blocks(H, W, 2, CU) == 257 and -(-257 // 64) == 5 and 257 % 64 == 1
    assert F.strided(H, W, 3) == (171, 171, 29241) and F.expected_blocks(H, W, 3, CU) == 115
    assert F.expected_blocks(48, 64, 1, CU) == 12                          # what the suite reached before


def test_the_room_and_the_poses():
    P = F.true_pose()
    assert P.dtype == np.float32 and np.allclose(P[:3, 3], F.AT) and abs(np.linalg.det(P[:3, :3].astype(np.float64)) - 1) < 1e-6
    Gs = F.guess_pose(P)
    m, r = R.pose_error(Gs, P)
    assert 5e-3 < m < 3e-2 and 5e-3 < r < 3e-2                              # half the twist: about 12 mm, 13 mrad
    c = F.case('solve')
    d = c.depth_s.astype(np.float64)
    X = R.vertices(c.depth_s, *c.intr, np.float64) @ P[:3, :3].astype(np.float64).T + P[:3, 3]
    assert d.min() > 0.5 and d.max() < 6 and np.abs(np.abs(X).max(-1) - F.ROOM).max() < 1e-6    # every pixel's point lies on a wall
    assert len({tuple(row) for row in np.argmax(np.abs(X), -1).reshape(-1, 1)}) >= 3            # three walls: a solvable view


@pytest.mark.parametrize('name', STEP_CASES)
def test_pair_share_status_and_count(flags, name):
    c = F.case(name)
    ns, nm = c.ref_normals
    assert not ns[-1].any() and not ns[:, -1].any()
    for stride in F.STRIDES:
        n = F.strided(c.H, c.W, stride)[2]
        fl = flags[name, stride]
        sums, _ = R.step_sums(c.depth_s, ns, c.depth_m, nm, c.G, c.G, *c.intr, stride=stride)
        _, row = R.solve(sums, c.G, min_pairs=float(np.ceil(0.05 * n)))
        print(f'{name} {c.H} x {c.W}, stride {stride}: {int(sums[28])} of {n} pair ({sums[28] / n:.4f}), pivot ratio {row[2]:.2e}')
        assert len(fl) == n and int(fl.sum()) == sums[28]                   # pair_flags restates step_sums' gates
        assert sums[28] >= 0.9 * n and row[5] == R.OK and row[2] > 1e-3


@pytest.mark.parametrize('name', STEP_CASES)
def test_every_mask_selects_a_pair_where_the_case_reaches_it(flags, name):
    c = F.case(name)
    H, W = c.H, c.W
    reach = {'first', 'last', 'corner', 'solve_second_pass', 'last_partial_row'}
    if name.startswith('pass'):
        reach.add('second_pass')
    if name.startswith('pass3'):
        reach.add('third_pass')
    empty = {'solve': {'solve_second_pass', 'last_partial_row'}, 'pass2': {'second_pass'}, 'pass3': {'third_pass'}}.get(name, set())
    fl = flags[name, 1]
    wn, hn, n = F.strided(H, W, 1)
    blocks = F.expected_blocks(H, W, 1, CU)
    for m in F.MASKS:
        idx = F.mask_indices(m, c, fl, 1, CU)
        pairs = int(fl[idx].sum()) if len(idx) else 0
        print(f'{name}, mask {m}: indices {idx[:1].tolist()} .. {idx[-1:].tolist()} ({len(idx)}), pairs {pairs}')
        if m not in reach:
            assert len(F.nominal_mask(m, H, W, 1, CU)) == 0 and len(idx) == 0
        elif m in empty:                                                    # the last row alone: see the generator's docstring
            assert pairs == 0 and (F.nominal_mask(m, H, W, 1, CU) // wn == H - 1).all()
        else:
            assert pairs >= 1, m
            if m in ('first', 'last', 'second_pass', 'third_pass', 'corner'):
                assert len(idx) == 1 and pairs == 1
    if name in ONE_SHORT.values():
        assert not empty
    # where the chosen pixels lie
    i = int(F.mask_indices('first', c, fl, 1, CU)[0])
    assert i < 64
    if 'second_pass' in reach and 'second_pass' not in empty:
        i = int(F.mask_indices('second_pass', c, fl, 1, CU)[0])
        assert blocks * 256 <= i < blocks * 256 + 64
    if 'third_pass' in reach and 'third_pass' not in empty:
        i = int(F.mask_indices('third_pass', c, fl, 1, CU)[0])
        assert 2 * blocks * 256 <= i < n
    i = int(F.mask_indices('corner', c, fl, 1, CU)[0])
    assert i % wn == W - 2 and i // wn == H - 2                              # the last column and the last row that carry a normal
    rows = F.mask_indices('solve_second_pass', c, fl, 1, CU)
    assert rows[0] == 64 * 256 and (rows // 256 == 64).all()
    rows = F.mask_indices('last_partial_row', c, fl, 1, CU)
    assert (rows // 256 == blocks - 1).all()


def test_corner_mask_at_stride_three_is_the_last_strided_pixel(flags):
    """513 x 512 at stride 3: the last strided column and row are 510 and 510, both carry normals, and the pixel is i = n - 1."""
    c = F.case('pass3')
    wn, hn, n = F.strided(c.H, c.W, 3)
    idx = F.mask_indices('corner', c, flags['pass3', 3], 3, CU)
    assert idx.tolist() == [n - 1] and flags['pass3', 3][n - 1]
    hot = F.one_hot(c.ref_normals[0], idx, c.W, 3)
    assert hot[510, 510].any() and int((hot != 0).any(-1).sum()) == 1


def test_one_hot_keeps_the_listed_pixels_only():
    c = F.case('solve_b')
    ns = c.ref_normals[0]
    hot = F.one_hot(ns, F.nominal_mask('solve_second_pass', c.H, c.W, 1, CU), c.W)
    assert hot is not ns and not hot[:128].any() and not hot[129:].any() and (hot[128] == ns[128]).all() and hot[128, :-1].any(-1).all()
    assert ns[5, 5].any()                                                   # the original is untouched
    sums, _ = R.step_sums(c.depth_s, hot, c.depth_m, c.ref_normals[1], c.G, c.G, *c.intr)
    assert sums[28] == 127


@pytest.mark.parametrize('H,W', F.ROWS_SHAPES + ((129, 128),))
def test_the_texture_has_a_gradient_where_the_workgroups_meet(H, W):
    c = F.rows_case(H, W) if (H, W) in F.ROWS_SHAPES else F.case('solve')
    assert bool((c.depth_s > 0).all()) and c.color_s.shape == (H, W, 3) and c.color_s.dtype == np.float32
    m = G.frame_map(c.color_s, c.depth_s)
    for u in (255, 256):
        if 1 <= u < W - 1:
            assert (np.abs(m[:, u, 1]) > 1e-5).all(), u                     # far above KERNEL_TOL_MAP
    if W > 257:
        n = R.normals(c.depth_s, *c.intr)
        assert n[:-1, 255].any(-1).all() and n[:-1, 256].any(-1).all()


@pytest.mark.parametrize('name', ['solve', 'pass2'])
def test_the_keyframe_yields_photometric_pairs(name):
    c = F.case(name)
    cur, key = G.frame_map(c.color_s, c.depth_s), G.frame_map(c.color_k, c.depth_k)
    for stride in (1, 2):
        idx, r, J = G.photo_pairs(cur, key, c.K, c.G, *c.intr, stride=stride)
        n = F.strided(c.H, c.W, stride)[2]
        print(f'{name}, stride {stride}: {len(idx)} of {n} photometric pairs, max |r| {np.abs(r).max():.3f}')
        assert len(idx) >= 0.5 * n and np.abs(J).max() > 0
