"""GPU: the depth ICP and the RGB-D ICP (csrc/adfp_icp.h, adfp_rgbd.h) at frame sizes past one pass of their loops, against the
float64 restatements (tests/icp_ref.py, rgbd_icp_ref.py) on the analytic room of tests/icp_frame_cases.py.

The other ICP files stay at 48 x 64 pixels or below: 12 workgroups of k_icp_step, one workgroup per image row, at most 12 partial rows
for a solve of 64 lanes.  Here:
  rows     3 x 513, 4 x 256, 4 x 257: k_depth_normals and k_rgbd_frame_map with two and three workgroups per image row, the right
           neighbour and the central difference reaching across u = 255 | 256
  solve    129 x 128, 65 workgroups: k_icp_solve's lane 0 adds two partial rows
  pass2    (CU + 1) x 512 and pass3 (2 CU + 1) x 512, CU the device's compute units: the grid is capped at 2 CU workgroups, so the
           step's grid-stride loop takes a second and a third pass; pass3 at stride 2 is 257 workgroups, five ragged solve passes
  *_b      each of the three one row taller.  At stride 1 the shapes above put only their last row -- which has no normals -- into the
           65th partial row, the second and the third pass; the siblings put a row with normals there (icp_frame_cases' docstring)
ADFP_ICP_MAX_BLOCKS (1024) cannot bind on a 256-CU part: the cap 2 * num_cu() = 512 is reached first, and no test fakes a device.
Every test first asserts the workgroup count it relies on from the device's own CU, so a device where a case no longer crosses its
edge fails instead of passing empty.

The bars are the restatements' own KERNEL_TOL_* (8 x their float32-against-float64 differences); pair counts may differ by at most
8 pairs where the whole image is summed (one lost partial row is about 250, one lost pass thousands) and not at all on the one-hot
masks.  The restatement is fed the device's own downloaded normal and frame maps, so that only the step is compared."""
import numpy as np
import pytest
import torch

import icp_frame_cases as F
import icp_ref as R
import rgbd_icp_ref as G
from attentive_dfprior_amd import synthetic
from attentive_dfprior_amd.icp import DepthICP, RgbdICP
from test_gpu_icp import ONE_SIDED, hold_pose, same_bytes, small_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAIRS = 8                                          # whole-image pair counts: at most this many pairs from the restatement's
NORMAL_SHAPES = F.ROWS_SHAPES + ((129, 128),)
ROW_MASKS = ('solve_second_pass', 'last_partial_row')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def world():
    sc = synthetic.mini_scene()
    vol, bnds = sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV)
    CU = torch.cuda.get_device_properties(0).multi_processor_count
    return sc, vol, bnds, CU


@pytest.fixture(scope='module')
def steps(world):
    """name -> (case, its DepthICP, the device's normal maps of (sensor, model) downloaded once and only read)"""
    sc, vol, bnds, CU = world
    cache = {}

    def get(name):
        if name not in cache:
            c = F.case(name, CU)
            icp = DepthICP(vol, bnds, *c.cam)
            n = icp.compute_normals(dev(np.stack([c.depth_s, c.depth_m]))).cpu().numpy()
            cache[name] = (c, icp, n)
        return cache[name]
    return get


def claim(c, stride, CU, blocks=None, passes=None):
    """The launch geometry a test relies on, from the device's CU"""
    b = F.expected_blocks(c.H, c.W, stride, CU)
    if blocks is not None:
        assert b == blocks, (c.name, stride, b)
    if passes is not None:
        assert F.passes(c.H, c.W, stride, CU)[0] == passes, (c.name, stride)
    return b


def check_sums(got, ref, scale, what):
    """A sum without a term is exactly 0 -> the worst |got - ref| / scale of the others, which the caller holds against its bar"""
    keep = scale > 0
    assert (got[~keep] == 0).all(), what
    ratio = float((np.abs(got - ref)[keep] / scale[keep]).max()) if keep.any() else 0.0
    return ratio


# ---- 1. normals across the 256-lane boundary ------------------------------------------------------------------------------------
@pytest.mark.parametrize('jump', [0.0, 0.05])
@pytest.mark.parametrize('H,W', NORMAL_SHAPES)
def test_normals_with_several_workgroups_per_row(world, H, W, jump):
    sc, vol, bnds, CU = world
    c = F.rows_case(H, W) if (H, W) in F.ROWS_SHAPES else F.case('solve', CU)
    icp = DepthICP(vol, bnds, *c.cam, max_jump=jump)
    depth = np.stack([c.depth_s, c.depth_m])                                # V = 2, one launch
    got = icp.compute_normals(dev(depth)).cpu().numpy()
    assert got.shape == (2, H, W, 3) and got.dtype == np.float32
    worst = 0.0
    for v in range(2):
        ref = R.normals(depth[v], *c.intr, max_jump=jump)
        a, b = (got[v] != 0).any(-1), (ref != 0).any(-1)
        assert not a[-1].any() and not a[:, -1].any()                       # the last row and the last column
        assert (a == b).all(), (v, np.argwhere(a != b)[:4].tolist())
        diff = np.abs(got[v].astype(np.float64) - ref)
        worst = max(worst, float(diff.max()))
        for u in (255, 256):
            if u < W - 1:                                                   # the two columns where the workgroups meet
                assert a[:-1, u].all() and diff[:, u].max() <= R.KERNEL_TOL_NORMAL, (v, u)
        assert a[:-1, :-1].mean() > 0.9
    print(f'icp frame sizes | normals {H} x {W}, max_jump {jump}: max |diff| {worst:.3e} (limit {R.KERNEL_TOL_NORMAL:.1e})')
    assert worst <= R.KERNEL_TOL_NORMAL


@pytest.mark.parametrize('H,W', [(3, 513), (4, 257)])
def test_a_depth_step_at_column_256_cuts_column_255(world, H, W):
    """+0.3 m on the columns 256..: with max_jump 0.05 the lane u = 255 of workgroup 0 must see it in its right neighbour, the first
    lane of workgroup 1; the columns up to 254 read nothing that changed and keep their bytes."""
    sc, vol, bnds, CU = world
    c = F.rows_case(H, W)
    icp = DepthICP(vol, bnds, *c.cam, max_jump=0.05)
    depth = np.stack([c.depth_s, c.depth_m])
    before = icp.compute_normals(dev(depth))
    depth[:, :, 256:] += np.float32(0.3)
    after = icp.compute_normals(dev(depth))
    assert bool((before[:, :-1, 255] != 0).any(-1).all()) and not bool(after[:, :, 255].any())
    assert same_bytes(after[:, :, :255], before[:, :, :255])
    ref = np.stack([R.normals(depth[v], *c.intr, max_jump=0.05) for v in range(2)])
    got = after.cpu().numpy()
    assert ((got != 0).any(-1) == (ref != 0).any(-1)).all() and np.abs(got.astype(np.float64) - ref).max() <= R.KERNEL_TOL_NORMAL


# ---- 2. frame map across the boundary -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W', NORMAL_SHAPES)
def test_frame_map_with_several_workgroups_per_row(world, H, W):
    sc, vol, bnds, CU = world
    c = F.rows_case(H, W) if (H, W) in F.ROWS_SHAPES else F.case('solve', CU)
    icp = RgbdICP(vol, bnds, *c.cam)
    got = icp.frame_map(dev(c.color_s), dev(c.depth_s)).cpu().numpy()
    ref = G.frame_map(c.color_s, c.depth_s)
    assert got.shape == (H, W, 4) and got[..., 3].tobytes() == c.depth_s.tobytes()
    assert not got[:, 0, 1].any() and not got[:, -1, 1].any() and not got[0, :, 2].any() and not got[-1, :, 2].any()
    diff = np.abs(got.astype(np.float64) - ref)
    for u in (255, 256):
        if 1 <= u < W - 1:
            assert (got[:, u, 1] != 0).all() and diff[:, u, 1].max() <= G.KERNEL_TOL_MAP, u
    print(f'icp frame sizes | frame map {H} x {W}: max |diff| {diff.max():.3e} (limit {G.KERNEL_TOL_MAP:.1e})')
    assert diff.max() <= G.KERNEL_TOL_MAP


# ---- 3. one step over the whole image -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(F.shapes()))
def test_one_step_over_the_whole_image(world, steps, name):
    sc, vol, bnds, CU = world
    c, icp, n = steps(name)
    if name.startswith('solve'):
        claim(c, 1, CU, blocks=65, passes=1)
    else:
        claim(c, 1, CU, blocks=2 * CU, passes=3 if name.startswith('pass3') else 2)
        assert 2 * CU > 64 and 2 * CU <= F.MAX_BLOCKS
    if name == 'pass3':                                                     # stride 2: CU + 1 workgroups, a ragged last solve pass
        assert claim(c, 2, CU, blocks=CU + 1, passes=1) > 64 and (CU + 1) % 64 != 0
    Gs = torch.from_numpy(c.G)
    d, nd = dev(np.stack([c.depth_s, c.depth_m])), dev(n)
    for stride in F.STRIDES:
        sums, row, _, _ = icp.step_system(Gs, d[0], nd[0], d[1], nd[1], Gs, stride=stride)
        ref, scale = R.step_sums(c.depth_s, n[0], c.depth_m, n[1], c.G, c.G, *c.intr, stride=stride)
        got = sums.cpu().numpy()
        ratio = check_sums(got, ref, scale, (name, stride))
        print(f'icp frame sizes | one step, {name} {c.H} x {c.W}, stride {stride}: {claim(c, stride, CU)} workgroups, '
              f'{F.passes(c.H, c.W, stride, CU)[0]} passes, {got[28]:.0f} pairs ({got[28] - ref[28]:+.0f}), '
              f'worst |sum - ref| / scale {ratio:.3e} (limit {R.KERNEL_TOL_SUMS:.1e})')
        assert abs(got[28] - ref[28]) <= PAIRS and ref[28] >= 0.9 * icp.strided_pixels(stride), (name, stride)
        assert ratio <= R.KERNEL_TOL_SUMS, (name, stride)
        assert row[0].item() == got[28] and row[5].item() == R.OK


# ---- 4. one step, one-hot sensor normals ----------------------------------------------------------------------------------------
def hot_step(c, icp, n, idx, stride=1):
    """A step whose sensor normals are the device's at the strided pixels idx and zero elsewhere -> (sums, restatement, scale)"""
    hot = F.one_hot(n[0], idx, c.W, stride)
    Gs = torch.from_numpy(c.G)
    sums = icp.step_system(Gs, dev(c.depth_s), dev(hot), dev(c.depth_m), dev(n[1]), Gs, stride=stride)[0].cpu().numpy()
    ref, scale = R.step_sums(c.depth_s, hot, c.depth_m, n[1], c.G, c.G, *c.intr, stride=stride)
    return sums, ref, scale


@pytest.mark.parametrize('name', ['pass3', 'pass3_b', 'solve', 'solve_b'])
def test_one_hot_masks_and_no_stale_partial_row(world, steps, name):
    """Per mask: the pair count is the restatement's exactly and the sums hold the bar, and a step with the `first` mask right after it
    on the same object counts that one pair and no more.  Before the masks the object runs a step over the whole image at stride 1,
    which fills every partial row it will ever use (2 CU of them, 65 for `solve`); the `first` mask is then also run at strides 2
    and 3, whose grids are smaller: a solve that read a row beyond the step's grid would add the full run's pairs."""
    sc, vol, bnds, CU = world
    c, icp, n = steps(name)
    blocks = claim(c, 1, CU, blocks=65 if name.startswith('solve') else 2 * CU)
    Gs = torch.from_numpy(c.G)
    d, nd = dev(np.stack([c.depth_s, c.depth_m])), dev(n)
    full = icp.step_system(Gs, d[0], nd[0], d[1], nd[1], Gs, stride=1)[0].cpu().numpy()
    assert full[28] >= 0.9 * c.H * c.W
    flags = F.pair_flags(c, n[0], n[1], 1)
    first = F.mask_indices('first', c, flags, 1, CU)
    assert len(first) == 1
    masks = F.MASKS if name.startswith('pass3') else ROW_MASKS
    for m in masks:
        idx = F.mask_indices(m, c, flags, 1, CU)
        if len(idx) == 0:                                                   # the one-row-short shape does not reach it with a normal
            assert name in ('pass3', 'solve') and m in ('third_pass',) + ROW_MASKS
            idx = F.nominal_mask(m, c.H, c.W, 1, CU)
        got, ref, scale = hot_step(c, icp, n, idx)
        ratio = check_sums(got, ref, scale, (name, m))
        print(f'icp frame sizes | one-hot, {name}, mask {m} [{idx[0]} .. {idx[-1]}]: {got[28]:.0f} pairs (restatement {ref[28]:.0f}), '
              f'worst ratio {ratio:.3e}')
        assert got[28] == ref[28] == int(flags[idx].sum()) and ratio <= R.KERNEL_TOL_SUMS, (name, m)
        assert ref[28] >= 1 or name in ('pass3', 'solve')                   # the sibling reaches every mask with a pair
        again, ref1, scale1 = hot_step(c, icp, n, first)
        assert again[28] == ref1[28] == 1 and check_sums(again, ref1, scale1, (name, m, 'first')) <= R.KERNEL_TOL_SUMS
    for stride in (2, 3):                                                   # a smaller grid after the full one
        assert claim(c, stride, CU) < blocks
        icp.step_system(Gs, d[0], nd[0], d[1], nd[1], Gs, stride=1)
        fl = F.pair_flags(c, n[0], n[1], stride)
        idx = F.mask_indices('first', c, fl, stride, CU)
        got, ref, scale = hot_step(c, icp, n, idx, stride)
        print(f'icp frame sizes | one-hot, {name}, mask first at stride {stride} after a full stride-1 step: {got[28]:.0f} pairs')
        assert got[28] == ref[28] == 1 and check_sums(got, ref, scale, (name, stride)) <= R.KERNEL_TOL_SUMS


def test_corner_mask_at_stride_three(world, steps):
    """513 x 512 at stride 3: i = n - 1 = 29 240 is (us, vs) = (510, 510), the largest quotient and remainder of i by wn."""
    sc, vol, bnds, CU = world
    c, icp, n = steps('pass3')
    assert (c.H, c.W) == (513, 512) or CU != 256
    fl = F.pair_flags(c, n[0], n[1], 3)
    idx = F.mask_indices('corner', c, fl, 3, CU)
    got, ref, scale = hot_step(c, icp, n, idx, 3)
    print(f'icp frame sizes | one-hot, pass3, mask corner at stride 3 [{idx[0]}]: {got[28]:.0f} pairs (restatement {ref[28]:.0f})')
    assert got[28] == ref[28] == 1 and check_sums(got, ref, scale, 'corner') <= R.KERNEL_TOL_SUMS


# ---- 5. the RGB-D step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['solve', 'solve_b', 'pass2', 'pass2_b'])
def test_rgbd_step_over_the_whole_image(world, steps, name):
    sc, vol, bnds, CU = world
    c, plain, n = steps(name)
    claim(c, 1, CU, blocks=65 if name.startswith('solve') else 2 * CU, passes=1 if name.startswith('solve') else 2)
    icp = RgbdICP(vol, bnds, *c.cam)
    cur_d, key_d = icp.frame_map(dev(c.color_s), dev(c.depth_s)), icp.frame_map(dev(c.color_k), dev(c.depth_k))
    cur, key = cur_d.cpu().numpy(), key_d.cpu().numpy()
    Gs, K = torch.from_numpy(c.G), torch.from_numpy(c.K)
    nd, dm = dev(n), dev(c.depth_m)
    for stride in (1, 2):
        sums, row, rgb_row, _, _ = icp.step_system_rgbd(Gs, cur_d, nd[0], dm, nd[1], Gs, key_map=key_d, p_key=K, stride=stride)
        ref, scale = G.step_sums(cur, n[0], c.depth_m, n[1], c.G, key, c.K, c.G, *c.intr, stride=stride)
        got = sums.cpu().numpy()
        ratio = check_sums(got, ref, scale, (name, stride))
        print(f'icp frame sizes | one joint step, {name} {c.H} x {c.W}, stride {stride}: {claim(c, stride, CU)} workgroups, '
              f'{got[28]:.0f} geometric ({got[28] - ref[28]:+.0f}) and {got[30]:.0f} photometric ({got[30] - ref[30]:+.0f}) pairs, '
              f'worst |sum - ref| / scale {ratio:.3e} (limit {G.KERNEL_TOL_SUMS:.1e})')
        assert abs(got[28] - ref[28]) <= PAIRS and abs(got[30] - ref[30]) <= PAIRS, (name, stride)
        assert ref[28] >= 0.9 * icp.strided_pixels(stride) and ref[30] >= 0.5 * icp.strided_pixels(stride)
        assert ratio <= G.KERNEL_TOL_SUMS, (name, stride)
        assert row[0].item() == got[28] and row[5].item() == R.OK and rgb_row[0].item() == got[30]
        # without the keyframe: the depth step's bytes, also when both loops iterate
        want, want_row, want_c2w, want_cam = plain.step_system(Gs, cur_d[..., 3].contiguous(), nd[0], dm, nd[1], Gs, stride=stride)
        sums0, row0, rgb0, c2w0, cam0 = icp.step_system_rgbd(Gs, cur_d, nd[0], dm, nd[1], Gs, stride=stride)
        assert same_bytes(sums0[:29], want) and not bool(sums0[29:].any()) and not bool(rgb0.any())
        assert same_bytes(row0, want_row) and same_bytes(c2w0, want_c2w) and same_bytes(cam0, want_cam)
        assert not same_bytes(sums[:27], want[:27])                          # the term does change the system


# ---- 6. a refinement at a multi-row size ----------------------------------------------------------------------------------------
def test_refine_at_129_x_128_on_the_mini_scene(world):
    """The mini scene's volume through 129 x 128 pixels, the default levels: 5, 17 and 65 workgroups at strides 4, 2, 1."""
    sc, vol, bnds, CU = world
    icp, cam, Gs, ds = small_case(sc, vol, bnds, 129, 128)
    assert [F.expected_blocks(129, 128, s, CU) for s in icp.strides] == [5, 17, 65]
    icp.refine(Gs, ds)
    first = (icp.cam_out.clone(), icp.c2w_out.clone(), icp.stats.clone())
    maps = icp.depth.cpu().numpy()
    ref_c2w, _, ref_status, ref_rows = R.refine(maps[0], maps[1], Gs.numpy(), *cam[2:])
    stats = icp.last_stats().numpy()
    print(f'icp frame sizes | refine 129 x 128: status {stats[:, 5].astype(int).tolist()}, pairs {stats[:-1, 0].astype(int).tolist()} '
          f'(restatement {ref_rows[:-1, 0].astype(int).tolist()})')
    assert stats.shape == (11, 6) and (stats[:, 5] == ref_rows[:, 5]).all() and ref_status == R.OK == icp.last_status()
    assert (np.abs(stats[:-1, 0] - ref_rows[:-1, 0]) <= ONE_SIDED * ref_rows[:-1, 0]).all()
    hold_pose(icp.c2w_out.cpu().numpy(), ref_c2w, 'refine 129 x 128')
    # two calls give the same bytes
    icp.stats.zero_(); icp.c2w_out.zero_(); icp.cam_out.zero_(); icp.workspace.zero_()
    icp.refine(Gs, ds)
    for a, b in zip((icp.cam_out, icp.c2w_out, icp.stats), first):
        assert same_bytes(a, b)
    # one capture, two replays
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        icp.run_steps()
    for _ in range(2):
        icp.set_frame(Gs, ds)
        icp.stats.zero_(); icp.cam_out.zero_(); icp.c2w_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip((icp.cam_out, icp.c2w_out, icp.stats), first):
            assert same_bytes(a, b)
