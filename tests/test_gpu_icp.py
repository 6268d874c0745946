"""GPU: the depth ICP (adfp_depth_normals, adfp_icp_*, icp.DepthICP) against its restatement (tests/icp_ref.py) on the mini scene
(TSDF 40 x 40 x 32, 48 x 64 pixels) and on images of a few pixels.

The bars are icp_ref's KERNEL_TOL_* = 8 x the float32-against-float64 differences tests/test_icp_host.py measures: the kernels load
float32 and compute in float64, the restatement they are held against is the float64 one, fed the device's own downloaded maps (the
raycast's depth images), so that what is compared is the ICP and not the raycast."""
import numpy as np
import pytest
import torch

import icp_ref as R
import attentive_dfprior_amd as A
from attentive_dfprior_amd import common, icp as icp_module, synthetic
from attentive_dfprior_amd.icp import DepthICP
from attentive_dfprior_amd.tsdf_raycast import TsdfRaycaster
from conftest import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAM = (48, 64, 57.76, 57.76, 31.5, 23.5)           # the mini scene's camera
INTR = CAM[2:]
ONE_SIDED = 1e-3                                   # normals valid on one side only / pair counts: at most 0.1 %
FIVE = dict(strides=(1,), iters=(5,))              # the issue's five stride-1 steps


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.fixture(scope='module')
def world():
    """The scene on the device, the nine (true pose, guess, sensor depth) cases -- sensor depth = the raycast at the true pose -- and
    per case the float64 restatement's refinement on the device's own maps (computed once, only read)."""
    sc = synthetic.mini_scene()
    vol, bnds = sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV)
    rc = TsdfRaycaster(vol, bnds)
    icp = DepthICP(vol, bnds, *CAM, **FIVE)
    cases = []
    for P, G in R.scene_cases(sc):
        ds = rc.render_depth(torch.from_numpy(P), *CAM)
        icp.set_frame(torch.from_numpy(G), ds)
        maps = icp.depth.cpu().numpy()
        cases.append(dict(P=P, G=G, ds=ds, maps=maps, ref=R.refine(maps[0], maps[1], G, *INTR, **FIVE)))
    return sc, vol, bnds, icp, cases


def hold_pose(got, ref, what):
    m, r = R.pose_error(got, ref)
    print(f'{what}: {m:.3e} m {r:.3e} rad from the restatement (limits {R.KERNEL_TOL_POSE_M:.1e}, {R.KERNEL_TOL_POSE_RAD:.1e})')
    assert m <= R.KERNEL_TOL_POSE_M and r <= R.KERNEL_TOL_POSE_RAD, what


@pytest.mark.parametrize('jump', [0.0, 0.05])
def test_normals_against_the_restatement(world, jump):
    sc, vol, bnds, _, cases = world
    icp = DepthICP(vol, bnds, *CAM, max_jump=jump)
    depth = torch.from_numpy(np.stack([c['maps'][k] for c in cases[::4] for k in (0, 1)])).to(DEV)        # six images, one launch
    got = icp.compute_normals(depth).cpu().numpy()
    assert got.shape == (6, 48, 64, 3) and got.dtype == np.float32
    worst = 0.0
    for v in range(6):
        ref = R.normals(depth[v].cpu().numpy(), *INTR, max_jump=jump)
        a, b = (got[v] != 0).any(-1), (ref != 0).any(-1)
        assert not a[-1].any() and not a[:, -1].any()                     # the last row and the last column
        assert int((a != b).sum()) <= ONE_SIDED * a.size, v
        both = a & b
        assert int(both.sum()) > 2500
        worst = max(worst, float(np.abs(got[v][both].astype(np.float64) - ref[both]).max()))
        ln = np.linalg.norm(got[v][a].astype(np.float64), axis=-1)
        assert np.abs(ln - 1).max() < 1e-6
    print(f'normals, max_jump {jump}: max |diff| {worst:.3e} (limit {R.KERNEL_TOL_NORMAL:.1e})')
    assert worst <= R.KERNEL_TOL_NORMAL


def test_max_jump_cuts_normals_at_a_depth_edge(world):
    sc, vol, bnds, _, cases = world
    d = torch.from_numpy(cases[0]['maps'][0].copy()).to(DEV)
    d[:, 32:] += 0.2                                                       # a step of 20 cm down the middle
    off = DepthICP(vol, bnds, *CAM).compute_normals(d[None])[0]
    on = DepthICP(vol, bnds, *CAM, max_jump=0.05).compute_normals(d[None])[0]
    assert bool((off[:-1, 31] != 0).any(-1).all()) and not bool((on[:, 31] != 0).any())
    assert same_bytes(on[:, :31], off[:, :31]) and same_bytes(on[:, 32:], off[:, 32:])


@pytest.mark.parametrize('stride', [1, 2])
def test_one_step_sums_against_the_restatement(world, stride):
    sc, vol, bnds, icp, cases = world
    worst = 0.0
    for k, c in enumerate(cases):
        depth = torch.from_numpy(c['maps']).to(DEV)
        nrm = icp.compute_normals(depth)
        G = torch.from_numpy(c['G'])
        sums, row, _, _ = icp.step_system(G, depth[0], nrm[0], depth[1], nrm[1], G, stride=stride)
        n = nrm.cpu().numpy()
        ref, scale = R.step_sums(c['maps'][0], n[0], c['maps'][1], n[1], c['G'], c['G'], *INTR, stride=stride)
        got = sums.cpu().numpy()
        assert abs(got[28] - ref[28]) <= ONE_SIDED * ref[28] and ref[28] > 0.85 * icp.strided_pixels(stride), k
        worst = max(worst, float((np.abs(got - ref) / scale).max()))
        assert row[0].item() == got[28] and row[5].item() == R.OK
    print(f'one step, stride {stride}: max |sum - ref| / scale {worst:.3e} (limit {R.KERNEL_TOL_SUMS:.1e})')
    assert worst <= R.KERNEL_TOL_SUMS


def test_refine_on_the_nine_cases(world):
    sc, vol, bnds, icp, cases = world
    for k, c in enumerate(cases):
        cam = icp.refine(torch.from_numpy(c['G']), c['ds'])
        got, stats = icp.c2w_out.cpu().numpy(), icp.last_stats().numpy()
        ref_c2w, ref_cam, ref_status, ref_rows = c['ref']
        assert ref_status == R.OK and (stats[:, 5] == R.OK).all() and stats.shape == (6, 6)
        assert (np.abs(stats[:-1, 0] - ref_rows[:-1, 0]) <= ONE_SIDED * ref_rows[:-1, 0]).all()
        hold_pose(got, ref_c2w, f'case {k}')
        e0, e1 = R.pose_error(c['G'], c['P']), R.pose_error(got, c['P'])
        print(f'case {k}: {e0[0] * 1e3:.2f} mm {np.degrees(e0[1]):.3f} deg -> {e1[0] * 1e3:.3f} mm {np.degrees(e1[1]):.4f} deg, '
              f'{stats[-2, 0]:.0f} pairs, pivot ratio {stats[:-1, 2].min():.2e}')
        assert e1[0] <= e0[0] / 10 and e1[1] <= e0[1] / 10, k
        assert np.abs(cam.cpu().numpy() - R.camera_tensor(got)).max() <= 2.0 ** -23
        assert icp.last_status() == R.OK


def test_default_levels_refine(world):
    """strides (4, 2, 1), iters (4, 3, 3): the constructor's defaults against the restatement with the same levels"""
    sc, vol, bnds, _, cases = world
    icp = DepthICP(vol, bnds, *CAM)
    for k in (0, 5):
        c = cases[k]
        icp.refine(torch.from_numpy(c['G']), c['ds'])
        ref_c2w, _, ref_status, ref_rows = R.refine(c['maps'][0], c['maps'][1], c['G'], *INTR)
        stats = icp.last_stats().numpy()
        assert stats.shape == (11, 6) and ref_status == R.OK == icp.last_status()
        assert (np.abs(stats[:-1, 0] - ref_rows[:-1, 0]) <= ONE_SIDED * ref_rows[:-1, 0]).all()
        hold_pose(icp.c2w_out.cpu().numpy(), ref_c2w, f'default levels, case {k}')


def test_the_three_fallbacks_return_the_guess(world):
    sc, vol, bnds, icp, cases = world
    c = cases[0]
    G = torch.from_numpy(c['G'])
    g_cam = common.get_tensor_from_camera(G)
    # DEGENERATE: the scene's default pose sees too few wall orientations
    P = sc.default_c2w()
    Gd = torch.from_numpy((R.exp_se3(np.asarray(R.TWIST)) @ P.numpy().astype(np.float64)).astype(np.float32))
    cam = icp.refine(Gd, icp.raycaster.render_depth(P, *CAM))
    stats = icp.last_stats().numpy()
    print('default pose: pivot ratio', stats[0, 2], 'pairs', stats[0, 0])
    assert (stats[:, 5] == R.DEGENERATE).all() and 0 <= stats[0, 2] < 1e-9 and stats[0, 0] > 2500 and (stats[1:, :5] == 0).all()
    assert same_bytes(icp.c2w_out, Gd) and (cam.cpu() - common.get_tensor_from_camera(Gd)).abs().max() <= 2.0 ** -23
    # FEW_PAIRS: a volume without a surface raycasts to an all-zero model depth
    empty = DepthICP(torch.ones_like(vol), bnds, *CAM, **FIVE)
    cam = empty.refine(G, c['ds'])
    stats = empty.last_stats().numpy()
    assert not bool(empty.depth[1].any()) and (stats[:, 5] == R.FEW_PAIRS).all() and (stats[:, :5] == 0).all()
    assert same_bytes(empty.c2w_out, G) and (cam.cpu() - g_cam).abs().max() <= 2.0 ** -23
    # REJECTED: a gate tighter than the correction (15-35 mm, 0.8-1.5 degrees)
    for kw, col in ((dict(max_shift=0.005), 4), (dict(max_angle=0.001), 3)):
        tight = DepthICP(vol, bnds, *CAM, **FIVE, **kw)
        cam = tight.refine(G, c['ds'])
        stats = tight.last_stats().numpy()
        assert (stats[:-1, 5] == R.OK).all() and stats[-1, 5] == R.REJECTED == tight.last_status()
        assert stats[-1, col] > list(kw.values())[0]
        assert same_bytes(tight.c2w_out, G) and (cam.cpu() - g_cam).abs().max() <= 2.0 ** -23


def test_two_calls_give_the_same_bytes(world):
    sc, vol, bnds, _, cases = world
    icp = DepthICP(vol, bnds, *CAM)
    c = cases[3]
    outs = []
    for _ in range(2):
        cam = icp.refine(torch.from_numpy(c['G']), c['ds'])
        outs.append((cam.clone(), icp.c2w_out.clone(), icp.stats.clone()))
        icp.stats.zero_(); icp.c2w_out.zero_(); icp.cam_out.zero_(); icp.workspace.zero_()
    for a, b in zip(*outs):
        assert same_bytes(a, b)
    assert outs[0][2][-1, 5].item() == R.OK


def small_case(sc, vol, bnds, H, W, **kw):
    """The mini scene seen through an H x W image of the same field of view from the first corner pose, guess half the twist off."""
    cam = (H, W, 57.76 * W / 64, 57.76 * W / 64, (W - 1) / 2, (H - 1) / 2)
    offset, yaw, pitch = R.POSES[0]
    P = sc.default_c2w(offset=offset, yaw=yaw, pitch=pitch)
    G = torch.from_numpy((R.exp_se3(np.asarray(R.TWIST) * 0.5) @ P.numpy().astype(np.float64)).astype(np.float32))
    icp = DepthICP(vol, bnds, *cam, **kw)
    ds = icp.raycaster.render_depth(P, *cam)
    assert bool((ds > 0).all())
    return icp, cam, G, ds


@pytest.mark.parametrize('H,W', [(1, 1), (1, 5), (5, 1)])
def test_images_without_a_valid_normal(world, H, W):
    """One row or one column: every pixel lies on the last row or the last column, so no normal is valid and no pair exists."""
    sc, vol, bnds, _, _ = world
    icp, cam, G, ds = small_case(sc, vol, bnds, H, W)
    out = icp.refine(G, ds)
    stats = icp.last_stats().numpy()
    assert not bool(icp.normals.any())
    assert (stats[:, 5] == R.FEW_PAIRS).all() and (stats[:, :5] == 0).all()
    assert same_bytes(icp.c2w_out, G) and (out.cpu() - common.get_tensor_from_camera(G)).abs().max() <= 2.0 ** -23


def test_two_by_two_image(world):
    """2 x 2: pixel (0, 0) alone has both neighbours, so there is at most one pair.  With the default share (one pair of four pixels
    is enough) one pair cannot constrain six unknowns: not OK either way, and what the restatement says; when two pairs are asked
    for, FEW_PAIRS."""
    sc, vol, bnds, _, _ = world
    icp, cam, G, ds = small_case(sc, vol, bnds, 2, 2, **FIVE)
    icp.refine(G, ds)
    n = icp.normals.cpu().numpy()
    assert (n[:, 0, 0] != 0).any(-1).all() and not n[:, 0, 1].any() and not n[:, 1].any()
    maps = icp.depth.cpu().numpy()
    _, _, ref_status, ref_rows = R.refine(maps[0], maps[1], G.numpy(), *cam[2:], **FIVE)
    stats = icp.last_stats().numpy()
    assert ref_status in (R.FEW_PAIRS, R.DEGENERATE) and (stats[:, 5] == ref_rows[:, 5]).all() and stats[0, 0] == ref_rows[0, 0] <= 1
    assert same_bytes(icp.c2w_out, G)
    icp2, _, _, _ = small_case(sc, vol, bnds, 2, 2, min_pairs=0.5, **FIVE)
    icp2.refine(G, ds)
    assert icp2.last_status() == R.FEW_PAIRS


@pytest.mark.parametrize('H,W', [(3, 5), (10, 13), (8, 8), (17, 16)])
def test_small_images_against_the_restatement(world, H, W):
    """3 x 5; 10 x 13 (a width and a height that are no multiple of the strides, less than one workgroup); 8 x 8 (exactly one wave);
    17 x 16 (one workgroup and a tail).  Strides 4, 2, 1 (3 x 5: 2, 1), two steps each: every row of the stats against the
    restatement on the device's maps -- the status, the pair count, and the pose when the refinement went through."""
    sc, vol, bnds, _, _ = world
    kw = dict(strides=(2, 1), iters=(2, 2)) if H < 8 else dict(strides=(4, 2, 1), iters=(2, 2, 2))
    icp, cam, G, ds = small_case(sc, vol, bnds, H, W, min_pairs=0.0, **kw)
    icp.refine(G, ds)
    maps = icp.depth.cpu().numpy()
    n = icp.normals.cpu().numpy()
    for v in range(2):
        ref_n = R.normals(maps[v], *cam[2:])
        assert ((n[v] != 0).any(-1) == (ref_n != 0).any(-1)).all() and np.abs(n[v].astype(np.float64) - ref_n).max() <= R.KERNEL_TOL_NORMAL
    ref_c2w, _, ref_status, ref_rows = R.refine(maps[0], maps[1], G.numpy(), *cam[2:], min_pairs=0.0, **kw)
    stats = icp.last_stats().numpy()
    print(f'{H} x {W}: status {stats[:, 5].astype(int).tolist()}, pairs {stats[:-1, 0].astype(int).tolist()}')
    assert (stats[:, 5] == ref_rows[:, 5]).all() and (stats[:-1, 0] == ref_rows[:-1, 0]).all()
    if ref_status == R.OK:
        hold_pose(icp.c2w_out.cpu().numpy(), ref_c2w, f'{H} x {W}')
    else:
        assert same_bytes(icp.c2w_out, G)
    nrm = torch.from_numpy(n).to(DEV)
    for stride in (1, 2, 3):
        sums, _, _, _ = icp.step_system(G, icp.depth[0], nrm[0], icp.depth[1], nrm[1], G, stride=stride)
        ref, scale = R.step_sums(maps[0], n[0], maps[1], n[1], G.numpy(), G.numpy(), *cam[2:], stride=stride)
        got = sums.cpu().numpy()
        assert got[28] == ref[28]
        assert (np.abs(got - ref) <= R.KERNEL_TOL_SUMS * scale).all(), stride


def rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    k = [[1, 0, 0], [0, c, -s], [0, s, c]] if axis == 0 else ([[c, 0, s], [0, 1, 0], [-s, 0, c]] if axis == 1 else [[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return np.asarray(k)


@pytest.mark.parametrize('branch', ['trace', 'x', 'y', 'z', 'negative_r', 'scaled_axes'])
def test_cam_out_follows_get_tensor_from_camera(world, branch):
    """adfp_icp_end's quaternion against common.get_tensor_from_camera on c2w_out, for rotations that reach the trace branch and each
    of the three largest-diagonal branches (a turn of 3 rad about x, y, z: trace -0.98), one whose raw r is negative, and one whose
    axes are not unit length (the rule normalises them).  An all-zero depth makes the step FEW_PAIRS, so c2w_out is the guess."""
    sc, vol, bnds, icp, _ = world
    tilt = rot(1, 0.05) @ rot(2, -0.04)
    Rm = {'trace': rot(0, 0.4) @ rot(1, -0.7), 'x': rot(0, 3.0) @ tilt, 'y': rot(1, 3.0) @ tilt, 'z': rot(2, 3.0) @ tilt,
          'negative_r': rot(2, -3.0) @ rot(0, 0.3), 'scaled_axes': (rot(0, 0.4) @ rot(2, 2.9)) * np.array([1.001, 0.999, 1.0005])}[branch]
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = Rm, (0.3, -1.2, 2.5)
    Rn = Rm / np.linalg.norm(Rm, axis=0)
    tr = np.trace(Rn)
    want = {'trace': tr > 0, 'x': tr <= 0 and np.argmax(np.diag(Rn)) == 0, 'y': tr <= 0 and np.argmax(np.diag(Rn)) == 1,
            'z': tr <= 0 and np.argmax(np.diag(Rn)) == 2}
    assert want.get(branch, True)
    G = torch.from_numpy(M.astype(np.float32))
    zd, zn = torch.zeros((48, 64), device=DEV), torch.zeros((48, 64, 3), device=DEV)
    _, row, c2w, cam = icp.step_system(G, zd, zn, zd, zn, G)
    assert row[5].item() == R.FEW_PAIRS and same_bytes(c2w, G)
    ref = common.get_tensor_from_camera(c2w.cpu())
    print(branch, cam.cpu().tolist())
    assert (cam.cpu() - ref).abs().max().item() <= 2.0 ** -23 and cam[0].item() >= 0
    assert np.abs(cam.cpu().numpy() - R.camera_tensor(c2w.cpu().numpy())).max() <= 2.0 ** -23
    assert abs(float((cam[:4].double() ** 2).sum()) - 1) < 1e-6


def test_steps_replay_in_a_captured_graph(world):
    sc, vol, bnds, _, cases = world
    icp = DepthICP(vol, bnds, *CAM)
    eager = []
    for c in (cases[1], cases[6]):
        icp.refine(torch.from_numpy(c['G']), c['ds'])
        eager.append((icp.cam_out.clone(), icp.c2w_out.clone(), icp.stats.clone()))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        icp.run_steps()
    for k in (0, 1, 0):
        c = (cases[1], cases[6])[k]
        icp.set_frame(torch.from_numpy(c['G']), c['ds'])
        icp.stats.zero_(); icp.cam_out.zero_(); icp.c2w_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip((icp.cam_out, icp.c2w_out, icp.stats), eager[k]):
            assert same_bytes(a, b)
    assert eager[0][2][-1, 5].item() == R.OK and not same_bytes(eager[0][0], eager[1][0])


def test_shares_the_renderers_engine_and_follows_the_volume(world):
    """One Engine for the Renderer and the ICP's raycaster; a write to the volume that PyTorch sees (what --prior online does) bumps
    its version counter, and the next refinement raycasts the new volume through a rebuilt empty-space bitmap."""
    sc, _, bnds, _, cases = world
    vol = sc.tsdf_volume.to(DEV).clone()
    scd = synthetic.mini_scene(device=DEV)
    rend = A.Renderer(make_cfg(32, 16), None, scd)
    icp = DepthICP(vol, bnds, *CAM, engine=rend._engine)
    assert icp.raycaster._engine is rend._engine
    c = cases[0]
    icp.refine(torch.from_numpy(c['G']), c['ds'])
    assert icp.last_status() == R.OK
    first = rend._engine._tsdf_bricks[1]
    vol.fill_(1.0)                                                   # no surface any more
    icp.refine(torch.from_numpy(c['G']), c['ds'])
    assert icp.last_status() == R.FEW_PAIRS and not bool(icp.depth[1].any())
    assert rend._engine._tsdf_bricks[1] is not first
    rend.invalidate_tsdf()
    assert rend._engine._tsdf_bricks is None
    assert icp_module.STATUS_NAMES[icp.last_status()] == 'few_pairs'
