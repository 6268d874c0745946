"""GPU: the RGB-D ICP (adfp_rgbd_frame_map, adfp_rgbd_step, icp.RgbdICP) against its restatement (tests/rgbd_icp_ref.py) on the mini
scene (TSDF 40 x 40 x 32, 48 x 64 pixels) and on images of a few pixels.

The bars are rgbd_icp_ref's KERNEL_TOL_* = 8 x the float32-against-float64 differences tests/test_rgbd_icp_host.py measures.  The
restatement is fed the device's own downloaded maps (the raycast's depth images, the frame maps), so that what is compared is the
step and not the raycast.  Colours are test_gpu_slam_run's rule at every pixel's world point (rgbd_icp_ref.color_of)."""
import numpy as np
import pytest
import torch

import icp_ref as R
import rgbd_icp_ref as G
from attentive_dfprior_amd import _lib
from attentive_dfprior_amd.icp import DepthICP, RgbdICP
from attentive_dfprior_amd.tsdf_raycast import TsdfRaycaster

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAM = (48, 64, 57.76, 57.76, 31.5, 23.5)           # the mini scene's camera
INTR = CAM[2:]
ONE_SIDED = 1e-3                                   # pair counts: at most 0.1 % (test_gpu_icp.py's cap)


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def view(rc, c2w, cam=CAM):
    """-> (depth [H,W] on the device, colour [H,W,3] on the device) of the scene seen from c2w"""
    d = rc.render_depth(torch.from_numpy(np.asarray(c2w, dtype=np.float32)), *cam)
    return d, dev(G.color_of(d.cpu().numpy(), c2w, *cam[2:]))


def hold_pose(got, ref, what):
    m, r = R.pose_error(got, ref)
    print(f'{what}: {m:.3e} m {r:.3e} rad from the restatement (limits {G.KERNEL_TOL_POSE_M:.1e}, {G.KERNEL_TOL_POSE_RAD:.1e})')
    assert m <= G.KERNEL_TOL_POSE_M and r <= G.KERNEL_TOL_POSE_RAD, what


@pytest.fixture(scope='module')
def world():
    """The scene on the device and the nine (true pose, guess) cases with their keyframe CASE_KEY_SCALE away: per case the device's
    maps, downloaded once and only read."""
    sc = synthetic_scene()
    vol, bnds = sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV)
    rc = TsdfRaycaster(vol, bnds)
    icp = RgbdICP(vol, bnds, *CAM)
    cases = []
    for P, Gs in R.scene_cases(sc):
        K = G.key_pose(P, G.CASE_KEY_SCALE)
        ds, cs = view(rc, P)
        dk, ck = view(rc, K)
        icp.set_frame(torch.from_numpy(Gs), ds)
        cur, key = icp.frame_map(cs, ds), icp.frame_map(ck, dk)
        cases.append(dict(P=P, G=Gs, K=K, depth=icp.depth.cpu().numpy(), normals=icp.normals.cpu().numpy(), cur=cur.cpu().numpy(),
                          key=key.cpu().numpy()))
    return sc, vol, bnds, rc, icp, cases


def synthetic_scene():
    from attentive_dfprior_amd import synthetic
    return synthetic.mini_scene()


def one_step(icp, c, stride=1, key=True, normals_m=None, T=None):
    """step_system_rgbd on a case's maps from the guess -> the five outputs"""
    Gs = torch.from_numpy(c['G'] if T is None else T)
    nm = c['normals'][1] if normals_m is None else normals_m
    return icp.step_system_rgbd(Gs, dev(c['cur']), dev(c['normals'][0]), dev(c['depth'][1]), dev(nm), torch.from_numpy(c['G']),
                                key_map=dev(c['key']) if key else None, p_key=torch.from_numpy(c['K']) if key else None, stride=stride)


def ref_step(c, stride=1, key=True, normals_m=None, **kw):
    nm = c['normals'][1] if normals_m is None else normals_m
    return G.step_sums(c['cur'], c['normals'][0], c['depth'][1], nm, c['G'], c['key'] if key else None, c['K'] if key else None, c['G'],
                       *INTR, stride=stride, **kw)


@pytest.mark.parametrize('H,W', [(48, 64), (3, 5)])
def test_frame_map_against_the_restatement(world, H, W):
    sc, vol, bnds, rc, _, cases = world
    icp = RgbdICP(vol, bnds, H, W, *INTR)
    rng = np.random.default_rng(H)
    color = rng.random((H, W, 3), dtype=np.float32)
    depth = cases[0]['depth'][0][:H, :W].copy()
    color[1, 2, 0] = np.nan                                        # an inner pixel: its I and four neighbours' differences
    color[0, 0, 2] = np.nan                                        # a corner: its I, its right neighbour's gx is 0 on the border
    depth[1, 1] = 0.0
    got = icp.frame_map(dev(color), dev(depth)).cpu().numpy()
    ref = G.frame_map(color, depth)
    assert got.shape == (H, W, 4) and got.dtype == np.float32
    assert got[..., 3].tobytes() == depth.tobytes()                # the depth's own bits
    assert not got[:, 0, 1].any() and not got[:, -1, 1].any() and not got[0, :, 2].any() and not got[-1, :, 2].any()
    assert (np.isnan(got) == np.isnan(ref)).all() and np.isnan(got[1, 2, 0]) and np.isnan(got[0, 0, 0]) and int(np.isnan(got).sum()) >= 4
    ok = ~np.isnan(ref)
    worst = float(np.abs(got[ok].astype(np.float64) - ref[ok]).max())
    print(f'frame map {H} x {W}: max |diff| {worst:.3e} (limit {G.KERNEL_TOL_MAP:.1e})')
    assert worst <= G.KERNEL_TOL_MAP


@pytest.mark.parametrize('stride', [1, 2])
def test_one_step_sums_against_the_restatement(world, stride):
    sc, vol, bnds, rc, icp, cases = world
    worst = 0.0
    for k, c in enumerate(cases):
        sums, row, rgb_row, _, _ = one_step(icp, c, stride)
        ref, scale = ref_step(c, stride)
        got = sums.cpu().numpy()
        for q in (28, 30):
            assert abs(got[q] - ref[q]) <= ONE_SIDED * ref[q] and ref[q] > 0.8 * icp.strided_pixels(stride), (k, q)
        worst = max(worst, float((np.abs(got - ref) / scale).max()))
        assert row[0].item() == got[28] and row[5].item() == R.OK and rgb_row[0].item() == got[30]
        assert abs(rgb_row[1].item() - np.sqrt(got[29] / got[30])) <= 1e-15
    print(f'one joint step, stride {stride}: max |sum - ref| / scale {worst:.3e} (limit {G.KERNEL_TOL_SUMS:.1e})')
    assert worst <= G.KERNEL_TOL_SUMS


@pytest.mark.parametrize('stride', [1, 2])
def test_without_the_term_the_step_is_the_depth_step_byte_for_byte(world, stride):
    """key_map = NULL, and rgb_weight 0 with a keyframe given: sums 0..28 and the pose after the step are DepthICP.step_system's."""
    sc, vol, bnds, rc, icp, cases = world
    plain = DepthICP(vol, bnds, *CAM)
    zero = RgbdICP(vol, bnds, *CAM, rgb_weight=0.0)
    for c in cases[::4]:
        Gs = torch.from_numpy(c['G'])
        d, n = dev(c['depth']), dev(c['normals'])
        want, want_row, want_c2w, want_cam = plain.step_system(Gs, dev(c['cur'][..., 3]), n[0], d[1], n[1], Gs, stride=stride)
        for obj, key in ((icp, False), (zero, True)):
            sums, row, rgb_row, c2w, cam = one_step(obj, c, stride, key=key)
            assert same_bytes(sums[:29], want) and not bool(sums[29:].any()) and not bool(rgb_row.any())
            assert same_bytes(row, want_row) and same_bytes(c2w, want_c2w) and same_bytes(cam, want_cam)
        joint = one_step(icp, c, stride)[0]
        assert not same_bytes(joint[:27], want[:27]) and same_bytes(joint[27:29], want[27:29])      # the term does change the system


def test_model_normals_all_zero_leaves_the_photometric_sums(world):
    sc, vol, bnds, rc, icp, cases = world
    zn = np.zeros((48, 64, 3), dtype=np.float32)
    for c in cases[1::3]:
        sums, row, rgb_row, _, _ = one_step(icp, c, normals_m=zn)
        ref, scale = ref_step(c, normals_m=zn)
        got = sums.cpu().numpy()
        assert got[27] == 0 and got[28] == 0 and ref[28] == 0 and row[0].item() == 0
        assert abs(got[30] - ref[30]) <= ONE_SIDED * ref[30] and ref[30] > 0.8 * 48 * 64
        keep = scale > 0
        assert keep[:27].all() and (np.abs(got - ref)[keep] <= G.KERNEL_TOL_SUMS * scale[keep]).all()


def degenerate_view(world, scale):
    sc, vol, bnds, rc, _, _ = world
    P = sc.default_c2w().numpy()
    Gd = (R.exp_se3(np.asarray(R.TWIST) * scale) @ P.astype(np.float64)).astype(np.float32)
    K = G.key_pose(P)
    return P, Gd, K, view(rc, P), view(rc, K)


@pytest.mark.parametrize('scale', R.SCALES)
def test_the_degenerate_view_goes_through(world, scale):
    """The headline: the scene's default pose, where the depth ICP returns the guess with DEGENERATE."""
    sc, vol, bnds, rc, _, _ = world
    P, Gd, K, (ds, cs), (dk, ck) = degenerate_view(world, scale)
    plain = DepthICP(vol, bnds, *CAM)
    plain.refine(torch.from_numpy(Gd), ds)
    assert plain.last_status() == R.DEGENERATE and same_bytes(plain.c2w_out, torch.from_numpy(Gd))
    icp = RgbdICP(vol, bnds, *CAM)
    icp.set_keyframe(torch.from_numpy(K), ck, dk)
    cam = icp.refine(torch.from_numpy(Gd), ds, cs)
    got, stats, rgb = icp.c2w_out.cpu().numpy(), icp.last_stats().numpy(), icp.last_rgb_stats().numpy()
    ref_c2w, _, ref_status, ref_rows, ref_rgb = G.refine(icp.maps[0].cpu().numpy(), icp.depth[1].cpu().numpy(), icp.maps[1].cpu().numpy(), K, Gd, *INTR)
    e0, e1 = R.pose_error(Gd, P), R.pose_error(got, P)
    print(f'scale {scale}: {e0[0] * 1e3:.2f} mm {e0[1] * 1e3:.2f} mrad -> {e1[0] * 1e3:.4f} mm {e1[1] * 1e3:.4f} mrad, pivot ratio '
          f'{stats[:-1, 2].min():.2e}, last step {stats[-2, 0]:.0f} geometric and {rgb[-2, 0]:.0f} photometric pairs, rmse {rgb[-2, 1]:.2e}')
    assert ref_status == R.OK == icp.last_status() and (stats[:, 5] == R.OK).all() and stats.shape == (11, 6) and rgb.shape == (11, 2)
    assert (np.abs(stats[:-1, 0] - ref_rows[:-1, 0]) <= np.maximum(ONE_SIDED * ref_rows[:-1, 0], 1)).all()
    assert (np.abs(rgb[:-1, 0] - ref_rgb[:-1, 0]) <= np.maximum(ONE_SIDED * ref_rgb[:-1, 0], 1)).all() and not rgb[-1].any()
    hold_pose(got, ref_c2w, f'degenerate view, scale {scale}')
    assert e1[0] <= e0[0] / 10 and e1[1] <= e0[1] / 10
    assert (stats[:-1, 2] > 100 * icp.min_pivot).all()
    assert np.abs(cam.cpu().numpy() - R.camera_tensor(got)).max() <= 2.0 ** -23


def test_an_empty_model_image_is_ok_on_photometric_pairs_alone(world):
    sc, vol, bnds, rc, _, _ = world
    P, Gd, K, (ds, cs), (dk, ck) = degenerate_view(world, 0.5)
    plain = DepthICP(torch.ones_like(vol), bnds, *CAM)
    plain.refine(torch.from_numpy(Gd), ds)
    assert plain.last_status() == R.FEW_PAIRS and not bool(plain.depth[1].any())
    icp = RgbdICP(torch.ones_like(vol), bnds, *CAM)
    icp.set_keyframe(torch.from_numpy(K), ck, dk)
    icp.refine(torch.from_numpy(Gd), ds, cs)
    stats, rgb = icp.last_stats().numpy(), icp.last_rgb_stats().numpy()
    assert not bool(icp.depth[1].any()) and (stats[:, 5] == R.OK).all() and (stats[:-1, :2] == 0).all() and (rgb[:-1, 0] > 100).all()
    ref_c2w, _, ref_status, _, ref_rgb = G.refine(icp.maps[0].cpu().numpy(), np.zeros((48, 64), np.float32), icp.maps[1].cpu().numpy(), K, Gd, *INTR)
    assert ref_status == R.OK and (np.abs(rgb[:-1, 0] - ref_rgb[:-1, 0]) <= np.maximum(ONE_SIDED * ref_rgb[:-1, 0], 1)).all()
    got = icp.c2w_out.cpu().numpy()
    hold_pose(got, ref_c2w, 'empty model image')
    e0, e1 = R.pose_error(Gd, P), R.pose_error(got, P)
    print(f'photometric pairs alone: {e0[0] * 1e3:.2f} mm -> {e1[0] * 1e3:.3f} mm')
    assert e1[0] < e0[0] and not same_bytes(icp.c2w_out, torch.from_numpy(Gd))
    # and before any keyframe is set the same object is the depth rule: FEW_PAIRS
    fresh = RgbdICP(torch.ones_like(vol), bnds, *CAM)
    fresh.refine(torch.from_numpy(Gd), ds, cs)
    assert fresh.last_status() == R.FEW_PAIRS and same_bytes(fresh.c2w_out, torch.from_numpy(Gd)) and not bool(fresh.rgb_stats.any())


def small_case(world, H, W, volume=None, **kw):
    """The mini scene through an H x W image of the same field of view from the first corner pose: the guess half the twist off, the
    keyframe CASE_KEY_SCALE away.  -> (RgbdICP with the frame and the keyframe set, camera, guess, keyframe pose, depth, colour)"""
    sc, vol, bnds, rc, _, _ = world
    cam = (H, W, 57.76 * W / 64, 57.76 * W / 64, (W - 1) / 2, (H - 1) / 2)
    offset, yaw, pitch = R.POSES[0]
    P = sc.default_c2w(offset=offset, yaw=yaw, pitch=pitch).numpy()
    Gs = (R.exp_se3(np.asarray(R.TWIST) * 0.5) @ P.astype(np.float64)).astype(np.float32)
    K = G.key_pose(P, G.CASE_KEY_SCALE)
    icp = RgbdICP(vol if volume is None else volume, bnds, *cam, **kw)
    (ds, cs), (dk, ck) = view(rc, P, cam), view(rc, K, cam)
    assert bool((ds > 0).all()) and bool((dk > 0).all())
    icp.set_keyframe(torch.from_numpy(K), ck, dk)
    return icp, cam, Gs, K, ds, cs


def small_step(icp, cam, Gs, K, stride):
    """One joint step on the maps the object holds against the restatement on their downloads -> (got [31], ref [31], scale [31])"""
    sums = icp.step_system_rgbd(torch.from_numpy(Gs), icp.maps[0], icp.normals[0], icp.depth[1], icp.normals[1], torch.from_numpy(Gs),
                                key_map=icp.maps[1].clone(), p_key=torch.from_numpy(K), stride=stride)[0]
    ref, scale = G.step_sums(icp.maps[0].cpu().numpy(), icp.normals[0].cpu().numpy(), icp.depth[1].cpu().numpy(), icp.normals[1].cpu().numpy(),
                             Gs, icp.maps[1].cpu().numpy(), K, Gs, *cam[2:], stride=stride, dist_tol=icp.dist_tol)
    return sums.cpu().numpy(), ref, scale


@pytest.mark.parametrize('H,W', [(3, 8), (8, 3)])
def test_three_rows_or_columns_form_no_footprint(world, H, W):
    """1 <= u0 <= W - 3 and 1 <= v0 <= H - 3 leave nothing: no photometric pair, so the refinement is the depth ICP's byte for byte,
    and FEW_PAIRS where the model image is empty."""
    sc, vol, bnds, rc, _, _ = world
    one = dict(strides=(1,), iters=(2,), min_pairs=0.0)
    icp, cam, Gs, K, ds, cs = small_case(world, H, W, **one)
    icp.refine(torch.from_numpy(Gs), ds, cs)
    plain = DepthICP(vol, bnds, *cam, **one)
    plain.refine(torch.from_numpy(Gs), ds)
    assert not bool(icp.rgb_stats.any()) and same_bytes(icp.stats, plain.stats) and same_bytes(icp.c2w_out, plain.c2w_out)
    assert icp.stats[0, 0].item() > 0                               # geometric pairs there were
    empty, _, _, _, _, _ = small_case(world, H, W, volume=torch.ones_like(vol))
    empty.refine(torch.from_numpy(Gs), ds, cs)
    stats = empty.last_stats().numpy()
    assert (stats[:, 5] == R.FEW_PAIRS).all() and (stats[:, :5] == 0).all() and not bool(empty.rgb_stats.any())
    assert same_bytes(empty.c2w_out, torch.from_numpy(Gs))


def test_four_by_four_has_one_footprint_origin(world):
    """4 x 4: the footprint's origin can only be (1, 1), so only sensor points that land in [1, 2) x [1, 2) of the keyframe pair: here
    pixel (2, 2), which lands at (1.96, 1.97).  A pixel is 0.55 m wide at this size, so neighbouring depths differ by 0.1 - 0.3 m and
    the occlusion gate is opened to 1 m for the four texels to agree."""
    icp, cam, Gs, K, ds, cs = small_case(world, 4, 4, min_pairs=0.0, dist_tol=1.0)
    icp.set_frame(torch.from_numpy(Gs), ds)
    icp.frame_map(cs, ds, out=icp.maps[0])
    got, ref, scale = small_step(icp, cam, Gs, K, 1)
    idx, _, _ = G.photo_pairs(icp.maps[0].cpu().numpy(), icp.maps[1].cpu().numpy(), K, Gs, *cam[2:], dist_tol=1.0)
    print('4 x 4: photometric pairs at pixels', idx.tolist())
    assert got[30] == ref[30] == len(idx) and idx.tolist() == [2 * 4 + 2] and got[28] == ref[28]
    keep = scale > 0
    assert (np.abs(got - ref)[keep] <= G.KERNEL_TOL_SUMS * scale[keep]).all() and (got[~keep] == 0).all()


@pytest.mark.parametrize('H,W', [(16, 17), (10, 13)])
def test_small_images_against_the_restatement(world, H, W):
    """16 x 17: 272 pixels, two workgroups.  10 x 13: 130 pixels, no multiple of 64 and less than one workgroup, sides that are no
    multiple of the strides.  Strides 1, 2, 3 and one larger than the image (the single pixel (0, 0), which can form no photometric
    pair: its point lands in the keyframe's first row or column, or nearby)."""
    icp, cam, Gs, K, ds, cs = small_case(world, H, W, min_pairs=0.0)
    icp.set_frame(torch.from_numpy(Gs), ds)
    icp.frame_map(cs, ds, out=icp.maps[0])
    for stride in (1, 2, 3, 100):
        got, ref, scale = small_step(icp, cam, Gs, K, stride)
        print(f'{H} x {W}, stride {stride}: {got[28]:.0f} geometric, {got[30]:.0f} photometric pairs')
        assert got[28] == ref[28] and got[30] == ref[30]
        assert (stride == 1 and got[30] > 0.25 * H * W) or stride > 1
        assert stride < 100 or (got[30] == 0 and got[28] <= 1)
        keep = scale > 0
        assert (np.abs(got - ref)[keep] <= G.KERNEL_TOL_SUMS * scale[keep]).all() and (got[~keep] == 0).all(), stride
    icp.refine(torch.from_numpy(Gs), ds, cs)
    ref_c2w, _, ref_status, ref_rows, ref_rgb = G.refine(icp.maps[0].cpu().numpy(), icp.depth[1].cpu().numpy(), icp.maps[1].cpu().numpy(), K, Gs,
                                                         *cam[2:], min_pairs=0.0)
    stats, rgb = icp.last_stats().numpy(), icp.last_rgb_stats().numpy()
    assert (stats[:, 5] == ref_rows[:, 5]).all() and (stats[:-1, 0] == ref_rows[:-1, 0]).all() and (rgb[:, 0] == ref_rgb[:, 0]).all()
    if ref_status == R.OK:
        hold_pose(icp.c2w_out.cpu().numpy(), ref_c2w, f'{H} x {W}')
    else:
        assert same_bytes(icp.c2w_out, torch.from_numpy(Gs))


def test_two_calls_give_the_same_bytes(world):
    sc, vol, bnds, rc, _, _ = world
    P, Gd, K, (ds, cs), (dk, ck) = degenerate_view(world, 1.0)
    icp = RgbdICP(vol, bnds, *CAM)
    icp.set_keyframe(torch.from_numpy(K), ck, dk)
    outs = []
    for _ in range(2):
        cam = icp.refine(torch.from_numpy(Gd), ds, cs)
        outs.append((cam.clone(), icp.c2w_out.clone(), icp.stats.clone(), icp.rgb_stats.clone(), icp.maps.clone()))
        icp.stats.zero_(); icp.rgb_stats.zero_(); icp.c2w_out.zero_(); icp.cam_out.zero_(); icp.rgbd_workspace.zero_(); icp.maps[0].zero_()
    for a, b in zip(*outs):
        assert same_bytes(a, b)
    assert outs[0][2][-1, 5].item() == R.OK and bool((outs[0][3][:-1, 0] > 0).all())


def test_steps_replay_in_a_captured_graph_across_a_promote(world):
    """Keyframe Q0, frame 1 at P (refined, then promoted at its result), frame 2 at Q2 against frame 1: eagerly, then with run_steps
    replayed from a graph captured before frame 1.  promote copies into the buffers the graph reads, so the replays give the eager
    bytes."""
    sc, vol, bnds, rc, _, cases = world
    P = cases[0]['P']
    Q0, Q2 = G.key_pose(P, 0.5), G.key_pose(P, -0.5)
    frames = [(cases[1]['G'], view(rc, P)), ((R.exp_se3(np.asarray(R.TWIST) * 0.5) @ Q2.astype(np.float64)).astype(np.float32), view(rc, Q2))]
    d0, c0 = view(rc, Q0)
    icp = RgbdICP(vol, bnds, *CAM)

    def outputs():
        return icp.cam_out.clone(), icp.c2w_out.clone(), icp.stats.clone(), icp.rgb_stats.clone()

    eager = []
    icp.set_keyframe(torch.from_numpy(Q0), c0, d0)
    for Gs, (ds, cs) in frames:
        icp.refine(torch.from_numpy(Gs), ds, cs)
        eager.append(outputs())
        icp.promote(icp.c2w_out.clone())
    assert all(e[2][-1, 5].item() == R.OK and bool((e[3][:-1, 0] > 100).all()) for e in eager) and not same_bytes(eager[0][0], eager[1][0])
    icp.set_keyframe(torch.from_numpy(Q0), c0, d0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        icp.run_steps()
    for k, (Gs, (ds, cs)) in enumerate(frames):
        icp.set_frame(torch.from_numpy(Gs), ds)
        icp.frame_map(cs, ds, out=icp.maps[0])
        icp.stats.zero_(); icp.rgb_stats.zero_(); icp.cam_out.zero_(); icp.c2w_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outputs(), eager[k]):
            assert same_bytes(a, b), k
        icp.promote(icp.c2w_out.clone())


def test_rgb_tol_zero_keeps_only_pairs_with_no_residual(world):
    """Keyframe intensity 0 everywhere (the interpolation of zeros is exactly 0), the frame's intensity 0 on its left half and 0.1 on
    its right half: with rgb_tol 0 exactly the left half's pairs remain, and their sum of squares is 0."""
    sc, vol, bnds, rc, icp, cases = world
    c = dict(cases[4])
    cur, key = c['cur'].copy(), c['key'].copy()
    cur[..., 1:3], key[..., :3] = 0.0, 0.0
    cur[:, :32, 0], cur[:, 32:, 0] = 0.0, 0.1
    c['cur'], c['key'] = cur, key
    strict = RgbdICP(vol, bnds, *CAM, rgb_tol=0.0)
    got0 = one_step(strict, c)[0].cpu().numpy()
    got = one_step(icp, c)[0].cpu().numpy()
    ref0, _ = ref_step(c, rgb_tol=0.0)
    ref, _ = ref_step(c)
    print(f'rgb_tol 0: {got0[30]:.0f} pairs (restatement {ref0[30]:.0f}); rgb_tol 0.25: {got[30]:.0f} (restatement {ref[30]:.0f})')
    assert got0[29] == 0 and abs(got0[30] - ref0[30]) <= ONE_SIDED * ref0[30] and abs(got[30] - ref[30]) <= ONE_SIDED * ref[30]
    assert 0.3 * ref[30] < ref0[30] < 0.7 * ref[30] and abs(got[29] - float(np.float32(0.1)) ** 2 * (got[30] - got0[30])) <= 1e-12 * got[29]
    assert got0[28] == got[28]


def test_constants():
    assert (_lib.RGBD_SUMS, _lib.RGBD_STATS) == (G.SUMS, G.STATS) == (31, 2)
