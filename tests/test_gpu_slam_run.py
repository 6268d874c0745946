"""GPU: the whole run (attentive_dfprior_amd.run / slam) on an analytic sequence, through the CLI's entry point.

The sequence: a camera inside the axis-aligned box room [0, 3]^3, 8 poses on a short arc, 48 x 64 pixels.  Depth is the z of the
ray / box exit in closed form (numpy f64), colour a smooth function of the hit point; the files are Replica's (frame*.jpg, 16-bit
depth*.png at 6553.5, traj.txt in the OpenCV camera) written with PIL.  The prior volume is fused here with fusion.TSDFVolume at
4/64 m voxels from the true poses.  Dataset and prior are made once per module and only read.

Config (the issue's worked example): every_frame 2, keyframe_every 4, ckpt_freq 4, mesh_freq 4, iters_first 6, iters 5, ratios
0.4 / 0.6, window 3, color_refine and eval_rec on, 240 mapping pixels (divisible by every window length), 4 tracking iterations
of 128 pixels, 16 + 8 samples, grids 0.32 / 0.16 / 0.16, meshing resolution 32.  The decoders are seed-initialised, so no test
asserts a tracking-quality threshold.

Bounds: 1e-5 on orthonormality and on the tracking.iters: 0 recursion -- float32 4 x 4 products on entries <= 4 (a few 2^-24 x 4
x 4 terms = 1e-6 per product) and one float32 unit-quaternion round trip per frame (a few 2^-24 per entry), over 7 frames."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

from attentive_dfprior_amd import config, datasets, fusion, mesh, render_eval, render_views, run, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT = os.path.join(HERE, 'golden', 'configs', 'df_prior.yaml')
N_IMG, H, W, FX, FY, CX, CY = 8, 48, 64, 40.0, 40.0, 31.5, 23.5
ROOM = 3.0
BOUND = [[-0.5, 3.5]] * 3
PNG = 6553.5
VOXEL = 4.0 / 64


def pose_cv(k):
    """OpenCV camera-to-world of frame k: on an arc around the room's centre, looking outward and slightly down."""
    a = 0.25 + 0.08 * k
    eye = np.array([1.5 + 0.3 * np.cos(a), 1.5 + 0.3 * np.sin(a), 1.4 + 0.02 * k])
    f = np.array([np.cos(a + 0.4), np.sin(a + 0.4), -0.15])
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, d, f, eye
    return m


def frame_images(c2w):
    """(depth [H,W] f64 metres, colour [H,W,3] uint8) of the box room from an OpenCV pose, in closed form."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones_like(u)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide='ignore'):
        t = np.where(d > 0, (ROOM - o) / d, np.where(d < 0, (0.0 - o) / d, np.inf)).min(-1)      # the ray's exit; z-depth, as d_z = 1
    hit = o + t[..., None] * d
    color = 0.5 + 0.4 * np.sin(hit * np.array([1.3, 1.7, 2.1]) + np.array([0.0, 1.0, 2.0]))
    return t, np.clip(np.rint(color * 255), 0, 255).astype(np.uint8)


def scene_cfg(root, out, **over):
    scene = {'dataset': 'replica', 'verbose': False, 'low_gpu_mem': False, 'pretrained_decoders': {'low_high': None},
             'data': {'dataset': 'replica', 'id': 'box', 'input_folder': root, 'output': out},
             'cam': {'H': H, 'W': W, 'fx': FX, 'fy': FY, 'cx': CX, 'cy': CY, 'png_depth_scale': PNG, 'crop_edge': 0},
             'grid_len': {'low': 0.32, 'high': 0.16, 'color': 0.16, 'bound_divisible': 0.32},
             'meshing': {'resolution': 32, 'eval_rec': True},
             'rendering': {'N_samples': 16, 'N_surface': 8},
             'tracking': {'iters': 4, 'pixels': 128, 'gt_camera': False, 'ignore_edge_W': 4, 'ignore_edge_H': 4},
             'mapping': {'bound': BOUND, 'marching_cubes_bound': BOUND, 'every_frame': 2, 'keyframe_every': 4, 'ckpt_freq': 4, 'mesh_freq': 4,
                         'no_log_on_first_frame': True, 'no_mesh_on_first_frame': True, 'iters_first': 6, 'iters': 5,
                         'low_iter_ratio': 0.4, 'high_iter_ratio': 0.6, 'mapping_window_size': 3, 'color_refine': True, 'pixels': 240}}
    for section, values in over.items():
        scene[section].update(values)
    return scene


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """The dataset directory, the prior's two files, the true poses (renderer's convention, what the loader hands out)."""
    from PIL import Image
    base = tmp_path_factory.mktemp('slam')
    root = str(base / 'box')
    os.makedirs(os.path.join(root, 'results'))
    lines = []
    for k in range(N_IMG):
        c2w = pose_cv(k)
        depth, color = frame_images(c2w)
        assert 0.5 < depth.min() and depth.max() < 4.0
        Image.fromarray(color).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(np.clip(np.rint(depth * PNG), 0, 65535).astype(np.uint16)).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
        lines.append(' '.join(repr(float(x)) for x in c2w.reshape(-1)))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    cfg = full_cfg(base, scene_cfg(root, str(base / 'unused')), 'world')[0]
    ds = datasets.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device=DEV)
    colors, depths, _ = ds.frames(range(N_IMG))
    gt = torch.stack([ds.pose(k) for k in range(N_IMG)])
    bound = synthetic.scene_bound(BOUND, 0.32, 1).numpy()
    vol = prior_of(bound, [(colors[k], depths[k], gt[k]) for k in range(N_IMG)])
    tsdf, bnds = vol.get_render_volume()
    vol_path, bnds_path = str(base / 'box_tsdf_volume.pt'), str(base / 'box_bounds.pt')
    torch.save(tsdf.cpu(), vol_path)
    torch.save(bnds.numpy(), bnds_path)
    return SimpleNamespace(base=base, root=root, vol=vol_path, bnds=bnds_path, gt=gt, colors=colors, depths=depths, bound=bound)


def prior_of(bound, frames):
    """What --prior online does, by hand: the frames into an empty volume over the scene bound, in order."""
    vol = fusion.TSDFVolume(bound, voxel_size=VOXEL, device=DEV)
    K = np.array([[FX, 0., CX], [0., FY, CY], [0., 0., 1.]])
    for color, depth, c2w in frames:
        m = c2w.numpy().copy()
        m[:3, 1] *= -1.0
        m[:3, 2] *= -1.0
        vol.integrate(torch.floor(color * 255), depth, K, m, obs_weight=1.)
    return vol


def full_cfg(base, scene, name):
    path = str(base / f'{name}.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(scene, f)
    return config.load_config(path, DEFAULT), path


def go(world, name, extra=(), **over):
    out = str(world.base / name)
    cfg, path = full_cfg(world.base, scene_cfg(world.root, out, **over), name)
    argv = [path, '--default_config', DEFAULT, '--seed', '0'] + list(extra)
    if '--prior' not in extra:
        argv += ['--tsdf_volume', world.vol, '--tsdf_bounds', world.bnds]
    slam = run.main(argv)
    torch.cuda.synchronize()
    return slam, cfg, out


def files_of(out):
    return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)


def test_the_worked_example_completes(world):
    slam, cfg, out = go(world, 'main')
    assert slam.mapper.keyframe_list == [0, 4, 6] and slam.mapper.keyframe_store.ids == [0, 4, 6]
    assert sorted(os.listdir(os.path.join(out, 'ckpts'))) == ['00004.tar', '00007.tar']
    est = slam.estimate_c2w_list
    assert est.device.type == 'cpu' and est.dtype == torch.float32 and tuple(est.shape) == (N_IMG, 4, 4)
    assert est[0].view(torch.int32).equal(world.gt[0].view(torch.int32))
    assert torch.equal(slam.gt_c2w_list, world.gt)
    assert torch.equal(est[:, 3, :], torch.tensor([[0., 0., 0., 1.]]).repeat(N_IMG, 1)) and torch.isfinite(est).all()
    R = est[:, :3, :3].double()
    err = (R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max().item()
    print('orthonormality of the tracked rotations: max |R^T R - I| =', err)
    assert err <= 1e-5
    assert slam.ate['compared_pose_pairs'] == N_IMG and np.isfinite(slam.ate['absolute_translational_error.rmse'])
    assert os.path.exists(os.path.join(out, 'eval_ate.json'))

    args = SimpleNamespace(input_folder=None, tsdf_volume=None, tsdf_bounds=world.bnds)
    ckpt = render_eval.newest_checkpoint(out)
    assert os.path.basename(ckpt) == '00007.tar'
    summary, frames, chosen = render_eval.eval_render(cfg, args, ckpt, every=2, device=DEV)
    assert chosen == [0, 2, 4, 6] and summary['n_frames'] == 4
    assert all(np.isfinite(summary[k]) for k in ('psnr', 'ssim', 'depth_l1')), summary
    renderer, decoders, c, tsdf_volume, tsdf_bnds = render_views.load_run(cfg, args, ckpt, device=DEV)
    assert set(c) == {'grid_low', 'grid_high', 'grid_color'} and all(torch.equal(c[k], slam.shared_c[k]) for k in c)
    assert torch.equal(tsdf_volume, slam.tsdf_volume_shared)
    ck = torch.load(ckpt, map_location='cpu', weights_only=False)
    assert ck['keyframe_list'] == [0, 4, 6] and ck['idx'] == 7 and torch.equal(ck['estimate_c2w_list'], est)

    meshes = sorted(os.listdir(os.path.join(out, 'mesh')))
    assert set(meshes) <= {'00004_mesh.ply', '00007_mesh.ply', 'final_mesh.ply', 'final_mesh_eval_rec.ply'}
    assert ('00007_mesh.ply' in meshes) == ('final_mesh.ply' in meshes)
    for name in meshes:                                    # an empty level set is the Mesher's printed notice, not a failure
        m = mesh.read_ply(os.path.join(out, 'mesh', name))
        assert len(m.faces) > 0 and len(m.verts) > 0, name


@pytest.fixture(scope='module')
def gt_camera_runs(world):
    """gt_camera with tracking.iters 0 and mapping on, decoded ahead and not: the same seed."""
    over = {'tracking': {'gt_camera': True, 'iters': 0}}
    a = go(world, 'ahead', **over)
    b = go(world, 'not_ahead', extra=['--no_prefetch'], **over)
    return a, b


def test_gt_camera_keeps_the_ground_truth(world, gt_camera_runs):
    (slam, _, _), _ = gt_camera_runs
    assert slam.estimate_c2w_list.view(torch.int32).equal(slam.gt_c2w_list.view(torch.int32))
    assert slam.gt_c2w_list.view(torch.int32).equal(world.gt.view(torch.int32))
    assert slam.ate['compared_pose_pairs'] == N_IMG


def test_gt_camera_ate_is_exactly_zero(gt_camera_runs):
    """With gt_camera the two pose lists are equal bit for bit (the test above), and eval_ate.align returns the identity bit for
    bit for identical trajectories (Horn's 4 x 4 matrix decouples exactly; tests/test_eval_ate.py), so every error is 0.0."""
    (slam, _, _), _ = gt_camera_runs
    print('gt_camera: ATE', slam.ate)
    assert slam.ate['absolute_translational_error.rmse'] == 0.0


def test_decode_ahead_changes_nothing(gt_camera_runs):
    (a, _, out_a), (b, _, out_b) = gt_camera_runs
    assert a.feed.prefetch and not b.feed.prefetch and a.feed.frames == b.feed.frames == N_IMG
    assert a.estimate_c2w_list.numpy().tobytes() == b.estimate_c2w_list.numpy().tobytes()
    assert a.mapper.keyframe_list == b.mapper.keyframe_list == [0, 4, 6]
    assert files_of(out_a) == files_of(out_b) and 'ckpts/00007.tar' in files_of(out_a)
    # the maps themselves are not compared: the Mapper's gradient scatter uses float atomics, so two runs of the SAME command
    # already differ in the grids' last bits (tests/test_gpu_mapper_iteration.py: "the atomics' order tells")


def test_zero_tracking_iterations_keep_the_constant_speed_guess(world):
    slam, _, _ = go(world, 'iters0', tracking={'iters': 0}, mapping={'mesh_freq': 100, 'color_refine': False}, meshing={'eval_rec': False})
    ref = [world.gt[0].double(), world.gt[0].double()]
    for k in range(2, N_IMG):
        ref.append(ref[k - 1] @ torch.linalg.inv(ref[k - 2]) @ ref[k - 1])
    err = (slam.estimate_c2w_list.double() - torch.stack(ref)).abs().max().item()
    print('tracking.iters 0: max |estimate - f64 constant-speed recursion| =', err)
    assert err <= 1e-5
    assert slam.tracker._it is None                        # no iteration was ever built


def test_online_prior_with_the_true_poses(world):
    slam, _, out = go(world, 'online_gt', extra=['--prior', 'online', '--prior_voxel_size', str(VOXEL)], tracking={'gt_camera': True})
    want = prior_of(world.bound, [(world.colors[k], world.depths[k], world.gt[k]) for k in (0, 2, 4, 6, 7)])
    for name in ('_tsdf', '_weight', '_color'):
        assert torch.equal(getattr(slam.prior, name), getattr(want, name)), name
    tsdf, bnds = want.get_render_volume()
    assert torch.equal(slam.tsdf_volume_shared, tsdf) and torch.equal(slam.tsdf_bnds.cpu(), bnds)
    assert slam.tsdf_volume_shared.data_ptr() == slam.prior._tsdf.data_ptr()           # the run's volume IS the prior's view
    assert int((want._weight > 0).sum()) > 1000
    ck = torch.load(os.path.join(out, 'ckpts', '00007.tar'), map_location='cpu', weights_only=False)
    assert ck['tsdf_volume'].shape == tsdf.shape and torch.equal(ck['tsdf_volume'], tsdf.cpu())
    ck4 = torch.load(os.path.join(out, 'ckpts', '00004.tar'), map_location='cpu', weights_only=False)
    early = prior_of(world.bound, [(world.colors[k], world.depths[k], world.gt[k]) for k in (0, 2, 4)])
    assert torch.equal(ck4['tsdf_volume'], early.get_render_volume()[0].cpu())         # ... as it stood when frame 4 was logged


def test_online_prior_with_tracked_poses(world):
    slam, _, _ = go(world, 'online', extra=['--prior', 'online', '--prior_voxel_size', str(VOXEL)])
    assert torch.isfinite(slam.estimate_c2w_list).all()
    assert int((slam.prior._weight > 0).sum()) > 0
    assert slam.tracker._it is not None and slam.tracker._it.tsdf is slam.tsdf_volume_shared
    assert slam.mapper.keyframe_list == [0, 4, 6]
