"""GPU: attentive_dfprior_amd.replay on a hand-made run directory -- two cube meshes, a checkpoint of six poses, a 48 x 64 viewing
camera.  A frame must be MeshViews.render's picture of the mesh in force with tests/segments_ref.py's lines over it, byte for byte."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import segments_ref as SR
from attentive_dfprior_amd import mesh, render_mesh, replay

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAM = (48, 64, 60.0, 60.0, 31.5, 23.5)
CFG = {'scale': 1.0}
RED, GREEN, WHITE = (255, 0, 0), (0, 255, 0), (255, 255, 255)
VIEW = replay._pose(np.array([0.0, 1.5, 5.0]), np.array([0.0, 1.0, 0.0]), np.array([0.0, -1.5, -5.0]))      # behind and above, looking at the origin

CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], dtype=np.int64)


def cube(centre, side):
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64)
    return v * side + np.asarray(centre, dtype=np.float64)


def run_poses():
    """(estimated, ground truth) [6,4,4], OpenCV axes: the camera passes in front of the cubes from left to right looking at them;
    the ground truth runs 0.15 below and drifts away."""
    est = np.stack([np.eye(4)] * 6)
    est[:, 0, 3] = -1.5 + 0.6 * np.arange(6)
    est[:, 2, 3] = -2.0
    gt = est.copy()
    gt[:, 1, 3] += 0.15
    gt[:, 0, 3] += 0.05 * np.arange(6)
    return est, gt


def stored(p):
    """Poses as a checkpoint holds them: float32, columns 1 and 2 negated (render_mesh.opencv_poses undoes it)."""
    q = np.array(p, dtype=np.float64)
    q[:, :3, 1] *= -1.0
    q[:, :3, 2] *= -1.0
    return torch.from_numpy(q).float()


def make_run(root, est, gt, meshes=(0, 4)):
    os.makedirs(os.path.join(root, 'ckpts'))
    os.makedirs(os.path.join(root, 'mesh'))
    torch.save({'estimate_c2w_list': stored(est), 'gt_c2w_list': stored(gt), 'idx': len(est) - 1}, os.path.join(root, 'ckpts', '00005.tar'))
    if 0 in meshes:
        mesh.write_ply(os.path.join(root, 'mesh', '00000_mesh.ply'), cube((0.0, 0.0, 0.0), 1.0), CUBE_F)
    if 4 in meshes:
        v = np.concatenate([cube((0.0, 0.0, 0.0), 1.0), cube((1.2, 0.2, 0.5), 0.8)])
        mesh.write_ply(os.path.join(root, 'mesh', '00004_mesh.ply'), v, np.concatenate([CUBE_F, CUBE_F + 8]))
    open(os.path.join(root, 'mesh', 'final_mesh.ply'), 'w').close()              # not of the form {idx:05d}_mesh.ply: never opened
    return str(root)


def picture(path):
    return np.asarray(Image.open(path).convert('RGB'))


def expected(root, k, frames, mesh_idx, gt_traj=True, width=2.0, hidden_alpha=0.0):
    """Frame k as the parts say it must look: the mesh's render, then the restatement's lines."""
    est, gt = (render_mesh.opencv_poses(stored(p)) for p in run_poses())       # through the checkpoint's float32
    segs, colors, ranges = replay.overlay_lists(est, gt, frames, CAM, 0.2, gt_traj)
    H, W, fx, fy, cx, cy = CAM
    if mesh_idx is None:
        rgb, depth = np.full((1, H, W, 3), 255, np.uint8), None
    else:
        m = mesh.read_ply(os.path.join(root, 'mesh', f'{mesh_idx:05d}_mesh.ply'))
        r = render_mesh.MeshViews(m.verts, m.faces, None, DEV).render(VIEW[None], H, W, fx, fy, cx, cy, far=replay.FAR)
        rgb, depth = r['rgb'].cpu().numpy(), r['depth'].cpu().numpy()
    i = frames.index(k)
    out, seg = SR.draw_segments(rgb, depth, VIEW[None], fx, fy, cx, cy, segs, colors, ranges[i:i + 1], 0.5 * width, hidden_alpha=hidden_alpha)
    return out[0], seg[0], rgb[0], colors


def test_replay_writes_the_growing_mesh_with_the_lines_over_it(tmp_path):
    root = make_run(tmp_path / 'run', *run_poses())
    paths = replay.replay(CFG, root, view=VIEW, cam=CAM, device=DEV)
    assert paths == [os.path.join(root, 'replay', f'{k:05d}.png') for k in range(6)]
    frames = list(range(6))
    for p in paths:
        assert Image.open(p).size == (64, 48) and Image.open(p).mode == 'RGB'
    # frame 0: the first mesh, both frusta, no trajectory yet
    want, seg, bare, colors = expected(root, 0, frames, 0)
    got = picture(paths[0])
    assert np.array_equal(got, want)
    assert set(np.unique(seg)) <= set(range(10, 26)) | {-1} and (seg >= 10).any()      # 5 + 5 trajectory segments come first in the list
    # a later frame: the second mesh (two cubes), red exactly where the estimated trajectory and frustum are drawn
    for k, mesh_idx in ((3, 0), (5, 4)):
        want, seg, bare, colors = expected(root, k, frames, mesh_idx)
        got = picture(paths[k])
        assert np.array_equal(got, want), k
        drawn = (seg >= 0) & (want != bare).any(-1)
        is_red, is_green = (got == RED).all(-1), (got == GREEN).all(-1)
        assert np.array_equal(is_red, drawn & (colors[np.maximum(seg, 0)] == RED).all(-1)) and is_red.sum() > 20
        assert np.array_equal(is_green, drawn & (colors[np.maximum(seg, 0)] == GREEN).all(-1)) and is_green.sum() > 20
        assert ((seg >= 0) & (seg < k)).any()                                           # part of the estimated trajectory's prefix
        assert not ((seg >= k) & (seg < 5)).any() and not ((seg >= 5 + k) & (seg < 10)).any()      # and nothing beyond frame k
    assert not np.array_equal(expected(root, 5, frames, 4)[2], expected(root, 5, frames, 0)[2])    # the mesh did change at frame 4
    # the same frames through `every`, the default directory replaced
    out = str(tmp_path / 'thinned')
    paths2 = replay.replay(CFG, root, out=out, every=2, view=VIEW, cam=CAM, device=DEV, chunk=2)
    assert [os.path.basename(p) for p in paths2] == ['00000.png', '00002.png', '00004.png']
    assert np.array_equal(picture(paths2[2]), expected(root, 4, [0, 2, 4], 4)[0])


def test_no_gt_traj_leaves_no_green_and_hidden_alpha_shows_hidden_lines(tmp_path):
    root = make_run(tmp_path / 'run', *run_poses())
    paths = replay.replay(CFG, root, out=str(tmp_path / 'a'), view=VIEW, cam=CAM, gt_traj=False, device=DEV)
    for k, p in enumerate(paths):
        got = picture(p)
        assert not (got == GREEN).all(-1).any() and (got == RED).all(-1).any()
    assert np.array_equal(picture(paths[5]), expected(root, 5, list(range(6)), 4, gt_traj=False)[0])
    # from straight ahead of the cube the far part of the path lies behind it; hidden_alpha keeps it, faintly
    paths = replay.replay(CFG, root, out=str(tmp_path / 'b'), view=VIEW, cam=CAM, hidden_alpha=0.5, width=1.0, device=DEV)
    assert np.array_equal(picture(paths[5]), expected(root, 5, list(range(6)), 4, width=1.0, hidden_alpha=0.5)[0])


def test_frames_before_the_first_mesh_are_background_plus_lines(tmp_path):
    root = make_run(tmp_path / 'run', *run_poses(), meshes=(4,))
    paths = replay.replay(CFG, root, view=VIEW, cam=CAM, device=DEV)
    frames = list(range(6))
    want, seg, bare, _ = expected(root, 2, frames, None)
    got = picture(paths[2])
    assert np.array_equal(got, want) and (bare == 255).all()
    assert set(map(tuple, got.reshape(-1, 3))) == {RED, GREEN, WHITE}                 # nothing hides a line: no mesh yet
    assert np.array_equal(picture(paths[4]), expected(root, 4, frames, 4)[0])


def test_with_nothing_to_draw_a_frame_is_the_render(tmp_path):
    lost = np.full((6, 4, 4), -np.inf)                                                  # ScanNet's lost poses, in both lists
    root = make_run(tmp_path / 'run', lost, lost)
    paths = replay.replay(CFG, root, view=VIEW, cam=CAM, device=DEV)
    H, W, fx, fy, cx, cy = CAM
    for k, mesh_idx in ((1, 0), (5, 4)):
        m = mesh.read_ply(os.path.join(root, 'mesh', f'{mesh_idx:05d}_mesh.ply'))
        r = render_mesh.MeshViews(m.verts, m.faces, None, DEV).render(VIEW[None], H, W, fx, fy, cx, cy, far=replay.FAR)
        assert np.array_equal(picture(paths[k]), r['rgb'][0].cpu().numpy())


def test_vis_input_frame_pastes_the_reduced_colour_image(tmp_path):
    """A Replica-style dataset of 24 x 32 frames: into a 64-wide view the image goes at stride 2 (16 = a quarter of the width)."""
    from types import SimpleNamespace
    from attentive_dfprior_amd import datasets
    root = make_run(tmp_path / 'run', *run_poses())
    data = str(tmp_path / 'data')
    os.makedirs(os.path.join(data, 'results'))
    for k in range(6):
        color = np.random.RandomState(40 + k).randint(0, 256, (24, 32, 3), dtype=np.uint8)
        Image.fromarray(color).save(os.path.join(data, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(np.full((24, 32), 2000, np.uint16)).save(os.path.join(data, 'results', f'depth{k:06d}.png'))
    with open(os.path.join(data, 'traj.txt'), 'w') as f:
        f.write('\n'.join(' '.join(repr(float(x)) for x in np.eye(4).reshape(-1)) for _ in range(6)) + '\n')
    cfg = {'scale': 1.0, 'dataset': 'replica', 'data': {'input_folder': data, 'dataset': 'replica', 'id': 'mini'},
           'cam': {'H': 24, 'W': 32, 'fx': 30.0, 'fy': 30.0, 'cx': 15.5, 'cy': 11.5, 'png_depth_scale': 1000.0, 'crop_edge': 0}}
    args = SimpleNamespace(input_folder=None)
    plain = replay.replay(cfg, root, out=str(tmp_path / 'plain'), every=2, view=VIEW, cam=CAM, device=DEV)
    pasted = replay.replay(cfg, root, out=str(tmp_path / 'pasted'), every=2, view=VIEW, cam=CAM, vis_input_frame=True, args=args, device=DEV)
    ds = datasets.get_dataset(cfg, args, 1.0, device=DEV)
    for i, k in enumerate((0, 2, 4)):
        a, b = picture(plain[i]), picture(pasted[i])
        color = ds.frames([k])[0][0].double().cpu().numpy()
        want = np.floor(np.clip(color[::2, ::2], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        assert want.shape == (12, 16, 3) and np.array_equal(b[:12, :16], want), k
        rest = np.ones((48, 64), bool)
        rest[:12, :16] = False
        assert np.array_equal(a[rest], b[rest]) and not np.array_equal(a[:12, :16], b[:12, :16])


def test_command_line(tmp_path, capsys):
    root = make_run(tmp_path / 'run', *run_poses())
    cfg = tmp_path / 'scene.yaml'
    cfg.write_text('scale: 1\ndataset: replica\ndata:\n  output: %s\ncam:\n  H: 48\n  W: 64\n  fx: 60.0\n  fy: 60.0\n  cx: 31.5\n  cy: 23.5\n'
                   '  crop_edge: 0\n  png_depth_scale: 1000.0\n' % root)
    poses = tmp_path / 'view.txt'
    poses.write_text(' '.join(repr(float(x)) for x in VIEW.reshape(-1)) + '\n')
    out = str(tmp_path / 'frames')
    paths = replay.main([str(cfg), '--view', str(poses), '--every', '5', '--out', out, '--default_config', str(tmp_path / 'none.yaml')])
    assert [os.path.basename(p) for p in paths] == ['00000.png', '00005.png']
    assert 'ffmpeg' in capsys.readouterr().out
    view32 = render_mesh.opencv_poses(replay_read(str(poses)))[0]                      # the file is read as float32
    assert np.abs(view32 - VIEW).max() < 1e-6
    got = picture(paths[1])
    assert (got == RED).all(-1).sum() > 20 and (got == GREEN).all(-1).sum() > 20
    # the follow and overview cameras, with one mesh throughout and another line width, through the options
    for view in ('follow', 'overview'):
        paths = replay.main([str(cfg), '--view', view, '--every', '5', '--out', out + view, '--mesh', os.path.join(root, 'mesh', '00004_mesh.ply'),
                             '--width', '3', '--back', '2.0', '--up', '1.0', '--H', '32', '--cx', '20.0', '--default_config',
                             str(tmp_path / 'none.yaml')])
        assert len(paths) == 2 and Image.open(paths[1]).size == (64, 32)
        got = picture(paths[1])
        assert not (got == 255).all()
        if view == 'follow':                                       # from above the path runs under the cubes: most of it is hidden
            assert (got == RED).all(-1).sum() > 10


def replay_read(path):
    from attentive_dfprior_amd.render_views import read_poses
    return read_poses(path)
