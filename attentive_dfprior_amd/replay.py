"""Replay of a finished run: the mesh as it grew, the estimated trajectory leaving the ground-truth one and the camera's frustum,
one PNG per chosen frame.  The reference's parent project shows this in an open3d window (its visualizer.py); here a frame is a
mesh view of render_mesh.MeshViews with the lines drawn over it by render_mesh.draw_segments, depth-tested against the view's own
depth image, so lines behind walls vanish (or stay faint with --hidden_alpha) and every step of a view stays on the device.

    python -m attentive_dfprior_amd.replay CONFIG [--input_folder ..] [--output ..] [--ckpt PATH] [--mesh PATH] [--every N]
           [--view follow|overview|FILE] [--back M] [--up M] [--width PX] [--hidden_alpha A] [--no_gt_traj] [--vis_input_frame]
           [--H .. --W .. --fx .. --fy .. --cx .. --cy ..] [--out DIR]

The run directory (--output, or the config's data.output) holds ckpts/*.tar (estimate_c2w_list, gt_c2w_list, idx) and
mesh/{idx:05d}_mesh.ply every mesh_freq frames.  For every N-th frame k <= idx the newest mesh with an index <= k is rendered shaded
(frames before the first mesh show the background) from the chosen viewpoint: `follow` = behind (--back) and above (--up) the
estimated camera, looking at it; `overview` = above the last mesh's box looking down; FILE = one camera-to-world 4x4 per line as
render_views reads poses (one line: a fixed camera; else line i for the i-th chosen frame).  Over it: the estimated trajectory up to k
and the estimated camera's frustum in red, the ground-truth ones in green (not with --no_gt_traj).  --mesh uses one mesh throughout.
--vis_input_frame pastes frame k's colour image, reduced by an integer stride to at most a quarter of the width, into the top-left
corner.  The viewing camera is the config's cam block (as render_mesh reads it) unless the six options replace it.  {out}/{k:05d}.png
is written with PIL, one download per chunk of views; no video is encoded: the ffmpeg line that would join the PNGs is printed."""
import argparse
import os
import re
from types import SimpleNamespace

import numpy as np
import torch

from . import mesh as mesh_io
from . import render_mesh
from .recon_eval import viewmatrix

EST_COLOR = (255, 0, 0)
GT_COLOR = (0, 255, 0)
FRUSTUM_SEGMENTS = 8
FAR = 1.0e3                                         # metres: an overview camera stands further off than a frame's far plane


# ---- geometry helpers (numpy f64, host) ----
def trajectory_segments(c2w):
    """[n,4,4] poses -> [max(n - 1, 0),2,3]: segment i joins the camera centres of poses i and i + 1.  A segment next to a
    non-finite pose (ScanNet's -inf ground truth) stays in the list, so indices are frame numbers, and draws nothing."""
    o = np.asarray(c2w, dtype=np.float64).reshape(-1, 4, 4)[:, :3, 3]
    if len(o) < 2:
        return np.zeros((0, 2, 3))
    return np.stack([o[:-1], o[1:]], 1)


def frustum_corners(H, W, fx, fy, cx, cy, size):
    """The four corners of the image (the outer edge of the pixel grid: screen points (-0.5, -0.5) .. (W - 0.5, H - 0.5), clockwise from
    the top left) in camera space at depth `size`, OpenCV axes: [4,3]."""
    uv = np.array([[-0.5, -0.5], [W - 0.5, -0.5], [W - 0.5, H - 0.5], [-0.5, H - 0.5]], dtype=np.float64)
    return np.stack([(uv[:, 0] - cx) / fx * size, (uv[:, 1] - cy) / fy * size, np.full(4, float(size))], 1)


def frustum_segments(c2w, H, W, fx, fy, cx, cy, size):
    """The wire frustum of one camera (c2w [4,4], OpenCV axes) as [8,2,3]: four segments from the centre to the image corners at depth
    `size`, then the four sides of the rectangle between them."""
    c2w = np.asarray(c2w, dtype=np.float64).reshape(4, 4)
    with np.errstate(all='ignore'):
        corners = frustum_corners(H, W, fx, fy, cx, cy, size) @ c2w[:3, :3].T + c2w[:3, 3]
    centre = np.broadcast_to(c2w[:3, 3], (4, 3))
    return np.concatenate([np.stack([centre, corners], 1), np.stack([corners, np.roll(corners, -1, 0)], 1)], 0)


def _pose(z, down, pos):
    m = np.eye(4)
    m[:3, :] = viewmatrix(z, down, pos)                 # x = unit(down x z), y = unit(z x x): y points down, OpenCV axes
    return m


def follow_pose(c2w, back, up):
    """A third-person camera for c2w [4,4] (OpenCV axes): `back` metres behind it along its viewing direction and `up` metres
    above it (against its y axis), looking at its centre, its image upright with respect to the followed camera.  [4,4]."""
    c2w = np.asarray(c2w, dtype=np.float64).reshape(4, 4)
    if not back > 0:
        raise ValueError(f'follow_pose: back {back} must be positive')
    o, down, fwd = c2w[:3, 3], c2w[:3, 1], c2w[:3, 2]
    pos = o - back * fwd - up * down
    return _pose(o - pos, down, pos)


def overview_pose(lo, hi, cam, up_axis=2, margin=1.05):
    """A camera above the box [lo, hi] looking straight down the `up_axis` with the whole box in frame: cam = (H, W, fx, fy, cx,
    cy); the box's longer horizontal side runs along the image's longer side; the height is the least at which the box's top
    face, grown by `margin`, projects inside the image.  [4,4], OpenCV axes."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    H, W, fx, fy, cx, cy = cam
    h1, h2 = [a for a in range(3) if a != up_axis]
    ext = hi - lo
    if (ext[h2] > ext[h1]) == (W >= H):
        h1, h2 = h2, h1                                 # image x along h1
    z = np.zeros(3)
    z[up_axis] = -1.0
    x = np.zeros(3)
    x[h1] = 1.0
    down = np.cross(z, x)
    room_u, room_v = min(cx, W - 1 - cx), min(cy, H - 1 - cy)
    if room_u <= 0 or room_v <= 0:
        raise ValueError('overview_pose: the principal point lies outside the image')
    d = margin * max(abs(fx) * 0.5 * ext[h1] / room_u, abs(fy) * 0.5 * ext[h2] / room_v, 1e-6)
    pos = 0.5 * (lo + hi)
    pos[up_axis] = hi[up_axis] + d
    return _pose(z, down, pos)


# ---- which mesh a frame shows ----
MESH_NAME = re.compile(r'^(\d+)_mesh\.ply$')


def mesh_index(names):
    """File names -> [(idx, name)] ascending for those of the form {idx:05d}_mesh.ply (a directory listing may hold others: culled
    or final meshes)."""
    found = []
    for n in names:
        m = MESH_NAME.match(os.path.basename(n))
        if m:
            found.append((int(m.group(1)), n))
    return sorted(found)


def mesh_for_frames(names, frames):
    """Per frame k the name of the mesh with the largest index <= k, or None before the first."""
    idx = mesh_index(names)
    out = []
    for k in frames:
        held = [n for i, n in idx if i <= k]
        out.append(held[-1] if held else None)
    return out


def run_poses(ckpt, scale):
    """(estimated, ground truth) float64 [idx + 1,4,4] with OpenCV axes of a checkpoint dict, translations divided by `scale` on a
    copy (eval_ate.convert_poses' units), and idx."""
    idx = int(ckpt['idx'])
    out = []
    for key in ('estimate_c2w_list', 'gt_c2w_list'):
        p = render_mesh.opencv_poses(ckpt[key])[:idx + 1]
        with np.errstate(all='ignore'):
            p[:, :3, 3] /= float(scale)
        out.append(p)
    return out[0], out[1], idx


def overlay_lists(est, gt, frames, cam, frustum_size, gt_traj=True):
    """The shared segment list of a replay and the ranges of each chosen frame: (segments [N,2,3], colors uint8 [N,3], ranges int64
    [len(frames),4,2]).  The list is the estimated trajectory, the ground-truth one, then per chosen frame the estimated and the
    ground-truth frustum; frame k draws the trajectories' first k segments and its own frusta (without gt_traj: nothing green)."""
    n = len(est)
    te, tg = trajectory_segments(est), trajectory_segments(gt)
    fr = [np.concatenate([frustum_segments(est[k], *cam, frustum_size), frustum_segments(gt[k], *cam, frustum_size)]) for k in frames]
    segs = np.concatenate([te, tg] + fr) if len(frames) else np.concatenate([te, tg])
    colors = np.zeros((len(segs), 3), np.uint8)
    colors[:len(te)] = EST_COLOR
    colors[len(te):len(te) + len(tg)] = GT_COLOR
    f0 = len(te) + len(tg)
    ranges = np.zeros((len(frames), 4, 2), np.int64)
    for i, k in enumerate(frames):
        b = f0 + 2 * FRUSTUM_SEGMENTS * i
        colors[b:b + FRUSTUM_SEGMENTS] = EST_COLOR
        colors[b + FRUSTUM_SEGMENTS:b + 2 * FRUSTUM_SEGMENTS] = GT_COLOR
        kk = min(k, n - 1)
        ranges[i, 0] = (0, kk)
        ranges[i, 1] = (len(te), len(te) + kk) if gt_traj else (0, 0)
        ranges[i, 2] = (b, b + FRUSTUM_SEGMENTS)
        ranges[i, 3] = (b + FRUSTUM_SEGMENTS, b + 2 * FRUSTUM_SEGMENTS) if gt_traj else (0, 0)
    return segs, colors, ranges


def paste_input_frame(rgb, color):
    """rgb uint8 [H,W,3] (device, in place) <- color [h,w,3] in [0, 1] (device) into the top-left corner, every s-th pixel with s the
    least integer stride that brings its width to at most W / 4.  Plain indexing."""
    W = int(rgb.shape[1])
    s = max(1, -(-int(color.shape[1]) * 4 // max(W, 1)))
    small = (color[::s, ::s, :3].to(torch.float64).clamp(0.0, 1.0) * 255.0 + 0.5).floor().to(torch.uint8)
    h, w = min(int(small.shape[0]), int(rgb.shape[0])), min(int(small.shape[1]), W)
    rgb[:h, :w] = small[:h, :w]


def replay(cfg, output, out=None, ckpt=None, mesh_path=None, every=1, view='follow', back=1.0, up=0.5, width=2.0, hidden_alpha=0.0,
           gt_traj=True, vis_input_frame=False, cam=None, args=None, bias=(0.0, 0.0), frustum_size=0.2, background=(255, 255, 255),
           chunk=render_mesh.CHUNK, device='cuda:0'):
    """Write {out}/{k:05d}.png for every `every`-th frame k <= idx of the run under `output` and return the paths.  cfg: the loaded
    config (scale; its cam block unless cam = (H, W, fx, fy, cx, cy) is given); ckpt: a checkpoint dict or path (default: the newest
    of {output}/ckpts); mesh_path: one mesh for all frames (default: {output}/mesh/{idx:05d}_mesh.ply, the newest not after the
    frame); view: 'follow', 'overview', a [4,4] or [n,4,4] array of OpenCV camera-to-world poses, or a pose file.  args: for
    vis_input_frame, what datasets.get_dataset takes (input_folder)."""
    from PIL import Image
    from .render_eval import newest_checkpoint
    if every < 1:
        raise ValueError(f'every {every} must be >= 1')
    if cam is None:
        from .get_tsdf import update_cam
        cam = update_cam(cfg)
    H, W, fx, fy, cx, cy = cam
    H, W = int(H), int(W)
    cam = (H, W, fx, fy, cx, cy)
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt or newest_checkpoint(output), map_location='cpu', weights_only=False)
    est, gt, idx = run_poses(ckpt, cfg['scale'])
    frames = list(range(0, idx + 1, every))
    out = out or os.path.join(output, 'replay')
    os.makedirs(out, exist_ok=True)

    if mesh_path is not None:
        chosen = [mesh_path] * len(frames)
    else:
        mesh_dir = os.path.join(output, 'mesh')
        names = sorted(os.listdir(mesh_dir)) if os.path.isdir(mesh_dir) else []
        chosen = [os.path.join(mesh_dir, n) if n is not None else None for n in mesh_for_frames(names, frames)]

    if isinstance(view, str) and view == 'follow':
        views = np.stack([follow_pose(est[k], back, up) for k in frames]) if frames else np.zeros((0, 4, 4))
    elif isinstance(view, str) and view == 'overview':
        last = [c for c in chosen if c is not None]
        if last:
            v = mesh_io.read_ply(last[-1]).verts
            lo, hi = v.min(0), v.max(0)
        else:
            o = est[np.isfinite(est).all((1, 2)), :3, 3]
            lo, hi = o.min(0) - 1.0, o.max(0) + 1.0
        views = np.broadcast_to(overview_pose(lo, hi, cam), (len(frames), 4, 4)).copy()
    else:
        if isinstance(view, str):
            from .render_views import read_poses
            view = render_mesh.opencv_poses(read_poses(view))
        v = np.asarray(view, dtype=np.float64).reshape(-1, 4, 4)
        views = np.stack([v[min(i, len(v) - 1)] for i in range(len(frames))]) if frames else np.zeros((0, 4, 4))

    segs, colors, ranges = overlay_lists(est, gt, frames, cam, frustum_size, gt_traj)
    dev = torch.device(device)
    segs_d, colors_d = torch.from_numpy(segs).to(dev), torch.from_numpy(colors).to(dev)
    dataset = None
    if vis_input_frame:
        from .datasets import get_dataset
        dataset = get_dataset(cfg, args if args is not None else SimpleNamespace(input_folder=None), cfg['scale'], device=device)

    paths = []
    g0 = 0
    while g0 < len(frames):                               # one group of consecutive frames per mesh: its MeshViews is built once
        g1 = g0
        while g1 < len(frames) and chosen[g1] == chosen[g0]:
            g1 += 1
        mv = None
        if chosen[g0] is not None:
            m = mesh_io.read_ply(chosen[g0])
            mv = render_mesh.MeshViews(m.verts, m.faces, m.colors[:, :3] if m.colors is not None else None, dev)
        for p0 in range(g0, g1, chunk):
            p1 = min(p0 + chunk, g1)
            if mv is not None:
                r = mv.render(views[p0:p1], H, W, fx, fy, cx, cy, far=FAR, background=background, chunk=chunk)
                rgb, depth = r['rgb'], r['depth']
            else:
                rgb = torch.tensor(background, dtype=torch.uint8, device=dev).expand(p1 - p0, H, W, 3).contiguous()
                depth = None
            render_mesh.draw_segments(rgb, depth, views[p0:p1], fx, fy, cx, cy, segs_d, colors_d, ranges[p0:p1], width=width, bias=bias,
                                      hidden_alpha=hidden_alpha, chunk=chunk)
            if dataset is not None:
                ks = [k for k in frames[p0:p1] if k < len(dataset)]
                for i, color in enumerate(dataset.frames(ks)[0] if ks else []):
                    paste_input_frame(rgb[i], color)
            host = rgb.cpu().numpy()                      # the chunk's one download
            for i, k in enumerate(frames[p0:p1]):
                paths.append(os.path.join(out, f'{k:05d}.png'))
                Image.fromarray(host[i], 'RGB').save(paths[-1])
        g0 = g1
    return paths


def main(argv=None):
    from .get_tsdf import load_config, update_cam
    ap = argparse.ArgumentParser(description='Replay a run: the growing mesh with the trajectories and the camera drawn over it.')
    ap.add_argument('config', type=str, help='YAML config of the scene')
    ap.add_argument('--input_folder', type=str, help="dataset directory; replaces the config's data.input_folder (--vis_input_frame)")
    ap.add_argument('--output', type=str, help="output directory of the run; replaces the config's data.output")
    ap.add_argument('--ckpt', type=str, help='checkpoint file (default: the newest {output}/ckpts/*.tar)')
    ap.add_argument('--mesh', type=str, help='one mesh for every frame (default: the newest {output}/mesh/{idx:05d}_mesh.ply not after it)')
    ap.add_argument('--every', type=int, default=1, help='replay every N-th frame')
    ap.add_argument('--view', type=str, default='follow', help="'follow', 'overview' or a file with one camera-to-world 4x4 per line")
    ap.add_argument('--back', type=float, default=1.0, help='follow: metres behind the camera')
    ap.add_argument('--up', type=float, default=0.5, help='follow: metres above the camera')
    ap.add_argument('--width', type=float, default=2.0, help='line width in pixels')
    ap.add_argument('--hidden_alpha', type=float, default=0.0, help='weight of a line where the mesh hides it (0: not drawn)')
    ap.add_argument('--no_gt_traj', action='store_true', help='leave the ground-truth trajectory and frustum out')
    ap.add_argument('--vis_input_frame', action='store_true', help="paste the frame's colour image into the top-left corner")
    for k, t in (('H', int), ('W', int), ('fx', float), ('fy', float), ('cx', float), ('cy', float)):
        ap.add_argument('--' + k, type=t)
    ap.add_argument('--out', type=str, help='directory of the PNGs (default: {output}/replay)')
    ap.add_argument('--default_config', type=str, default='configs/df_prior.yaml', help='the config every other one inherits from')
    ap.add_argument('--device', type=str, default='cuda:0')
    args = ap.parse_args(argv)
    cfg = load_config(args.config, args.default_config if os.path.exists(args.default_config) else None)
    if args.every < 1:
        ap.error('--every must be at least 1')
    given = [getattr(args, k) for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy')]
    cam = tuple(g if g is not None else c for g, c in zip(given, update_cam(cfg)))
    output = args.output or cfg['data']['output']
    paths = replay(cfg, output, args.out, args.ckpt, args.mesh, args.every, args.view, args.back, args.up, args.width, args.hidden_alpha,
                   not args.no_gt_traj, args.vis_input_frame, cam, args, device=args.device)
    if paths:
        d = os.path.dirname(paths[0])
        print(f'{len(paths)} frames under {d}; to join them: ffmpeg -framerate 30 -pattern_type glob -i "{d}/*.png" -pix_fmt yuv420p {d}/replay.mp4')
    return paths


if __name__ == '__main__':
    main()
