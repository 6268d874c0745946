"""Rendering evaluation of a finished run: PSNR, SSIM, MS-SSIM and depth L1 over every n-th frame of the trajectory, the table the
papers of this family of methods report.  The reference has no counterpart (it publishes no render-quality figure).

    python -m attentive_dfprior_amd.render_eval CONFIG [--input_folder ..] [--output ..] [--ckpt PATH] [--every N] [--gt_pose]
                                                       [--tsdf_volume PATH --tsdf_bounds PATH] [--guide sensor|tsdf]

--guide tsdf renders every frame as a NOVEL view (Renderer.render_novel: the raycast of the TSDF prior takes the sensor depth
image's place as the sampler's guide), scores it against the same ground truth and writes eval_render_tsdf_guide.json beside
eval_render.json: the difference is what the rendering metrics owe to the sensor's depth guide.

Each chosen frame is rendered with Renderer.render_img and handed, still on the device, to adfp_frame_metrics
(csrc/adfp_metrics.h), which writes one row of 35 doubles into a device table; the table comes down once, at the end.

SSIM and MS-SSIM follow the convention of the pytorch_msssim package (11-tap Gaussian window of sigma 1.5 without padding, data
range 1, 2 x 2 average pooling between five levels, the published weights), restated from its formula in include/adfp.h and
tests/render_ref.py.  The numbers are pinned to that statement; they have not been compared with pytorch_msssim or skimage."""
import argparse
import ctypes as C
import glob
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, synthetic
from ._lib import lib

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_LEVELS = 5
CHUNK = 8                                            # frames per upload and ingestion launch (get_tsdf.CHUNK)
PER_FRAME = ('psnr', 'depth_l1', 'ssim', 'ms_ssim', 'n_valid', 'n_nonfinite')


def max_levels(H, W):
    """The largest `levels` adfp_frame_metrics accepts for an H x W frame: every level's image must hold one 11 x 11 window.
    5 for every frame whose sides exceed 160."""
    win = (C.c_longlong * MAX_LEVELS)()
    for levels in range(MAX_LEVELS, 0, -1):
        geom = _lib.AdfpMetricsGeom(H, W, levels, 0)
        if lib().adfp_frame_metrics_windows(C.byref(geom), win) == 0:
            return levels
    return 0


class FrameMetrics(object):
    """A device table [n_frames][35] of adfp_frame_metrics rows, the workspace of one frame shape, and a frame count.

    `add` queues a frame into the next row and returns at once; `table` is the one download.  One object serves one stream at
    a time: every add writes the same workspace, so adds queued on different streams would race on it."""

    def __init__(self, n_frames, H, W, levels=5, device='cuda:0', gt_color_dtype=torch.float32):
        if gt_color_dtype not in (torch.float32, torch.float64):
            raise ValueError(f'gt_color_dtype {gt_color_dtype}: torch.float32 or torch.float64')
        if int(n_frames) < 0:
            raise ValueError(f'n_frames {n_frames} is negative')
        self.n_frames, self.H, self.W, self.levels = int(n_frames), int(H), int(W), int(levels)
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.gt_color_dtype = gt_color_dtype
        self._geom = _lib.AdfpMetricsGeom(self.H, self.W, self.levels, int(gt_color_dtype == torch.float64))
        win = (C.c_longlong * MAX_LEVELS)()
        _lib.host.adfp_frame_metrics_windows(C.byref(self._geom), win)
        self.windows = [int(v) for v in win]
        self._ws_bytes = lib().adfp_frame_metrics_workspace_bytes(C.byref(self._geom))
        self._ws = torch.empty(self._ws_bytes // 8, dtype=torch.float64, device=self.device)
        self._table = torch.zeros((self.n_frames, _lib.FRAME_METRICS), dtype=torch.float64, device=self.device)
        self.count = 0

    def add(self, gt_depth, gt_color, depth, color):
        """Queues one frame -- gt_depth [H,W], gt_color [H,W,3], and the rendered depth [H,W] and color [H,W,3] as render_img
        returns them -- into the next row on the current stream and returns the row index.  Does not synchronise."""
        if self.count >= self.n_frames:
            raise IndexError(f'FrameMetrics: the table of {self.n_frames} frames is full')
        _lib.require_cuda(gt_depth, 'gt_depth')
        dev = gt_depth.device
        if dev != self.device:
            raise ValueError(f'FrameMetrics on {self.device}: gt_depth is on {dev}')
        H, W = gt_depth.shape
        if gt_color.dtype != self.gt_color_dtype:
            raise ValueError(f'FrameMetrics for {self.gt_color_dtype} gt_color: got {gt_color.dtype}')
        gt_depth = gt_depth.to(torch.float32).contiguous()
        gt_color = gt_color.to(device=dev).contiguous()
        depth = depth.to(device=dev, dtype=torch.float64).contiguous()
        color = color.to(device=dev, dtype=torch.float32).contiguous()
        if (H, W) != (self.H, self.W) or tuple(gt_color.shape) != (H, W, 3) or tuple(depth.shape) != (H, W) or tuple(color.shape) != (H, W, 3):
            raise ValueError(f'add: gt_depth {tuple(gt_depth.shape)}, gt_color {tuple(gt_color.shape)}, depth {tuple(depth.shape)}, '
                             f'color {tuple(color.shape)} are not one {self.H} x {self.W} frame')
        row = self.count
        with _lib.on(dev) as L:
            L.adfp_frame_metrics(C.byref(self._geom), gt_depth, gt_color, depth, color, self._table[row], self._ws, self._ws_bytes)
        self.count += 1
        return row

    def table(self):
        """The rows added so far as numpy float64 [count, 35]: the one download (it waits for the queued frames)."""
        return self._table[:self.count].cpu().numpy()

    def per_frame(self):
        return per_frame(self.table(), self.windows, self.levels)

    def summary(self):
        """The means over the frames added, taken in f64 on the host, and the number of frames."""
        pf = self.per_frame()
        out = {k: (float(np.mean(pf[k])) if self.count else float('nan')) for k in PER_FRAME}
        out['n_frames'] = self.count
        return out


def per_frame(table, windows, levels):
    """Rows [n, 35] -> dict of numpy arrays [n]: psnr and depth_l1 by the formulas of visualizer.stats_dict; ssim, level 0's sums
    over the window count, then the mean over the three channels; ms_ssim, per channel prod_k relu(cs_k)^w_k for k < levels - 1
    times relu(ssim_{levels-1})^w_{levels-1}, then the mean over channels -- NaN unless levels == 5; n_valid and n_nonfinite."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, _lib.FRAME_METRICS)
    n = len(t)
    out = {'n_valid': t[:, 0].astype(np.int64), 'n_nonfinite': t[:, 4].astype(np.int64)}
    with np.errstate(all='ignore'):
        out['depth_l1'] = t[:, 1] / t[:, 0]
        out['psnr'] = -10.0 * np.log10(t[:, 2] / (3.0 * t[:, 3]))
    maps = t[:, 5:].reshape(n, MAX_LEVELS, 3, 2)                       # [frame, level, channel, (ssim, cs)]
    out['ssim'] = (maps[:, 0, :, 0] / windows[0]).mean(axis=1) if levels >= 1 else np.full(n, np.nan)
    if levels == MAX_LEVELS:
        w = np.asarray(MS_SSIM_WEIGHTS)
        means = np.stack([maps[:, k, :, 0 if k == levels - 1 else 1] / windows[k] for k in range(levels)], axis=1)      # [n, 5, 3]
        out['ms_ssim'] = np.prod(np.maximum(means, 0.0) ** w[None, :, None], axis=1).mean(axis=1)
    else:
        out['ms_ssim'] = np.full(n, np.nan)
    return out


def frame_metrics(gt_depth, gt_color, depth, color, levels=None):
    """One frame's dict of floats (PER_FRAME's keys); levels None = max_levels of the frame."""
    H, W = gt_depth.shape
    fm = FrameMetrics(1, H, W, max_levels(H, W) if levels is None else levels, gt_depth.device, gt_color.dtype)
    fm.add(gt_depth, gt_color, depth, color)
    return {k: v[0].item() for k, v in fm.per_frame().items()}


def newest_checkpoint(output):
    paths = sorted(glob.glob(os.path.join(output, 'ckpts', '*.tar')))
    if not paths:
        raise FileNotFoundError(f'no checkpoint under {os.path.join(output, "ckpts")}')
    return paths[-1]


def eval_render(cfg, args, ckpt, every=5, gt_pose=False, levels=None, device='cuda:0', guide='sensor'):
    """Renders frames 0, every, 2 every, ... <= idx of a checkpoint and returns (summary, per-frame dict of lists, frame indices).

    cfg: the loaded config; args: input_folder / tsdf_volume / tsdf_bounds (paths or None); ckpt: the dict src/utils/Logger.py
    saves, or its path.  The decoders come from get_model, the bound is built the way get_tsdf.init_tsdf_volume builds it, the
    camera is get_tsdf.update_cam's and the frames are datasets.get_dataset(...).frames(...) in chunks.  The pose is the estimated
    one, or the ground-truth one with gt_pose; frames whose ground-truth pose holds a non-finite entry are skipped, as
    eval_ate.convert_poses skips them.  One synchronisation, at the end.
    guide: 'sensor' renders with the frame's depth image as the sampler's guide (render_img); 'tsdf' with the raycast of the TSDF
    prior instead (render_novel), as a pose without a sensor image would be rendered.  The ground truth is the same."""
    from . import Renderer, get_model
    from .datasets import get_dataset
    from .get_tsdf import update_cam
    if every < 1:
        raise ValueError(f'every {every} must be >= 1')
    if guide not in ('sensor', 'tsdf'):
        raise ValueError(f"guide {guide!r}: 'sensor' or 'tsdf'")
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt, map_location='cpu', weights_only=False)
    scale = cfg['scale']
    bound = synthetic.scene_bound(cfg['mapping']['bound'], cfg['grid_len']['bound_divisible'], scale)
    H, W, fx, fy, cx, cy = update_cam(cfg)

    dataset, scene_id = cfg['data'].get('dataset', cfg['dataset']), cfg['data'].get('id')
    stem = f'scene{scene_id}' if dataset == 'scannet' else f'{scene_id}'
    bounds_path = getattr(args, 'tsdf_bounds', None) or f'{dataset}_tsdf_volume/{stem}_bounds.pt'
    tsdf_bnds = torch.as_tensor(torch.load(bounds_path, map_location='cpu', weights_only=False)).to(device)
    volume_path = getattr(args, 'tsdf_volume', None)
    tsdf_volume = torch.load(volume_path, map_location='cpu', weights_only=False) if volume_path else ckpt['tsdf_volume']
    tsdf_volume = tsdf_volume.to(device)

    decoders = get_model(cfg)
    decoders.load_state_dict(ckpt['decoder_state_dict'])
    decoders.bound = bound
    decoders = decoders.to(device)
    c = {k: v.to(device) for k, v in ckpt['c'].items()}
    renderer = Renderer(cfg, args, SimpleNamespace(bound=bound, vol_bnds=tsdf_bnds, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy))

    frames = get_dataset(cfg, args, scale, device=device)
    last = min(int(ckpt['idx']), len(frames) - 1)
    gt_list, est_list = ckpt['gt_c2w_list'], ckpt['estimate_c2w_list']
    chosen = [i for i in range(0, last + 1, every) if bool(torch.isfinite(torch.as_tensor(gt_list[i])).all())]
    levels = max_levels(H, W) if levels is None else levels
    fm = FrameMetrics(len(chosen), H, W, levels, device, frames.color_dtype)
    poses = gt_list if gt_pose else est_list
    for k in range(0, len(chosen), CHUNK):
        chunk = chosen[k:k + CHUNK]
        colors, depths, _ = frames.frames(chunk)
        for i, gt_color, gt_depth in zip(chunk, colors, depths):
            c2w = torch.as_tensor(poses[i]).to(device=device, dtype=torch.float32)
            if guide == 'tsdf':
                depth, _, color, _ = renderer.render_novel(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage='color')
            else:
                depth, _, color = renderer.render_img(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage='color', gt_depth=gt_depth)
            fm.add(gt_depth, gt_color, depth, color)
    pf = fm.per_frame()                                # the one synchronisation
    summary = {k: (float(np.mean(pf[k])) if chosen else float('nan')) for k in PER_FRAME}
    summary['n_frames'] = len(chosen)
    return summary, {k: pf[k].tolist() for k in PER_FRAME}, chosen


def main(argv=None):
    """Write {output}/eval_render.json (summary, per-frame lists, frame indices) for the newest checkpoint of a run and print the
    summary (also returned); with --guide tsdf, {output}/eval_render_tsdf_guide.json."""
    from .get_tsdf import load_config, update_cam
    parser = argparse.ArgumentParser(description='Rendering metrics (PSNR, SSIM, MS-SSIM, depth L1) of a finished run.')
    parser.add_argument('config', type=str, help='YAML config of the scene')
    parser.add_argument('--input_folder', type=str, help="dataset directory; replaces the config's data.input_folder")
    parser.add_argument('--output', type=str, help="output directory of the run; replaces the config's data.output")
    parser.add_argument('--ckpt', type=str, help='checkpoint file (default: the newest {output}/ckpts/*.tar)')
    parser.add_argument('--every', type=int, default=5, help='evaluate every N-th frame')
    parser.add_argument('--gt_pose', action='store_true', help='render from the ground-truth poses instead of the estimated ones')
    parser.add_argument('--tsdf_volume', type=str, help="prior TSDF volume file (default: the checkpoint's)")
    parser.add_argument('--tsdf_bounds', type=str, help='bounds file of the TSDF volume (default: <dataset>_tsdf_volume/<scene>_bounds.pt)')
    parser.add_argument('--guide', choices=('sensor', 'tsdf'), default='sensor',
                        help="the sampler's depth guide: the sensor's depth image, or the raycast of the TSDF prior (a novel view)")
    parser.add_argument('--default_config', type=str, default='configs/df_prior.yaml', help='the config every other one inherits from')
    parser.add_argument('--device', type=str, default='cuda:0')
    args = parser.parse_args(argv)
    cfg = load_config(args.config, args.default_config if os.path.exists(args.default_config) else None)
    output = args.output or cfg['data']['output']
    ckpt = args.ckpt or newest_checkpoint(output)
    summary, frames, indices = eval_render(cfg, args, ckpt, every=args.every, gt_pose=args.gt_pose, device=args.device, guide=args.guide)
    result = {'checkpoint': os.path.basename(ckpt), 'every': args.every, 'gt_pose': bool(args.gt_pose), 'levels': max_levels(*update_cam(cfg)[:2]),
              'summary': summary, 'frames': frames, 'frame_indices': indices}
    if args.guide == 'tsdf':
        result['guide'] = 'tsdf'
    os.makedirs(output, exist_ok=True)
    with open(os.path.join(output, 'eval_render_tsdf_guide.json' if args.guide == 'tsdf' else 'eval_render.json'), 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(summary)
    return summary


if __name__ == '__main__':
    main()
