"""Render a finished run from poses that have no sensor image: fly-throughs, held-out poses.  The reference cannot (its
render_img needs a depth image per frame, src/utils/Renderer.py:292); here the raycast of the TSDF prior guides the sampler
(Renderer.render_novel, tsdf_raycast.TsdfRaycaster).

    python -m attentive_dfprior_amd.render_views CONFIG --poses FILE [--ckpt PATH] [--out DIR] [--output ..]
                                                        [--tsdf_volume PATH --tsdf_bounds PATH]

FILE holds one camera-to-world matrix per line, 16 numbers in row-major order in the layout of Replica's traj.txt (the OpenCV
camera: the loader's flip of the y and z columns is applied here too).  Per view k the output directory (default
{output}/views) receives depth_{k:05d}.npy (float64 [H,W], metres), color_{k:05d}.npy (float32 [H,W,3]), guide_{k:05d}.npy (the
raycast depth, float32 [H,W], 0 where the ray meets no surface), and depth_{k:05d}.png (16 bit, millimetres) and color_{k:05d}.png
(8 bit) written with PIL."""
import argparse
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import synthetic


def read_poses(path, scale=1.0):
    """The poses of a traj.txt-style file as float32 [n,4,4] in the renderer's convention (datasets._flipped, translation x scale)."""
    from .datasets import _flipped
    poses = []
    with open(path, 'r') as f:
        for n, line in enumerate(f):
            vals = line.split()
            if not vals:
                continue
            if len(vals) != 16:
                raise ValueError(f'{path}:{n + 1}: {len(vals)} numbers, a pose is 16')
            c2w = _flipped([float(v) for v in vals])
            c2w[:3, 3] *= scale
            poses.append(c2w)
    if not poses:
        raise ValueError(f'{path}: no pose')
    return torch.stack(poses)


def load_run(cfg, args, ckpt, device='cuda:0'):
    """(renderer, decoders, c, tsdf_volume, tsdf_bnds) of a checkpoint, put together the way render_eval.eval_render does."""
    from . import Renderer, get_model
    from .get_tsdf import update_cam
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt, map_location='cpu', weights_only=False)
    bound = synthetic.scene_bound(cfg['mapping']['bound'], cfg['grid_len']['bound_divisible'], cfg['scale'])
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
    return renderer, decoders, c, tsdf_volume, tsdf_bnds


def render_views(cfg, args, ckpt, poses, out, device='cuda:0'):
    """Renders `poses` [n,4,4] (renderer's convention) and writes the files the module's header lists into `out`; returns the number
    of pixels per view whose ray met no surface of the prior."""
    from PIL import Image
    renderer, decoders, c, tsdf_volume, tsdf_bnds = load_run(cfg, args, ckpt, device)
    os.makedirs(out, exist_ok=True)
    unguided = []
    for k, c2w in enumerate(poses):
        c2w = c2w.to(device=device, dtype=torch.float32)
        depth, _, color, guide = renderer.render_novel(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage='color')
        depth, color, guide = depth.cpu().numpy(), color.cpu().numpy(), guide.cpu().numpy()
        np.save(os.path.join(out, f'depth_{k:05d}.npy'), depth)
        np.save(os.path.join(out, f'color_{k:05d}.npy'), color)
        np.save(os.path.join(out, f'guide_{k:05d}.npy'), guide)
        mm = np.clip(np.rint(np.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0) * 1000.0), 0, 65535).astype(np.uint16)
        Image.fromarray(mm).save(os.path.join(out, f'depth_{k:05d}.png'))
        rgb = np.clip(np.rint(np.nan_to_num(color, nan=0.0) * 255.0), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(os.path.join(out, f'color_{k:05d}.png'))
        unguided.append(int((guide == 0).sum()))
    return unguided


def main(argv=None):
    from .get_tsdf import load_config
    from .render_eval import newest_checkpoint
    parser = argparse.ArgumentParser(description='Render a finished run from a list of poses that have no sensor image.')
    parser.add_argument('config', type=str, help='YAML config of the scene')
    parser.add_argument('--poses', type=str, required=True, help='one 4x4 camera-to-world matrix per line (traj.txt layout)')
    parser.add_argument('--ckpt', type=str, help='checkpoint file (default: the newest {output}/ckpts/*.tar)')
    parser.add_argument('--out', type=str, help='directory for the rendered views (default: {output}/views)')
    parser.add_argument('--output', type=str, help="output directory of the run; replaces the config's data.output")
    parser.add_argument('--tsdf_volume', type=str, help="prior TSDF volume file (default: the checkpoint's)")
    parser.add_argument('--tsdf_bounds', type=str, help='bounds file of the TSDF volume (default: <dataset>_tsdf_volume/<scene>_bounds.pt)')
    parser.add_argument('--default_config', type=str, default='configs/df_prior.yaml', help='the config every other one inherits from')
    parser.add_argument('--device', type=str, default='cuda:0')
    args = parser.parse_args(argv)
    cfg = load_config(args.config, args.default_config if os.path.exists(args.default_config) else None)
    output = args.output or cfg['data']['output']
    ckpt = args.ckpt or newest_checkpoint(output)
    out = args.out or os.path.join(output, 'views')
    poses = read_poses(args.poses, cfg['scale'])
    unguided = render_views(cfg, args, ckpt, poses, out, device=args.device)
    print({'views': len(poses), 'out': out, 'pixels_without_guide': unguided})
    return unguided


if __name__ == '__main__':
    main()
