"""
Drop-in for the reference's ``get_tsdf.py``: ``update_cam(cfg)`` and ``init_tsdf_volume(cfg, args, space=10)`` with the reference's
signatures and return values, and a ``main()`` that saves the two ``.pt`` files under the reference's names.  The frames come from
``datasets.get_dataset`` (decoded on the host, ingested on the device in chunks) and go into ``fusion.TSDFVolume.integrate`` as
device tensors; no open3d (the intrinsics are a plain 3 x 3 matrix), pycuda or cv2.

    python -m attentive_dfprior_amd.get_tsdf configs/Replica/room0.yaml --space 10
"""
import argparse
import os

import numpy as np
import torch
import yaml

from . import fusion, synthetic
from .datasets import get_dataset

CHUNK = 8                                            # frames per upload and launch


def load_config(path, default_path=None):
    """A YAML config merged over what it inherits: its `inherit_from` file (recursively), else `default_path`, else nothing
    (src/config.py:10-42)."""
    with open(path, 'r') as f:
        special = yaml.full_load(f)
    parent = special.get('inherit_from')
    if parent is not None:
        cfg = load_config(parent, default_path)
    elif default_path is not None:
        with open(default_path, 'r') as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    _merge(cfg, special)
    return cfg


def _merge(base, over):
    for k, v in over.items():
        if k not in base:
            base[k] = dict()
        if isinstance(v, dict):
            _merge(base[k], v)
        else:
            base[k] = v


def update_cam(cfg):
    """(H, W, fx, fy, cx, cy) after the pre-processing of cfg cam: crop_size rescales all six, crop_edge shrinks H, W and shifts
    cx, cy (get_tsdf.py:12-41)."""
    cam = cfg['cam']
    H, W, fx, fy, cx, cy = cam['H'], cam['W'], cam['fx'], cam['fy'], cam['cx'], cam['cy']
    if 'crop_size' in cam:
        crop_h, crop_w = cam['crop_size']
        sx, sy = crop_w / W, crop_h / H
        fx, fy, cx, cy = sx * fx, sy * fy, sx * cx, sy * cy
        H, W = crop_h, crop_w
    edge = cam['crop_edge']
    if edge > 0:
        H -= edge * 2
        W -= edge * 2
        cx -= edge
        cy -= edge
    return H, W, fx, fy, cx, cy


def init_tsdf_volume(cfg, args, space=10):
    """The prior TSDF volume of a dataset directory (get_tsdf.py:44-99): every `space`-th frame whose pose has a finite entry
    (the reference's test, np.isfinite(c2w).any()) is integrated at obs_weight 1 into a volume of 4/256 voxels over the bound
    enlarged to bound_divisible.  Returns (tsdf_volume [1,1,Z,Y,X], bounds, verts, faces, norms, colors)."""
    scale = cfg['scale']
    bound = synthetic.scene_bound(cfg['mapping']['bound'], cfg['grid_len']['bound_divisible'], scale)

    H, W, fx, fy, cx, cy = update_cam(cfg)
    intrinsic = np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])

    print('Initializing voxel volume...')
    tsdf_vol = fusion.TSDFVolume(bound.numpy(), voxel_size=4.0 / 256)
    frame_reader = get_dataset(cfg, args, scale, color_dtype=torch.float64)      # the reference floors the float64 colour

    picked = []
    for idx in range(0, len(frame_reader), space):
        c2w = frame_reader.pose(idx).numpy()
        if np.isfinite(c2w).any():
            c2w[:3, 1] *= -1.0                      # back to the camera convention the volume integrates in
            c2w[:3, 2] *= -1.0
            picked.append((idx, c2w))
    for k in range(0, len(picked), CHUNK):
        chunk = picked[k:k + CHUNK]
        colors, depths, _ = frame_reader.frames([idx for idx, _ in chunk])
        for (idx, c2w), color, depth in zip(chunk, colors, depths):
            print(f'frame: {idx}')
            tsdf_vol.integrate(torch.floor(color * 255), depth, intrinsic, c2w, obs_weight=1.)      # floor: .astype(np.uint8)

    print('Getting TSDF volume')
    tsdf_volume, _, bounds = tsdf_vol.get_volume()
    print('Getting mesh')
    verts, faces, norms, colors = tsdf_vol.get_mesh()
    tsdf_volume = torch.tensor(tsdf_volume)
    tsdf_volume = tsdf_volume.reshape(1, 1, tsdf_volume.shape[0], tsdf_volume.shape[1], tsdf_volume.shape[2])
    tsdf_volume = tsdf_volume.permute(0, 1, 4, 3, 2)
    return tsdf_volume, bounds, verts, faces, norms, colors


def main(argv=None):
    """Save <dataset>_tsdf_volume/<scene>_tsdf_volume.pt and <scene>_bounds.pt (get_tsdf.py:101-138)."""
    parser = argparse.ArgumentParser(description='Build the prior TSDF volume of a dataset directory.')
    parser.add_argument('config', type=str, help='YAML config of the scene')
    parser.add_argument('--input_folder', type=str, help="dataset directory; replaces the config's data.input_folder")
    parser.add_argument('--output', type=str, help='accepted like the reference does; the files go to <dataset>_tsdf_volume/')
    parser.add_argument('--space', type=int, default=10, help='integrate every space-th frame')
    parser.add_argument('--default_config', type=str, default='configs/df_prior.yaml', help='the config every other one inherits from')
    args = parser.parse_args(argv)
    cfg = load_config(args.config, args.default_config)
    dataset, scene_id = cfg['data']['dataset'], cfg['data']['id']
    path = f'{dataset}_tsdf_volume'
    os.makedirs(path, exist_ok=True)
    tsdf_volume, bounds, _, _, _, _ = init_tsdf_volume(cfg, args, space=args.space)
    stem = f'scene{scene_id}' if dataset == 'scannet' else f'{scene_id}'
    torch.save(tsdf_volume, os.path.join(path, f'{stem}_tsdf_volume.pt'))
    torch.save(bounds, os.path.join(path, f'{stem}_bounds.pt'))


if __name__ == '__main__':
    main()
