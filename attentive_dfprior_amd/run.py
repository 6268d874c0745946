"""Run the whole system on a dataset directory: checkpoints, meshes and the trajectory error (the reference's run.py).

    python -m attentive_dfprior_amd.run CONFIG [--input_folder ..] [--output ..] [--tsdf_volume PATH --tsdf_bounds PATH]
                                               [--prior file|online] [--prior_voxel_size M] [--seed N] [--last_frame N]
                                               [--no_prefetch] [--default_config PATH] [--tracking_init guess|icp]
                                               [--tracking_rgb_weight W] [--tracking_icp_bilateral]

The prior TSDF volume comes from the files ``python -m attentive_dfprior_amd.get_tsdf CONFIG`` writes
(``<dataset>_tsdf_volume/<scene>_tsdf_volume.pt`` and ``_bounds.pt``, or the two paths given), or with ``--prior online`` is fused
during the run from the estimated poses.  The reference's run.py defines ``setup_seed`` and never calls it; here ``--seed N`` calls it
(no flag: unseeded, as the reference runs)."""
import argparse
import os

from .config import DEFAULT_CONFIG, load_config
from .slam import DF_Prior, setup_seed


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Arguments for running the code.')
    parser.add_argument('config', type=str, help='Path to config file.')
    parser.add_argument('--input_folder', type=str, help='input folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--output', type=str, help='output folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--tsdf_volume', type=str, help='prior TSDF volume file (default: <dataset>_tsdf_volume/<scene>_tsdf_volume.pt)')
    parser.add_argument('--tsdf_bounds', type=str, help='bounds file of the TSDF volume (default: <dataset>_tsdf_volume/<scene>_bounds.pt)')
    parser.add_argument('--prior', choices=('file', 'online'), default='file',
                        help='file: the volume fused beforehand from the ground-truth poses; online: fused during the run from the estimated poses')
    parser.add_argument('--prior_voxel_size', type=float, default=4.0 / 256, help='voxel edge of the online prior volume in metres')
    parser.add_argument('--seed', type=int, help='seed torch, numpy and random before anything is initialised')
    parser.add_argument('--last_frame', type=int, help='end the run at this frame index')
    parser.add_argument('--no_prefetch', action='store_true', help='decode every frame when it is needed instead of one frame ahead')
    parser.add_argument('--default_config', type=str, default=DEFAULT_CONFIG, help='the config every other one inherits from')
    parser.add_argument('--tracking_init', choices=('guess', 'icp'),
                        help="replaces the config's tracking.init: guess = the constant-speed guess as it is; icp = the guess refined by "
                             'point-to-plane ICP of the depth image against the TSDF prior (icp.DepthICP)')
    parser.add_argument('--tracking_rgb_weight', type=float, metavar='W',
                        help="replaces the config's tracking.icp_rgb.weight: W > 0 adds a photometric term against the last tracked frame "
                             'to every ICP step (icp.RgbdICP; needs tracking.init icp), 0 turns it off')
    parser.add_argument('--tracking_icp_bilateral', action='store_true',
                        help="sets the config's tracking.icp.bilateral to its defaults where the config has none: the sensor depth goes "
                             'through a bilateral filter before the ICP takes its normals (icp.depth_bilateral; needs tracking.init icp)')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    cfg = load_config(args.config, args.default_config if os.path.exists(args.default_config) else None)
    if args.tracking_init is not None:
        cfg.setdefault('tracking', {})['init'] = args.tracking_init
    if args.tracking_rgb_weight is not None:
        t = cfg.setdefault('tracking', {})
        t['icp_rgb'] = dict(t.get('icp_rgb') or {}, weight=args.tracking_rgb_weight)
    if args.tracking_icp_bilateral:
        t = cfg.setdefault('tracking', {})
        if t.get('init', 'guess') != 'icp':
            raise ValueError('--tracking_icp_bilateral needs tracking.init: icp')
        t['icp'] = dict(t.get('icp') or {})
        if not t['icp'].get('bilateral'):
            t['icp']['bilateral'] = {}
    if args.seed is not None:
        setup_seed(args.seed)
    slam = DF_Prior(cfg, args)
    slam.run()
    return slam


if __name__ == '__main__':
    main()
