"""Where a frame's time goes in a whole run (attentive_dfprior_amd.slam): a synthetic sequence at Replica's frame size
(680 x 1200) in room0's bound, with configs/df_prior.yaml's iteration counts (tracking 10 x 200 pixels; mapping 1500 first, then
60 x 1000 pixels every 5th frame, window 5, colour refinement on the last frame).  No thresholds.

    python tools/run_bench.py [--frames 21] [--out profiles/run_bench.json] [--default_config tests/golden/configs/df_prior.yaml]

Three runs of the same sequence and seed, DF_Prior.measure on (a device synchronise at every frame end, so wall times are
per-frame times): the fused prior decoded ahead, the same without decode-ahead, and --prior online.  Reported:
  track_frame_ms / map_frame_ms   wall time of a tracked frame (fetch + tracking) and of an ordinary mapped frame's mapping (not
                                  frame 0, not the last frame), medians;
  decode_ms                       host decode of one frame (JPEG + PNG, PIL or cv2), and how long the loop waited for it, with
                                  and without decode-ahead;
  track_gpu_ms, gpu_idle_share    the tracked frame's iterations replayed back to back between two device events -- an UPPER
                                  bound of the GPU's busy time in a tracked frame -- and 1 - that / track_frame_ms;
  online_prior                    per mapped frame: one integrate and one re-lay of the corner-block copy, each timed alone
                                  with synchronises, beside map_frame_ms, and the difference of the two runs' mapped frames.
The sequence is the box room of the tests scaled to room0: depth in closed form, colour a smooth function of the hit point."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from attentive_dfprior_amd import config, datasets, fusion, slam, synthetic  # noqa: E402

H, W, FX, FY, CX, CY, PNG = 680, 1200, 600.0, 600.0, 599.5, 339.5, 6553.5
BOUND = synthetic.SCENE_BOUNDS['room0']
LO = np.array([b[0] + 0.4 for b in BOUND])
HI = np.array([b[1] - 0.4 for b in BOUND])
DEV = 'cuda:0'


def pose_cv(k):
    a = 0.25 + 0.02 * k
    eye = (LO + HI) / 2 + np.array([0.5 * np.cos(a), 0.5 * np.sin(a), 0.005 * k])
    f = np.array([np.cos(a + 0.4), np.sin(a + 0.4), -0.15])
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, np.cross(f, r), f, eye
    return m


def frame_images(c2w):
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones_like(u)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide='ignore'):
        t = np.where(d > 0, (HI - o) / d, np.where(d < 0, (LO - o) / d, np.inf)).min(-1)
    hit = o + t[..., None] * d
    color = 0.5 + 0.4 * np.sin(hit * np.array([1.3, 1.7, 2.1]) + np.array([0.0, 1.0, 2.0]))
    return t, np.clip(np.rint(color * 255), 0, 255).astype(np.uint8)


def write_dataset(root, n):
    from PIL import Image
    os.makedirs(os.path.join(root, 'results'))
    lines = []
    for k in range(n):
        c2w = pose_cv(k)
        depth, color = frame_images(c2w)
        Image.fromarray(color).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(np.clip(np.rint(depth * PNG), 0, 65535).astype(np.uint16)).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
        lines.append(' '.join(repr(float(x)) for x in c2w.reshape(-1)))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def scene(root, out):
    return {'dataset': 'replica', 'verbose': False, 'low_gpu_mem': False, 'pretrained_decoders': {'low_high': None},
            'data': {'dataset': 'replica', 'id': 'bench', 'input_folder': root, 'output': out},
            'cam': {'H': H, 'W': W, 'fx': FX, 'fy': FY, 'cx': CX, 'cy': CY, 'png_depth_scale': PNG, 'crop_edge': 0},
            'meshing': {'resolution': 128, 'eval_rec': False},
            'tracking': {'gt_camera': False},
            'mapping': {'bound': BOUND, 'marching_cubes_bound': BOUND}}


def med(xs):
    return statistics.median(xs) * 1e3 if xs else float('nan')


def one_run(base, root, name, default, extra):
    out = os.path.join(base, name)
    path = os.path.join(base, f'{name}.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(scene(root, out), f)
    cfg = config.load_config(path, default)
    args = SimpleNamespace(input_folder=None, output=None, tsdf_volume=None, tsdf_bounds=None, prior='file', prior_voxel_size=4.0 / 256,
                           last_frame=None, no_prefetch=False)
    for k, v in extra.items():
        setattr(args, k, v)
    slam.setup_seed(0)
    t0 = time.perf_counter()
    s = slam.DF_Prior(cfg, args)
    s.measure = True
    s.run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ft = s.frame_times
    n = s.n_img
    tracked = [f for f in ft if 0 < f['idx']]
    ordinary = [f for f in ft if f['mapped'] and 0 < f['idx'] < n - 1]
    res = {'frames': n, 'wall_s': wall, 'track_frame_ms': med([f['fetch_s'] + f['track_s'] for f in tracked]),
           'track_only_ms': med([f['track_s'] for f in tracked]), 'fetch_ms': med([f['fetch_s'] for f in tracked]),
           'track_frame_after_map_ms': med([f['fetch_s'] + f['track_s'] for f in tracked if f['idx'] % cfg['mapping']['every_frame'] == 1]),
           'map_frame_ms': med([f['map_s'] for f in ordinary]), 'map_first_frame_ms': ft[0]['map_s'] * 1e3, 'map_last_frame_ms': ft[-1]['map_s'] * 1e3,
           'decode_ms': s.feed.decode_s / s.feed.frames * 1e3, 'decode_wait_ms': s.feed.wait_s / s.feed.frames * 1e3,
           'prior_host_ms': med([f['prior_host_s'] for f in ordinary]), 'ate_rmse_m': s.ate['absolute_translational_error.rmse'] if s.ate else None}
    return s, cfg, res


def main(argv=None):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = argparse.ArgumentParser()
    p.add_argument('--frames', type=int, default=21)
    p.add_argument('--out', default=os.path.join(here, 'profiles', 'run_bench.json'))
    p.add_argument('--default_config', default=os.path.join(here, 'tests', 'golden', 'configs', 'df_prior.yaml'))
    a = p.parse_args(argv)
    result = {'frame': [H, W], 'bound': 'room0', 'device': torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as base:
        root = os.path.join(base, 'seq')
        write_dataset(root, a.frames)
        cfg0 = config.load_config(_yaml(base, scene(root, os.path.join(base, 'unused'))), a.default_config)
        result['iterations'] = {'tracking': [cfg0['tracking']['iters'], cfg0['tracking']['pixels']],
                                'mapping': [cfg0['mapping']['iters_first'], cfg0['mapping']['iters'], cfg0['mapping']['pixels'], cfg0['mapping']['every_frame']]}
        # the fused prior, from the true poses of every 5th frame (get_tsdf's --space would be 10 on a real sequence)
        ds = datasets.get_dataset(cfg0, SimpleNamespace(input_folder=None), 1, device=DEV)
        bound = synthetic.scene_bound(BOUND, 0.32, 1).numpy()
        vol = fusion.TSDFVolume(bound, voxel_size=4.0 / 256, device=DEV)
        K = np.array([[FX, 0., CX], [0., FY, CY], [0., 0., 1.]])
        for k in range(0, a.frames, 5):
            _, color, depth, pose = ds[k]
            m = pose.cpu().numpy().copy()
            m[:3, 1] *= -1.0
            m[:3, 2] *= -1.0
            vol.integrate(torch.floor(color * 255), depth, K, m, obs_weight=1.)
        tsdf, bnds = vol.get_render_volume()
        result['volume'] = [int(v) for v in vol._vol_dim]
        files = {'tsdf_volume': os.path.join(base, 'vol.pt'), 'tsdf_bounds': os.path.join(base, 'bounds.pt')}
        torch.save(tsdf.cpu(), files['tsdf_volume'])
        torch.save(bnds.numpy(), files['tsdf_bounds'])
        del vol, tsdf, ds
        torch.cuda.empty_cache()

        s, cfg, result['decode_ahead'] = one_run(base, root, 'ahead', a.default_config, files)
        # the tracked frame's iterations replayed back to back: an upper bound of the GPU's busy time in a tracked frame
        it, iters, pixels = s.tracker.iteration, cfg['tracking']['iters'], cfg['tracking']['pixels']
        gpu = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                it.step(pixels)
            e1.record()
            torch.cuda.synchronize()
            gpu.append(e0.elapsed_time(e1))
        r = result['decode_ahead']
        r['track_gpu_ms'] = statistics.median(gpu)
        r['gpu_idle_share'] = 1.0 - r['track_gpu_ms'] / r['track_frame_ms']
        del s, it
        torch.cuda.empty_cache()

        s, cfg, result['no_decode_ahead'] = one_run(base, root, 'not_ahead', a.default_config, dict(files, no_prefetch=True))
        r = result['no_decode_ahead']
        r['gpu_idle_share'] = 1.0 - result['decode_ahead']['track_gpu_ms'] / r['track_frame_ms']
        del s
        torch.cuda.empty_cache()

        s, cfg, result['online_prior'] = one_run(base, root, 'online', a.default_config, {'prior': 'online'})
        # one integrate and one re-lay of the corner-block copy, each alone
        _, color, depth, pose = s.frame_reader[5]
        m = pose.cpu().numpy().copy()
        m[:3, 1] *= -1.0
        m[:3, 2] *= -1.0
        col = torch.floor(color * 255)
        integ, relay = [], []
        mit = next(iter(s.mapper._iterations.values()))
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.prior.integrate(col, depth, K, m, obs_weight=1.)
            torch.cuda.synchronize()
            integ.append(time.perf_counter() - t0)
            if mit._cb is not None:
                t0 = time.perf_counter()
                s.renderer._engine.refresh_tsdf_blocks(s.tsdf_volume_shared, mit._cb)
                torch.cuda.synchronize()
                relay.append(time.perf_counter() - t0)
        r = result['online_prior']
        r['integrate_ms'] = med(integ)
        r['relay_corner_blocks_ms'] = med(relay) if relay else None
        r['corner_block_bytes'] = int(mit._cb.numel() * 4) if mit._cb is not None else 0
        r['map_frame_minus_fused_prior_ms'] = r['map_frame_ms'] - result['decode_ahead']['map_frame_ms']
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result))
    return result


def _yaml(base, d):
    path = os.path.join(base, 'cfg0.yaml')
    with open(path, 'w') as f:
        yaml.safe_dump(d, f)
    return path


if __name__ == '__main__':
    main()
