"""The replay's line overlay on the MI355X (attentive_dfprior_amd.replay, render_mesh.draw_segments) beside the render it sits on.

On tools/recon_bench.py's room (a 512^3 lattice, ~1 M faces) in Replica's frame, 680 x 1200, with trajectories of 200 and 2 000
poses (estimated and ground truth) and the two frusta of every view:

  * per view, over one chunk of --views follow cameras: render_hits, adfp_shade_hits and adfp_draw_segments (its two launches
    together) between device events -- the overlay with every view drawing the whole trajectory (the last frame of a run, the most
    a view ever draws) and with the prefixes of frames spread evenly over the run (what a replay draws on average);
  * the whole replay of a run directory written for the purpose (the mesh as a PLY, a checkpoint): frames per second with the mesh
    read, the BVH build, the downloads and the PNG writing, over --frames frames.

Device legs: one warm-up, then --reps repetitions, min / median / max.  Writes profiles/replay_bench.json (or --out) and prints the
same JSON line.

    python tools/replay_bench.py [--reps 7] [--views 20] [--frames 100] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, 'tools')]
DEV = 'cuda:0'
CAM = (680, 1200, 600.0, 600.0, 599.5, 339.5)           # Replica's frame
TARGET = np.array([0.6, -0.3, -0.2])                     # the room's ball


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'min_ms': round(min(ms), 4), 'median_ms': round(float(np.median(ms)), 4), 'max_ms': round(max(ms), 4)}


def trajectory(n, drift=0.0):
    """n poses (OpenCV axes) on a loop through the room, looking at the ball; `drift` pulls the loop outward as it goes."""
    from attentive_dfprior_amd import replay
    t = np.linspace(0.0, 1.0, n)
    g = 1.0 + drift * t
    pos = np.stack([1.1 * g * np.cos(2 * np.pi * 2 * t), 0.7 * g * np.sin(2 * np.pi * 3 * t), 0.3 + 0.2 * np.sin(2 * np.pi * 5 * t)], 1)
    return np.stack([replay._pose(TARGET - p, np.array([0.0, 0.0, -1.0]), p) for p in pos])


def stored(p):
    q = np.array(p, dtype=np.float64)
    q[:, :3, 1] *= -1.0
    q[:, :3, 2] *= -1.0
    return torch.from_numpy(q).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--frames', type=int, default=100, help='frames of the whole-replay leg')
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'replay_bench.json'))
    a = ap.parse_args()
    import recon_bench
    from attentive_dfprior_amd import mesh, render_mesh, replay

    H, W, fx, fy, cx, cy = CAM
    out = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'views': a.views, 'H': H, 'W': W}
    v, f = recon_bench.room(a.res)
    out['faces'], out['verts'] = int(f.shape[0]), int(v.shape[0])
    mv = render_mesh.MeshViews(v, f, None, DEV)
    for n in (200, 2000):
        r = out[f'poses_{n}'] = {}
        est, gt = trajectory(n), trajectory(n, 0.08)
        for name, frames in (('last_frame', [n - 1] * a.views), ('spread', [int(k) for k in np.linspace(0, n - 1, a.views)])):
            views = np.stack([replay.follow_pose(est[k], 0.6, 0.3) for k in frames])
            segs, colors, ranges = replay.overlay_lists(est, gt, frames, CAM, 0.2)
            segs_d, colors_d = torch.from_numpy(segs).to(DEV), torch.from_numpy(colors).to(DEV)        # the ranges go up per call, as in replay()
            leg = r[name] = {'segments_in_list': int(len(segs)), 'listed_per_view_max': int((ranges[..., 1] - ranges[..., 0]).sum(1).max()),
                             'listed_per_view_mean': round(float((ranges[..., 1] - ranges[..., 0]).sum(1).mean()), 1)}
            leg['render_hits'] = timed(lambda: mv.bvh.render_hits(views, H, W, fx, fy, cx, cy, mv.near, replay.FAR), a.reps)
            h = mv.bvh.render_hits(views, H, W, fx, fy, cx, cy, mv.near, replay.FAR)
            leg['shade_hits'] = timed(lambda: mv.shade(h['face'], h['bary'], views, fx, fy, cx, cy, want=('rgb',)), a.reps)
            rgb = mv.shade(h['face'], h['bary'], views, fx, fy, cx, cy, want=('rgb',))['rgb']
            leg['draw_segments'] = timed(lambda: render_mesh.draw_segments(rgb, h['depth'], views, fx, fy, cx, cy, segs_d, colors_d, ranges),
                                         a.reps)
            seg = render_mesh.draw_segments(rgb, h['depth'], views, fx, fy, cx, cy, segs_d, colors_d, ranges, want_seg=True)
            leg['pixels_with_a_line'] = round(float((seg >= 0).float().mean()), 5)
            base = leg['render_hits']['median_ms'] + leg['shade_hits']['median_ms']
            leg['per_view_ms'] = {'render': round(base / a.views, 4), 'overlay': round(leg['draw_segments']['median_ms'] / a.views, 4)}
            leg['overlay_over_render'] = round(leg['draw_segments']['median_ms'] / base, 4)
            del h, rgb, seg
        # the whole replay of a run directory: `frames` frames spread over the run
        every = max(1, n // a.frames)
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, 'ckpts'))
            os.makedirs(os.path.join(d, 'mesh'))
            mesh.write_ply(os.path.join(d, 'mesh', '00000_mesh.ply'), v.cpu().numpy(), f.cpu().numpy())
            torch.save({'estimate_c2w_list': stored(est), 'gt_c2w_list': stored(gt), 'idx': n - 1}, os.path.join(d, 'ckpts', f'{n - 1:05d}.tar'))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            paths = replay.replay({'scale': 1.0}, d, every=every, back=0.6, up=0.3, cam=CAM, device=DEV, chunk=a.views)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            r['whole_replay'] = {'frames': len(paths), 'every': every, 'seconds': round(dt, 3), 'frames_per_s': round(len(paths) / dt, 2),
                                 'png_bytes_mean': int(np.mean([os.path.getsize(p) for p in paths]))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
