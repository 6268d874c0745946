"""One frame's rendering metrics (PSNR / depth L1 sums, SSIM and CS sums of five levels: the 35 values of adfp_frame_metrics), host
route against device route, at the two frames the reference's configs use (Replica's 680 x 1200, ScanNet's 460 x 620 after its
crop), from device-resident sensor images and rendered images:

  host      four downloads (gt_depth f32, gt_color f32, depth f64, color f32) and the f64 statement of include/adfp.h
            "rendering metrics" on the host: tests/render_ref.py's numpy, and the same statement with scipy.ndimage.correlate1d
            doing the two window passes (the faster host, the one the ratios use), ended by a device synchronise
  device    render_eval.FrameMetrics.add for 1 frame and its download, and for `--frames` frames with one final download (per
            frame), ended by a device synchronise
  launch    the launches of one add alone: device events around `--iters` back-to-back adds (nothing read back)
  pair      Renderer.render_img and render_img + add at the same frame (room0 box room, seeded decoders, N_samples 32 +
            N_surface 16), device events around `--pair-iters` calls: add's share of the pair

The sides alternate within a repetition; median (min, spread = max - min) of `--reps` repetitions.  The device row is held to the
host's (tests/test_gpu_render_eval.py's bounds) before anything is timed.

    python tools/render_eval_bench.py [--reps 7] [--iters 200] [--frames 100] [--json profiles/render_eval_bench.json]

For the kernels' own times, a trace run of its own (profiles/render_eval_kernels.csv):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/render_eval_bench.py --launch-only
    python tools/render_eval_bench.py --summarize-trace DIR profiles/render_eval_kernels.csv
(--launch-only dispatches `--iters` adds per frame one frame after the other, so the k-th block of dispatches is frame k.)
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import render_ref                                              # noqa: E402
import vis_ref                                                 # noqa: E402
from attentive_dfprior_amd.render_eval import FrameMetrics     # noqa: E402

DEV = 'cuda:0'
# frame -> (H, W), (fx, fy, cx, cy): configs/Replica/replica.yaml; configs/ScanNet/scannet.yaml after crop_edge 10
FRAMES = {'replica': ((680, 1200), (600.0, 600.0, 599.5, 339.5)), 'scannet': ((460, 620), (577.590698, 578.729797, 308.905426, 232.683609))}
LEVELS = 5
KERNELS = ('k_vis_reduce', 'k_met_ssim', 'k_met_pool', 'k_met_final')
PER_ADD = {'k_vis_reduce': 1, 'k_met_ssim': LEVELS, 'k_met_pool': LEVELS - 1, 'k_met_final': 1}


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2], 'min_ms': ms[0], 'spread_ms': ms[-1] - ms[0], 'all_ms': ms}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def device_frame(hw):
    return [torch.from_numpy(a).to(DEV) for a in vis_ref.frame(1, hw, np.float32, top=6.0)]


def scipy_rows(gt_depth, gt_color, depth, color, levels):
    """render_ref.rows with scipy.ndimage.correlate1d for the two window passes."""
    from scipy.ndimage import correlate1d
    g = render_ref.window()
    h = render_ref.TAPS // 2

    def blur(img):
        return correlate1d(correlate1d(img, g, axis=1, mode='constant'), g, axis=0, mode='constant')[h:-h, h:-h]

    row = render_ref.rows(gt_depth, gt_color, depth, color, 0)
    x, y = render_ref.images(gt_color, color)
    for k in range(levels):
        mx, my = blur(x), blur(y)
        sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        cs = (2.0 * sxy + render_ref.C2) / (sxx + syy + render_ref.C2)
        ssim = (2.0 * mx * my + render_ref.C1) / (mx * mx + my * my + render_ref.C1) * cs
        row[5 + 6 * k:11 + 6 * k:2], row[6 + 6 * k:11 + 6 * k:2] = ssim.sum(axis=(0, 1)), cs.sum(axis=(0, 1))
        if k + 1 < levels:
            x, y = render_ref.pool(x), render_ref.pool(y)
    return row


def bytes_per_frame(hw):
    """Bytes the launches of one add need to move when every pixel is fetched once per launch that uses it: k_vis_reduce reads the
    four inputs; level 0's k_met_ssim and k_met_pool each read gt_color and color; a pooled level is written once and read by its
    own k_met_ssim and k_met_pool (the aprons and the partials are left out)."""
    sizes = render_ref.level_sizes(hw[0], hw[1], LEVELS)
    px = [h * w for h, w in sizes]
    read = px[0] * (4 + 12 + 8 + 12) + 2 * px[0] * 24 + sum(48 * p for p in px[1:]) + sum(48 * p for p in px[1:-1])
    written = sum(48 * p for p in px[1:])
    return read, written


def ops_per_frame(hw):
    """f64 operations of the SSIM maps: per window position and channel 5 moments x 2 passes x 11 taps x 2 (multiply, add), the
    row pass over 26 / 16 as many rows as the tile has positions, three products, and about 20 for the variances and quotients."""
    return sum(3 * n * (5 * 11 * 2 * (1 + 26 / 16) + 23) for n in render_ref.windows(hw[0], hw[1], LEVELS))


def launch_only(iters):
    for hw, _ in FRAMES.values():
        dev = device_frame(hw)
        fm = FrameMetrics(iters, hw[0], hw[1], LEVELS, DEV)
        for _ in range(iters):
            fm.add(*dev)
        torch.cuda.synchronize()


def summarize_trace(d, out, iters):
    """kernel_trace.csv of a --launch-only run -> one row per frame and kernel: launches per add and their summed time per add."""
    f = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Dispatch_Id']))
    with open(out, 'w') as o:
        o.write(f'# source: {os.path.basename(f)} (rocprofv3 --kernel-trace, tools/render_eval_bench.py --launch-only --iters {iters})\n')
        o.write('frame,kernel,launches_per_add,avg_us_per_add,avg_us_per_launch,min_us_per_launch,max_us_per_launch\n')
        for kernel in KERNELS:
            us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if kernel in r['Kernel_Name']]
            per = PER_ADD[kernel] * iters
            assert len(us) == per * len(FRAMES), (kernel, len(us))
            for k, name in enumerate(FRAMES):
                v = us[k * per:(k + 1) * per]
                o.write('%s,%s,%d,%.1f,%.1f,%.1f,%.1f\n' % (name, kernel, PER_ADD[kernel], sum(v) / iters, sum(v) / len(v), min(v), max(v)))
    print(open(out).read())


def render_pair(name, hw, cam, dev, fm, iters):
    """render_img alone and render_img + add, ms per call by device events."""
    import attentive_dfprior_amd as A
    from attentive_dfprior_amd import synthetic
    sc = synthetic.Scene('room0', H=hw[0], W=hw[1], fx=cam[0], fy=cam[1], cx=cam[2], cy=cam[3], device=DEV, grid_std_scale=20.0)
    sc.c['grid_high'] = sc.c['grid_high'] * 100
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
           'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}
    rend = A.Renderer(cfg, None, sc)
    c2w = sc.default_c2w(yaw=0.7, pitch=-0.15)
    gt_depth = sc.depth_image(c2w)
    gt_color = dev[1]
    tb = sc.tsdf_bnds.to(DEV)

    def render():
        return rend.render_img(sc.c, dec, c2w, DEV, sc.tsdf_volume, tb, 'color', gt_depth=gt_depth)

    def pair():
        depth, _, color = render()
        fm.count = 0
        fm.add(gt_depth, gt_color, depth, color)

    for _ in range(2):
        pair()
    r = [events(render, iters) for _ in range(3)]
    p = [events(pair, iters) for _ in range(3)]
    r2 = [events(render, iters) for _ in range(3)]                      # again: the spread of the same thing
    return {'render_img_ms': sorted(r)[1], 'render_img_again_ms': sorted(r2)[1], 'render_img_and_add_ms': sorted(p)[1], 'iters': iters,
            'rays': hw[0] * hw[1], 'samples_per_ray': 48}


def bench(name, hw, cam, reps, iters, frames, pair_iters):
    dev = device_frame(hw)
    H, W = hw
    one, many, loop = FrameMetrics(1, H, W, LEVELS, DEV), FrameMetrics(frames, H, W, LEVELS, DEV), FrameMetrics(1, H, W, LEVELS, DEV)

    def downloads():
        return [t.cpu().numpy() for t in dev]

    def host_numpy():
        return render_ref.rows(*downloads(), LEVELS)

    def host_scipy():
        return scipy_rows(*downloads(), LEVELS)

    def device_1():
        one.count = 0
        one.add(*dev)
        return one.table()

    def device_many():
        many.count = 0
        for _ in range(frames):
            many.add(*dev)
        return many.table()

    def add_only():
        loop.count = 0
        loop.add(*dev)

    ref, got, alt = host_numpy(), device_1()[0], host_scipy()
    n = np.array(render_ref.windows(H, W, LEVELS)).repeat(6)
    mean_diff = float(np.abs((got[5:] - ref[5:]) / n).max())
    scipy_diff = float(np.abs((alt[5:] - ref[5:]) / n).max())
    parity = bool(mean_diff <= 1e-10 and scipy_diff <= 1e-10 and (got[[0, 3, 4]] == ref[[0, 3, 4]]).all()
                  and (np.abs(got[1:3] - ref[1:3]) <= 1e-10 * np.abs(ref[1:3])).all())
    t = {'host_numpy': [], 'host_scipy': [], 'downloads': [], 'device_1': [], 'device_many': []}
    device_many()
    for _ in range(reps):
        t['host_scipy'].append(wall(host_scipy))
        t['device_1'].append(wall(device_1))
        t['host_numpy'].append(wall(host_numpy))
        t['device_many'].append(wall(device_many) / frames)
        t['downloads'].append(wall(downloads))
    launches = events(add_only, iters)
    read, written = bytes_per_frame(hw)
    res = {'frame': [H, W], 'levels': LEVELS, 'windows': one.windows, 'parity_ok': parity, 'worst_mean_difference': mean_diff,
           'scipy_against_numpy_statement': scipy_diff,
           'host_numpy_statement': stats(t['host_numpy']), 'host_scipy': stats(t['host_scipy']), 'host_downloads_alone': stats(t['downloads']),
           'device_1_frame': stats(t['device_1']), f'device_{frames}_frames_per_frame': stats(t['device_many']), 'frames_per_table': frames,
           'launches_ms': launches, 'launches_per_add': sum(PER_ADD.values()),
           'input_bytes': H * W * (4 + 12 + 8 + 12), 'bytes_read': read, 'bytes_written': written, 'f64_operations': ops_per_frame(hw),
           'workspace_bytes': one._ws_bytes, 'download_bytes_device_route': 35 * 8}
    res['host_over_device_1_median'] = res['host_scipy']['median_ms'] / res['device_1_frame']['median_ms']
    res['host_over_device_many_median'] = res['host_scipy']['median_ms'] / res[f'device_{frames}_frames_per_frame']['median_ms']
    res['pair'] = render_pair(name, hw, cam, dev, loop, pair_iters)
    pr = res['pair']
    pr['add_ms_by_difference'] = pr['render_img_and_add_ms'] - pr['render_img_ms']
    pr['add_share_of_pair_by_launches'] = launches / (pr['render_img_ms'] + launches)
    h, d1, dm = res['host_scipy'], res['device_1_frame'], res[f'device_{frames}_frames_per_frame']
    print(f'{name}: host scipy {h["median_ms"]:.1f} ms ({h["min_ms"]:.1f}, {h["spread_ms"]:.1f}), numpy statement {res["host_numpy_statement"]["median_ms"]:.1f}, '
          f'downloads alone {res["host_downloads_alone"]["median_ms"]:.2f}; device 1 frame {d1["median_ms"]:.3f} ({d1["min_ms"]:.3f}, {d1["spread_ms"]:.3f}), '
          f'{frames} frames {dm["median_ms"]:.3f} per frame, launches {launches * 1e3:.1f} us; render_img {pr["render_img_ms"]:.2f} ms, with add '
          f'{pr["render_img_and_add_ms"]:.2f} ms, add share {100 * pr["add_share_of_pair_by_launches"]:.1f} %; parity {parity} ({mean_diff:.1e})', flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--pair-iters', type=int, default=10)
    ap.add_argument('--json', default=None)
    ap.add_argument('--launch-only', action='store_true', help='only --iters adds per frame (for a kernel trace)')
    ap.add_argument('--summarize-trace', nargs=2, metavar=('DIR', 'OUT'), help='kernel_trace.csv of a --launch-only run -> per-frame kernel times')
    a = ap.parse_args()
    if a.summarize_trace:
        summarize_trace(a.summarize_trace[0], a.summarize_trace[1], a.iters)
        return 0
    assert torch.cuda.is_available(), 'render_eval_bench needs a GPU'
    if a.launch_only:
        launch_only(a.iters)
        return 0
    assert a.reps >= 7, 'at least 7 repetitions'
    import scipy
    res = {'host': {'cpus': len(os.sched_getaffinity(0)), 'torch_threads': torch.get_num_threads(), 'numpy': np.__version__, 'scipy': scipy.__version__},
           'reps': a.reps, 'iters': a.iters,
           'frames': {n: bench(n, hw, cam, a.reps, a.iters, a.frames, a.pair_iters) for n, (hw, cam) in FRAMES.items()}}
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    ok = all(g['parity_ok'] for g in res['frames'].values())
    print('parity:', 'ok' if ok else 'FAILED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
