"""The Visualizer's work after render_img, host chain against device route, at the two frames the reference's configs use (Replica's
680 x 1200, ScanNet's 460 x 620), from device-resident input images and rendered images:

  host      what the reference's Visualizer does up to the pixels (src/utils/Visualizer.py:43-44, :71-102 and what matplotlib maps
            the arrays to): four downloads (gt_depth f32, gt_color f32, depth f64, color f32) and tests/vis_ref.py's numpy steps --
            residuals, masks, Normalize, the colormap, the float-RGB rule, the canvas -- ended by a device synchronise
  figure    where matplotlib imports: the reference's own six imshows into its 640 x 480 figure and savefig with its arguments,
            into memory as raw RGBA (no encoder); reported separately, from host arrays (the downloads are not in it)
  device    visualizer.Visualizer.panels (two launches, the stats read) and the canvas download, at strides 1 and 2, ended by a
            device synchronise
  launch    the two launches alone, device events around `--iters` back-to-back calls (panels_async: nothing read back)

Image encoding (PIL's jpg / png) is outside all sides.  The sides alternate within a repetition; median (min, spread = max - min)
of `--reps` repetitions.  The device canvas is held to the host's byte for byte before anything is timed.

    python tools/vis_bench.py [--reps 7] [--iters 200] [--json profiles/vis_bench.json]

For the two kernels' own times, a trace run of its own (profiles/vis_kernels.csv):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vis_bench.py --launch-only
    python tools/vis_bench.py --summarize-trace DIR profiles/vis_kernels.csv
(per frame and stride: --launch-only dispatches `--iters` calls per configuration one configuration after the other, so the k-th
block of `--iters` dispatches of a kernel is configuration k.)
"""
import argparse
import csv
import glob
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import vis_ref                                                 # noqa: E402
from attentive_dfprior_amd.visualizer import Visualizer        # noqa: E402

DEV = 'cuda:0'
FRAMES = {'replica': (680, 1200), 'scannet': (460, 620)}
STRIDES = (1, 2)
GAP = 8


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


def figure(plt, gt_depth, gt_color, depth, color):
    """What the reference's Visualizer asks of matplotlib (Visualizer.py:82-118), restated for timing: a 2 x 3 grid of images in
    the default 640 x 480 figure -- the depth row through 'plasma' scaled to [0, max sensor depth], the colour row as clipped float
    RGB -- with a title on each, no ticks and no space between the panels, saved tightly cropped.  Saved into memory as raw RGBA,
    so that no encoder is timed."""
    depth_res, color_res = vis_ref.residuals(gt_depth, gt_color, depth, color)
    top = float(np.max(gt_depth))
    panels = [('Input Depth', gt_depth, dict(vmin=0, vmax=top)), ('Generated Depth', depth, dict(vmin=0, vmax=top)),
              ('Depth Residual', depth_res, dict(vmin=0, vmax=top)),
              ('Input RGB', np.clip(gt_color, 0, 1), {}), ('Generated RGB', np.clip(color, 0, 1), {}), ('RGB Residual', np.clip(color_res, 0, 1), {})]
    fig, axes = plt.subplots(2, 3)
    fig.tight_layout()
    for ax, (title, image, scale) in zip(axes.flat, panels):
        ax.imshow(image, cmap='plasma', **scale)
        ax.set_title(title)
        ax.set(xticks=[], yticks=[])
    fig.subplots_adjust(wspace=0, hspace=0)
    fig.savefig(io.BytesIO(), format='raw', bbox_inches='tight', pad_inches=0.2)
    plt.close(fig)


def launch_only(iters):
    """`iters` calls of the two launches per frame and stride on device-resident inputs and nothing else: what a kernel trace
    should see."""
    with tempfile.TemporaryDirectory() as tmp:
        for hw in FRAMES.values():
            dev = device_frame(hw)
            for stride in STRIDES:
                vis = Visualizer(1, 1, tmp, None, False, DEV, stride=stride, gap=GAP)
                for _ in range(iters):
                    vis.panels_async(*dev)
                torch.cuda.synchronize()


def summarize_trace(d, out, iters):
    """kernel_trace.csv of a --launch-only run -> one row per configuration and kernel."""
    f = glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Dispatch_Id']))
    configs = [(n, s) for n in FRAMES for s in STRIDES]
    with open(out, 'w') as o:
        o.write(f'# source: {os.path.basename(f)} (rocprofv3 --kernel-trace, tools/vis_bench.py --launch-only --iters {iters})\n')
        o.write('frame,stride,kernel,calls,avg_us,median_us,min_us,max_us\n')
        for kernel in ('k_vis_reduce', 'k_vis_panels'):
            us = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows if kernel in r['Kernel_Name']]
            assert len(us) == iters * len(configs), (kernel, len(us))
            for k, (name, stride) in enumerate(configs):
                v = sorted(us[k * iters:(k + 1) * iters])
                o.write('%s,%d,%s,%d,%.1f,%.1f,%.1f,%.1f\n' % (name, stride, kernel, len(v), sum(v) / len(v), v[len(v) // 2], v[0], v[-1]))
    print(open(out).read())


def bench(name, hw, reps, iters, plt, tmp):
    dev = device_frame(hw)
    vis = {s: Visualizer(1, 1, tmp, None, False, DEV, stride=s, gap=GAP) for s in STRIDES}

    def downloads():
        return [t.cpu().numpy() for t in dev]

    def host_chain():
        return vis_ref.canvas(*downloads(), stride=1, gap=GAP)

    def device_route(s):
        canvas, st = vis[s].panels(*dev)
        return canvas.cpu().numpy(), st

    parity = all(np.array_equal(device_route(s)[0], vis_ref.canvas(*downloads(), stride=s, gap=GAP)) for s in STRIDES)
    host_arrays = downloads()
    for _ in range(2):
        host_chain(), [device_route(s) for s in STRIDES]
    if plt is not None:
        figure(plt, *host_arrays)
    t = {'host': [], 'downloads': [], 'figure': [], **{f'device_stride_{s}': [] for s in STRIDES}}
    for _ in range(reps):
        t['host'].append(wall(host_chain))
        for s in STRIDES:
            t[f'device_stride_{s}'].append(wall(lambda: device_route(s)))
        t['downloads'].append(wall(downloads))
        if plt is not None:
            t['figure'].append(wall(lambda: figure(plt, *host_arrays)))
    H, W = hw
    res = {'frame': [H, W], 'gap': GAP, 'parity_ok': bool(parity),
           'host_chain': stats(t['host']), 'host_downloads_alone': stats(t['downloads']),
           'matplotlib_figure': stats(t['figure']) if t['figure'] else None,
           'download_bytes_host_route': H * W * (4 + 12 + 8 + 12), 'input_bytes': H * W * (4 + 12 + 8 + 12), 'by_stride': {}}
    for s in STRIDES:
        rows, cols = vis[s].canvas_shape(H, W)
        la = events(lambda: vis[s].panels_async(*dev), iters)
        d = stats(t[f'device_stride_{s}'])
        res['by_stride'][str(s)] = {'canvas': [rows, cols], 'canvas_bytes': rows * cols * 3, 'device': d, 'launches_ms': la,
                                    'host_over_device_median': res['host_chain']['median_ms'] / d['median_ms'],
                                    'host_numpy_over_device_median': (res['host_chain']['median_ms'] - res['host_downloads_alone']['median_ms']) / d['median_ms']}
    h, dl = res['host_chain'], res['host_downloads_alone']
    fig = res['matplotlib_figure']
    print(f'{name}: host {h["median_ms"]:.2f} ms ({h["min_ms"]:.2f}, {h["spread_ms"]:.2f}), its downloads alone {dl["median_ms"]:.2f}'
          + (f'  figure {fig["median_ms"]:.1f} ms' if fig else '  figure: no matplotlib')
          + ''.join(f'  stride {s}: device {r["device"]["median_ms"]:.3f} ({r["device"]["min_ms"]:.3f}, {r["device"]["spread_ms"]:.3f}), launches '
                    f'{r["launches_ms"] * 1e3:.1f} us' for s, r in res['by_stride'].items()) + f'  parity {parity}', flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--json', default=None)
    ap.add_argument('--launch-only', action='store_true', help='only --iters calls of the two launches per frame and stride (for a kernel trace)')
    ap.add_argument('--summarize-trace', nargs=2, metavar=('DIR', 'OUT'), help='kernel_trace.csv of a --launch-only run -> per-configuration kernel times')
    a = ap.parse_args()
    if a.summarize_trace:
        summarize_trace(a.summarize_trace[0], a.summarize_trace[1], a.iters)
        return 0
    assert torch.cuda.is_available(), 'vis_bench needs a GPU'
    assert a.reps >= 7, 'at least 7 repetitions'
    if a.launch_only:
        launch_only(a.iters)
        return 0
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        mpl = matplotlib.__version__
    except ImportError:
        plt, mpl = None, None
    with tempfile.TemporaryDirectory() as tmp:
        res = {'host': {'cpus': len(os.sched_getaffinity(0)), 'torch_threads': torch.get_num_threads(), 'matplotlib': mpl},
               'reps': a.reps, 'iters': a.iters, 'frames': {n: bench(n, hw, a.reps, a.iters, plt, tmp) for n, hw in FRAMES.items()}}
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    ok = all(g['parity_ok'] for g in res['frames'].values())
    print('parity:', 'ok' if ok else 'FAILED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
