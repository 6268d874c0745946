"""Frame ingestion, host chain against device route, at the two frames the reference's configs use:

  replica   680 x 1200 colour and depth, same size, no crop (1 colour tap per pixel)
  scannet   968 x 1296 colour resized to the 480 x 640 depth frame, crop_edge 10 (4 taps)

  host      what the reference's BaseDataset.__getitem__ does from the decoded bytes on (tests/ingest_ref.py: numpy f64 for / 255 and
            the cv2.resize rule on one thread, torch's CPU F.interpolate where crop_size is set) plus the float64 colour / float32
            depth upload, ended by a device synchronise
  device    datasets.FrameIngest on the same host arrays: staging copy, 5-byte-per-pixel upload, one launch; 1 frame and 8 frames
            per launch, ended by a device synchronise
  launch    adfp_ingest_frames alone on device-resident inputs, device events around `--iters` back-to-back launches; the bytes the
            chain has to move (decoded inputs once + outputs once) over that time

  tum       480 x 640 colour and depth, crop_size [384, 512], crop_edge 8, freiburg1's calibration: the launch that undistorts
            (adfp_ingest_frames_undistort, datasets.FrameIngest(undistort='device')) beside the plain launch of the same geometry
            and beside the numpy statement of the rule on the host (tests/undistort_ref.py), 1 frame and 8 frames per launch

The two sides alternate within a repetition; median (min, spread = max - min) of `--reps` repetitions.  The device result is held to
the host's at the tests' bounds before anything is timed.

    python tools/ingest_bench.py [--reps 7] [--iters 200] [--json profiles/ingest_bench.json] [--tum-only]

For the kernel's own time, a trace run of its own per batch size (profiles/ingest_kernels_1.csv, ingest_kernels_8.csv):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ingest_bench.py --launch-only 8
    python profiles/summarize.py DIR profiles/ingest_kernels_8.csv
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import ingest_ref                                              # noqa: E402
import undistort_ref                                           # noqa: E402
from attentive_dfprior_amd.datasets import FrameIngest, undistort_map         # noqa: E402

DEV = 'cuda:0'
GEOMETRIES = {'replica': dict(color=(680, 1200), depth=(680, 1200), edge=0, png=6553.5),
              'scannet': dict(color=(968, 1296), depth=(480, 640), edge=10, png=1000.0)}
BATCH = 8


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


def launch_only(g, n, iters):
    """`iters` launches of n frames on device-resident inputs and nothing else: what a kernel trace should see."""
    rng = np.random.RandomState(1)
    cam = {'H': g['depth'][0], 'W': g['depth'][1], 'png_depth_scale': g['png'], 'crop_edge': g['edge']}
    ing = FrameIngest(cam, 1.0, DEV, color_order='bgr')
    H, W = ing.out_shape
    dcol = [torch.from_numpy(rng.randint(0, 256, g['color'] + (3,), dtype=np.uint8)).to(DEV) for _ in range(n)]
    ddep = [torch.from_numpy(rng.randint(0, 32768, g['depth']).astype(np.int16)).to(DEV) for _ in range(n)]
    oc = torch.empty((n, H, W, 3), dtype=torch.float32, device=DEV)
    od = torch.empty((n, H, W), dtype=torch.float32, device=DEV)
    for _ in range(iters):
        ing.batch(dcol, ddep, out=(oc, od))
    torch.cuda.synchronize()


def bench(name, g, reps, iters):
    rng = np.random.RandomState(1)
    frames = [(rng.randint(0, 256, g['color'] + (3,), dtype=np.uint8), rng.randint(0, 65536, g['depth']).astype(np.uint16)) for _ in range(BATCH)]
    color, depth = frames[0]
    cam = {'H': g['depth'][0], 'W': g['depth'][1], 'png_depth_scale': g['png'], 'crop_edge': g['edge']}
    ing = FrameIngest(cam, 1.0, DEV, color_order='bgr')
    ing64 = FrameIngest(cam, 1.0, DEV, color_order='bgr', color_dtype=torch.float64)
    H, W = ing.out_shape

    def host_chain():
        c, d = ingest_ref.ingest(color, depth, g['png'], 1.0, None, g['edge'], 'bgr')
        return torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV)

    # parity at the tests' bounds
    hc, hd = host_chain()
    dc, dd = ing(color, depth)
    dc64, _ = ing64(color, depth)
    err64 = float((dc64 - hc).abs().max())
    err32 = float((dc.double() - hc.float().double()).abs().max())
    parity = bool(torch.equal(dd, hd)) and err64 <= 1e-12 and err32 <= 6e-8

    colors, depths = [c for c, _ in frames], [d for _, d in frames]
    for _ in range(2):                                         # warm both routes and both staging buffers
        host_chain(), ing(color, depth), ing.batch(colors, depths)
    host, dev1, dev8 = [], [], []
    for _ in range(reps):
        host.append(wall(host_chain))
        dev1.append(wall(lambda: ing(color, depth)))
        dev8.append(wall(lambda: ing.batch(colors, depths)) / BATCH)

    # the launch alone, on device-resident inputs and destinations
    dcol = [torch.from_numpy(c).to(DEV) for c in colors]
    ddep = [torch.from_numpy(d.view(np.int16)).to(DEV) for d in depths]
    oc = torch.empty((BATCH, H, W, 3), dtype=torch.float32, device=DEV)
    od = torch.empty((BATCH, H, W), dtype=torch.float32, device=DEV)
    l1 = events(lambda: ing(dcol[0], ddep[0], out=(oc[0], od[0])), iters)
    l8 = events(lambda: ing.batch(dcol, ddep, out=(oc, od)), iters)
    bytes_frame = color.nbytes + depth.nbytes + H * W * 16                  # decoded inputs once, f32 colour and depth out once
    res = {'color': list(g['color']), 'depth': list(g['depth']), 'crop_edge': g['edge'], 'out': [H, W], 'parity_ok': parity,
           'max_abs_diff_f64': err64, 'max_abs_diff_f32': err32,
           'host_chain': stats(host), 'device_1_frame': stats(dev1), 'device_8_frames_per_frame': stats(dev8),
           'host_over_device_median': stats(host)['median_ms'] / stats(dev1)['median_ms'],
           'upload_bytes_host_route': H * W * 28, 'upload_bytes_device_route': color.nbytes + depth.nbytes,
           'launch': {'bytes_per_frame': bytes_frame, 'ms_1_frame': l1, 'ms_8_frames': l8, 'ms_per_frame_of_8': l8 / BATCH,
                      'gbps_1_frame': bytes_frame / (l1 * 1e-3) / 1e9, 'gbps_8_frames': BATCH * bytes_frame / (l8 * 1e-3) / 1e9}}
    h, d1, d8 = res['host_chain'], res['device_1_frame'], res['device_8_frames_per_frame']
    print(f'{name}: host {h["median_ms"]:.2f} ms ({h["min_ms"]:.2f}, {h["spread_ms"]:.2f})  device {d1["median_ms"]:.3f} ({d1["min_ms"]:.3f}, '
          f'{d1["spread_ms"]:.3f})  8 per launch {d8["median_ms"]:.3f} per frame  launch alone {l1 * 1e3:.1f} us, {l8 / BATCH * 1e3:.1f} us per frame of 8 '
          f'({res["launch"]["gbps_8_frames"]:.0f} GB/s)  parity {parity}', flush=True)
    return res


def bench_tum(reps, iters):
    """The undistorting launch beside the plain one of the same geometry (device-resident inputs, device events), and the whole
    route from host arrays beside the numpy statement."""
    hw, fx, fy, cx, cy, dist = undistort_ref.FREIBURG1
    crop, edge, png = (384, 512), 8, 5000.0
    rng = np.random.RandomState(1)
    frames = [(rng.randint(0, 256, hw + (3,), dtype=np.uint8), rng.randint(0, 65536, hw).astype(np.uint16)) for _ in range(BATCH)]
    color, depth = frames[0]
    cam = {'H': hw[0], 'W': hw[1], 'png_depth_scale': png, 'crop_edge': edge, 'crop_size': list(crop),
           'fx': fx, 'fy': fy, 'cx': cx, 'cy': cy, 'distortion': dist}
    plain = FrameIngest(cam, 1.0, DEV, color_order='bgr')
    lens = FrameIngest(cam, 1.0, DEV, color_order='bgr', undistort='device')
    lens64 = FrameIngest(cam, 1.0, DEV, color_order='bgr', color_dtype=torch.float64, undistort='device')
    H, W = lens.out_shape
    t0 = time.perf_counter()
    lens_map = undistort_ref.undistort_map(hw, fx, fy, cx, cy, dist)
    map_numpy_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    undistort_map(hw, fx, fy, cx, cy, dist)
    map_library_ms = (time.perf_counter() - t0) * 1e3           # adfp_undistort_map on the host, once per dataset

    def host_chain():
        c, d = ingest_ref.ingest(undistort_ref.remap(color, lens_map), depth, png, 1.0, crop, edge, 'bgr')
        return torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV)

    hc, hd = host_chain()
    dc, dd = lens(color, depth)
    dc64, _ = lens64(color, depth)
    err64 = float((dc64 - hc).abs().max())
    err32 = float((dc.double() - hc.float().double()).abs().max())
    same_bytes = bool(np.array_equal(lens.undistort(color).cpu().numpy(), undistort_ref.remap(color, lens_map)))
    same_map = bool(np.array_equal(lens._map(hw).cpu().numpy(), lens_map))
    parity = bool(torch.equal(dd, hd)) and err64 <= 1e-12 and err32 <= 6e-8 and same_bytes and same_map

    colors, depths = [c for c, _ in frames], [d for _, d in frames]
    for _ in range(2):
        host_chain(), lens(color, depth), lens.batch(colors, depths), plain(color, depth), plain.batch(colors, depths)
    host, dev1, dev8, pl1, pl8 = [], [], [], [], []
    for _ in range(reps):
        host.append(wall(host_chain))
        wall(lambda: plain(color, depth))                       # untimed: the first device call after the host's 30 ms pays for the idle device
        dev1.append(wall(lambda: lens(color, depth)))
        pl1.append(wall(lambda: plain(color, depth)))
        dev8.append(wall(lambda: lens.batch(colors, depths)) / BATCH)
        pl8.append(wall(lambda: plain.batch(colors, depths)) / BATCH)

    dcol = [torch.from_numpy(c).to(DEV) for c in colors]
    ddep = [torch.from_numpy(d.view(np.int16)).to(DEV) for d in depths]
    oc = torch.empty((BATCH, H, W, 3), dtype=torch.float32, device=DEV)
    od = torch.empty((BATCH, H, W), dtype=torch.float32, device=DEV)
    launch = {}
    for _ in range(2):                                          # the two kernels in turn, twice: the second pass is reported
        for name, ing in (('plain', plain), ('undistort', lens)):
            launch[name] = {'ms_1_frame': events(lambda: ing(dcol[0], ddep[0], out=(oc[0], od[0])), iters),
                            'ms_8_frames': events(lambda: ing.batch(dcol, ddep, out=(oc, od)), iters)}
    res = {'color': list(hw), 'depth': list(hw), 'crop_size': list(crop), 'crop_edge': edge, 'out': [H, W], 'distortion': dist,
           'parity_ok': parity, 'max_abs_diff_f64': err64, 'max_abs_diff_f32': err32, 'undistorted_bytes_equal': same_bytes,
           'map_equal': same_map, 'map_numpy_ms': map_numpy_ms, 'map_library_ms': map_library_ms,
           'host_statement': stats(host), 'device_1_frame': stats(dev1), 'device_8_frames_per_frame': stats(dev8),
           'plain_device_1_frame': stats(pl1), 'plain_device_8_frames_per_frame': stats(pl8), 'launch': launch,
           'launch_undistort_over_plain_1_frame': launch['undistort']['ms_1_frame'] / launch['plain']['ms_1_frame'],
           'launch_undistort_over_plain_8_frames': launch['undistort']['ms_8_frames'] / launch['plain']['ms_8_frames']}
    print(f'tum: host statement {stats(host)["median_ms"]:.2f} ms  device {stats(dev1)["median_ms"]:.3f} (plain {stats(pl1)["median_ms"]:.3f})  '
          f'8 per launch {stats(dev8)["median_ms"]:.3f} per frame (plain {stats(pl8)["median_ms"]:.3f})  launch alone '
          f'{launch["undistort"]["ms_1_frame"] * 1e3:.1f} us (plain {launch["plain"]["ms_1_frame"] * 1e3:.1f}), 8 frames '
          f'{launch["undistort"]["ms_8_frames"] * 1e3:.1f} us (plain {launch["plain"]["ms_8_frames"] * 1e3:.1f})  parity {parity}', flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--json', default=None)
    ap.add_argument('--launch-only', type=int, default=0, metavar='N', help='only --iters launches of N frames per geometry (for a kernel trace)')
    ap.add_argument('--tum-only', action='store_true', help="only the TUM leg; with --json, the file's other legs are kept")
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ingest_bench needs a GPU'
    if a.launch_only:
        for g in GEOMETRIES.values():
            launch_only(g, a.launch_only, a.iters)
        return 0
    host = {'cpus': len(os.sched_getaffinity(0)), 'torch_threads': torch.get_num_threads()}
    if a.tum_only:                                              # the TUM leg alone, kept beside the other legs of an earlier run
        res = json.load(open(a.json)) if a.json and os.path.exists(a.json) else {'geometries': {}}
    else:
        res = {'host': host, 'frames_per_batch': BATCH, 'reps': a.reps, 'iters': a.iters,
               'geometries': {n: bench(n, g, a.reps, a.iters) for n, g in GEOMETRIES.items()}}
    res['tum'] = dict(bench_tum(a.reps, a.iters), host=host, reps=a.reps, iters=a.iters, frames_per_batch=BATCH)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    ok = all(g['parity_ok'] for g in list(res['geometries'].values()) + [res['tum']])
    print('parity:', 'ok' if ok else 'FAILED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
