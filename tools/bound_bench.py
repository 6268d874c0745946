"""The mesh bound, host route (Mesher.get_bound_planes: numpy back-projection, Qhull per keyframe and over the union) against the
device route (Mesher.bound_planes: mesh.depth_hull's rounds over the resident depth block), both in this one run, alternating,
wall clock with a device synchronisation on both ends; milliseconds, median (min, spread = max - min) of the repetitions.

  (a) tools/mesh_bench.py's own: 4 keyframes of 480 x 640, the noise-free synthetic room0
  (b) Replica at the end of a run: 40 keyframes of 680 x 1200, 1 % depth noise
  (c) ScanNet at the end of a run: 1 000 keyframes of 480 x 640, 1 % depth noise; the host side is timed once

Also: the rounds, the survivors per round and Qhull's share of the device route, the same route at other direction counts D
(mesh.BOUND_DIRECTIONS is the default), and bound_planes' share of a whole get_mesh at 256^3 and 512^3 on workload (a).

    python tools/bound_bench.py [--workloads a b c] [--reps 5] [--directions 64 128 256 512] [--res 256 512] [--device-only]
                                [--out profiles/mesh_bound_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import attentive_dfprior_amd as A                     # noqa: E402
from attentive_dfprior_amd import mesh, synthetic      # noqa: E402
from attentive_dfprior_amd.keyframes import KeyframeStore      # noqa: E402
from attentive_dfprior_amd.mesher import Mesher        # noqa: E402
import bound_clouds as BC                              # noqa: E402

DEV = 'cuda:0'
WORKLOADS = {'a': dict(K=4, H=480, W=640, fx=577.6, fy=577.6, cx=319.5, cy=239.5, noise=0.0, host_reps=None,
                       what="mesh_bench's own: 4 keyframes of 480 x 640, noise-free room0"),
             'b': dict(K=40, H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5, noise=0.01, host_reps=3,
                       what='Replica at the end of a run: 40 keyframes of 680 x 1200, 1 % depth noise'),
             'c': dict(K=1000, H=480, W=640, fx=577.6, fy=577.6, cx=319.5, cy=239.5, noise=0.01, host_reps=1,
                       what='ScanNet at the end of a run: 1 000 keyframes of 480 x 640, 1 % depth noise; host side timed once')}


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(x):
    return {'min_ms': round(min(x), 3), 'median_ms': round(float(np.median(x)), 3), 'spread_ms': round(max(x) - min(x), 3),
            'all_ms': [round(t, 3) for t in x]}


def scene_and_keyframes(w):
    sc = BC.room0_scene()
    sc.device = DEV
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = w['H'], w['W'], w['fx'], w['fy'], w['cx'], w['cy']
    g = torch.Generator().manual_seed(7)
    color = torch.zeros(sc.H, sc.W, 3)
    kfs = []
    for k in range(w['K']):
        if w['K'] == 4:
            c2w = sc.default_c2w(offset=(0.1 * k, -0.05 * k, 0.0), yaw=1.2 * k, pitch=-0.1)
        else:
            c2w = sc.default_c2w(offset=(0.3 * np.sin(0.3 * k), 0.3 * np.cos(0.2 * k), 0.05 * np.sin(0.11 * k)), yaw=0.21 * k,
                                 pitch=0.3 * np.sin(0.17 * k))
        d = sc.depth_image(c2w).cpu()
        if w['noise']:
            d = (d * (1.0 + w['noise'] * torch.randn(d.shape, generator=g))).float()
        kfs.append({'est_c2w': c2w.cpu(), 'depth': d, 'color': color, 'idx': k})
    return sc, kfs


def bound_workload(name, w, reps, directions, device_only=False):
    say(f'workload ({name}): {w["what"]}')
    sc, kfs = scene_and_keyframes(w)
    m = BC.mesher_for(sc)
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    r = {'what': w['what'], 'keyframes': w['K'], 'frame': [w['H'], w['W']]}
    host = lambda: m.get_bound_planes(kfs, 1)               # noqa: E731
    device = lambda: m.bound_planes(kfs, 1, DEV, store)     # noqa: E731
    from_dict = lambda: m.bound_planes(kfs, 1, DEV)         # noqa: E731
    _, pd = once(device)                                    # warm-up (scipy's import, the first launches)
    h, d, dd = [], [], []
    host_reps = 0 if device_only else (w['host_reps'] or reps)
    if host_reps > 1:
        once(host)
    for i in range(max(reps, host_reps)):
        if i < host_reps:
            t, ph = once(host)
            h.append(t)
            say(f'  host {t:.1f} ms')
        if i < reps:
            d.append(once(device)[0])
            dd.append(once(from_dict)[0])
            say(f'  device {d[-1]:.2f} ms (from the store), {dd[-1]:.2f} ms (stacked from keyframe_dict)')
    r['device'], r['device_from_keyframe_dict'] = stats(d), stats(dd)
    if h:
        r['host'] = stats(h)
        r['host_over_device_median'] = round(float(np.median(h) / np.median(d)), 1)
        r['device_wins_by_more_than_both_spreads'] = bool(np.median(h) - np.median(d) > max(r['host']['spread_ms'], r['device']['spread_ms']))
        r['hull_planes'] = {'host': int(ph.shape[0]), 'device': int(pd.shape[0])}
    depth, poses = store.depths(), store.poses()
    ids, pts, st = mesh.depth_hull(depth, poses, sc.fx, sc.fy, sc.cx, sc.cy, return_stats=True)
    b = mesh._DeviceBound(depth, poses, sc.fx, sc.fy, sc.cx, sc.cy)
    n_points = b.support(mesh.bound_directions())[2]
    r['points'], r['vertices'], r['D'], r['rounds'] = n_points, int(len(ids)), mesh.BOUND_DIRECTIONS, len(st)
    r['survivors_per_round'] = [int(s[2]) for s in st]
    r['planes_per_round'] = [int(s[1].shape[0]) for s in st]
    r['qhull_ms_per_round'] = [round(s[4] * 1e3, 3) for s in st]
    r['by_directions'] = {}
    for D in directions:
        dirs = mesh.bound_directions(D)
        run = lambda: mesh.depth_hull(depth, poses, sc.fx, sc.fy, sc.cx, sc.cy, directions=dirs, return_stats=True)      # noqa: E731
        once(run)
        t = [once(run) for _ in range(max(3, reps))]
        s = t[-1][1][2]
        r['by_directions'][str(D)] = {'depth_hull': stats([x[0] for x in t]), 'rounds': len(s), 'survivors_per_round': [int(x[2]) for x in s],
                                      'qhull_ms': round(sum(x[4] for x in s) * 1e3, 3)}
        say(f'  D = {D}: depth_hull {r["by_directions"][str(D)]["depth_hull"]["median_ms"]} ms, survivors {r["by_directions"][str(D)]["survivors_per_round"]}')
    del store
    torch.cuda.empty_cache()
    return r


class Slam(object):
    pass


def get_mesh_share(resolutions, reps):
    """bound_planes' share of a whole get_mesh on workload (a), as tools/mesh_bench.py sets it up."""
    sc = synthetic.Scene('room0', device=DEV, grid_std_scale=30.0)
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(seed=0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    kfs = []
    for k in range(4):
        c2w = sc.default_c2w(offset=(0.1 * k, -0.05 * k, 0.0), yaw=1.2 * k, pitch=-0.1)
        kfs.append({'est_c2w': c2w.cpu(), 'depth': sc.depth_image(c2w).cpu(), 'color': torch.zeros(sc.H, sc.W, 3), 'idx': k})
    est = torch.stack([kf['est_c2w'] for kf in kfs])
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    out = {}
    for res in resolutions:
        cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
               'scale': 1, 'occupancy': True,
               'meshing': {'resolution': res, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02, 'remove_small_geometry_threshold': 0.2,
                           'color_mesh_extraction_method': 'direct_point_query', 'get_largest_components': False, 'depth_test': False},
               'mapping': {'marching_cubes_bound': sc.bound.tolist()}}
        slam = Slam()
        slam.bound, slam.verbose = sc.bound, False
        slam.vol_bnds = slam.tsdf_bnds = sc.tsdf_bnds.to(DEV)
        slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
        slam.renderer = A.Renderer(cfg, None, slam)
        m = Mesher(cfg, None, slam)
        with tempfile.TemporaryDirectory() as d:
            whole = lambda: m.get_mesh(os.path.join(d, 'm.ply'), sc.c, dec, kfs, est, 0, sc.tsdf_volume, DEV, keyframe_store=store)   # noqa: E731
            bound = lambda: m.bound_planes(kfs, 1, DEV, store)      # noqa: E731
            host = lambda: m.get_bound_planes(kfs, 1)               # noqa: E731
            once(whole)
            tw, tb, th = [], [], []
            for _ in range(reps):
                tw.append(once(whole)[0])
                tb.append(once(bound)[0])
                th.append(once(host)[0])
        out[str(res)] = {'get_mesh': stats(tw), 'bound_planes': stats(tb), 'get_bound_planes_host': stats(th),
                         'bound_share_of_get_mesh': round(float(np.median(tb) / np.median(tw)), 4),
                         'get_mesh_with_the_host_bound_ms': round(float(np.median(tw) - np.median(tb) + np.median(th)), 3)}
        say(f'get_mesh at {res}^3: {out[str(res)]["get_mesh"]["median_ms"]} ms, bound_planes {out[str(res)]["bound_planes"]["median_ms"]} ms')
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workloads', nargs='+', default=['a', 'b', 'c'], choices=sorted(WORKLOADS))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--directions', type=int, nargs='*', default=[64, 128, 256, 512])
    ap.add_argument('--res', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--device-only', action='store_true', help='skip the host route (a short run for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_bound_bench.json'))
    a = ap.parse_args()
    out = {'workload': 'the mesh bound: Mesher.get_bound_planes (host) against Mesher.bound_planes (device), one run, alternating',
           'device': torch.cuda.get_device_name(0), 'D': mesh.BOUND_DIRECTIONS, 'workloads': {}}
    for name in a.workloads:
        out['workloads'][name] = bound_workload(name, WORKLOADS[name], a.reps, a.directions, a.device_only)
    if a.res:
        out['get_mesh'] = get_mesh_share(a.res, max(3, a.reps))
    if not a.device_only:
        out['single_routing'] = bool(all(w['device_wins_by_more_than_both_spreads'] for w in out['workloads'].values()))
    with open(a.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
