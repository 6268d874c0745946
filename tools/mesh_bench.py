"""Mesh extraction on the synthetic room at 256^3 and 512^3 (Mesher.get_mesh's pieces): lattice query, hull fill, marching cubes
(count + emit), the mesh bound, the clean-up after marching cubes through the retained host methods against the device path, the
whole get_mesh, and the CPU oracle (tests/mesh_ref.py) on the same lattice.  One JSON line.
Device legs: warm-up, then `--reps` timed repetitions (torch.cuda events around the leg), min and median reported.
Host-against-device legs (`tail`): both sides in this one run, alternating, wall clock with a device synchronisation on both
ends, every repetition listed: seen mask (torch point_masks against the one-launch kernel; the run's 4 keyframes, and
`--poses` poses in the get_mask_use_all_frames form), culling (Mesher.clean against mesh.clean_components), vertex merge, and
the whole tail from the marching-cubes output to the arrays for write_ply.

    python tools/mesh_bench.py [--res 256 512] [--reps 5] [--poses 300] [--skip-oracle]
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
from attentive_dfprior_amd.mesher import Mesher, merge_coincident        # noqa: E402
from oracle import adfp_oracle as O                    # noqa: E402
import mesh_ref                                        # noqa: E402

DEV = 'cuda:0'


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
    return {'min_ms': round(min(ms), 4), 'median_ms': round(float(np.median(ms)), 4)}


def wall(fn, reps):
    fn()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    return {'min_s': round(min(s), 4), 'median_s': round(float(np.median(s)), 4)}


def against(host, device, reps):
    """Both sides alternating, one warm-up each: wall milliseconds of every repetition, min, median and spread (max - min)."""
    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    once(host)
    once(device)
    h, d = [], []
    for _ in range(reps):
        h.append(once(host))
        d.append(once(device))

    def stats(x):
        return {'min_ms': round(min(x), 3), 'median_ms': round(float(np.median(x)), 3), 'spread_ms': round(max(x) - min(x), 3),
                'all_ms': [round(t, 3) for t in x]}
    return {'host': stats(h), 'device': stats(d), 'host_over_device_median': round(float(np.median(h) / np.median(d)), 2)}


def host_tail(m, verts, faces, c, dec, kfs, est, idx, tv, all_frames=False):
    """The parent's get_mesh from the marching-cubes output to the arrays for write_ply, through the retained host methods."""
    with torch.no_grad():
        vertices = verts.cpu().numpy()
        f = faces.cpu().numpy()
        seen, _, _ = m.point_masks(verts, kfs, est, idx, device=DEV, get_mask_use_all_frames=all_frames)
        vertices, f = m.clean(vertices, f, seen)
        vc = []
        for pnts in torch.split(torch.from_numpy(vertices).to(DEV).float(), m.points_batch_size, dim=0):
            vc.append(m.eval_points(pnts, dec, tv, m.tsdf_bnds, c, 'color', DEV)[..., :3])
        col = torch.cat(vc, 0).cpu().numpy() if vc else np.zeros((0, 3), np.float32)
        col = (np.clip(col, 0, 1) * 255).astype(np.uint8)
        vertices, f, col = merge_coincident(vertices, f, col)
        return vertices / np.float32(m.scale), f, col


class Slam(object):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--poses', type=int, default=300, help='poses of the get_mask_use_all_frames seen-mask leg')
    ap.add_argument('--skip-oracle', action='store_true', help='skip the CPU oracle extraction (minutes at 512^3)')
    a = ap.parse_args()
    sc = synthetic.Scene('room0', device=DEV, grid_std_scale=30.0)
    sd = synthetic.seeded_state_dict(seed=0)
    dec = A.DF()
    dec.load_state_dict(sd)
    dec.bound = sc.bound
    dec = dec.to(DEV)
    out = {'workload': 'synthetic room0 (TSDF 256^3 box room), Mesher.get_mesh pieces', 'device': torch.cuda.get_device_name(0),
           'by_resolution': {}}
    for res in a.res:
        cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
               'scale': 1, 'occupancy': True,
               'meshing': {'resolution': res, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02,
                           'remove_small_geometry_threshold': 0.2, 'color_mesh_extraction_method': 'direct_point_query',
                           'get_largest_components': False, 'depth_test': False},
               'mapping': {'marching_cubes_bound': sc.bound.tolist()}}
        slam = Slam()
        slam.bound = sc.bound
        slam.vol_bnds = slam.tsdf_bnds = sc.tsdf_bnds.to(DEV)
        slam.verbose = False
        slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
        slam.renderer = A.Renderer(cfg, None, slam)
        kfs = []
        for k in range(4):
            c2w = sc.default_c2w(offset=(0.1 * k, -0.05 * k, 0.0), yaw=1.2 * k, pitch=-0.1)
            kfs.append({'est_c2w': c2w.cpu(), 'depth': sc.depth_image(c2w).cpu(), 'color': torch.zeros(sc.H, sc.W, 3)})
        est = torch.stack([kf['est_c2w'] for kf in kfs])
        m = Mesher(cfg, None, slam)
        xyz = m.get_grid_uniform(res)['xyz']
        tv = sc.tsdf_volume
        r = {}
        holder = {}

        def query():
            holder['z'], holder['ax'] = m.lattice(sc.c, dec, tv, xyz, DEV)
        r['lattice_query'] = timed(query, a.reps)
        t0 = time.perf_counter()
        planes = m.get_bound_planes(kfs, 1)
        r['get_bound_planes_host_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
        z0 = holder['z'].clone()
        r['hull_planes'] = int(planes.shape[0])

        def fill():
            holder['z'].copy_(z0)
            mesh.hull_fill(holder['z'], holder['ax'], planes, 100.)
        cp = timed(lambda: holder['z'].copy_(z0), a.reps)
        hf = timed(fill, a.reps)
        r['hull_fill'] = {k: round(hf[k] - cp[k], 4) for k in hf}
        r['hull_fill']['note'] = 'minus a timed copy of the lattice that restores it before each fill'
        sp = tuple(x[2] - x[1] for x in xyz)
        org = tuple(x[0] for x in xyz)
        z = holder['z']
        mc = {}
        r['count_emit'] = timed(lambda: mc.setdefault('o', mesh.marching_cubes(z, 0.0, sp, org)), a.reps)
        r['count_emit']['note'] = 'whole marching_cubes call: count + scan, the read of the two totals (host sync), allocation, emit'
        v, f, _ = mesh.marching_cubes(z, 0.0, sp, org)
        r['verts'], r['faces'] = int(v.shape[0]), int(f.shape[0])
        vn, fn = v.cpu().numpy(), f.cpu().numpy()
        seen, _, _ = m.point_masks(v, kfs, est, 0, DEV)
        t0 = time.perf_counter()
        for _ in range(3):
            m.clean(vn, fn, seen)
        r['host_culling_ms'] = round((time.perf_counter() - t0) / 3 * 1e3, 2)
        # the clean-up after marching cubes: the retained host methods (the parent commit's path) against the device path
        thr = m.remove_small_geometry_threshold * m.scale * m.scale
        seen_d = torch.from_numpy(seen).to(DEV).to(torch.uint8)
        many = torch.stack([sc.default_c2w(offset=(0.3 * np.sin(0.3 * k), 0.3 * np.cos(0.2 * k), 0.05 * np.sin(0.11 * k)), yaw=0.21 * k,
                                           pitch=0.3 * np.sin(0.17 * k)).cpu() for k in range(a.poses)])
        tail = {}
        tail['seen_mask_4_keyframes'] = against(lambda: m.point_masks(v, kfs, est, 0, DEV), lambda: m.seen_mask(v, kfs, est, 0, DEV), a.reps)
        tail[f'seen_mask_{a.poses}_poses_all_frames'] = against(
            lambda: m.point_masks(v, kfs, many, a.poses - 1, DEV, get_mask_use_all_frames=True),
            lambda: m.seen_mask(v, kfs, many, a.poses - 1, DEV, get_mask_use_all_frames=True), max(1, a.reps // 2))
        tail['clean'] = against(lambda: m.clean(vn, fn, seen), lambda: mesh._clean_components(v, f, seen_d, thr, False), a.reps)
        cv, cf = m.clean(vn, fn, seen)
        rng = np.random.default_rng(0)
        col = rng.integers(0, 256, size=(len(cv), 3)).astype(np.uint8)
        dup = cv.copy()
        dup[rng.choice(len(cv), len(cv) // 100, replace=False)] = dup[rng.choice(len(cv), len(cv) // 100)]      # 1 % coincide
        dv, df, dc = torch.from_numpy(dup).to(DEV), torch.from_numpy(cf).to(DEV), torch.from_numpy(col).to(DEV)
        tail['merge_coincident'] = against(lambda: merge_coincident(dup, cf, col), lambda: mesh._merge_coincident(dv, df, dc), a.reps)
        res_h, res_d = {}, {}
        tail['whole_tail'] = against(lambda: res_h.setdefault('o', host_tail(m, v, f, sc.c, dec, kfs, est, 0, tv)),
                                     lambda: res_d.setdefault('o', m.mesh_arrays(v, f, sc.c, dec, kfs, est, 0, tv, DEV)), a.reps)
        tail['whole_tail']['note'] = 'marching-cubes output (device) -> vertices, faces, colours for write_ply (host)'
        tail['whole_tail']['equal'] = bool(all(np.array_equal(x, y) for x, y in zip(res_h['o'], res_d['o'])))
        tail['kept_verts'], tail['kept_faces'] = int(len(res_d['o'][0])), int(len(res_d['o'][1]))
        r['tail'] = tail
        with tempfile.TemporaryDirectory() as d:
            r['get_mesh_total'] = wall(lambda: m.get_mesh(os.path.join(d, 'm.ply'), sc.c, dec, kfs, est, 0, tv, DEV), max(1, a.reps // 2))
        if not a.skip_oracle:
            zc = z.cpu().numpy()
            t0 = time.perf_counter()
            rv, rf, _ = mesh_ref.marching_cubes(zc, 0.0, sp, org)
            r['oracle_cpu_extraction_s'] = round(time.perf_counter() - t0, 3)
            r['oracle_faces_equal'] = bool(np.array_equal(rf, fn))
        out['by_resolution'][str(res)] = r
        del holder, z, z0, mc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
