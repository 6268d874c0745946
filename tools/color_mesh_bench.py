"""Mesh colours from the keyframes (mesh.project_colors) on the mesh of tools/mesh_bench.py: the synthetic room0 at 512^3 after the
Mesher's clean-up, against 10, 40 and 200 synthetic keyframes at Replica's frame (680 x 1200, f = 600), both blends.  The keyframes
look at the room from mesh_bench's many-pose path; depth is the room's analytic depth (with its band of zero depth), colour a
smooth function of the hit point.  Per case: the device call (pose inversion on the host, one launch; `--inner` calls back to back
between two device synchronisations per repetition, wall clock over the calls), the tests' numpy statement of the same rule (tests/project_colors_ref.py) on every
`--host-stride`-th vertex, once, and whether the two agree there; the covered share; the vertex-keyframe pairs that pass the
frame test (a torch f32 evaluation of the projection); and the mean absolute colour difference, in byte steps, of the mesh
coloured by the direct point query and by the projection against the keyframes' own images, through render_mesh's colour view
(MeshViews.render, mode 'color') at the first `--views` keyframes' poses, over the pixels where the mesh is hit and the keyframe
has depth.  No thresholds.  One JSON document.

    python tools/color_mesh_bench.py [--res 512] [--reps 5] [--keyframes 10 40 200] [--out profiles/color_mesh_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import attentive_dfprior_amd as A                     # noqa: E402
from attentive_dfprior_amd import mesh, synthetic      # noqa: E402
from attentive_dfprior_amd.common import get_rays      # noqa: E402
from attentive_dfprior_amd.keyframes import KeyframeStore      # noqa: E402
from attentive_dfprior_amd.mesher import Mesher        # noqa: E402
from attentive_dfprior_amd.render_mesh import MeshViews, opencv_poses      # noqa: E402
from mesh_bench import DEV, Slam                       # noqa: E402
import project_colors_ref as R                         # noqa: E402

H, W, F, CX, CY = 680, 1200, 600.0, 599.5, 339.5        # Replica's frame


def wall_ms(fn, reps, inner):
    """One warm-up, then per repetition the wall milliseconds of `inner` back-to-back calls between two device synchronisations,
    divided by `inner`: a single call is a fraction of a millisecond, too short a window on its own."""
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / inner)
    return {'min_ms': round(min(ms), 3), 'median_ms': round(float(np.median(ms)), 3), 'spread_ms': round(max(ms) - min(ms), 3),
            'all_ms': [round(t, 3) for t in ms]}


def room(res):
    """(scene, decoders, Mesher, verts, faces): mesh_bench's scene at Replica's frame through lattice, hull fill, marching cubes,
    seen mask and component clean-up."""
    sc = synthetic.Scene('room0', H=H, W=W, fx=F, fy=F, cx=CX, cy=CY, device=DEV, grid_std_scale=30.0)
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(seed=0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
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
    with torch.no_grad():
        xyz = m.get_grid_uniform(res)['xyz']
        z, ax = m.lattice(sc.c, dec, sc.tsdf_volume, xyz, DEV)
        mesh.hull_fill(z, ax, m.get_bound_planes(kfs, 1), 100.)
        sp = tuple(x[2] - x[1] for x in xyz)
        v, f, _ = mesh.marching_cubes(z, 0.0, sp, tuple(x[0] for x in xyz))
        seen = m.seen_mask(v, kfs, est, 0, DEV)
        v, f = mesh._clean_components(v, f, seen.to(torch.uint8), m.remove_small_geometry_threshold, False)
    return sc, dec, m, v, f


def keyframe_store(sc, K):
    """K keyframes on mesh_bench's many-pose path: analytic depth, colour 0.5 + 0.4 sin(hit * (1.3, 1.7, 2.1) + (0, 1, 2))."""
    store = KeyframeStore(H, W, DEV, capacity=K)
    freq, phase = torch.tensor([1.3, 1.7, 2.1], device=DEV), torch.tensor([0.0, 1.0, 2.0], device=DEV)
    for k in range(K):
        c2w = sc.default_c2w(offset=(0.3 * np.sin(0.3 * k), 0.3 * np.cos(0.2 * k), 0.05 * np.sin(0.11 * k)), yaw=0.21 * k,
                             pitch=0.3 * np.sin(0.17 * k))
        depth = sc.depth_image(c2w)
        rays_o, rays_d = get_rays(H, W, F, F, CX, CY, c2w, DEV)
        hit = rays_o.reshape(H, W, 3) + rays_d.reshape(H, W, 3) * depth[..., None]
        store.append(k, 0.5 + 0.4 * torch.sin(hit * freq + phase), depth, c2w)
    return store


def pairs_in_frame(v, poses):
    """How many vertex-keyframe pairs pass the frame test (border 0): the rule's projection in torch f32."""
    w2c = torch.from_numpy(np.linalg.inv(poses.cpu().numpy())[:, :3, :]).to(DEV).float()
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    n = 0
    for w in w2c:
        X = -(((w[0, 0] * x + w[0, 1] * y) + w[0, 2] * z) + w[0, 3])
        Y = ((w[1, 0] * x + w[1, 1] * y) + w[1, 2] * z) + w[1, 3]
        Z = ((w[2, 0] * x + w[2, 1] * y) + w[2, 2] * z) + w[2, 3]
        zz = Z + 1e-8
        u, vv = (F * X + CX * Z) / zz, (F * Y + CY * Z) / zz
        n += int(((zz < 0) & (u >= 0) & (u <= W - 1) & (vv >= 0) & (vv <= H - 1)).sum())
    return n


def image_difference(v, f, colors, store, views):
    """Mean |rendered - keyframe| in byte steps over the first `views` keyframes, where the mesh is hit and the keyframe has depth."""
    mv = MeshViews(v, f, colors, DEV)
    r = mv.render(opencv_poses(store.poses(views)), H, W, F, F, CX, CY, mode='color', chunk=4)
    ok = (r['face'] >= 0) & (store.depths(views) > 0)
    want = (store.colors(views).clamp(0, 1) * 255).floor()
    return float((r['rgb'].float() - want).abs()[ok].mean()), int(ok.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50, help='calls per timed repetition')
    ap.add_argument('--keyframes', type=int, nargs='+', default=[10, 40, 200])
    ap.add_argument('--host-stride', type=int, default=16, help='the numpy statement runs on every n-th vertex')
    ap.add_argument('--views', type=int, default=8, help='keyframes whose poses the colour difference is rendered at')
    ap.add_argument('--depth_tol', type=float, default=0.05)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'color_mesh_bench.json'))
    a = ap.parse_args()
    sc, dec, m, v, f = room(a.res)
    V = int(v.shape[0])
    with torch.no_grad():
        direct = torch.cat([mesh.color_bytes(m.eval_points(p, dec, sc.tsdf_volume, m.tsdf_bnds, sc.c, 'color', DEV))
                            for p in torch.split(v, m.points_batch_size, dim=0)])
    normals = mesh.vertex_normals(v, f).to(torch.float32)
    sub = slice(0, V, a.host_stride)
    v_host, n_host = v[sub].cpu().numpy(), normals[sub].cpu().numpy()
    out = {'workload': f'synthetic room0, Mesher clean-up output at {a.res}^3, keyframes {H} x {W} f = {F}',
           'device': torch.cuda.get_device_name(0), 'date': time.strftime('%Y-%m-%d'), 'reps': a.reps, 'calls_per_rep': a.inner, 'verts': V, 'faces': int(f.shape[0]),
           'depth_tol': a.depth_tol, 'border': 0, 'host_vertices': int(v_host.shape[0]), 'cases': {}}
    store = keyframe_store(sc, max(a.keyframes))
    for K in a.keyframes:
        depth, color, poses = store.depths(K), store.colors(K), store.poses(K)
        in_frame = pairs_in_frame(v, poses)
        w2c, center = R.invert_poses(poses.cpu().numpy())
        depth_host, color_host = depth.cpu().numpy(), color.cpu().numpy()
        for blend in ('weighted', 'best'):
            got = {}
            r = {'device': wall_ms(lambda: got.__setitem__('o', mesh.project_colors(v, normals, depth, color, poses, F, F, CX, CY, a.depth_tol, 0,
                                                                                 blend)), a.reps, a.inner)}
            rgb, _, count, best = got['o']
            t0 = time.perf_counter()
            h_rgb, _, h_count, h_best = R.project_colors_ref(v_host, n_host, w2c, center, depth_host, color_host, F, F, CX, CY, a.depth_tol, 0,
                                                             blend)
            r['host_s'] = round(time.perf_counter() - t0, 3)
            r['host_s_scaled_to_all_vertices'] = round(r['host_s'] * V / max(1, v_host.shape[0]), 2)
            r['count_equal_share'] = float((count[sub].cpu().numpy() == h_count).mean())
            r['best_equal_share'] = float((best[sub].cpu().numpy() == h_best).mean())
            same = count[sub].cpu().numpy() == h_count
            r['max_colour_difference_where_counts_agree'] = float(np.abs(rgb[sub].cpu().numpy() - h_rgb)[same].max()) if same.any() else 0.0
            seen = count > 0
            r['covered_share'] = float(seen.float().mean())
            r['mean_views_per_covered_vertex'] = float(count[seen].float().mean()) if bool(seen.any()) else 0.0
            r['pairs'] = V * K
            r['pairs_in_frame'] = in_frame
            r['pairs_contributing'] = int(count.sum())
            views = min(K, a.views)
            projected = torch.where(seen[:, None], mesh.color_bytes(rgb), direct)
            r['image_difference_direct_point_query'], r['image_difference_pixels'] = image_difference(v, f, direct, store, views)
            r['image_difference_keyframe_projection'], _ = image_difference(v, f, projected, store, views)
            r['image_difference_views'] = views
            out['cases'][f'{K}_{blend}'] = r
            print(f'{K} {blend}: device {r["device"]["median_ms"]} ms, host {r["host_s"]} s on {v_host.shape[0]} vertices, covered '
                  f'{r["covered_share"]:.3f}', file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
