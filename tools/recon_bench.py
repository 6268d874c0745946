"""Reconstruction evaluation on the MI355X (attentive_dfprior_amd.recon / recon_eval / cull_mesh).  One JSON line.

  * the 3D metric at 200 000 / 200 000 points on the synthetic room: index build, query (Morton-sorted queries and unsorted),
    metric reduction, next to scipy's cKDTree (build + query) at workers=1 (what eval_recon.py runs) and workers=16;
  * the same query with the reconstruction moved by 3 x the room's extent (the disjoint case; issue bar: <= 10 x overlapping);
  * ICP between two room meshes extracted at 512^3 (one moved by ~3 degrees / 5 cm): vertex counts, iterations, time per iteration;
  * culling of 1 M vertices against 2 000 poses, next to cull_mesh.py's per-pose loop restated in torch on the GPU;
  * --2d: the 2D metric alone -- the triangle BVH build over the 512^3 room (~1 M faces) and the depth render of one chunk of
    100 views at 500 x 500 (M rays/s), for each leaf size, and the whole metric_2d for 1 000 views on two synthetic 512^3 rooms
    (no ICP); median and range.
ADFP_LIB_PATH selects another build of the library (an A/B of leaf sizes: --nn_only runs the 3D-metric legs alone).
Device legs: warm-up, then `--reps` repetitions between torch.cuda events (host clock around a synchronised call where the leg
reads results back), min and median.

    python tools/recon_bench.py [--reps 5] [--2d]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from attentive_dfprior_amd import mesh, recon, recon_eval, synthetic      # noqa: E402
from scipy.spatial import cKDTree                                         # noqa: E402

DEV = 'cuda:0'
BOUND = [[-2.0, 2.0], [-1.5, 1.5], [-1.2, 1.3]]


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


def wall(fn, reps, warm=True):
    if warm:
        fn()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return {'min_ms': round(min(s), 3), 'median_ms': round(float(np.median(s)), 3)}


def room(res, moved=False):
    """Room mesh (verts f64, faces int32, device) from the synthetic box room TSDF + a ball, on a res^3-ish lattice."""
    b = torch.tensor(BOUND, dtype=torch.float64)
    voxel = 4.0 / res
    tv, bn, _ = synthetic.make_box_room_tsdf(b, voxel=voxel, inset=0.4, device=DEV)
    vol = tv[0, 0].permute(2, 1, 0).contiguous()
    X, Y, Z = vol.shape
    ax = [float(bn[i, 0]) + torch.arange(n, device=DEV, dtype=torch.float32) * voxel for i, n in enumerate((X, Y, Z))]
    gx, gy, gz = torch.meshgrid(*ax, indexing='ij')
    ball = (torch.sqrt((gx - 0.6) ** 2 + (gy + 0.3) ** 2 + (gz + 0.2) ** 2) - 0.45) / (5 * voxel)
    vol = torch.minimum(vol, ball.clamp(-1, 1)).contiguous()
    del gx, gy, gz, ball
    v, f, _ = mesh.marching_cubes(vol, 0.0, (voxel,) * 3, tuple(bn[:, 0].tolist()))
    v = v.double()
    if moved:
        a = np.deg2rad(3.0)
        T = np.eye(4)
        T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
        T[:3, 3] = [0.03, 0.02, -0.035]
        v = torch.from_numpy(recon_eval.apply_transform(v.cpu().numpy(), T)).to(DEV)
    return v, f


def metric_leg(gt, rec, reps, workers):
    r = {}
    h = {}
    r['build'] = timed(lambda: h.__setitem__('i', recon.NNIndex(rec)), reps)
    idx = h['i']
    r['query_sorted'] = timed(lambda: h.__setitem__('q', idx.query(gt, sort_queries=True)), reps)
    r['query_unsorted'] = timed(lambda: idx.query(gt, sort_queries=False), reps)
    d = h['q'][0]
    r['reduction_incl_readback'] = wall(lambda: recon.metric_sums(d, 0.05), reps)
    g, q = gt.cpu().numpy(), rec.cpu().numpy()
    for w in workers:
        s = []
        for _ in range(max(1, reps // 2)):
            t0 = time.perf_counter()
            cKDTree(q).query(g, workers=w)
            s.append((time.perf_counter() - t0) * 1e3)
        r[f'ckdtree_workers{w}_build_query_ms'] = round(min(s), 2)
    return r


def torch_cull_loop(pc, poses, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5):
    """cull_mesh.py:48-71 as the reference runs it (per pose: projection on the GPU, a device-to-host copy)."""
    whole = np.ones(pc.shape[0]).astype(bool)
    K = torch.from_numpy(np.array([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]])).to(DEV)
    for c2w in poses:
        points = pc.clone()
        w2c = torch.from_numpy(np.linalg.inv(c2w.numpy())).to(DEV).float()
        ones = torch.ones_like(points[:, 0]).reshape(-1, 1)
        homo = torch.cat([points, ones], dim=1).reshape(-1, 4, 1).float()
        cam = (w2c @ homo)[:, :3]
        cam[:, 0] *= -1
        uv = K.float() @ cam.float()
        z = uv[:, -1:] + 1e-5
        uv = (uv[:, :2] / z).float().squeeze(-1).cpu().numpy()
        mask = (0 <= -z[:, 0, 0].cpu().numpy()) & (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
        whole &= ~mask
    return whole


def spread(fn, reps):
    """Host clock around a synchronised call, after one warm-up: median and range in ms."""
    fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(float(np.median(t)), 3), 'min_ms': round(min(t), 3), 'max_ms': round(max(t), 3)}


def leg_2d(reps, res, n_imgs, chunk):
    import tempfile
    from attentive_dfprior_amd import _lib, raycast
    out = {}
    v, f = room(res)
    rv, rf = room(res, moved=True)
    vn, fn_ = v.cpu().numpy(), f.cpu().numpy()
    out['faces'] = int(f.shape[0])
    rng = np.random.default_rng(0)
    pc = np.stack([rng.uniform(-1.6, -1.0, 2000), rng.uniform(0.6, 1.1, 2000), np.full(2000, 0.9)], 1)    # a ceiling corner
    with tempfile.TemporaryDirectory() as d:
        gt_p, rec_p = os.path.join(d, 'gt.ply'), os.path.join(d, 'rec.ply')
        mesh.write_ply(gt_p, vn, fn_)
        mesh.write_ply(rec_p, rv.cpu().numpy(), rf.cpu().numpy())
        extents, transform = recon_eval.get_cam_position(gt_p)
        views, _ = recon_eval.sample_views(pc, extents, transform, chunk, device=DEV)
        c2w = np.stack(views)
        H = W = recon_eval.H_2D
        near = recon_eval.NEAR_FRACTION * float((vn.max(0) - vn.min(0)).max())
        for leaf in _lib.TRI_LEAVES:
            h = {}
            b = timed(lambda: h.__setitem__('b', raycast.MeshBVH(v, f, DEV, leaf=leaf)), reps)
            bvh = h['b']
            r = timed(lambda: bvh.render_depth(c2w, H, W, 300.0, 300.0, 249.5, 249.5, near, 20.0), reps)
            out[f'leaf{leaf}'] = {'bvh_build': b, 'render_100_views': r,
                                  'mrays_per_s_median': round(len(views) * H * W / (r['median_ms'] * 1e-3) / 1e6, 1)}
        out['metric_2d_1000_views'] = spread(lambda: recon_eval.metric_2d(rec_p, gt_p, align=False, n_imgs=n_imgs, pc_unseen=pc,
                                                                           chunk=chunk, device=DEV), reps)
        out['metric_2d_note'] = f'{n_imgs} views, chunks of {chunk}, read_ply + oriented bounds + view sampling + 2 BVH builds + renders'
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--icp_res', type=int, default=512)
    ap.add_argument('--cull_verts', type=int, default=1000000)
    ap.add_argument('--cull_poses', type=int, default=2000)
    ap.add_argument('--nn_only', action='store_true', help='only the two 3D-metric legs (for an A/B of library builds)')
    ap.add_argument('--2d', dest='two_d', action='store_true', help='only the 2D-metric legs (BVH build, render, metric_2d)')
    ap.add_argument('--res_2d', type=int, default=512)
    ap.add_argument('--n_imgs', type=int, default=1000)
    a = ap.parse_args()
    from attentive_dfprior_amd import _lib
    out = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'lib': os.path.basename(_lib.LIB_PATH)}
    if a.two_d:
        out['metric_2d'] = leg_2d(a.reps, a.res_2d, a.n_imgs, 100)
        print(json.dumps(out))
        return
    v, f = room(256)
    g = torch.Generator().manual_seed(0)
    gt, _ = recon.sample_surface(v, f, a.n, generator=g)
    rec, _ = recon.sample_surface(v, f, a.n, generator=g)
    rec = rec + 0.01 * torch.randn(rec.shape, dtype=torch.float64, generator=g).to(DEV)
    uf, ub = recon.draw_uniforms(a.n, DEV, g)                  # drawn outside the timed region: the leg times the kernels alone
    out['sample_surface_200k'] = timed(lambda: recon.sample_surface(v, f, u_face=uf, u_bary=ub), a.reps)
    out['metric_3d_overlapping'] = metric_leg(gt, rec, a.reps, (1, 16))
    ext = float((gt.amax(0) - gt.amin(0)).max())
    far = rec + torch.tensor([3 * ext, 0.0, 0.0], dtype=torch.float64, device=DEV)
    out['metric_3d_disjoint'] = metric_leg(gt, far, a.reps, (16,))
    out['disjoint_over_overlapping_query'] = round(out['metric_3d_disjoint']['query_sorted']['min_ms']
                                                   / out['metric_3d_overlapping']['query_sorted']['min_ms'], 3)

    if a.nn_only:
        print(json.dumps(out))
        return
    src, _ = room(a.icp_res, moved=True)
    tgt, _ = room(a.icp_res - 64)
    res = {}
    t = wall(lambda: res.__setitem__('r', recon_eval.registration_icp(src, tgt)), max(1, a.reps // 2))
    r = res['r']
    out['icp'] = {'src_verts': int(src.shape[0]), 'tgt_verts': int(tgt.shape[0]), 'lattices': [a.icp_res, a.icp_res - 64],
                  'iterations': r.iterations, 'fitness': r.fitness, 'rmse': r.inlier_rmse, 'total': t,
                  'per_iteration_ms': round(t['min_ms'] / (r.iterations + 1), 3),
                  'note': 'per iteration = total / (iterations + 1) correspondence passes, index build included in total'}
    del src, tgt

    rng = np.random.default_rng(0)
    pc = torch.from_numpy(rng.uniform([-4, -3, -2], [4, 3, 2], (a.cull_verts, 3))).to(DEV)
    poses = []
    for _ in range(a.cull_poses):
        yaw = rng.uniform(-np.pi, np.pi)
        c2w = np.eye(4)
        c2w[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        c2w[:3, 3] = rng.uniform(-2, 2, 3)
        poses.append(torch.from_numpy(c2w).float())
    w = torch.from_numpy(recon.w2c_rows(poses)).to(DEV)
    seen = torch.empty(a.cull_verts, dtype=torch.uint8, device=DEV)
    L = _lib.lib()

    def kernel_only():
        _lib.check(L.adfp_cull_vertices(_lib.ptr(pc), a.cull_verts, _lib.ptr(w), len(poses), 600., 600., 599.5, 339.5, 1200, 680,
                                        _lib.ptr(seen), _lib.current_stream(torch.device(DEV))), 'adfp_cull_vertices')
    out['cull'] = {'verts': a.cull_verts, 'poses': a.cull_poses, 'kernel': timed(kernel_only, a.reps),
                   'frustum_seen_incl_host_inverse': wall(lambda: recon.frustum_seen(pc, poses, 680, 1200, 600., 600., 599.5, 339.5), a.reps)}
    ref = wall(lambda: out.__setitem__('_w', torch_cull_loop(pc, poses)), 1)
    out['cull']['reference_torch_loop'] = ref
    whole = out.pop('_w')
    out['cull']['seen_vertices'] = int(seen.sum())
    out['cull']['mismatches_vs_torch_loop'] = int(((seen.cpu().numpy() == 0) != whole).sum())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
