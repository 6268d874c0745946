"""Reconstruction evaluation on the MI355X (attentive_dfprior_amd.recon / recon_eval / cull_mesh).  One JSON line.

  * the 3D metric at 200 000 / 200 000 points on the synthetic room: index build, query (Morton-sorted queries and unsorted),
    metric reduction, next to scipy's cKDTree (build + query) at workers=1 (what eval_recon.py runs) and workers=16;
  * the same query with the reconstruction moved by 3 x the room's extent (the disjoint case; issue bar: <= 10 x overlapping);
  * ICP between two room meshes extracted at 512^3 (one moved by ~3 degrees / 5 cm): vertex counts, iterations, time per iteration;
  * culling of 1 M vertices against 2 000 poses, next to cull_mesh.py's per-pose loop restated in torch on the GPU;
  * --2d: the 2D metric alone -- the triangle BVH build over the 512^3 room (~1 M faces) and the depth render of one chunk of
    100 views at 500 x 500 (M rays/s), for each leaf size, and the whole metric_2d for 1 000 views on two synthetic 512^3 rooms
    (no ICP); median and range.
  * --visible: occlusion-aware visibility alone -- adfp_points_visible for 1 M surface points x 2 000 poses inside the 512^3 room
    (~1 M faces) next to the frustum-only cull (adfp_cull_vertices) of the same points and poses and of the default run's cull
    leg, the share of point/pose pairs that reach the shadow-ray walk, and visibility.unseen_points at 200 000 samples.
ADFP_LIB_PATH selects another build of the library (an A/B of leaf sizes: --nn_only runs the 3D-metric legs alone).
Device legs: warm-up, then `--reps` repetitions between torch.cuda events (host clock around a synchronised call where the leg
reads results back), min and median.

    python tools/recon_bench.py [--reps 5] [--2d | --visible]
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


def cull_leg_inputs(n_verts, n_poses):
    """The cull leg's inputs: uniform points in a box, poses turned about z at uniform positions (load_poses's convention)."""
    rng = np.random.default_rng(0)
    pc = torch.from_numpy(rng.uniform([-4, -3, -2], [4, 3, 2], (n_verts, 3))).to(DEV)
    poses = []
    for _ in range(n_poses):
        yaw = rng.uniform(-np.pi, np.pi)
        c2w = np.eye(4)
        c2w[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        c2w[:3, 3] = rng.uniform(-2, 2, 3)
        poses.append(torch.from_numpy(c2w).float())
    return pc, poses


def leg_visible(reps, res, n_points, n_poses, count):
    """adfp_points_visible against the frustum-only cull on the same inputs: n_points points on the room's surface (its vertices,
    then area-weighted samples), n_poses poses at uniform positions in the room's free space looking in uniform directions."""
    from attentive_dfprior_amd import _lib, raycast, visibility
    from attentive_dfprior_amd.cull_mesh import H, W, FX, FY, CX, CY
    out = {}
    v, f = room(res)
    out['faces'], out['verts'] = int(f.shape[0]), int(v.shape[0])
    g = torch.Generator().manual_seed(0)
    pts = v[:n_points]
    if pts.shape[0] < n_points:
        pts = torch.cat([pts, recon.sample_surface(v, f, n_points - int(pts.shape[0]), generator=g)[0]])
    pts = pts.contiguous()
    rng = np.random.default_rng(0)
    poses = []
    while len(poses) < n_poses:
        eye = rng.uniform([-1.4, -0.9, -0.6], [1.4, 0.9, 0.7])           # the room's walls are 0.4 inside BOUND
        if np.linalg.norm(eye - [0.6, -0.3, -0.2]) < 0.55:                # inside the ball
            continue
        d = rng.normal(size=3)
        m = np.eye(4)
        m[:3, :] = recon_eval.viewmatrix(d, recon_eval.UP_2D, eye)
        if not np.isfinite(m).all():
            continue
        m[:3, 1] *= -1
        m[:3, 2] *= -1
        poses.append(torch.from_numpy(m).float())
    out['points'], out['poses'] = int(pts.shape[0]), len(poses)
    dev = torch.device(DEV)
    h = {}
    out['bvh_build'] = timed(lambda: h.__setitem__('b', raycast.MeshBVH(v, f, DEV)), reps)
    bvh = h['b']
    w = torch.from_numpy(recon.w2c_rows(poses)).to(DEV)
    m = torch.from_numpy(visibility.opencv_rows(poses)).to(DEV)
    seen_v = torch.empty(n_points, dtype=torch.uint8, device=DEV)
    seen_f = torch.empty(n_points, dtype=torch.uint8, device=DEV)
    L = _lib.lib()

    def visible():
        _lib.check(L.adfp_points_visible(_lib.ptr(bvh.bvh), bvh.bvh.numel(), bvh.n_faces, bvh.leaf, _lib.ptr(pts), n_points, _lib.ptr(w),
                                         _lib.ptr(m), len(poses), FX, FY, CX, CY, W, H, 0.0, visibility.OCCLUSION_EPS, _lib.ptr(seen_v),
                                         _lib.current_stream(dev)), 'adfp_points_visible')

    def frustum(p=pts, rows=w, dst=seen_f):
        _lib.check(L.adfp_cull_vertices(_lib.ptr(p), n_points, _lib.ptr(rows), int(rows.shape[0]), FX, FY, CX, CY, W, H, _lib.ptr(dst),
                                        _lib.current_stream(dev)), 'adfp_cull_vertices')
    out['points_visible'] = timed(visible, reps)
    out['frustum_only_same_inputs'] = timed(frustum, reps)
    pc, cposes = cull_leg_inputs(n_points, n_poses)
    cw = torch.from_numpy(recon.w2c_rows(cposes)).to(DEV)
    scratch = torch.empty(n_points, dtype=torch.uint8, device=DEV)
    out['frustum_only_cull_leg'] = timed(lambda: frustum(pc, cw, scratch), reps)
    out['visible_over_frustum_same_inputs'] = round(out['points_visible']['median_ms'] / out['frustum_only_same_inputs']['median_ms'], 2)
    out['visible_over_frustum_cull_leg'] = round(out['points_visible']['median_ms'] / out['frustum_only_cull_leg']['median_ms'], 2)
    out['seen_visible'], out['seen_frustum'] = int(seen_v.sum()), int(seen_f.sum())
    out['visible_not_in_frustum'] = int((seen_v & (1 - seen_f)).sum())     # 0: occlusion only removes
    # the pairs that reach the walk, counted pose by pose as the kernel meets them: in the frustum, the point not yet seen
    done = torch.zeros(n_points, dtype=torch.bool, device=DEV)
    walked = torch.zeros((), dtype=torch.int64, device=DEV)
    in_frustum = torch.zeros((), dtype=torch.int64, device=DEV)
    for c in poses:
        fr = recon.frustum_seen(pts, [c], H, W, FX, FY, CX, CY, device=DEV).bool()
        in_frustum += fr.sum()
        walked += (fr & ~done).sum()
        done |= visibility.points_visible(bvh, pts, [c], H, W, FX, FY, CX, CY).bool()
    out['pose_by_pose_equals_one_launch'] = bool(torch.equal(done, seen_v.bool()))
    pairs = n_points * len(poses)
    out['pairs'] = pairs
    out['pairs_in_frustum_share'] = round(int(in_frustum) / pairs, 5)
    out['pairs_walked_share'] = round(int(walked) / pairs, 5)
    out['walks_per_point'] = round(int(walked) / n_points, 2)
    gu = torch.Generator().manual_seed(1)
    res_u = {}
    out['unseen_points'] = wall(lambda: res_u.__setitem__('u', visibility.unseen_points(v, f, poses, count=count, generator=gu)), reps)
    out['unseen_points']['samples'], out['unseen_points']['unseen'] = count, int(len(res_u['u']))
    out['unseen_points']['note'] = 'BVH build + draws + sampling + points_visible + read-back'
    out['morton_ordered_points'] = 'not run'
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
    ap.add_argument('--visible', action='store_true', help='only the occlusion-aware visibility legs')
    ap.add_argument('--unseen_count', type=int, default=200000)
    ap.add_argument('--res_2d', type=int, default=512)
    ap.add_argument('--n_imgs', type=int, default=1000)
    a = ap.parse_args()
    from attentive_dfprior_amd import _lib
    out = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'lib': os.path.basename(_lib.LIB_PATH)}
    if a.two_d:
        out['metric_2d'] = leg_2d(a.reps, a.res_2d, a.n_imgs, 100)
        print(json.dumps(out))
        return
    if a.visible:
        out['visible'] = leg_visible(a.reps, a.res_2d, a.cull_verts, a.cull_poses, a.unseen_count)
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

    pc, poses = cull_leg_inputs(a.cull_verts, a.cull_poses)
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
