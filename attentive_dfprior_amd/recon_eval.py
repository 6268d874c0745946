"""Drop-in for the 3D path of the reference's src/tools/eval_recon.py, on the MI355X.

The reference imports open3d and trimesh at module level and scores with scipy's cKDTree on the host.  Here:
  * accuracy / completion / completion_ratio (eval_recon.py:32-50): an exact f64 nearest-neighbour index on the device
    (recon.NNIndex, adfp_nn_build / adfp_nn_query) and a deterministic reduction (adfp_nn_metric_sums).  Inputs are numpy arrays
    (what the reference passes) or device tensors; results are Python floats;
  * get_align_transformation (:53-67): a restatement of open3d's point-to-point registration_icp as the reference calls it
    (threshold 0.1, identity init, at most 30 iterations, relative fitness and RMSE 1e-6).  The correspondences and their
    moments are computed on the device (adfp_nn_query with the radius and the current transform, adfp_icp_moments); the 3x3 SVD
    runs on the host in numpy f64.  open3d is not available to compare with, so this restatement is NOT pinned to open3d's
    numbers: it follows open3d's published algorithm (Umeyama without scaling, reflection-corrected; fitness = correspondences /
    source points, rmse = sqrt(sum d^2 / correspondences)), and the tests hold it to a numpy/scipy restatement of the same loop;
  * calc_3d_metric (:99-125): meshes read by mesh.read_ply, the alignment applied to the reconstruction's vertices in f64, 200 000
    area-weighted samples per mesh (adfp_sample_surface on uniforms drawn by torch), the three numbers x100, printed as the
    reference prints them and returned as a dict.
  * calc_2d_metric (:139-219): the views are drawn from the reference's streams (np.random for the origins, Python's random for
    the targets) and screened against the ground truth's unseen points in batches (raycast.views_in_sight, check_proj's f32 test);
    both meshes are rendered in chunks of views by an exact f64 ray caster (raycast.MeshBVH.render_depth) in place of open3d's
    OpenGL depth buffer; the per-view L1 comes from a deterministic reduction (raycast.depth_l1_sums).  The deviations from the
    reference are listed in INTEGRATION.md 2b.

    python -m attentive_dfprior_amd.recon_eval --rec_mesh REC.ply --gt_mesh GT.ply -2d -3d
"""
import argparse
import math
import os
import random
import sys

import numpy as np
import torch

from . import mesh
from .recon import NNIndex, device_of, as_points, metric_sums, icp_moments, sample_surface, draw_uniforms
from .raycast import MeshBVH, views_in_sight, depth_l1_sums

SAMPLES = 200000                      # eval_recon.py:115, :118
ICP_THRESHOLD = 0.1                   # eval_recon.py:63
ICP_MAX_ITERATION = 30                # open3d ICPConvergenceCriteria defaults
ICP_RELATIVE_FITNESS = 1e-6
ICP_RELATIVE_RMSE = 1e-6


def _nn_dist(ref, query):
    dev = device_of(ref, query)
    d, _ = NNIndex(ref, dev).query(query)
    return d


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """Fraction of gt points whose nearest rec point lies closer than dist_th (eval_recon.py:32-36)."""
    d = _nn_dist(rec_points, gt_points)
    _, c = metric_sums(d, dist_th)
    return c / d.numel()


def accuracy(gt_points, rec_points):
    """Mean distance from each rec point to its nearest gt point (eval_recon.py:39-43)."""
    d = _nn_dist(gt_points, rec_points)
    s, _ = metric_sums(d, 0.0)
    return s / d.numel()


def completion(gt_points, rec_points):
    """Mean distance from each gt point to its nearest rec point (eval_recon.py:46-50)."""
    d = _nn_dist(rec_points, gt_points)
    s, _ = metric_sums(d, 0.0)
    return s / d.numel()


def kabsch(moments):
    """The rigid 4x4 update of open3d's TransformationEstimationPointToPoint (Eigen::umeyama without scaling) from the 17
    moments of adfp_icp_moments, taken about `moments.origin`: sigma = E[q p^T] - E[q] E[p]^T, sigma = U S V^T, the last singular
    direction flipped when det(U) det(V) < 0, R = U D V^T, t = E[q] - R E[p] (then moved back from the common origin).
    Identity when there are no correspondences."""
    m, org = moments
    n = m[0]
    T = np.eye(4)
    if n <= 0:
        return T
    mp, mq = m[2:5] / n, m[5:8] / n
    spq = m[8:17].reshape(3, 3)                      # sum p q^T
    sigma = spq.T / n - np.outer(mq, mp)            # E[q p^T] - E[q] E[p]^T
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    t = mq - R @ mp
    T[:3, :3] = R
    T[:3, 3] = t + org - R @ org
    return T


class IcpResult(object):
    def __init__(self, transformation, fitness, inlier_rmse, iterations):
        self.transformation, self.fitness, self.inlier_rmse, self.iterations = transformation, fitness, inlier_rmse, iterations


def registration_icp(source, target, threshold=ICP_THRESHOLD, init=None, max_iteration=ICP_MAX_ITERATION,
                     relative_fitness=ICP_RELATIVE_FITNESS, relative_rmse=ICP_RELATIVE_RMSE):
    """Point-to-point ICP of source [N,3] onto target [M,3] (open3d.pipelines.registration.registration_icp's loop):

        result = correspondences(source . T)
        repeat up to max_iteration times:
            T = kabsch(result) . T;  prev = result;  result = correspondences(source . T)
            stop if |d fitness| < relative_fitness and |d rmse| < relative_rmse

    The source points are never moved: every query applies T to the untouched coordinates.  Returns an IcpResult."""
    dev = device_of(source, target)
    src = as_points(source, dev)
    tgt = as_points(target, dev)
    n = int(src.shape[0])
    index = NNIndex(tgt, dev)
    lo, hi = (tgt.amin(0), tgt.amax(0)) if tgt.shape[0] else (torch.zeros(3, dtype=torch.float64),) * 2
    org = ((lo + hi) * 0.5).cpu().numpy()           # the common origin of the moments: the target's box centre
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()

    def correspondences(T):
        _, idx = index.query(src, T, radius=threshold) if n else (None, torch.empty(0, dtype=torch.int32, device=dev))
        m = icp_moments(src, T, org, tgt, idx)
        fitness = m[0] / n if n else 0.0
        rmse = math.sqrt(m[1] / m[0]) if m[0] > 0 else 0.0
        return (m, org), fitness, rmse

    result = correspondences(T)
    it = 0
    for it in range(1, max_iteration + 1):
        T = kabsch(result[0]) @ T
        prev = result
        result = correspondences(T)
        if abs(prev[1] - result[1]) < relative_fitness and abs(prev[2] - result[2]) < relative_rmse:
            break
    return IcpResult(T, result[1], result[2], it)


def get_align_transformation(rec_meshfile, gt_meshfile):
    """The 4x4 transformation aligning the reconstructed mesh to the ground truth (eval_recon.py:53-67): point-to-point ICP of
    every vertex of the reconstruction onto every vertex of the ground truth, threshold 0.1, identity init.  A restatement of
    open3d's registration_icp, which is absent here: unpinned (see the module docstring)."""
    rec = mesh.read_ply(rec_meshfile)
    gt = mesh.read_ply(gt_meshfile)
    return registration_icp(rec.verts, gt.verts).transformation


def apply_transform(verts, T):
    """trimesh's apply_transform on vertices, in f64: x' = ((R00 x + R01 y) + R02 z) + t0, ..."""
    v = np.asarray(verts, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def metric_3d(rec_meshfile, gt_meshfile, align=True, generator=None, count=SAMPLES, device=None):
    """calc_3d_metric's numbers without the printing: {'accuracy', 'completion', 'completion_ratio'} (x100: cm, cm, %).
    The surface samples consume torch uniforms, the reconstruction's (u_face [count], u_bary [count,2]) and then the ground
    truth's, drawn from `generator` when one is given."""
    dev = torch.device(device) if device is not None else device_of()
    rec = mesh.read_ply(rec_meshfile)
    gt = mesh.read_ply(gt_meshfile)
    rv = rec.verts
    if align:
        rv = apply_transform(rv, get_align_transformation(rec_meshfile, gt_meshfile))
    ur = draw_uniforms(count, dev, generator)
    ug = draw_uniforms(count, dev, generator)
    rec_pts, _ = sample_surface(rv, rec.faces, u_face=ur[0], u_bary=ur[1], device=dev)
    gt_pts, _ = sample_surface(gt.verts, gt.faces, u_face=ug[0], u_bary=ug[1], device=dev)
    d_acc = NNIndex(gt_pts, dev).query(rec_pts)[0]
    d_comp = NNIndex(rec_pts, dev).query(gt_pts)[0]
    s_acc, _ = metric_sums(d_acc, 0.0)
    s_comp, c_comp = metric_sums(d_comp, 0.05)
    return {'accuracy': s_acc / d_acc.numel() * 100, 'completion': s_comp / d_comp.numel() * 100,
            'completion_ratio': c_comp / d_comp.numel() * 100}


def calc_3d_metric(rec_meshfile, gt_meshfile, align=True):
    """3D reconstruction metric (eval_recon.py:99-125): prints accuracy (cm), completion (cm) and completion ratio (%) as the
    reference does, and returns them as a dict."""
    r = metric_3d(rec_meshfile, gt_meshfile, align)
    print('accuracy: ', r['accuracy'])
    print('completion: ', r['completion'])
    print('completion ratio: ', r['completion_ratio'])
    return r


# calc_2d_metric's camera (eval_recon.py:144-150) and far plane (:195, set_constant_z_far)
H_2D = W_2D = 500
FOCAL_2D = 300.0
FAR_2D = 20.0
UP_2D = [0, 0, -1]                    # eval_recon.py:171
NEAR_FRACTION = 0.01                  # near = 0.01 x the largest AABB extent of the rendered mesh


def setup_seed(seed):
    """Seed every stream the evaluation draws from: torch (CPU and GPU), numpy's global stream and Python's random."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


def normalize(x):
    """x scaled to unit length."""
    return x / np.linalg.norm(x)


def viewmatrix(z, up, pos):
    """The 3x4 camera-to-world [x y z pos] looking along z: x = unit(up x z), y = unit(z x x)."""
    axis_z = normalize(z)
    axis_x = normalize(np.cross(up, axis_z))
    axis_y = normalize(np.cross(axis_z, axis_x))
    return np.stack([axis_x, axis_y, axis_z, pos], 1)


def check_proj(points, W, H, fx, fy, cx, cy, c2w):
    """Whether the pose c2w projects any of points [N,3] into the W x H image (eval_recon.py:70-96), as a numpy bool: one pose
    through raycast.views_in_sight."""
    return np.bool_(bool(views_in_sight(points, [np.asarray(c2w, dtype=np.float64)], H, W, fx, fy, cx, cy)[0]))


def _min_area_rect(p2):
    """The minimum-area rectangle around 2D points over the directions of their hull's edges: (u, v, ext_u, ext_v, mid_u, mid_v),
    u and v the unit axes."""
    from scipy.spatial import ConvexHull
    ring = p2[ConvexHull(p2).vertices]
    e = np.roll(ring, -1, 0) - ring
    e = e[np.linalg.norm(e, axis=1) > 0]
    u = e / np.linalg.norm(e, axis=1)[:, None]
    v = np.stack([-u[:, 1], u[:, 0]], 1)
    pu, pv = ring @ u.T, ring @ v.T
    lo_u, hi_u, lo_v, hi_v = pu.min(0), pu.max(0), pv.min(0), pv.max(0)
    j = int(np.argmin((hi_u - lo_u) * (hi_v - lo_v)))
    return u[j], v[j], hi_u[j] - lo_u[j], hi_v[j] - lo_v[j], (lo_u[j] + hi_u[j]) * 0.5, (lo_v[j] + hi_v[j]) * 0.5


def oriented_bounds(verts):
    """trimesh.bounds.oriented_bounds(mesh) (ordered=True), restated with scipy's ConvexHull: for each distinct normal of the hull's
    faces, the hull is projected onto that normal's plane, and the box is the 2D minimum-area rectangle over the projected hull's
    edge directions times the height along the normal; the smallest volume wins.  Returns (to_origin 4x4, extents [3]): extents
    ascending, to_origin the rigid transform taking the box to the origin, its axes permuted to that order and sign-fixed to a
    right-handed frame."""
    from scipy.spatial import ConvexHull
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    hull = ConvexHull(v)
    hv = v[hull.vertices]
    normals = hull.equations[:, :3] / np.linalg.norm(hull.equations[:, :3], axis=1)[:, None]
    lead = np.argmax(np.abs(normals) > 1e-12, axis=1)
    normals = normals * np.sign(normals[np.arange(len(normals)), lead])[:, None]          # n and -n are one plane direction
    _, first = np.unique(np.round(normals, 9), axis=0, return_index=True)
    best = None
    for n in normals[np.sort(first)]:
        a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
        e0 = normalize(np.cross(n, a))
        e1 = np.cross(n, e0)
        h = hv @ n
        height = h.max() - h.min()
        u, w, eu, ew, mu, mw = _min_area_rect(np.stack([hv @ e0, hv @ e1], 1))
        vol = eu * ew * height
        if best is None or vol < best[0]:
            axes = np.stack([u[0] * e0 + u[1] * e1, w[0] * e0 + w[1] * e1, n])
            best = (vol, axes, np.array([eu, ew, height]), np.array([mu, mw, (h.max() + h.min()) * 0.5]))
    _, axes, ext, mid = best
    centre = mid @ axes                                                  # mid is in the (u, w, n) frame
    order = np.argsort(ext, kind='stable')
    axes, ext = axes[order], ext[order]
    if np.linalg.det(axes) < 0:
        axes[2] = -axes[2]
    to_origin = np.eye(4)
    to_origin[:3, :3] = axes
    to_origin[:3, 3] = -(axes @ centre)
    return to_origin, ext


def get_cam_position(gt_meshfile):
    """The box the cameras are drawn from (eval_recon.py:128-136): the ground truth's oriented bounds with the extents scaled by
    (0.3, 0.7, 0.7) (smallest, middle, largest) and the box moved up by 0.4 along world z.  Returns (extents, transform)."""
    to_origin, extents = oriented_bounds(mesh.read_ply(gt_meshfile).verts)
    extents = extents * np.array([0.3, 0.7, 0.7])
    transform = np.linalg.inv(to_origin)
    transform[2, 3] += 0.4
    return extents, transform


def volume_rectangular(extents, count, transform=None):
    """trimesh.sample.volume_rectangular restated: count points uniform in a box of `extents` centred at the origin, from numpy's
    global stream (np.random.random((count, 3)) - 0.5, times extents), then moved by transform as
    x' = ((T00 x + T01 y) + T02 z) + T03.  count draws at once consume the stream as count draws of one."""
    s = (np.random.random((count, 3)) - 0.5) * np.asarray(extents, dtype=np.float64)
    return s if transform is None else apply_transform(s, transform)


def sample_views(pc_unseen, extents, transform, n_imgs, H=H_2D, W=W_2D, fx=FOCAL_2D, fy=FOCAL_2D, cx=H_2D / 2.0 - 0.5,
                 cy=W_2D / 2.0 - 0.5, device=None):
    """The views of calc_2d_metric (eval_recon.py:167-186): candidates drawn as the reference draws them (per candidate three
    numpy uniforms for the origin, then three Python random.uniform(-1e4, 1e4) rounded to 0.01 for the target), screened in batches
    by views_in_sight, and accepted exactly as the reference's sequential loop accepts them: the first n_imgs candidates that see
    none of pc_unseen.  A candidate whose viewmatrix is degenerate (target parallel to up) is rejected.  The last batch is drawn
    whole, so both global streams end up further on than the reference leaves them.  Returns (c2w list [4x4], candidates the
    sequential loop would have drawn)."""
    out, used = [], 0
    while len(out) < n_imgs:
        k = min(1024, max(32, 2 * (n_imgs - len(out))))
        origins = volume_rectangular(extents, k, transform)
        cands, ok = [], []
        for c in range(k):
            target = np.array([round(random.uniform(-10000, +10000), 2) for _ in range(3)]) - np.array(origins[c])
            with np.errstate(all='ignore'):
                m = viewmatrix(target, UP_2D, origins[c])
            c2w = np.eye(4)
            c2w[:3, :] = m
            ok.append(bool(np.isfinite(c2w).all()))
            cands.append(c2w)
        seen = views_in_sight(pc_unseen, [c if o else np.eye(4) for c, o in zip(cands, ok)], H, W, fx, fy, cx, cy,
                              device).cpu().numpy()
        for c in range(k):
            used += 1
            if ok[c] and not seen[c]:
                out.append(cands[c])
                if len(out) == n_imgs:
                    break
    return out, used


def pc_unseen_file(gt_meshfile):
    return gt_meshfile.replace('.ply', '_pc_unseen.npy')


def load_pc_unseen(gt_meshfile):
    path = pc_unseen_file(gt_meshfile)
    if not os.path.exists(path):
        raise FileNotFoundError(
            f'{path} is missing: calc_2d_metric needs the ground truth\'s unseen-region points beside it.  The file ships with '
            'NICE-SLAM\'s culled Replica meshes; it is not built by cull_mesh.')
    return np.load(path)


def metric_2d(rec_meshfile, gt_meshfile, align=True, n_imgs=1000, pc_unseen=None, near=None, far=FAR_2D, chunk=100, device=None):
    """calc_2d_metric's number without the printing: (Depth L1 in cm, the accepted c2w list).  The views come from sample_views
    over get_cam_position's box; both meshes are rendered at 500 x 500 (fx = fy = 300, cx = cy = 249.5) in chunks of `chunk`
    views, near defaulting per mesh to 0.01 x the largest AABB extent of its vertices (the reconstruction's after alignment), far
    = 20.  The per-view L1 is depth_l1_sums / (H W), and the result is 100 x the mean over views (f64).  pc_unseen: the ground
    truth's unseen-region points; None reads them from the _pc_unseen.npy file beside gt_meshfile."""
    dev = torch.device(device) if device is not None else device_of()
    if pc_unseen is None:
        pc_unseen = load_pc_unseen(gt_meshfile)
    H, W, f = H_2D, W_2D, FOCAL_2D
    cx, cy = H / 2.0 - 0.5, W / 2.0 - 0.5
    gt = mesh.read_ply(gt_meshfile)
    rec = mesh.read_ply(rec_meshfile)
    rv = rec.verts
    if align:
        rv = apply_transform(rv, get_align_transformation(rec_meshfile, gt_meshfile))
    extents, transform = get_cam_position(gt_meshfile)
    views, _ = sample_views(pc_unseen, extents, transform, n_imgs, H, W, f, f, cx, cy, dev)

    def near_of(v):
        if near is not None:
            return float(near)
        v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
        return NEAR_FRACTION * float((v.max(0) - v.min(0)).max()) if len(v) else 0.0

    bvh_gt, bvh_rec = MeshBVH(gt.verts, gt.faces, dev), MeshBVH(rv, rec.faces, dev)
    n_gt, n_rec = near_of(gt.verts), near_of(rv)
    sums = []
    for c0 in range(0, len(views), chunk):
        c2w = np.stack(views[c0:c0 + chunk])
        sums.append(depth_l1_sums(bvh_gt.render_depth(c2w, H, W, f, f, cx, cy, n_gt, far),
                                  bvh_rec.render_depth(c2w, H, W, f, f, cx, cy, n_rec, far)))
    errors = torch.cat(sums).cpu().numpy() / (H * W) if sums else np.zeros(0)
    return float(np.mean(errors) * 100) if len(errors) else float('nan'), views


def calc_2d_metric(rec_meshfile, gt_meshfile, align=True, n_imgs=1000):
    """2D reconstruction metric (eval_recon.py:139-219): the mean depth L1 over n_imgs rendered views, printed in cm as the
    reference prints it, and returned.  Needs the ground truth's _pc_unseen.npy beside gt_meshfile."""
    d, _ = metric_2d(rec_meshfile, gt_meshfile, align, n_imgs)
    print('Depth L1: ', d)
    return d


def main(argv=None):
    parser = argparse.ArgumentParser(description='Arguments to evaluate the reconstruction.')
    parser.add_argument('--rec_mesh', type=str, help='reconstructed mesh file path')
    parser.add_argument('--gt_mesh', type=str, help='ground truth mesh file path')
    parser.add_argument('-2d', '--metric_2d', action='store_true', help='enable 2D metric')
    parser.add_argument('-3d', '--metric_3d', action='store_true', help='enable 3D metric')
    args = parser.parse_args(argv)
    if args.metric_3d:
        calc_3d_metric(args.rec_mesh, args.gt_mesh)
    if args.metric_2d:
        try:
            calc_2d_metric(args.rec_mesh, args.gt_mesh, n_imgs=1000)
        except FileNotFoundError as e:
            sys.exit(str(e))


if __name__ == '__main__':
    main()
