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
calc_2d_metric is not built (see its docstring).

    python -m attentive_dfprior_amd.recon_eval --rec_mesh REC.ply --gt_mesh GT.ply -3d
"""
import argparse
import math
import sys

import numpy as np
import torch

from . import mesh
from .recon import NNIndex, device_of, as_points, metric_sums, icp_moments, sample_surface, draw_uniforms

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


NO_2D = ('calc_2d_metric (depth L1 over rendered views) is not built: it needs open3d\'s OpenGL depth capture and '
         'trimesh.bounds.oriented_bounds, neither of which is available here')


def calc_2d_metric(rec_meshfile, gt_meshfile, align=True, n_imgs=1000):
    """Not built: the reference renders depth through open3d's OpenGL visualiser (eval_recon.py:139-219)."""
    raise NotImplementedError(NO_2D)


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
        except NotImplementedError as e:
            sys.exit(str(e))


if __name__ == '__main__':
    main()
