"""Occlusion-aware visibility on the MI355X (libadfp.so, adfp_points_visible in csrc/adfp_raycast.h): is a point seen from a pose,
with the mesh itself in the way?  One launch tests every point against every pose: cull_mesh's f32 frustum rule per pair, and for
the pairs that pass it a shadow ray through the mesh's triangle BVH in the depth renderer's f64 arithmetic (include/adfp.h).

Two tools are built on it.  cull_mesh.cull_mesh(..., occlusion=True) is the occlusion-aware cull, and unseen_points makes the
ground truth's unseen-region points, the `<gt>_pc_unseen.npy` that recon_eval's 2D metric reads:

    python -m attentive_dfprior_amd.visibility --input_mesh GT_UNCULLED.ply --traj traj.txt --unseen_points GT_pc_unseen.npy

"Unseen points" is this package's own definition: surface samples of the unculled ground-truth mesh that no pose of the trajectory
observes.  NICE-SLAM ships such files with its culled Replica meshes and does not publish how they were made, so numbers obtained
with a file made here are not comparable with numbers obtained with theirs.
"""
import argparse

import numpy as np
import torch

from . import _lib, mesh
from .raycast import MeshBVH
from .recon import as_numpy, as_points, sample_surface, w2c_rows

# metres by which a hit must lie in front of the point to occlude it, so that a surface point is not hidden by the face it lies
# on.  Unpinned: the reference has no such test.  The package's own choice, below the 5 cm the 3D metrics resolve and far above
# f64 rounding.
OCCLUSION_EPS = 0.03
UNSEEN_SAMPLES = 200000

H, W = 680, 1200                      # cull_mesh's Replica constants (cull_mesh.py:31-37)
FX, FY, CX, CY = 600.0, 600.0, 599.5, 339.5


def opencv_rows(c2w_list):
    """[P,12] float64: the top three rows of each pose of c2w_list (cull_mesh.load_poses's convention: float32, columns 1 and 2
    negated) in OpenCV axes -- the float32 pose widened to f64 with columns 1 and 2 negated back."""
    out = np.empty((len(c2w_list), 12), dtype=np.float64)
    for k, c2w in enumerate(c2w_list):
        m = as_numpy(c2w).astype(np.float32).astype(np.float64)
        m[:3, 1] *= -1.0
        m[:3, 2] *= -1.0
        out[k] = m[:3, :4].reshape(-1)
    return out


def points_visible(bvh, points, c2w_list, H, W, fx, fy, cx, cy, eps=OCCLUSION_EPS, near=0.0):
    """uint8 device tensor [n]: 1 iff some pose of c2w_list (cull_mesh.load_poses's convention, as recon.frustum_seen takes them)
    has the point in its frustum and sees it unoccluded by the mesh of `bvh` (a raycast.MeshBVH): no triangle is hit at a camera
    depth in [near, z_p - eps), z_p the point's own (adfp_points_visible)."""
    if not isinstance(bvh, MeshBVH):
        raise TypeError(f'points_visible: bvh must be a raycast.MeshBVH, got {type(bvh).__name__}')
    dev = bvh.device
    v = as_points(points, dev, 'points')
    n = int(v.shape[0])
    w = torch.from_numpy(w2c_rows(c2w_list)).to(dev).contiguous()
    m = torch.from_numpy(opencv_rows(c2w_list)).to(dev).contiguous()
    P = int(w.shape[0])
    seen = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return seen
    with _lib.on(dev) as L:
        L.adfp_points_visible(bvh._tree(), bvh.bvh.numel(), bvh.n_faces, bvh.leaf, v, n, w, m, P, float(fx), float(fy), float(cx), float(cy),
                              int(W), int(H), float(near), float(eps), seen)
    return seen


def unseen_points(verts, faces, c2w_list, count=UNSEEN_SAMPLES, generator=None, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY,
                  eps=OCCLUSION_EPS):
    """float64 numpy [m,3]: of `count` area-weighted surface samples of the (unculled ground-truth) mesh (recon.sample_surface on
    torch uniforms, from `generator` if given), those that no pose of c2w_list sees, the mesh itself occluding, in sample order."""
    bvh = MeshBVH(verts, faces)
    pts, _ = sample_surface(verts, faces, int(count), generator=generator, device=bvh.device)
    seen = points_visible(bvh, pts, c2w_list, H, W, fx, fy, cx, cy, eps=eps)
    return pts[seen == 0].cpu().numpy()


def main(argv=None):
    from .cull_mesh import load_poses
    parser = argparse.ArgumentParser(description='Arguments to make the unseen-region points of a ground-truth mesh.')
    parser.add_argument('--input_mesh', type=str, help='path to the unculled ground-truth mesh')
    parser.add_argument('--traj', type=str, help='path to the trajectory')
    parser.add_argument('--unseen_points', type=str, help='path to the output .npy (recon_eval reads <culled mesh>_pc_unseen.npy)')
    parser.add_argument('--count', type=int, default=UNSEEN_SAMPLES, help='surface samples to test')
    parser.add_argument('--eps', type=float, default=OCCLUSION_EPS, help='occlusion margin in metres')
    parser.add_argument('--seed', type=int, default=None, help='seed of the sampling (default: torch\'s global stream)')
    args = parser.parse_args(argv)
    poses = load_poses(args.traj)
    m = mesh.read_ply(args.input_mesh)
    g = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
    pc = unseen_points(m.verts, m.faces, poses, count=args.count, generator=g, eps=args.eps)
    with open(args.unseen_points, 'wb') as out:           # np.save on a file object keeps the name as given
        np.save(out, pc)
    return pc


if __name__ == '__main__':
    main()
