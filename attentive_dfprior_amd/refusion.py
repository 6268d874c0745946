"""Refusion of a mesh on the device (libadfp.so, csrc/adfp_refuse.h): open3d-style unit touch marks, unit-gated TSDF integration
over a dense box of 16^3-voxel units, extraction of the observed surface with the marching cubes of mesh.py, and open3d-style voxel
downsampling.  evaluate_scannet.refuse / evaluate are built on these; the contracts are include/adfp.h's "ScanNet mesh evaluation".
"""
import ctypes as C
import numpy as np
import torch

from . import _lib, mesh
from ._lib import lib
from .recon import as_points

UNIT = _lib.UNIT_VOXELS
MAX_BOX_VOXELS = 2 ** 31


def _i3(x):
    return (C.c_int * 3)(*[int(v) for v in x])


class UnitBox(object):
    """A dense box of whole units: world unit indices lo .. lo + dim - 1 per axis, voxel lattice [16 dim0][16 dim1][16 dim2]."""

    def __init__(self, lo, dim, voxel):
        self.lo = [int(v) for v in lo]
        self.dim = [int(v) for v in dim]
        self.voxel = float(voxel)
        self.unit_length = self.voxel * UNIT
        self.shape = tuple(UNIT * d for d in self.dim)
        self.n_units = self.dim[0] * self.dim[1] * self.dim[2]
        n = self.shape[0] * self.shape[1] * self.shape[2]
        if n > MAX_BOX_VOXELS:
            raise ValueError(f'refusion: the box of {self.dim} units holds {n} voxels, more than 2^31')

    @classmethod
    def around(cls, verts, voxel, sdf_trunc):
        """The units that a depth point on the mesh can touch: the mesh's AABB grown by sdf_trunc, then by one unit per side."""
        v = np.asarray(verts, np.float64).reshape(-1, 3)
        L = float(voxel) * UNIT
        if len(v) == 0:
            return cls([0, 0, 0], [1, 1, 1], voxel)
        lo = np.floor((v.min(0) - sdf_trunc) / L).astype(np.int64) - 1
        hi = np.floor((v.max(0) + sdf_trunc) / L).astype(np.int64) + 1
        return cls(lo.tolist(), (hi - lo + 1).tolist(), voxel)

    def origin_voxel(self):
        """World voxel index of the lattice's first voxel, per axis."""
        return [UNIT * v for v in self.lo]


def touch(depth, c2w, box, fx, fy, cx, cy, stride, depth_trunc, sdf_trunc, outside):
    """uint8 device tensor [P, units]: adfp_refuse_touch over depth [P,H,W] (f32 device) and c2w [P,12] (f64 device); `outside`:
    one device int32 the out-of-box touches are added to."""
    P, H, W = (int(s) for s in depth.shape)
    out = torch.empty((P, box.n_units), dtype=torch.uint8, device=depth.device)
    if P == 0:
        return out
    dev = depth.device
    with _lib.on(dev) as L:
        L.adfp_refuse_touch(depth, P, H, W, c2w, float(fx), float(fy), float(cx), float(cy), int(stride), float(depth_trunc),
                            float(sdf_trunc), box.unit_length, C.byref(_i3(box.lo)), C.byref(_i3(box.dim)), out, outside)
    return out


def integrate(tsdf, weight, box, units, depth, w2c, touched, fx, fy, cx, cy, sdf_trunc, depth_trunc):
    """In place: adfp_refuse_integrate of one chunk of views over the listed units (int32 device tensor)."""
    P, H, W = (int(s) for s in depth.shape)
    n = int(units.numel())
    if n == 0 or P == 0:
        return
    dev = tsdf.device
    with _lib.on(dev) as L:
        L.adfp_refuse_integrate(tsdf, weight, C.byref(_i3(box.lo)), C.byref(_i3(box.dim)), box.voxel, units, n, depth, w2c, touched,
                                P, H, W, float(fx), float(fy), float(cx), float(cy), float(sdf_trunc), float(depth_trunc))


def extract(tsdf, weight, box):
    """The observed surface: marching cubes of where(weight > 0, -tsdf, NaN) at level 0 (inside iff tsdf < 0; a cube with a
    weight-0 corner emits nothing), then only the vertices some face references, renumbered in order.  Returns device tensors
    (verts f32 [V,3], faces int32 [F,3])."""
    values = torch.where(weight > 0, -tsdf, torch.full_like(tsdf, float('nan')))
    org = [(o + 0.5) * box.voxel for o in box.origin_voxel()]
    verts, faces, _ = mesh.marching_cubes(values, 0.0, spacing=(box.voxel,) * 3, origin=org, outward='lower')
    return compact(verts, faces)


def compact(verts, faces):
    """Drop the vertices no face references; the others keep their order."""
    used = torch.zeros(int(verts.shape[0]), dtype=torch.bool, device=verts.device)
    if faces.numel():
        used[faces.reshape(-1).long()] = True
    new = torch.cumsum(used.to(torch.int64), 0) - 1
    return verts[used].contiguous(), new[faces.long()].to(torch.int32).contiguous() if faces.numel() else faces


def voxel_down_sample(points, voxel_size, device=None):
    """open3d's PointCloud.voxel_down_sample as adfp_voxel_down_sample reads it: (means f64 [M,3], counts int32 [M]) device
    tensors, one row per occupied cell in ascending cell-key order."""
    dev = torch.device(device) if device is not None else (points.device if torch.is_tensor(points) and points.is_cuda else
                                                           torch.device('cuda', torch.cuda.current_device()))
    p = as_points(points, dev, 'points')
    n = int(p.shape[0])
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty((0, 3), dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    lo, hi = torch.aminmax(p, dim=0)
    lo3 = (C.c_double * 3)(*lo.tolist())
    hi3 = (C.c_double * 3)(*hi.tolist())
    out = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    wsb = lib().adfp_voxel_down_sample_workspace_bytes(n)
    with _lib.on(dev) as L:
        L.adfp_voxel_down_sample(p, n, float(voxel_size), C.byref(lo3), C.byref(hi3), _lib.workspace(wsb, dev), wsb, out, cnt, total)
    m = int(total.item())
    return out[:m], cnt[:m]


def w2c_rows(poses):
    """[P,12] f32: the top rows of inv(pose) for each f32 pose, inverted in f64 and rounded (np.linalg.inv of a float32 matrix)."""
    out = np.empty((len(poses), 12), dtype=np.float32)
    for k, m in enumerate(poses):
        with np.errstate(all='ignore'):
            try:
                inv = np.linalg.inv(np.asarray(m, np.float32).astype(np.float64))
            except np.linalg.LinAlgError:
                inv = np.full((4, 4), np.nan)
        out[k] = inv[:3, :4].astype(np.float32).reshape(-1)
    return out


def backproject_rows(w2c):
    """[P,12] f64: the pose that back-projects, open3d's extrinsic.inverse() of the f32 extrinsic rows (bottom row 0 0 0 1)."""
    out = np.empty((len(w2c), 12), dtype=np.float64)
    for k, r in enumerate(w2c):
        m = np.eye(4)
        m[:3, :4] = np.asarray(r, np.float64).reshape(3, 4)
        with np.errstate(all='ignore'):
            try:
                inv = np.linalg.inv(m) if np.isfinite(m).all() else np.full((4, 4), np.nan)
            except np.linalg.LinAlgError:
                inv = np.full((4, 4), np.nan)
        out[k] = inv[:3, :4].reshape(-1)
    return out


def chunk_views(H, W, cap=64, budget_bytes=256 * 2 ** 20):
    """Views per integration chunk: at most `cap`, and no more depth images than fit the 256 MB Infinity Cache."""
    return max(1, min(int(cap), budget_bytes // max(1, 4 * int(H) * int(W))))
