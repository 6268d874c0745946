"""Depth rendering of triangle meshes on the device (libadfp.so, csrc/adfp_raycast.h): a triangle BVH, batched f64 depth renders
with the watertight ray/triangle test, check_proj over a batch of poses and per-view depth L1 sums.  recon_eval.calc_2d_metric is
built on these; the conventions (camera, intersection, clipping) are include/adfp.h's "mesh depth rendering".
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib
from .recon import device_of, as_points, as_faces, as_numpy, pose_rows


def near_rows(near, P, dev, what):
    """The near planes of P views, a scalar or [P] -> contiguous f64 [P] on `dev`; `what` names the caller in the refusal."""
    nr = torch.as_tensor(near, dtype=torch.float64).reshape(-1).to(dev)
    if nr.numel() == 1:
        nr = nr.expand(P)
    if nr.numel() != P:
        raise ValueError(f'{what}: {nr.numel()} near values for {P} views')
    return nr.contiguous()


class MeshBVH(object):
    """A triangle BVH over (verts [V,3], faces [F,3]) on the device (adfp_tri_bvh_build): faces in Morton order of their centroids,
    leaves of `leaf` triangles (4, 8 or 16) with their f64 vertices, an implicit binary tree of leaf boxes.  A face with an index
    outside [0, V) is never hit."""

    def __init__(self, verts, faces, device=None, leaf=_lib.TRI_LEAF_DEFAULT):
        dev = torch.device(device) if device is not None else device_of(verts, faces)
        self.device = dev
        if leaf not in _lib.TRI_LEAVES:
            raise ValueError(f'MeshBVH: leaf must be one of {_lib.TRI_LEAVES}, got {leaf}')
        self.leaf = int(leaf)
        v = as_points(verts, dev, 'vertices')
        f = as_faces(faces, dev, np.int64)
        self.n_verts, self.n_faces = int(v.shape[0]), int(f.shape[0])
        if self.n_faces >= 2 ** 31 - 1024 or self.n_verts >= 2 ** 31 - 1024:
            raise ValueError(f'MeshBVH: {self.n_faces} faces / {self.n_verts} vertices are more than the BVH takes')
        self.bvh = _lib.workspace(lib().adfp_tri_bvh_bytes(self.n_faces, self.leaf), dev)
        if self.n_faces:
            wsb = lib().adfp_tri_bvh_build_workspace_bytes(self.n_faces)
            with _lib.on(dev) as L:
                L.adfp_tri_bvh_build(v, self.n_verts, f, self.n_faces, self.leaf, self.bvh, self.bvh.numel(), _lib.workspace(wsb, dev), wsb)

    def _tree(self):
        """what the walks take as `bvh`: NULL for a mesh without faces, whose buffer holds nothing"""
        return self.bvh if self.n_faces else None

    def render_depth(self, c2w, H, W, fx, fy, cx, cy, near, far, cull='none'):
        """f32 device tensor [P,H,W]: camera z of the nearest surface with near <= z <= far, 0 where there is none.  c2w: [P,4,4]
        or [4,4] (OpenCV axes, f64, numpy or tensor); near: a scalar or [P]; far: a scalar.  cull: 'none' (adfp_render_depth),
        'back' or 'front' (adfp_render_depth_cull: front faces have their normal (v1 - v0) x (v2 - v0) toward the camera)."""
        if cull not in _lib.CULL:
            raise ValueError(f"render_depth: cull must be one of {tuple(_lib.CULL)}, got {cull!r}")
        dev = self.device
        m = pose_rows(c2w, dev)
        P = int(m.shape[0])
        nr = near_rows(near, P, dev, 'render_depth')
        depth = torch.empty((P, int(H), int(W)), dtype=torch.float32, device=dev)
        if P == 0:
            return depth
        with _lib.on(dev) as L:
            if cull == 'none':
                L.adfp_render_depth(self._tree(), self.bvh.numel(), self.n_faces, self.leaf, m, nr, float(far), P, int(H), int(W),
                                    float(fx), float(fy), float(cx), float(cy), depth)
            else:
                L.adfp_render_depth_cull(self._tree(), self.bvh.numel(), self.n_faces, self.leaf, m, nr, float(far), P, int(H), int(W),
                                         float(fx), float(fy), float(cx), float(cy), _lib.CULL[cull], depth)
        return depth

    def render_hits(self, c2w, H, W, fx, fy, cx, cy, near, far, cull='none', want=('depth', 'face', 'bary')):
        """What each pixel sees (adfp_render_hits), a dict of device tensors with the keys of `want`: 'depth' f32 [P,H,W],
        render_depth's image bit for bit; 'face' int32 [P,H,W], the row of `faces` of the nearest hit (the smallest row among hits
        of equal z), -1 where there is none; 'bary' f32 [P,H,W,2], the weights of that face's v1 and v2 (v0 has the rest), 0
        where there is none.  The arguments are render_depth's."""
        if cull not in _lib.CULL:
            raise ValueError(f"render_hits: cull must be one of {tuple(_lib.CULL)}, got {cull!r}")
        want = (want,) if isinstance(want, str) else tuple(want)
        if not want or any(k not in ('depth', 'face', 'bary') for k in want):
            raise ValueError(f"render_hits: want must name some of 'depth', 'face', 'bary', got {want!r}")
        dev = self.device
        m = pose_rows(c2w, dev)
        P = int(m.shape[0])
        nr = near_rows(near, P, dev, 'render_hits')
        H, W = int(H), int(W)
        shapes = {'depth': ((P, H, W), torch.float32), 'face': ((P, H, W), torch.int32), 'bary': ((P, H, W, 2), torch.float32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        if P == 0:
            return out
        with _lib.on(dev) as L:
            L.adfp_render_hits(self._tree(), self.bvh.numel(), self.n_faces, self.leaf, m, nr, float(far), P, H, W, float(fx), float(fy),
                               float(cx), float(cy), _lib.CULL[cull], out.get('depth'), out.get('face'), out.get('bary'))
        return out


def proj_rows(c2w_list):
    """[P,12] float32: the top three rows of inv(c2w') for each pose, c2w' = c2w with columns 1 and 2 negated, inverted in f64
    and rounded to f32 (eval_recon.py:75-80)."""
    out = np.empty((len(c2w_list), 12), dtype=np.float32)
    for k, c2w in enumerate(c2w_list):
        m = np.array(as_numpy(c2w), dtype=np.float64, copy=True)
        m[:3, 1] *= -1.0
        m[:3, 2] *= -1.0
        out[k] = np.linalg.inv(m)[:3, :4].astype(np.float32).reshape(-1)
    return out


def views_in_sight(points, c2w_list, H, W, fx, fy, cx, cy, device=None):
    """bool device tensor [P]: check_proj(points, W, H, fx, fy, cx, cy, c2w) for each pose of c2w_list (adfp_views_in_sight)."""
    dev = torch.device(device) if device is not None else device_of(points)
    v = as_points(points, dev, 'points')
    w = torch.from_numpy(proj_rows(c2w_list)).to(dev).contiguous()
    P = int(w.shape[0])
    out = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return out.bool()
    n = int(v.shape[0])
    with _lib.on(dev) as L:
        L.adfp_views_in_sight(v, n, w, P, float(fx), float(fy), float(cx), float(cy), int(W), int(H), out)
    return out.bool()


def depth_l1_sums(a, b):
    """f64 device tensor [P]: per view, the sum over pixels of |a - b| (the f32 difference, widened) for two f32 [P,...] tensors
    (adfp_depth_l1_sums; deterministic)."""
    if a.shape != b.shape:
        raise ValueError(f'depth_l1_sums: shapes {tuple(a.shape)} and {tuple(b.shape)} differ')
    dev = a.device
    a = a.detach().to(torch.float32).contiguous()
    b = b.detach().to(device=dev, dtype=torch.float32).contiguous()
    P = int(a.shape[0]) if a.dim() else 1
    n = int(a.numel() // P) if P else 0
    out = torch.empty(P, dtype=torch.float64, device=dev)
    if P == 0:
        return out
    wsb = lib().adfp_depth_l1_workspace_bytes(P, n)
    with _lib.on(dev) as L:
        L.adfp_depth_l1_sums(a, b, P, n, _lib.workspace(wsb, dev), wsb, out)
    return out
