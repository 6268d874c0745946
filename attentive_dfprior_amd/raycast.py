"""Depth rendering of triangle meshes on the device (libadfp.so, csrc/adfp_raycast.h): a triangle BVH, batched f64 depth renders
with the watertight ray/triangle test, check_proj over a batch of poses and per-view depth L1 sums.  recon_eval.calc_2d_metric is
built on these; the conventions (camera, intersection, clipping) are include/adfp.h's "mesh depth rendering".
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check
from .recon import device_of, as_points, _ws


def _faces(faces, dev):
    f = faces if torch.is_tensor(faces) else torch.from_numpy(np.asarray(faces, dtype=np.int64))
    return f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()


def _c2w_rows(c2w, dev):
    """[P,4,4] / [4,4] / [P,3,4] (numpy or tensor) -> f64 device [P,12]: the top three rows of each pose."""
    t = c2w if torch.is_tensor(c2w) else torch.from_numpy(np.asarray(c2w, dtype=np.float64))
    t = t.detach().to(device=dev, dtype=torch.float64)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[1] not in (3, 4) or t.shape[2] != 4:
        raise ValueError(f'c2w must be [P,4,4] or [4,4], got {tuple(t.shape)}')
    return t[:, :3, :].reshape(-1, 12).contiguous()


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
        f = _faces(faces, dev)
        self.n_verts, self.n_faces = int(v.shape[0]), int(f.shape[0])
        if self.n_faces >= 2 ** 31 - 1024 or self.n_verts >= 2 ** 31 - 1024:
            raise ValueError(f'MeshBVH: {self.n_faces} faces / {self.n_verts} vertices are more than the BVH takes')
        L = lib()
        self.bvh = _ws(L.adfp_tri_bvh_bytes(self.n_faces, self.leaf), dev)
        if self.n_faces:
            wsb = L.adfp_tri_bvh_build_workspace_bytes(self.n_faces)
            ws = _ws(wsb, dev)
            with _lib.device_guard(dev):
                check(L.adfp_tri_bvh_build(ptr(v) if self.n_verts else None, self.n_verts, ptr(f), self.n_faces, self.leaf,
                                           ptr(self.bvh), self.bvh.numel(), ptr(ws), wsb, _lib.current_stream(dev)),
                      'adfp_tri_bvh_build')

    def render_depth(self, c2w, H, W, fx, fy, cx, cy, near, far, cull='none'):
        """f32 device tensor [P,H,W]: camera z of the nearest surface with near <= z <= far, 0 where there is none.  c2w: [P,4,4]
        or [4,4] (OpenCV axes, f64, numpy or tensor); near: a scalar or [P]; far: a scalar.  cull: 'none' (adfp_render_depth),
        'back' or 'front' (adfp_render_depth_cull: front faces have their normal (v1 - v0) x (v2 - v0) toward the camera)."""
        if cull not in _lib.CULL:
            raise ValueError(f"render_depth: cull must be one of {tuple(_lib.CULL)}, got {cull!r}")
        dev = self.device
        m = _c2w_rows(c2w, dev)
        P = int(m.shape[0])
        nr = torch.as_tensor(near, dtype=torch.float64).reshape(-1).to(dev)
        if nr.numel() == 1:
            nr = nr.expand(P)
        if nr.numel() != P:
            raise ValueError(f'render_depth: {nr.numel()} near values for {P} views')
        nr = nr.contiguous()
        depth = torch.empty((P, int(H), int(W)), dtype=torch.float32, device=dev)
        if P == 0:
            return depth
        with _lib.device_guard(dev):
            if cull == 'none':
                check(lib().adfp_render_depth(ptr(self.bvh) if self.n_faces else None, self.bvh.numel(), self.n_faces, self.leaf,
                                              ptr(m), ptr(nr), float(far), P, int(H), int(W), float(fx), float(fy), float(cx),
                                              float(cy), ptr(depth), _lib.current_stream(dev)), 'adfp_render_depth')
            else:
                check(lib().adfp_render_depth_cull(ptr(self.bvh) if self.n_faces else None, self.bvh.numel(), self.n_faces,
                                                   self.leaf, ptr(m), ptr(nr), float(far), P, int(H), int(W), float(fx), float(fy),
                                                   float(cx), float(cy), _lib.CULL[cull], ptr(depth), _lib.current_stream(dev)),
                      'adfp_render_depth_cull')
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
        m = _c2w_rows(c2w, dev)
        P = int(m.shape[0])
        nr = torch.as_tensor(near, dtype=torch.float64).reshape(-1).to(dev)
        if nr.numel() == 1:
            nr = nr.expand(P)
        if nr.numel() != P:
            raise ValueError(f'render_hits: {nr.numel()} near values for {P} views')
        nr = nr.contiguous()
        H, W = int(H), int(W)
        shapes = {'depth': ((P, H, W), torch.float32), 'face': ((P, H, W), torch.int32), 'bary': ((P, H, W, 2), torch.float32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        if P == 0:
            return out
        with _lib.device_guard(dev):
            check(lib().adfp_render_hits(ptr(self.bvh) if self.n_faces else None, self.bvh.numel(), self.n_faces, self.leaf, ptr(m),
                                         ptr(nr), float(far), P, H, W, float(fx), float(fy), float(cx), float(cy), _lib.CULL[cull],
                                         ptr(out.get('depth')), ptr(out.get('face')), ptr(out.get('bary')),
                                         _lib.current_stream(dev)), 'adfp_render_hits')
        return out


def proj_rows(c2w_list):
    """[P,12] float32: the top three rows of inv(c2w') for each pose, c2w' = c2w with columns 1 and 2 negated, inverted in f64
    and rounded to f32 (eval_recon.py:75-80)."""
    out = np.empty((len(c2w_list), 12), dtype=np.float32)
    for k, c2w in enumerate(c2w_list):
        m = np.array(c2w.detach().cpu().numpy() if torch.is_tensor(c2w) else c2w, dtype=np.float64, copy=True)
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
    with _lib.device_guard(dev):
        check(lib().adfp_views_in_sight(ptr(v) if n else None, n, ptr(w), P, float(fx), float(fy), float(cx), float(cy), int(W),
                                        int(H), ptr(out), _lib.current_stream(dev)), 'adfp_views_in_sight')
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
    L = lib()
    wsb = L.adfp_depth_l1_workspace_bytes(P, n)
    ws = _ws(wsb, dev)
    with _lib.device_guard(dev):
        check(L.adfp_depth_l1_sums(ptr(a) if n else None, ptr(b) if n else None, P, n, ptr(ws), wsb, ptr(out),
                                   _lib.current_stream(dev)), 'adfp_depth_l1_sums')
    return out
