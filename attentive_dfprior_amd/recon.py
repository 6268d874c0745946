"""Device pieces of reconstruction evaluation (libadfp.so, csrc/adfp_recon.h): the exact f64 nearest-neighbour index, the
deterministic metric and ICP reductions, area-weighted surface sampling and frustum culling.  recon_eval.py and cull_mesh.py
build the reference's tools (src/tools/eval_recon.py, src/tools/cull_mesh.py) on these; the conventions are include/adfp.h's.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib


def device_of(*xs):
    """The CUDA device of the first device tensor among xs, else the current one."""
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise RuntimeError('attentive_dfprior_amd.recon needs a GPU (there is no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device())


def as_points(x, dev, what='points'):
    """numpy array or tensor [N,3] -> contiguous f64 device tensor."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
    t = t.detach().to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()
    return t


def as_faces(x, dev, dtype=None):
    """numpy array or tensor -> detached contiguous int32 [F,3] on `dev`.  dtype: what np.asarray makes of an array before torch
    sees it.  raycast, render_mesh and mesh.vertex_normals have always widened to np.int64 (any integer array goes through, a
    uint32 index >= 2^31 wraps); sample_surface and faces_kept hand torch the array's own dtype (None) and so refuse what
    torch.from_numpy refuses: the two are kept as they were."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, dtype=dtype))
    return t.detach().to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()


def as_numpy(x):
    """tensor (anywhere) or array -> numpy array on the host, None -> None"""
    if x is None:
        return None
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def pose_rows(c2w, dev):
    """[P,4,4] / [4,4] / [P,3,4] (numpy or tensor) -> f64 device [P,12]: the top three rows of each pose."""
    t = c2w if torch.is_tensor(c2w) else torch.from_numpy(np.asarray(c2w, dtype=np.float64))
    t = t.detach().to(device=dev, dtype=torch.float64)
    if t.dim() == 2:
        t = t[None]
    if t.dim() != 3 or t.shape[1] not in (3, 4) or t.shape[2] != 4:
        raise ValueError(f'c2w must be [P,4,4] or [4,4], got {tuple(t.shape)}')
    return t[:, :3, :].reshape(-1, 12).contiguous()


def _t12(transform):
    if transform is None:
        return None
    T = np.asarray(transform, dtype=np.float64)
    return (C.c_double * 12)(*[float(v) for v in T[:3, :4].reshape(-1)])


class NNIndex(object):
    """Exact nearest-neighbour index over ref [N,3] (f64 on the device): Morton-ordered leaves of 16 points under an implicit
    binary tree of leaf boxes (adfp_nn_build).  query() answers with the distance and the ORIGINAL index of the nearest point."""

    def __init__(self, ref, device=None):
        dev = torch.device(device) if device is not None else device_of(ref)
        self.device = dev
        self.ref = as_points(ref, dev, 'reference points')
        self.n = int(self.ref.shape[0])
        if self.n >= 2 ** 31 - 1024:
            raise ValueError(f'NNIndex: {self.n} reference points are more than the index takes')
        self.index = _lib.workspace(lib().adfp_nn_index_bytes(self.n), dev)
        if self.n:
            wsb = lib().adfp_nn_build_workspace_bytes(self.n)
            with _lib.on(dev) as L:
                L.adfp_nn_build(self.ref, self.n, self.index, self.index.numel(), _lib.workspace(wsb, dev), wsb)

    def query(self, points, transform=None, radius=math.inf, sort_queries=True):
        """points [M,3] -> (dist f64 [M], idx int32 [M]) device tensors.  transform: optional 3x4 (or 4x4) applied to the points
        on the fly; radius: only d^2 < radius^2 counts (else idx -1, dist inf)."""
        q = as_points(points, self.device, 'query points')
        m = int(q.shape[0])
        dist = torch.empty(m, dtype=torch.float64, device=self.device)
        idx = torch.empty(m, dtype=torch.int32, device=self.device)
        if m == 0:
            return dist, idx
        if self.n == 0:
            raise ValueError('NNIndex.query: the index holds no points')
        flags = _lib.NN_SORT_QUERIES if sort_queries else 0
        wsb = lib().adfp_nn_query_workspace_bytes(m, flags)
        t = _t12(transform)
        with _lib.on(self.device) as L:
            L.adfp_nn_query(self.index, self.index.numel(), self.n, q, m, C.byref(t) if t is not None else None, float(radius), flags,
                            _lib.workspace(wsb, self.device), wsb, dist, idx)
        return dist, idx


def metric_sums(dist, threshold):
    """(sum of dist, count of dist < threshold) over a f64 device tensor, as two Python floats (one synchronisation)."""
    d = dist.detach().to(torch.float64).contiguous()
    dev = d.device
    n = int(d.numel())
    wsb = lib().adfp_recon_reduce_workspace_bytes(n)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with _lib.on(dev) as L:
        L.adfp_nn_metric_sums(d, n, float(threshold), _lib.workspace(wsb, dev), wsb, out)
    s, c = out.tolist()
    return s, c


def icp_moments(src, transform, origin, tgt, idx):
    """The 17 moments of adfp_icp_moments (count, sum d^2, sum p, sum q, sum p q^T) as a float64 numpy array."""
    dev = src.device
    n = int(src.shape[0])
    wsb = lib().adfp_recon_reduce_workspace_bytes(n)
    out = torch.empty(_lib.ICP_MOMENTS, dtype=torch.float64, device=dev)
    t = _t12(transform)
    o = (C.c_double * 3)(*[float(v) for v in origin])
    with _lib.on(dev) as L:
        L.adfp_icp_moments(src, n, C.byref(t), C.byref(o), tgt, int(tgt.shape[0]), idx, _lib.workspace(wsb, dev), wsb, out)
    return out.cpu().numpy()


def draw_uniforms(count, device, generator=None):
    """The uniforms sample_surface consumes, drawn by torch: u_face [count], u_bary [count, 2] (f64, on `device`)."""
    g = generator
    gdev = g.device if g is not None else torch.device('cpu')
    u_face = torch.rand(count, dtype=torch.float64, generator=g, device=gdev).to(device)
    u_bary = torch.rand((count, 2), dtype=torch.float64, generator=g, device=gdev).to(device)
    return u_face, u_bary


def sample_surface(verts, faces, count=None, u_face=None, u_bary=None, generator=None, device=None):
    """trimesh.sample.sample_surface(mesh, count) on the device (adfp_sample_surface): area-weighted faces, folded barycentric
    pairs.  Either `count` (uniforms drawn with torch, from `generator` if given) or the uniforms themselves.
    Returns (points f64 [count,3], face_index int32 [count]) device tensors."""
    dev = torch.device(device) if device is not None else device_of(verts, faces, u_face)
    v = as_points(verts, dev, 'vertices')
    f = as_faces(faces, dev)
    if u_face is None:
        u_face, u_bary = draw_uniforms(int(count), dev, generator)
    uf = torch.as_tensor(u_face).to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    ub = torch.as_tensor(u_bary).to(device=dev, dtype=torch.float64).reshape(-1, 2).contiguous()
    n = int(uf.numel())
    if ub.shape[0] != n:
        raise ValueError(f'sample_surface: {n} face draws but {ub.shape[0]} barycentric pairs')
    pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    fi = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return pts, fi
    if f.shape[0] == 0:
        raise ValueError('sample_surface: the mesh has no faces')
    wsb = lib().adfp_sample_surface_workspace_bytes(int(f.shape[0]))
    with _lib.on(dev) as L:
        L.adfp_sample_surface(v, int(v.shape[0]), f, int(f.shape[0]), uf, ub, n, _lib.workspace(wsb, dev), wsb, pts, fi)
    return pts, fi


def w2c_rows(c2w_list):
    """[P,12] float32: the top three rows of np.linalg.inv(c2w) for each float32 pose -- numpy inverts a float32 matrix in f64 and
    rounds the result to float32, which is what cull_mesh.py:53 gets."""
    out = np.empty((len(c2w_list), 12), dtype=np.float32)
    for k, c2w in enumerate(c2w_list):
        w2c = np.linalg.inv(as_numpy(c2w).astype(np.float32))
        out[k] = w2c[:3, :4].astype(np.float32).reshape(-1)
    return out


def frustum_seen(verts, c2w_list, H, W, fx, fy, cx, cy, device=None):
    """uint8 [V] device tensor: 1 iff some pose of c2w_list sees the vertex (adfp_cull_vertices, cull_mesh.py:49-71)."""
    dev = torch.device(device) if device is not None else device_of(verts)
    v = as_points(verts, dev, 'vertices')
    w = torch.from_numpy(w2c_rows(c2w_list)).to(dev).contiguous()
    seen = torch.empty(int(v.shape[0]), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as L:
        L.adfp_cull_vertices(v, int(v.shape[0]), w, int(w.shape[0]), float(fx), float(fy), float(cx), float(cy), int(W), int(H), seen)
    return seen


def faces_kept(seen, faces):
    """uint8 [F] device tensor: 0 iff all three vertices of the face are unseen (adfp_cull_faces, cull_mesh.py:72-74)."""
    dev = seen.device
    f = as_faces(faces, dev)
    keep = torch.empty(int(f.shape[0]), dtype=torch.uint8, device=dev)
    with _lib.on(dev) as L:
        L.adfp_cull_faces(seen, int(seen.numel()), f, int(f.shape[0]), keep)
    return keep
