"""Iso-surface extraction on the MI355X (libadfp.so adfp_mc_count / adfp_mc_emit, csrc/adfp_mesh.h) and a PLY writer.

What the reference does with skimage.measure.marching_cubes on the host (src/utils/Mesher.py:455-486, src/fusion.py:303-342);
the conventions -- inside iff v > level, one vertex per crossed lattice edge, the face-ambiguity rule, the canonical order of
vertices and triangles -- are those of include/adfp.h.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, check, require_cuda


def marching_cubes(values, level=0., spacing=(1., 1., 1.), origin=(0., 0., 0.), normals=False, outward='lower'):
    """values: device tensor [X,Y,Z] (float32, z fastest).  Returns device tensors (verts f32 [V,3], faces int32 [F,3],
    normals f32 [V,3] or None); vertex = origin + (index + t) * spacing.  outward='lower': triangles wound (and normals
    pointing) toward lower values; 'higher': toward higher values.  An empty surface gives empty tensors."""
    require_cuda(values, 'marching_cubes values')
    if values.dim() != 3:
        raise ValueError(f'marching_cubes: values must be [X,Y,Z], got {tuple(values.shape)}')
    if outward not in _lib.MC_OUT:
        raise ValueError(f"marching_cubes: outward must be 'lower' or 'higher', got {outward!r}")
    v = values.detach().to(torch.float32).contiguous()
    X, Y, Z = (int(s) for s in v.shape)
    dev = v.device
    L = lib()
    nbytes = L.adfp_mc_workspace_bytes(X, Y, Z)
    ws = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    lev = float(np.float32(level))
    with _lib.device_guard(dev):
        st = _lib.current_stream(dev)
        check(L.adfp_mc_count(ptr(v), X, Y, Z, lev, ptr(ws), nbytes, ptr(totals), st), 'adfp_mc_count')
        n_verts, n_faces = (int(t) for t in totals.tolist())          # the one synchronisation of the extraction
        verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
        keys = torch.empty(n_verts, dtype=torch.int64, device=dev)
        nrm = torch.empty((n_verts, 3), dtype=torch.float32, device=dev) if normals else None
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
        org = (C.c_float * 3)(*[float(o) for o in origin])
        sp = (C.c_float * 3)(*[float(s) for s in spacing])
        check(L.adfp_mc_emit(ptr(v), X, Y, Z, lev, C.byref(org), C.byref(sp), _lib.MC_OUT[outward], ptr(ws), nbytes,
                             n_verts, n_faces, ptr(verts) if n_verts else None, ptr(nrm) if (nrm is not None and n_verts) else None,
                             ptr(keys) if n_verts else None, n_verts, ptr(faces) if n_faces else None, n_faces, st), 'adfp_mc_emit')
    return verts, faces, nrm


def hull_fill(values, axes, planes, fill=100.):
    """In place: every lattice point (axes[0][i], axes[1][j], axes[2][k]) outside the convex hull max_f(n_f . p + d_f) > 0
    (planes [F,4] float64) gets `fill` (src/utils/Mesher.py:436-439, :450)."""
    require_cuda(values, 'hull_fill values')
    if not values.is_contiguous() or values.dtype != torch.float32 or values.dim() != 3:
        raise ValueError('hull_fill: values must be a contiguous float32 [X,Y,Z] tensor')
    dev = values.device
    ax = [torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous() for a in axes]
    if tuple(a.numel() for a in ax) != tuple(values.shape):
        raise ValueError('hull_fill: axis lengths do not match the lattice')
    pl = torch.as_tensor(np.asarray(planes, dtype=np.float64).reshape(-1, 4)).to(dev).contiguous()
    X, Y, Z = values.shape
    with _lib.device_guard(dev):
        check(lib().adfp_lattice_hull_fill(ptr(values), ptr(ax[0]), ptr(ax[1]), ptr(ax[2]), X, Y, Z,
                                           ptr(pl) if pl.shape[0] else None, int(pl.shape[0]), float(fill),
                                           _lib.current_stream(dev)), 'adfp_lattice_hull_fill')
    return values


def unpack_colors(verts_index, color_vol):
    """uint8 [V,3] r,g,b of the packed colour volume at the rounded (half-to-even) index-space vertices (src/fusion.py:311-319)."""
    require_cuda(color_vol, 'unpack_colors color volume')
    dev = color_vol.device
    vi = verts_index.to(dev, torch.float32).contiguous()
    cv = color_vol.to(torch.float32).contiguous()
    out = torch.empty((vi.shape[0], 3), dtype=torch.uint8, device=dev)
    X, Y, Z = cv.shape
    with _lib.device_guard(dev):
        check(lib().adfp_mesh_unpack_colors(ptr(vi) if vi.shape[0] else None, int(vi.shape[0]), ptr(cv), X, Y, Z,
                                            ptr(out) if vi.shape[0] else None, _lib.current_stream(dev)), 'adfp_mesh_unpack_colors')
    return out


def _np(x):
    if x is None:
        return None
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def write_ply(path, verts, faces, colors=None, normals=None, ascii=False):
    """Write a triangle mesh as PLY: binary little-endian (default) or ascii.  Vertex properties x y z [nx ny nz] [red green
    blue] (float, float, uchar) and 'property list uchar int vertex_index' faces: the property list of src/fusion.py:meshwrite."""
    v = _np(verts).astype(np.float32).reshape(-1, 3)
    f = _np(faces).astype(np.int32).reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    n = _np(normals)
    c = _np(colors)
    if n is not None:
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
    if c is not None:
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    rec = np.empty(v.shape[0], dtype=fields)
    rec['x'], rec['y'], rec['z'] = v[:, 0], v[:, 1], v[:, 2]
    if n is not None:
        n = n.astype(np.float32).reshape(-1, 3)
        rec['nx'], rec['ny'], rec['nz'] = n[:, 0], n[:, 1], n[:, 2]
    if c is not None:
        c = c.astype(np.uint8).reshape(-1, 3)
        rec['red'], rec['green'], rec['blue'] = c[:, 0], c[:, 1], c[:, 2]
    kind = {'<f4': 'float', 'u1': 'uchar'}
    head = ['ply', 'format ascii 1.0' if ascii else 'format binary_little_endian 1.0', f'element vertex {v.shape[0]}']
    head += [f'property {kind[t]} {name}' for name, t in fields]
    head += [f'element face {f.shape[0]}', 'property list uchar int vertex_index', 'end_header']
    with open(path, 'wb') as out:
        out.write(('\n'.join(head) + '\n').encode('ascii'))
        if ascii:
            fmt = ' '.join('%d' if t == 'u1' else '%f' for _, t in fields)
            for r in rec:
                out.write((fmt % tuple(r) + '\n').encode('ascii'))
            for tri in f:
                out.write(('3 %d %d %d\n' % tuple(tri)).encode('ascii'))
        else:
            out.write(rec.tobytes())
            fr = np.empty(f.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
            fr['n'] = 3
            fr['i'] = f
            out.write(fr.tobytes())
