"""Iso-surface extraction on the MI355X (libadfp.so adfp_mc_count / adfp_mc_emit, csrc/adfp_mesh.h) and a PLY writer.

What the reference does with skimage.measure.marching_cubes on the host (src/utils/Mesher.py:455-486, src/fusion.py:303-342);
the conventions -- inside iff v > level, one vertex per crossed lattice edge, the face-ambiguity rule, the canonical order of
vertices and triangles -- are those of include/adfp.h.
"""
import ctypes as C
import struct
import time

import numpy as np
import torch

from . import _lib
from ._lib import lib, require_cuda
from .recon import as_faces, as_numpy


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
    nbytes = lib().adfp_mc_workspace_bytes(X, Y, Z)
    ws = _lib.workspace(nbytes, dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    lev = float(np.float32(level))
    with _lib.on(dev) as L:
        L.adfp_mc_count(v, X, Y, Z, lev, ws, nbytes, totals)
        n_verts, n_faces = (int(t) for t in totals.tolist())          # the one synchronisation of the extraction
        verts = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
        keys = torch.empty(n_verts, dtype=torch.int64, device=dev)
        nrm = torch.empty((n_verts, 3), dtype=torch.float32, device=dev) if normals else None
        faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
        org = (C.c_float * 3)(*[float(o) for o in origin])
        sp = (C.c_float * 3)(*[float(s) for s in spacing])
        L.adfp_mc_emit(v, X, Y, Z, lev, C.byref(org), C.byref(sp), _lib.MC_OUT[outward], ws, nbytes, n_verts, n_faces, verts, nrm, keys,
                       n_verts, faces, n_faces)
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
    with _lib.on(dev) as L:
        L.adfp_lattice_hull_fill(values, ax[0], ax[1], ax[2], X, Y, Z, pl, int(pl.shape[0]), float(fill))
    return values


def unpack_colors(verts_index, color_vol):
    """uint8 [V,3] r,g,b of the packed colour volume at the rounded (half-to-even) index-space vertices (src/fusion.py:311-319)."""
    require_cuda(color_vol, 'unpack_colors color volume')
    dev = color_vol.device
    vi = verts_index.to(dev, torch.float32).contiguous()
    cv = color_vol.to(torch.float32).contiguous()
    out = torch.empty((vi.shape[0], 3), dtype=torch.uint8, device=dev)
    X, Y, Z = cv.shape
    with _lib.on(dev) as L:
        L.adfp_mesh_unpack_colors(vi, int(vi.shape[0]), cv, X, Y, Z, out)
    return out


# ---- mesh clean-up on the device (csrc/adfp_meshclean.h; contracts: include/adfp.h, "mesh clean-up") ---------------------------
def _mesh_tensors(verts, faces, what):
    if faces is None:
        raise ValueError(f'{what}: faces is None')
    require_cuda(faces, f'{what} faces')
    f = as_faces(faces, faces.device)
    if verts is None:
        return None, f
    require_cuda(verts, f'{what} verts')
    return verts.detach().reshape(-1, 3).to(f.device, torch.float32).contiguous(), f


def _check_indices(faces, n_verts, what):
    """Reject indices outside [0, n_verts) on the host (one read-back); the kernels never dereference them either way."""
    if faces.numel():
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(faces)).tolist())
        if lo < 0 or hi >= n_verts:
            raise ValueError(f'{what}: face indices span [{lo}, {hi}], outside [0, {n_verts})')


def _vertex_colors(colors, v, what):
    """The optional uint8 [V,3] colours of the vertices v, contiguous on their device."""
    if colors is None:
        return None
    require_cuda(colors, f'{what} colors')
    c = colors.detach().reshape(-1, 3).to(v.device, torch.uint8).contiguous()
    if c.shape[0] != v.shape[0]:
        raise ValueError(f'{what}: {c.shape[0]} colours for {v.shape[0]} vertices')
    return c


def _face_labels(faces, n_verts, keep=None):
    """labels int32 [F] (-1 where keep is 0) of contiguous int32 device faces; see face_components."""
    dev = faces.device
    F = int(faces.shape[0])
    labels = torch.empty(F, dtype=torch.int32, device=dev)
    if F == 0:
        return labels
    mate = torch.empty(3 * F, dtype=torch.int32, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    with _lib.on(dev) as L:
        nbytes = lib().adfp_mesh_face_labels_workspace_bytes(F)
        if nbytes == 0:
            raise RuntimeError(f'face_components: {F} faces are more than the int32 sort carries')
        L.adfp_mesh_face_labels_begin(faces, F, int(n_verts), keep, mate, labels, _lib.workspace(nbytes, dev), nbytes)
        done, step = 0, 4
        while True:
            L.adfp_mesh_face_labels_rounds(mate, labels, F, step, changed)
            done += step
            if int(changed.item()) == 0:                  # the convergence flag: one scalar per `step` rounds
                return labels
            if done >= _lib.LABEL_ROUNDS_MAX:
                raise RuntimeError(f'face_components: no fixed point after {done} rounds (the worst case is 2 log2(F) + 2)')


def face_components(faces, n_verts):
    """Component label of every face (int32 [F], device): two faces are joined only through an edge that exactly two faces use
    (trimesh.graph.face_adjacency, what Mesher.clean derives with scipy); a face's label is the smallest face index of its
    component, so the labels order the components as scipy does (by first face) and do not depend on any launch order."""
    _, f = _mesh_tensors(None, faces, 'face_components')
    _check_indices(f, int(n_verts), 'face_components')
    return _face_labels(f, int(n_verts))


def _clean_components(v, f, seen, min_area, largest):
    dev = f.device
    V, F = int(v.shape[0]), int(f.shape[0])
    with _lib.on(dev) as L:
        keep = torch.empty(max(F, 1), dtype=torch.uint8, device=dev)
        L.adfp_cull_faces(seen, V, f, F, keep)
        labels = _face_labels(f, V, keep)
        if F:
            nbytes = lib().adfp_mesh_component_keep_workspace_bytes(F)
            L.adfp_mesh_component_keep(v, V, f, F, labels, 1 if largest else 0, 0.0 if largest else float(min_area), keep,
                                       _lib.workspace(nbytes, dev), nbytes)
        nbytes = lib().adfp_mesh_compact_workspace_bytes(V, F)
        ws = _lib.workspace(nbytes, dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        L.adfp_mesh_compact_plan(f, F, V, keep, ws, nbytes, totals)
        nv, nf = (int(t) for t in totals.tolist())                       # the counts: one read-back
        vo = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        fo = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        L.adfp_mesh_compact_emit(v, V, f, F, ws, nbytes, vo, nv, fo, nf)
    return vo, fo


def clean_components(verts, faces, seen, min_area=None, largest=False):
    """Mesher.clean on device tensors: drop the faces whose three vertices are unseen (seen: bool / uint8 [V]), split the rest into
    components (face_components), keep the component of largest area (largest=True; the first among equals) or those whose area
    exceeds min_area, keep the referenced vertices.  Returns (verts f32 [V',3], faces int32 [F',3]): kept faces in their order,
    vertices in ascending index, the arrays Mesher.clean returns.  Areas are summed in f64 in a fixed order that is not
    np.bincount's: a component within rounding of min_area (or of the runner-up) can fall on the other side."""
    v, f = _mesh_tensors(verts, faces, 'clean_components')
    if not largest and min_area is None:
        raise ValueError('clean_components: min_area is required unless largest=True')
    require_cuda(seen, 'clean_components seen')
    s = seen.detach().reshape(-1).to(f.device).ne(0).to(torch.uint8).contiguous()
    if s.shape[0] != v.shape[0]:
        raise ValueError(f'clean_components: seen has {s.shape[0]} entries for {v.shape[0]} vertices')
    _check_indices(f, int(v.shape[0]), 'clean_components')
    return _clean_components(v, f, s, min_area, largest)


def _merge_coincident(v, f, c):
    dev = v.device
    V, F = int(v.shape[0]), int(f.shape[0])
    if V == 0:
        return v, f, c
    with _lib.on(dev) as L:
        nbytes = lib().adfp_mesh_merge_workspace_bytes(V)
        ws = _lib.workspace(nbytes, dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)
        L.adfp_mesh_merge_plan(v, V, ws, nbytes, total)
        n = int(total.item())
        if n == V:                                          # nothing coincides: the inputs, as the host function returns them
            return v, f, c
        vo = torch.empty((n, 3), dtype=torch.float32, device=dev)
        co = torch.empty((n, 3), dtype=torch.uint8, device=dev) if c is not None else None
        fo = torch.empty((F, 3), dtype=torch.int32, device=dev)
        L.adfp_mesh_merge_emit(v, c, V, f, F, ws, nbytes, vo, co, n, fo)
    return vo, fo, co


def merge_coincident(verts, faces, colors=None):
    """mesher.merge_coincident on device tensors: vertices whose three f32 bit patterns are equal collapse into their first
    occurrence, survivors keep their order, faces and colours (uint8 [V,3]) follow.  Returns (verts, faces, colors)."""
    v, f = _mesh_tensors(verts, faces, 'merge_coincident')
    return _merge_coincident(v, f, _vertex_colors(colors, v, 'merge_coincident'))


# ---- mesh simplification (csrc/adfp_meshsimplify.h; contract: include/adfp.h, "mesh simplification") ---------------------------
SIMPLIFY_CONTRACTIONS = _lib.SIMPLIFY


def _simplify_vertex_clustering(v, f, voxel_size, contraction, c):
    dev = v.device
    V, F = int(v.shape[0]), int(f.shape[0])
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
             torch.empty((0, 3), dtype=torch.uint8, device=dev) if c is not None else None)
    if V == 0 or F == 0:
        return empty
    with _lib.on(dev) as L:
        lo, hi = (x.tolist() for x in torch.aminmax(v, dim=0))           # the bounds: one read-back
        if not np.isfinite(lo + hi).all():
            raise ValueError('simplify_vertex_clustering: the vertices are not all finite')
        nbytes = lib().adfp_mesh_simplify_workspace_bytes(V, F)
        if nbytes == 0:
            raise RuntimeError(f'simplify_vertex_clustering: {V} vertices, {F} faces are more than the int32 sort carries')
        ws = _lib.workspace(nbytes, dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        lo_c, hi_c = (C.c_double * 3)(*lo), (C.c_double * 3)(*hi)
        L.adfp_mesh_simplify_plan(v, V, f, F, c, float(voxel_size), SIMPLIFY_CONTRACTIONS[contraction], C.byref(lo_c), C.byref(hi_c), ws,
                                  nbytes, totals)
        nv, nf = (int(t) for t in totals.tolist())                       # the counts: one read-back
        if nf == 0:
            return empty
        vo = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        fo = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        co = torch.empty((nv, 3), dtype=torch.uint8, device=dev) if c is not None else None
        L.adfp_mesh_simplify_emit(V, F, ws, nbytes, vo, co, nv, fo, nf)
    return vo, fo, co


def simplify_vertex_clustering(verts, faces, voxel_size, contraction='quadric', colors=None):
    """Vertex clustering on the device (what open3d users call simplify_vertex_clustering): one vertex per occupied cell of a
    voxel_size lattice (adfp_voxel_down_sample's cells), at the cell's average (contraction='average') or where the quadric of
    the cell's faces puts it, moving from the average only along well-conditioned directions and by at most a voxel
    ('quadric'); faces follow, collapsed and duplicate faces and the clusters no face uses are dropped.  colors (uint8 [V,3])
    are averaged per cell, rounding half up.  Returns (verts f32 [V',3], faces int32 [F',3], colors uint8 [V',3] or None) as
    device tensors: vertices in ascending cell key, faces in input order, smallest index first; the same bits every run.
    A voxel larger than the model gives an empty mesh.  The rules are include/adfp.h's ("mesh simplification"), this package's
    own statement of vertex clustering: open3d is not installed here and its function was never run against this one."""
    v, f = _mesh_tensors(verts, faces, 'simplify_vertex_clustering')
    if v is None:
        raise ValueError('simplify_vertex_clustering: verts is None')
    vs = float(voxel_size)
    if not (vs > 0.0 and np.isfinite(vs)):
        raise ValueError(f'simplify_vertex_clustering: voxel_size must be positive and finite, got {voxel_size!r}')
    if contraction not in SIMPLIFY_CONTRACTIONS:
        raise ValueError(f'simplify_vertex_clustering: contraction must be one of {sorted(SIMPLIFY_CONTRACTIONS)}, got {contraction!r}')
    c = _vertex_colors(colors, v, 'simplify_vertex_clustering')
    _check_indices(f, int(v.shape[0]), 'simplify_vertex_clustering')
    return _simplify_vertex_clustering(v, f, vs, contraction, c)


def color_bytes(rgb):
    """(clip(rgb[:, :3], 0, 1) * 255) truncated to uint8 [n,3] on the device; rgb: float32 rows of at least three channels."""
    require_cuda(rgb, 'color_bytes rgb')
    x = rgb.detach().to(torch.float32)
    x = x.reshape(-1, x.shape[-1]).contiguous()
    if x.shape[1] < 3:
        raise ValueError(f'color_bytes: rows of {x.shape[1]} channels')
    out = torch.empty((x.shape[0], 3), dtype=torch.uint8, device=x.device)
    with _lib.on(x.device) as L:
        L.adfp_mesh_color_bytes(x, int(x.shape[0]), int(x.shape[1]), out)
    return out


def vertex_normals(verts, faces, device=None):
    """Area-weighted vertex normals on the device (adfp_vertex_normals; open3d's compute_vertex_normals as we read it): f64 [V,3],
    per vertex the sum of (v1 - v0) x (v2 - v0) over its faces in ascending face index, normalised; zeros for a vertex that no
    face uses or whose sum has no direction.  A face with an index outside [0, V) is skipped.  The same bits every run.  verts,
    faces: tensors or arrays (f64 and int32 on the device are used as they are).  write_ply(path, verts, faces, colors,
    normals=vertex_normals(verts, faces)) saves the mesh with its normals."""
    v = verts if torch.is_tensor(verts) else torch.from_numpy(np.asarray(verts, dtype=np.float64))
    dev = torch.device(device) if device is not None else (v.device if v.is_cuda or not torch.is_tensor(faces) else faces.device)
    v = v.detach().reshape(-1, 3).to(dev, torch.float64).contiguous()
    f = as_faces(faces, dev, np.int64)
    require_cuda(v, 'vertex_normals verts')
    V, F = int(v.shape[0]), int(f.shape[0])
    out = torch.empty((V, 3), dtype=torch.float64, device=dev)
    if V == 0:
        return out
    nbytes = lib().adfp_vertex_normals_workspace_bytes(F)
    if F and nbytes == 0:
        raise RuntimeError(f'vertex_normals: {F} faces are more than the int32 sort carries')
    with _lib.on(dev) as L:
        L.adfp_vertex_normals(v, V, f, F, _lib.workspace(nbytes, dev) if F else None, nbytes, out)
    return out


# ---- mesh colours from the keyframes (csrc/adfp_meshcolor.h; the rule: include/adfp.h, "mesh colours from the keyframes") ------
BLENDS = _lib.BLEND


def w2c_rows_own_dtype(c2w, dev):
    """numpy poses [K,4,4] -> f32 device [K,12]: the top three rows of np.linalg.inv(c2w) in the array's own dtype, then f32, as
    Mesher._project inverts them (recon.w2c_rows inverts a float32 copy, raycast.proj_rows negates two columns first)."""
    return torch.from_numpy(np.ascontiguousarray(np.linalg.inv(c2w)[:, :3, :])).to(dev).float().reshape(-1, 12).contiguous()


def _project_colors(v, n, depth, color, c2w, fx, fy, cx, cy, depth_tol, border, blend):
    """project_colors on prepared tensors: v f32 [V,3], n f32 [V,3] or None, depth f32 [K,H,W], color f32 [K,H,W,3], all contiguous
    on one device; c2w [K,4,4] on any device (read back once and inverted on the host, as Mesher.seen_mask does)."""
    dev = v.device
    V, K, H, W = int(v.shape[0]), int(depth.shape[0]), int(depth.shape[1]), int(depth.shape[2])
    rgb = torch.zeros((V, 3), dtype=torch.float32, device=dev)
    wsum = torch.zeros(V, dtype=torch.float32, device=dev)
    count = torch.zeros(V, dtype=torch.int32, device=dev)
    best = torch.full((V,), -1, dtype=torch.int32, device=dev)
    w2c = center = None
    if K:
        m = c2w.detach().cpu().numpy()
        w2c = w2c_rows_own_dtype(m, dev)
        center = torch.from_numpy(np.ascontiguousarray(m[:, :3, 3])).to(dev).float().contiguous()
    with _lib.on(dev) as L:
        L.adfp_mesh_project_colors(v, n, V, w2c, center, depth, color, K, float(fx), float(fy), float(cx), float(cy), W, H,
                                   float(depth_tol), int(border), BLENDS[blend], rgb, wsum, count, best)
    return rgb, wsum, count, best


def project_colors(verts, normals, depth, color, c2w, fx, fy, cx, cy, depth_tol, border=0, blend='weighted'):
    """Vertex colours from the keyframes' images on the device (adfp_mesh_project_colors): every vertex is projected into every
    keyframe, a view counts only where the four depth pixels around the projection all lie within depth_tol of the vertex's
    depth (no hole, no depth edge in the footprint), and the bilinear colours of the views that count are blended: 'weighted'
    by cos(view, normal) / depth^2, or 'best' = the view of largest weight alone.  verts [V,3] (the keyframes' world); normals
    [V,3] (mesh.vertex_normals' output: its f32 rounding is used) or None (every weight's cosine is 1); depth [K,H,W], color
    [K,H,W,3], c2w [K,4,4] (est_c2w, inverted on the host as Mesher.seen_mask inverts them); border: pixels kept clear of the
    image's edge.  Returns device tensors (rgb f32 [V,3], wsum f32 [V], count int32 [V], best int32 [V]): zeros and best = -1
    where no keyframe sees the vertex.  The same bits every run.  The rule, operation for operation: include/adfp.h."""
    if blend not in BLENDS:
        raise ValueError(f'project_colors: blend must be one of {sorted(BLENDS)}, got {blend!r}')
    tol = float(depth_tol)
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError(f'project_colors: depth_tol must be finite and not negative, got {depth_tol!r}')
    require_cuda(verts, 'project_colors verts')
    v = verts.detach().reshape(-1, 3).to(torch.float32).contiguous()
    dev = v.device
    n = None
    if normals is not None:
        n = (normals if torch.is_tensor(normals) else torch.from_numpy(np.asarray(normals)))
        n = n.detach().reshape(-1, 3).to(dev, torch.float32).contiguous()
        if n.shape[0] != v.shape[0]:
            raise ValueError(f'project_colors: {n.shape[0]} normals for {v.shape[0]} vertices')
    d = depth.detach().to(dev, torch.float32)
    if d.dim() != 3:
        raise ValueError(f'project_colors: depth must be [K,H,W], got {tuple(d.shape)}')
    K, H, W = (int(s) for s in d.shape)
    col = color.detach().to(dev, torch.float32)
    if tuple(col.shape) != (K, H, W, 3):
        raise ValueError(f'project_colors: color must be [{K},{H},{W},3], got {tuple(col.shape)}')
    m = c2w if torch.is_tensor(c2w) else torch.from_numpy(np.asarray(c2w))
    if tuple(m.shape) != (K, 4, 4):
        raise ValueError(f'project_colors: c2w must be [{K},4,4], got {tuple(m.shape)}')
    if int(border) < 0 or 2 * int(border) > min(W, H) - 2:
        raise ValueError(f'project_colors: border {border} leaves no pixel of a {W} x {H} image')
    return _project_colors(v, n, d.contiguous(), col.contiguous(), m, fx, fy, cx, cy, tol, int(border), blend)


# ---- mesh bound: the convex hull of the keyframes' camera centres and back-projected valid depth pixels, as a quickhull in
# rounds (csrc/adfp_bound.h; contracts and the fixed formulae: include/adfp.h, "mesh bound").  A point is named by its id
# k (H W + 1) + j: j = 0 the camera centre of keyframe k, j = 1 + row W + col a pixel.  The device does the point work (support
# pass, classification, compaction, per-facet farthest); Qhull keeps the facets of the few hundred vertices on the host.  The
# *_host functions are the numpy statement of the same formulae and rounds, bit for bit, and run without a GPU.
BOUND_DIRECTIONS = 64          # D of the support pass (tools/bound_bench.py measures the choice)
BOUND_MAX_ROUNDS = 64
BOUND_EPS_REL = 1e-12          # eps = this x the largest AABB extent: two decades above the f64 rounding of a plane evaluation
_BOUND_CAP_ALL = 1 << 25       # candidate lists up to this length get a survivor buffer of their own length; longer ones a quarter


def bound_directions(D=BOUND_DIRECTIONS):
    """The support pass's fixed directions [D,3] f64: +x, -x, +y, -y, +z, -z (so the AABB falls out), then D - 6 points of the
    Fibonacci lattice on the unit sphere (z_i = 1 - (2 i + 1) / n, azimuth i pi (3 - sqrt 5))."""
    if not 6 <= D <= _lib.BOUND_MAX_DIRECTIONS:
        raise ValueError(f'bound_directions: D must lie in [6, {_lib.BOUND_MAX_DIRECTIONS}], got {D}')
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    n = D - 6
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / max(n, 1)
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.ascontiguousarray(np.concatenate([axes, np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)]))


def _bound_scene_arrays(depth, c2w):
    d = as_numpy(depth)
    m = as_numpy(c2w)
    if d.ndim != 3 or m.shape != (d.shape[0], 4, 4):
        raise ValueError(f'mesh bound: depth must be [K,H,W] and c2w [K,4,4], got {d.shape} and {m.shape}')
    return np.ascontiguousarray(d, np.float32), np.ascontiguousarray(m, np.float32)


def depth_points_host(depth, c2w, fx, fy, cx, cy):
    """(ids int64 [n] ascending, points f64 [n,3]) of every point of the scene -- depth [K,H,W] f32, c2w [K,4,4] f32 -- by the fixed
    formulae of include/adfp.h, elementwise (no matrix product), so that adfp_bound_points gives the same bits."""
    depth, c2w = _bound_scene_arrays(depth, c2w)
    K, H, W = depth.shape
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    M = c2w.astype(np.float64)
    row, col = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    ids, pts = [], []
    for k in range(K):
        R0, R1, R2, t = M[k, :3, 0], -M[k, :3, 1], -M[k, :3, 2], M[k, :3, 3]
        d = depth[k].astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            ok = (d > 0) & (d < 1000)
            d = d[ok]
            x = ((col[ok] - cx) / fx) * d
            y = ((row[ok] - cy) / fy) * d
            p = np.stack([((R0[c] * x + R1[c] * y) + R2[c] * d) + t[c] for c in range(3)], 1)
        base = k * (H * W + 1)
        ids += [np.array([base], np.int64), base + 1 + np.flatnonzero(ok.reshape(-1)).astype(np.int64)]
        pts += [t[None].copy(), p]
    if K == 0:
        return np.zeros(0, np.int64), np.zeros((0, 3))
    return np.concatenate(ids), np.concatenate(pts)


class _HostBound(object):
    """The numpy statement of adfp_bound_support / _classify / _points over the stored points of depth_points_host."""

    def __init__(self, depth, c2w, fx, fy, cx, cy):
        self.ids, self.pts = depth_points_host(depth, c2w, fx, fy, cx, cy)

    def support(self, dirs):
        fin = np.isfinite(self.pts).all(1)
        p = self.pts[fin]
        ids = self.ids[fin]
        best = np.full(len(dirs), -1, np.int64)
        if len(p):
            for i, u in enumerate(dirs):
                dot = (u[0] * p[:, 0] + u[1] * p[:, 1]) + u[2] * p[:, 2]
                j = int(np.argmax(dot))                          # the first among equals: the lowest id
                if dot[j] > -np.inf:
                    best[i] = ids[j]
        aabb = np.concatenate([p.min(0), p.max(0)]) if len(p) else np.array([np.inf] * 3 + [-np.inf] * 3)
        return best, aabb, int(fin.sum()), int((~fin).sum())

    def points(self, ids):
        ids = np.asarray(ids, np.int64)
        out = np.full((len(ids), 3), np.nan)
        if len(self.ids) and len(ids):
            j = np.minimum(np.searchsorted(self.ids, ids), len(self.ids) - 1)
            hit = self.ids[j] == ids
            out[hit] = self.pts[j[hit]]
        return out

    def classify(self, cand, planes, eps):
        ids = self.ids if cand is None else cand
        p = self.points(ids) if cand is not None else self.pts
        m = np.full(len(ids), -np.inf)
        fac = np.full(len(ids), -1, np.int64)
        with np.errstate(invalid='ignore'):
            for f, (nx, ny, nz, d) in enumerate(planes):
                s = ((nx * p[:, 0] + ny * p[:, 1]) + nz * p[:, 2]) + d
                w = s > m
                m[w] = s[w]
                fac[w] = f
            keep = m > eps
        ids, m, fac = ids[keep], m[keep], fac[keep]
        far_id = np.full(len(planes), -1, np.int64)
        far_dist = np.zeros(len(planes))
        if len(ids):
            order = np.lexsort((ids, -m, fac))                    # per facet: the largest m first, the lowest id among equals
            first = order[np.concatenate([[True], fac[order][1:] != fac[order][:-1]])]
            far_id[fac[first]] = ids[first]
            far_dist[fac[first]] = m[first]
        return ids, len(ids), far_id, far_dist


class _DeviceBound(object):
    """The same three operations through libadfp.so over device tensors: depth [K,H,W] f32, c2w [K,4,4] f32."""

    def __init__(self, depth, c2w, fx, fy, cx, cy):
        require_cuda(depth, 'depth_hull depth')
        self.dev = depth.device
        self.depth = depth.detach().to(torch.float32).contiguous()
        if self.depth.dim() != 3 or tuple(c2w.shape) != (self.depth.shape[0], 4, 4):
            raise ValueError(f'depth_hull: depth must be [K,H,W] and c2w [K,4,4], got {tuple(depth.shape)} and {tuple(c2w.shape)}')
        self.poses = c2w.detach().to(self.dev, torch.float32).contiguous()
        K, H, W = (int(s) for s in self.depth.shape)
        self.K, self.H, self.W = K, H, W
        self.n_ids = K * (H * W + 1)
        self.scene = (self.depth, self.poses, K, H, W, float(fx), float(fy), float(cx), float(cy))

    def support(self, dirs):
        D = int(dirs.shape[0])
        d = torch.from_numpy(np.ascontiguousarray(dirs, np.float64)).to(self.dev)
        out = torch.empty(D + 8, dtype=torch.int64, device=self.dev)          # best ids, aabb (f64 bits), counts
        with _lib.on(self.dev) as L:
            nbytes = lib().adfp_bound_support_workspace_bytes(self.K, self.H, self.W, D)
            L.adfp_bound_support(*self.scene, d, D, _lib.workspace(nbytes, self.dev), nbytes, out, out[D:], out[D + 6:])
            h = out.cpu().numpy()
        return h[:D].copy(), h[D:D + 6].view(np.float64).copy(), int(h[D + 6]), int(h[D + 7])

    def points(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        out = torch.empty((len(ids), 3), dtype=torch.float64, device=self.dev)
        if len(ids):
            t = torch.from_numpy(ids).to(self.dev)
            with _lib.on(self.dev) as L:
                L.adfp_bound_points(*self.scene, t, len(ids), out)
        return out.cpu().numpy()

    def classify(self, cand, planes, eps):
        F = int(planes.shape[0])
        ids_in, n_in = (None, self.n_ids) if cand is None else cand
        pl = torch.from_numpy(np.ascontiguousarray(planes, np.float64)).to(self.dev)
        res = torch.empty(2 * F + 1, dtype=torch.int64, device=self.dev)      # far ids, far distances (f64 bits), the count
        cap = n_in if n_in <= _BOUND_CAP_ALL else max(_BOUND_CAP_ALL, n_in // 4)
        with _lib.on(self.dev) as L:
            nbytes = lib().adfp_bound_classify_workspace_bytes(n_in)
            ws = _lib.workspace(nbytes, self.dev)
            while True:
                out = torch.empty(max(cap, 1), dtype=torch.int64, device=self.dev)
                L.adfp_bound_classify(*self.scene, ids_in, n_in, pl, F, float(eps), ws, nbytes, out, cap, res[2 * F:], res, res[F:])
                h = res.cpu().numpy()                                         # the round's one synchronisation
                count = int(h[2 * F])
                if count <= cap:
                    break
                cap = count                                                   # more survivors than the buffer held: once more, in full
        return (out, count), count, h[:F].copy(), h[F:2 * F].view(np.float64).copy()


def _hull_rounds(b, directions, max_rounds):
    from scipy.spatial import ConvexHull
    dirs = bound_directions() if directions is None else np.ascontiguousarray(directions, np.float64).reshape(-1, 3)
    best, aabb, _, n_bad = b.support(dirs)
    if n_bad:
        raise ValueError(f'depth_hull: {n_bad} points are not finite (a pose or an intrinsic holds a NaN or an inf)')
    V = np.unique(best[best >= 0])
    eps = BOUND_EPS_REL * float((aabb[3:] - aabb[:3]).max())
    cand, stats = None, []
    for _ in range(max_rounds):
        pts = b.points(V)
        t0 = time.perf_counter()
        hull = ConvexHull(pts)                                    # Qhull's own errors for a degenerate set, as on the host path
        qhull_s = time.perf_counter() - t0
        V = V[np.sort(hull.vertices)]
        planes = np.ascontiguousarray(hull.equations)
        cand, count, far_id, _ = b.classify(cand, planes, eps)
        stats.append((V, planes, count, far_id, qhull_s))
        if count == 0:
            return V, b.points(V), stats
        V = np.union1d(V, far_id[far_id >= 0])
    raise RuntimeError(f'depth_hull: points remain outside the hull after {max_rounds} rounds; no partial hull is returned')


def _no_keyframes(depth):
    if int(depth.shape[0]) == 0:
        raise ValueError('depth_hull: need at least one keyframe')


def depth_hull_host(depth, c2w, fx, fy, cx, cy, directions=None, return_stats=False, max_rounds=BOUND_MAX_ROUNDS):
    """depth_hull in numpy, round for round: the same support points, survivors, farthest ids and vertex ids, bit for bit."""
    _no_keyframes(depth)
    ids, pts, stats = _hull_rounds(_HostBound(depth, c2w, fx, fy, cx, cy), directions, max_rounds)
    return (ids, pts, stats) if return_stats else (ids, pts)


def depth_hull(depth, c2w, fx, fy, cx, cy, directions=None, return_stats=False, max_rounds=BOUND_MAX_ROUNDS):
    """The vertices of the convex hull of the scene's points -- device tensors depth [K,H,W] f32, c2w [K,4,4] f32 (est_c2w as
    KeyframeStore.poses() holds it) -- as (ids int64 ascending, points f64 [n,3]) numpy arrays.  Rounds: the support points of
    `directions` (default bound_directions()) start the vertex set; each round Qhull hulls the set on the host, the device drops
    every candidate within eps = 1e-12 x the largest AABB extent of the hull's planes, compacts the rest in id order and reports
    each facet's farthest point, which joins the set; one synchronisation per round, until nothing remains outside.  More than
    max_rounds rounds raise RuntimeError; non-finite points ValueError.  return_stats: also the per-round list of (vertex ids,
    planes, survivors, farthest id per facet, seconds in Qhull)."""
    _no_keyframes(depth)
    ids, pts, stats = _hull_rounds(_DeviceBound(depth, c2w, fx, fy, cx, cy), directions, max_rounds)
    return (ids, pts, stats) if return_stats else (ids, pts)


def write_ply(path, verts, faces, colors=None, normals=None, ascii=False):
    """Write a triangle mesh as PLY: binary little-endian (default) or ascii.  Vertex properties x y z [nx ny nz] [red green
    blue] (float, float, uchar) and 'property list uchar int vertex_index' faces: the property list of src/fusion.py:meshwrite."""
    v = as_numpy(verts).astype(np.float32).reshape(-1, 3)
    f = as_numpy(faces).astype(np.int32).reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    n = as_numpy(normals)
    c = as_numpy(colors)
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


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


class PlyMesh(object):
    """What read_ply returns: verts float64 [V,3]; faces int64 [F,3] (polygons fan-triangulated (0, i, i+1), as trimesh loads
    them); normals float64 [V,3] or None; colors uint8 [V,3|4] or None; vertex: every vertex property as a structured array."""

    def __init__(self, vertex, faces):
        self.vertex = vertex
        names = vertex.dtype.names
        self.verts = np.stack([vertex[k].astype(np.float64) for k in 'xyz'], 1) if len(vertex) else np.zeros((0, 3))
        self.normals = np.stack([vertex[k].astype(np.float64) for k in ('nx', 'ny', 'nz')], 1) \
            if all(k in names for k in ('nx', 'ny', 'nz')) else None
        cols = [k for k in ('red', 'green', 'blue', 'alpha') if k in names]
        self.colors = np.stack([vertex[k] for k in cols], 1).astype(np.uint8) if cols[:3] == ['red', 'green', 'blue'] else None
        self.faces = faces


def _ply_header(data):
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError('not a PLY file')
    nl = data.index(b'\n', end)
    lines = data[:nl].decode('ascii').replace('\r', '').split('\n')
    fmt, elements = None, []
    for line in lines[1:]:
        w = line.split()
        if not w or w[0] in ('comment', 'obj_info', 'end_header'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append((w[1], int(w[2]), []))
        elif w[0] == 'property':
            if w[1] == 'list':
                elements[-1][2].append((w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]))
            else:
                elements[-1][2].append((w[2], _PLY_TYPES[w[1]], None))
    if fmt not in ('ascii', 'binary_little_endian', 'binary_big_endian'):
        raise ValueError(f'PLY format {fmt!r} is not supported')
    return fmt, elements, nl + 1


def _ply_binary_element(body, off, count, props, endian):
    """-> (dict name -> array (scalars) or list of arrays (lists), new offset)."""
    if all(lt is None for _, _, lt in props):
        dt = np.dtype([(n, endian + t) for n, t, _ in props])
        rec = np.frombuffer(body, dtype=dt, count=count, offset=off)
        return {n: rec[n] for n, _, _ in props}, off + dt.itemsize * count
    if count == 0:
        return {n: (np.zeros(0, t) if lt is None else []) for n, t, lt in props}, off
    # fast path: every list of the element as long as the first row's
    fields, pos = [], off
    for n, t, lt in props:
        if lt is None:
            fields.append((n, endian + t))
            pos += np.dtype(t).itemsize
        else:
            k = int(np.frombuffer(body, dtype=endian + t, count=1, offset=pos)[0])
            fields.append((n + '#n', endian + t))
            if k:
                fields.append((n, endian + lt, (k,)))
            pos += np.dtype(t).itemsize + k * np.dtype(lt).itemsize
    dt = np.dtype(fields)
    if off + dt.itemsize * count <= len(body):
        rec = np.frombuffer(body, dtype=dt, count=count, offset=off)
        ok = all((rec[n + '#n'] == (rec.dtype[n].shape[0] if n in rec.dtype.names else 0)).all() for n, _, lt in props if lt is not None)
        if ok:
            out = {}
            for n, t, lt in props:
                if lt is None:
                    out[n] = rec[n]
                else:
                    out[n] = rec[n].reshape(count, -1) if n in rec.dtype.names else np.zeros((count, 0), lt)
            return out, off + dt.itemsize * count
    # mixed list lengths: one walk over the rows for the offsets (only the count fields are read), then every property is
    # gathered with numpy; lists come back ragged, as (flat values, counts)
    nprop = len(props)
    isz = [np.dtype(t).itemsize for _, t, _ in props]
    lsz = [np.dtype(lt).itemsize if lt is not None else 0 for _, _, lt in props]
    cfmt = [endian + np.dtype(t).char if lt is not None else None for _, t, lt in props]
    one_byte = [lt is not None and np.dtype(t).itemsize == 1 and np.dtype(t).kind == 'u' for _, t, lt in props]
    pos_l, cnt_l = [], []
    row = off
    for _ in range(count):
        for j in range(nprop):
            pos_l.append(row)
            if cfmt[j] is None:
                cnt_l.append(0)
                row += isz[j]
            else:
                k = body[row] if one_byte[j] else int(struct.unpack_from(cfmt[j], body, row)[0])
                cnt_l.append(k)
                row += isz[j] + k * lsz[j]
    pos = np.array(pos_l, np.int64).reshape(count, nprop)
    cnt = np.array(cnt_l, np.int64).reshape(count, nprop)
    buf = np.frombuffer(body, dtype=np.uint8)
    out = {}
    for j, (n, t, lt) in enumerate(props):
        if lt is None:
            out[n] = buf[pos[:, j, None] + np.arange(isz[j])].copy().view(endian + t).reshape(count)
        else:
            c = cnt[:, j]
            first = np.repeat(pos[:, j] + isz[j], c)
            k = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
            flat = buf[(first + k * lsz[j])[:, None] + np.arange(lsz[j])].copy().view(endian + lt).reshape(-1)
            out[n] = (flat, c)
    return out, row


def _ply_ascii_element(lines, start, count, props):
    out = {n: [] for n, _, _ in props}
    for r in range(count):
        w = lines[start + r].split()
        j = 0
        for n, t, lt in props:
            if lt is None:
                out[n].append(w[j])
                j += 1
            else:
                k = int(w[j])
                out[n].append(np.array([float(x) for x in w[j + 1:j + 1 + k]]).astype(lt))
                j += 1 + k
    for n, t, lt in props:
        if lt is None:
            kind = np.dtype(t).kind
            out[n] = np.array([float(x) if kind == 'f' else int(x) for x in out[n]], dtype=t)
    return out, start + count


def _fan(rows):
    """Polygons (a [F,k] array, a list of index arrays or ragged (flat, counts)) -> triangles (0, i, i+1), in polygon order."""
    if isinstance(rows, np.ndarray):
        k = rows.shape[1]
        if k < 3:
            return np.zeros((0, 3), np.int64)
        tri = np.stack([np.stack([rows[:, 0], rows[:, i], rows[:, i + 1]], 1) for i in range(1, k - 1)], 1)
        return tri.reshape(-1, 3).astype(np.int64)
    if isinstance(rows, tuple):
        flat, c = rows
    else:
        c = np.array([len(r) for r in rows], np.int64)
        flat = np.concatenate([np.asarray(r, np.int64) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    flat = np.asarray(flat).astype(np.int64)
    start = np.cumsum(c) - c
    ntri = np.maximum(c - 2, 0)
    poly = np.repeat(np.arange(len(c)), ntri)
    t = np.arange(int(ntri.sum())) - np.repeat(np.cumsum(ntri) - ntri, ntri) + 1
    s0 = start[poly]
    return np.stack([flat[s0], flat[s0 + t], flat[s0 + t + 1]], 1)


def read_ply(path):
    """Read a PLY mesh: ascii, binary_little_endian or binary_big_endian; any vertex properties (x y z required; nx ny nz and
    red green blue [alpha] carried through); faces as a list property named vertex_indices or vertex_index, of any count and
    index types.  Returns a PlyMesh.  Reads what write_ply writes and the Replica ground-truth meshes."""
    with open(path, 'rb') as fh:
        data = fh.read()
    fmt, elements, off = _ply_header(data)
    endian = {'binary_little_endian': '<', 'binary_big_endian': '>'}.get(fmt)
    lines = data[off:].decode('ascii').replace('\r', '').split('\n') if fmt == 'ascii' else None
    pos = 0
    vertex, faces = None, np.zeros((0, 3), np.int64)
    for name, count, props in elements:
        if fmt == 'ascii':
            vals, pos = _ply_ascii_element(lines, pos, count, props)
        else:
            vals, off = _ply_binary_element(data, off, count, props, endian)
        if name == 'vertex':
            missing = [k for k in 'xyz' if k not in vals]
            if missing:
                raise ValueError(f'{path}: vertex element has no {missing}')
            scal = [(n, t) for n, t, lt in props if lt is None]
            vertex = np.empty(count, dtype=[(n, t) for n, t in scal])
            for n, _ in scal:
                vertex[n] = vals[n]
        elif name == 'face':
            key = 'vertex_indices' if 'vertex_indices' in vals else ('vertex_index' if 'vertex_index' in vals else None)
            if key is None:
                raise ValueError(f'{path}: face element has no vertex_indices / vertex_index list')
            faces = _fan(vals[key])
    if vertex is None:
        raise ValueError(f'{path}: no vertex element')
    return PlyMesh(vertex, faces)


def read_obj(path):
    """Read a Wavefront OBJ mesh: 'v x y z [r g b ...]' (extra columns ignored) and 'f' with a, a/b, a//c or a/b/c corners, 1-based
    or negative (relative to the vertices read so far) indices, polygons fan-triangulated (0, i, i+1) as read_ply does.  Every
    other statement is skipped.  Returns a PlyMesh (vertex x y z as float64)."""
    verts, polys = [], []
    with open(path, 'r') as fh:
        for line in fh:
            w = line.split()
            if not w:
                continue
            if w[0] == 'v':
                if len(w) < 4:
                    raise ValueError(f'{path}: vertex line {line.strip()!r} has fewer than three coordinates')
                verts.append((float(w[1]), float(w[2]), float(w[3])))
            elif w[0] == 'f':
                idx = []
                for c in w[1:]:
                    k = int(c.split('/')[0])
                    idx.append(k - 1 if k > 0 else len(verts) + k)
                polys.append(np.array(idx, np.int64))
    vertex = np.empty(len(verts), dtype=[('x', '<f8'), ('y', '<f8'), ('z', '<f8')])
    if verts:
        v = np.array(verts, np.float64)
        vertex['x'], vertex['y'], vertex['z'] = v[:, 0], v[:, 1], v[:, 2]
    return PlyMesh(vertex, _fan(polys) if polys else np.zeros((0, 3), np.int64))
