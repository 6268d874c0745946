"""Views of a triangle mesh on the MI355X: the shaded picture, the vertex-colour image, the normal map and the depth of a
reconstruction from any batch of poses.  The reference shows its meshes in open3d's viewer; here the renderer is the package's own
exact f64 ray caster (raycast.MeshBVH.render_hits: per pixel the face hit and where on it) followed by one shading pass
(adfp_shade_hits), so a view is a function of the mesh and the pose alone: the same bytes every run, on every leaf size.

    python -m attentive_dfprior_amd.render_mesh --input_mesh M.ply (--traj traj.txt | --poses FILE)
           (CONFIG | --H .. --W .. --fx .. --fy .. --cx .. --cy ..) [--mode shaded|color|normal] [--flat] [--cull none|back|front]
           [--every N] [--depth] [--out DIR]

--traj is a Replica traj.txt read as cull_mesh reads it, --poses a file read as render_views reads it; both hold one row-major
camera-to-world 4x4 per line with OpenCV axes.  The camera comes from CONFIG's `cam` block (after crop_size / crop_edge, as
get_tsdf reads it) or from the six options.  Per view k the output directory (default ./mesh_views) receives {mode}_{k:05d}.png
(8 bit RGB, written with PIL) and, with --depth, depth_{k:05d}.npy (float32 [H,W], metres, 0 where the ray meets nothing).

modes: 'shaded' = the base colour times ambient + (1 - ambient) cos(angle between the normal and the ray), a light at the camera;
'color' = the base colour alone; 'normal' = the camera-space normal as a normal map ((n . (1, -1, -1) + 1) / 2).  The base colour
is the interpolated vertex colour, or a uniform albedo for a mesh without colours.  Normals are the area-weighted vertex normals
(mesh.vertex_normals) interpolated over the face, or the face's own with --flat, turned toward the camera.  The exact arithmetic
is include/adfp.h's "mesh views".
"""
import argparse
import os

import numpy as np
import torch

from . import _lib, mesh
from ._lib import lib
from .raycast import MeshBVH, near_rows
from .recon import device_of, as_points, as_faces, pose_rows

CHUNK = 100                                         # views per launch and download: recon_eval.metric_2d's


def near_of(verts, fraction=0.01):
    """calc_2d_metric's near plane for a vertex tensor [V,3]: a hundredth of the longest side of the mesh's box."""
    if verts.shape[0] == 0:
        return 0.0
    return fraction * float((verts.amax(0) - verts.amin(0)).max())


class MeshViews(object):
    """A mesh made ready to be looked at: verts [V,3], faces [F,3], colors uint8 [V,3] or None (numpy or tensors).  Builds the
    triangle BVH and, with smooth=True, the vertex normals once; render() may then be called for any poses."""

    def __init__(self, verts, faces, colors=None, device=None, smooth=True, leaf=_lib.TRI_LEAF_DEFAULT):
        dev = torch.device(device) if device is not None else device_of(verts, faces)
        self.device = dev
        self.verts = as_points(verts, dev, 'vertices')
        self.faces = as_faces(faces, dev, np.int64)
        self.colors = None
        if colors is not None:
            c = colors if torch.is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(colors))
            if c.dim() != 2 or c.shape[0] != self.verts.shape[0] or c.shape[1] < 3:
                raise ValueError(f'MeshViews: colours {tuple(c.shape)} for {self.verts.shape[0]} vertices')
            if c.dtype != torch.uint8:
                raise ValueError(f'MeshViews: colours must be uint8, got {c.dtype}')
            self.colors = c[:, :3].to(dev).contiguous()
        self.bvh = MeshBVH(self.verts, self.faces, dev, leaf)
        self.normals = mesh.vertex_normals(self.verts, self.faces, dev) if smooth else None
        self.near = near_of(self.verts)

    def shade(self, face, bary, c2w, fx, fy, cx, cy, mode='shaded', ambient=0.3, albedo=(0.8, 0.8, 0.8),
              background=(255, 255, 255), want=('normal', 'rgb')):
        """adfp_shade_hits over face int32 [P,H,W] and bary f32 [P,H,W,2] (render_hits' or a caller's): {'normal': f32 [P,H,W,3],
        'rgb': uint8 [P,H,W,3]}, the keys of `want`."""
        if mode not in _lib.SHADE_MODE:
            raise ValueError(f'MeshViews: mode must be one of {tuple(_lib.SHADE_MODE)}, got {mode!r}')
        dev = self.device
        m = pose_rows(c2w, dev)
        face = face.to(dev, torch.int32).contiguous()
        bary = bary.to(dev, torch.float32).contiguous()
        if face.dim() == 2:
            face, bary = face[None], bary[None]
        P, H, W = (int(s) for s in face.shape)
        if int(m.shape[0]) != P or tuple(bary.shape) != (P, H, W, 2):
            raise ValueError(f'MeshViews: face {tuple(face.shape)}, bary {tuple(bary.shape)} and {int(m.shape[0])} poses do not agree')
        out = {}
        if 'normal' in want:
            out['normal'] = torch.empty((P, H, W, 3), dtype=torch.float32, device=dev)
        if 'rgb' in want:
            out['rgb'] = torch.empty((P, H, W, 3), dtype=torch.uint8, device=dev)
        if P == 0 or not out:
            return out
        alb = (_lib.C.c_float * 3)(*[float(a) for a in albedo])
        bg = (_lib.C.c_ubyte * 3)(*[int(b) for b in background])
        with _lib.on(dev) as L:
            L.adfp_shade_hits(face, bary, P, H, W, self.verts, int(self.verts.shape[0]), self.faces, int(self.faces.shape[0]), m, float(fx),
                              float(fy), float(cx), float(cy), self.normals, self.colors, _lib.C.byref(alb), float(ambient),
                              _lib.C.byref(bg), _lib.SHADE_MODE[mode], out.get('normal'), out.get('rgb'))
        return out

    def render(self, c2w, H, W, fx, fy, cx, cy, near=None, far=20.0, mode='shaded', cull='none', ambient=0.3,
               albedo=(0.8, 0.8, 0.8), background=(255, 255, 255), chunk=CHUNK):
        """Device tensors of P views: {'depth': f32 [P,H,W] (render_depth's), 'face': int32 [P,H,W] (-1: nothing hit),
        'normal': f32 [P,H,W,3] (camera space, toward the camera), 'rgb': uint8 [P,H,W,3]}.  c2w: [P,4,4] or [4,4], OpenCV axes;
        near=None is a hundredth of the mesh's longest side (calc_2d_metric's rule).  The views go through the kernels `chunk` at
        a time, so the face and barycentric images of only one chunk are alive at once."""
        m = pose_rows(c2w, self.device)
        P = int(m.shape[0])
        near = self.near if near is None else near
        nr = near_rows(near, P, self.device, 'render_hits')          # refused here as render_hits would refuse it
        parts = {k: [] for k in ('depth', 'face', 'normal', 'rgb')}
        for p0 in range(0, max(P, 1), chunk):
            mc = m[p0:p0 + chunk].reshape(-1, 3, 4)
            h = self.bvh.render_hits(mc, H, W, fx, fy, cx, cy, nr[p0:p0 + chunk], far, cull)
            s = self.shade(h['face'], h['bary'], mc, fx, fy, cx, cy, mode, ambient, albedo, background)
            for k, t in (('depth', h['depth']), ('face', h['face']), ('normal', s['normal']), ('rgb', s['rgb'])):
                parts[k].append(t)
        return {k: v[0] if len(v) == 1 else torch.cat(v) for k, v in parts.items()}


def draw_segments(rgb, depth, c2w, fx, fy, cx, cy, segments, colors, ranges=None, width=2.0, near_clip=1e-3, bias=(0.0, 0.0),
                  hidden_alpha=0.0, want_seg=False, chunk=CHUNK):
    """3D line segments painted over views IN PLACE (adfp_draw_segments; the arithmetic is include/adfp.h's): rgb uint8 [P,H,W,3]
    and depth f32 [P,H,W] (MeshViews.render's, device tensors; depth None = nothing occludes), c2w [P,4,4] OpenCV axes; segments
    [N,2,3] world endpoints and colors uint8 [N,3], one list for all views; ranges int64 [P,R,2] (R <= 8) or [R,2] for all views:
    view p draws the segments k with b <= k < e for one of its ranges [b, e); None draws all.  width: the line's width in pixels
    (round caps); a segment's pixel is drawn where the line lies no deeper than depth (1 + bias[0]) + bias[1] or nothing was hit, and
    is otherwise blended with weight hidden_alpha (0: hidden lines vanish).  The views go through the kernels `chunk` at a time.
    Returns None, or with want_seg the int32 [P,H,W] image of segment indices (-1: none)."""
    _lib.require_cuda(rgb, 'rgb')
    dev = rgb.device
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or not rgb.is_contiguous():
        raise ValueError(f'draw_segments: rgb must be a contiguous uint8 [P,H,W,3] tensor, got {rgb.dtype} {tuple(rgb.shape)}')
    P, H, W = (int(s) for s in rgb.shape[:3])
    m = pose_rows(c2w, dev)
    if int(m.shape[0]) != P:
        raise ValueError(f'draw_segments: {int(m.shape[0])} poses for {P} views')
    if depth is not None:
        if tuple(depth.shape) != (P, H, W):
            raise ValueError(f'draw_segments: depth {tuple(depth.shape)} for views {(P, H, W)}')
        depth = depth.to(dev, torch.float32).contiguous()
    s = segments if torch.is_tensor(segments) else torch.from_numpy(np.asarray(segments, dtype=np.float64))
    s = s.detach().to(dev, torch.float64).reshape(-1, 2, 3).contiguous()
    c = colors if torch.is_tensor(colors) else torch.from_numpy(np.ascontiguousarray(colors))
    if c.dtype != torch.uint8:
        raise ValueError(f'draw_segments: colours must be uint8, got {c.dtype}')
    c = c.to(dev).reshape(-1, 3).contiguous()
    N = int(s.shape[0])
    if int(c.shape[0]) != N:
        raise ValueError(f'draw_segments: {int(c.shape[0])} colours for {N} segments')
    r, R, n_listed = None, 0, N
    if ranges is not None:
        r = ranges if torch.is_tensor(ranges) else torch.from_numpy(np.asarray(ranges, dtype=np.int64))
        r = r.detach().to(torch.int64)
        if r.dim() == 2:
            r = r[None].expand(P, -1, -1)
        if r.dim() != 3 or int(r.shape[0]) != P or r.shape[2] != 2 or not 1 <= int(r.shape[1]) <= _lib.SEG_MAX_RANGES:
            raise ValueError(f'draw_segments: ranges must be [P,R,2] or [R,2] with R in [1, {_lib.SEG_MAX_RANGES}], got {tuple(r.shape)}')
        R = int(r.shape[1])
        lens = (r[..., 1].clamp(max=N) - r[..., 0].clamp(min=0)).clamp(min=0).sum(1)
        n_listed = int(lens.max()) if P else 0                                  # the one read of the ranges on the host
        r = r.to(dev).contiguous()
    seg = torch.empty((P, H, W), dtype=torch.int32, device=dev) if want_seg else None
    ws = None
    for p0 in range(0, P, chunk):
        n = min(chunk, P - p0)
        need = lib().adfp_draw_segments_workspace_bytes(n, n_listed)
        if need and (ws is None or ws.numel() < need):
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with _lib.on(dev) as L:
            L.adfp_draw_segments(rgb[p0:p0 + n], depth[p0:p0 + n] if depth is not None else None, seg[p0:p0 + n] if want_seg else None,
                                 n, H, W, m[p0:p0 + n], float(fx), float(fy), float(cx), float(cy), s, c, N,
                                 r[p0:p0 + n] if r is not None else None, R, n_listed, 0.5 * float(width), float(near_clip),
                                 float(bias[0]), float(bias[1]), float(hidden_alpha), ws, need)
    return seg


def render_mesh(input_mesh, poses, cam, out, mode='shaded', smooth=True, cull='none', depth=False, near=None, far=20.0,
                ambient=0.3, albedo=(0.8, 0.8, 0.8), background=(255, 255, 255), chunk=CHUNK, device='cuda:0'):
    """Render the PLY `input_mesh` (its vertex colours when it has them) from `poses` ([P,4,4] camera-to-world, OpenCV axes) with
    cam = (H, W, fx, fy, cx, cy) and write {out}/{mode}_{k:05d}.png, and depth_{k:05d}.npy when depth=True.  One download per
    chunk of views.  Returns the list of PNG paths."""
    from PIL import Image
    m = mesh.read_ply(input_mesh)
    colors = m.colors[:, :3] if m.colors is not None else None
    mv = MeshViews(m.verts, m.faces, colors, device, smooth)
    poses = np.asarray(poses.detach().cpu().numpy() if torch.is_tensor(poses) else poses, dtype=np.float64).reshape(-1, 4, 4)
    H, W, fx, fy, cx, cy = cam
    os.makedirs(out, exist_ok=True)
    paths = []
    for p0 in range(0, len(poses), chunk):
        r = mv.render(poses[p0:p0 + chunk], H, W, fx, fy, cx, cy, near, far, mode, cull, ambient, albedo, background, chunk)
        rgb = r['rgb'].cpu().numpy()
        dep = r['depth'].cpu().numpy() if depth else None
        for k in range(rgb.shape[0]):
            paths.append(os.path.join(out, f'{mode}_{p0 + k:05d}.png'))
            Image.fromarray(rgb[k], 'RGB').save(paths[-1])
            if depth:
                np.save(os.path.join(out, f'depth_{p0 + k:05d}.npy'), dep[k])
    return paths


def opencv_poses(flipped):
    """float64 [P,4,4] with OpenCV axes from poses in the renderer's convention (columns 1 and 2 negated), which is how
    cull_mesh.load_poses and render_views.read_poses return them."""
    p = torch.stack(list(flipped)) if not torch.is_tensor(flipped) else flipped
    p = p.detach().cpu().numpy().astype(np.float64).reshape(-1, 4, 4).copy()
    p[:, :3, 1] *= -1.0
    p[:, :3, 2] *= -1.0
    return p


def main(argv=None):
    ap = argparse.ArgumentParser(description='Render views of a mesh: shaded, vertex colours or normals.')
    ap.add_argument('config', nargs='?', help='a run config: its cam block gives H, W, fx, fy, cx, cy')
    ap.add_argument('--input_mesh', required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--traj', help='Replica traj.txt (read as cull_mesh reads it)')
    src.add_argument('--poses', help='one camera-to-world 4x4 per line (read as render_views reads it)')
    for k, t in (('H', int), ('W', int), ('fx', float), ('fy', float), ('cx', float), ('cy', float)):
        ap.add_argument('--' + k, type=t)
    ap.add_argument('--mode', choices=tuple(_lib.SHADE_MODE), default='shaded')
    ap.add_argument('--flat', action='store_true', help="shade with each face's own normal")
    ap.add_argument('--cull', choices=tuple(_lib.CULL), default='none')
    ap.add_argument('--every', type=int, default=1, help='render every N-th pose')
    ap.add_argument('--depth', action='store_true', help='also write depth_{k:05d}.npy')
    ap.add_argument('--far', type=float, default=20.0)
    ap.add_argument('--out', default='mesh_views')
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    given = [getattr(args, k) for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy')]
    if args.config is not None:
        from .get_tsdf import load_config, update_cam
        cam = list(update_cam(load_config(args.config)))
        cam = [g if g is not None else c for g, c in zip(given, cam)]
    elif any(g is None for g in given):
        ap.error('give a CONFIG or all of --H --W --fx --fy --cx --cy')
    else:
        cam = given
    if args.every < 1:
        ap.error('--every must be at least 1')
    if args.traj:
        from .cull_mesh import load_poses
        poses = opencv_poses(load_poses(args.traj))
    else:
        from .render_views import read_poses
        poses = opencv_poses(read_poses(args.poses))
    return render_mesh(args.input_mesh, poses[::args.every], tuple(cam), args.out, args.mode, not args.flat, args.cull, args.depth,
                       far=args.far, device=args.device)


if __name__ == '__main__':
    main()
