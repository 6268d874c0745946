"""
Drop-in for the reference's ``src/utils/Mesher.py`` ``Mesher``: same constructor, same cfg keys (Mesher.py:30-46), same
``slam`` attributes, ``get_mesh(...)`` with the reference's signature, return value and ``.ply`` output -- without open3d,
trimesh or scikit-image.

Where the work runs: the lattice is formed on the device chunk by chunk and queried through the package's ``eval_points``
(libadfp.so); the convex-hull mask is one kernel (``adfp_lattice_hull_fill``); marching cubes is ``mesh.marching_cubes``
(``adfp_mc_count`` / ``adfp_mc_emit``); the seen mask is one launch over all poses (``seen_mask``, ``adfp_mesh_seen_mask``); the
component culling, the colour bytes and the merge of coincident vertices are ``mesh.clean_components`` / ``color_bytes`` /
``merge_coincident`` (csrc/adfp_meshclean.h); the mesh bound is ``bound_planes`` (``mesh.depth_hull``: a quickhull in rounds whose
point work -- support pass, classification, ordered compaction, per-facet farthest -- runs over the resident depth block,
csrc/adfp_bound.h, while Qhull keeps the facets of the few hundred hull vertices).  The host keeps those small hulls and the file.
``point_masks`` (the reference's torch code, the only source of the forecast / unseen masks), ``clean`` (scipy.sparse.csgraph),
``get_bound_planes`` (numpy and Qhull over every point) and the module's ``merge_coincident`` remain as the host statements of the
same steps: the tests compare the device path against them.

Two cfg keys the reference does not have (``config.MESHING_DEFAULTS``): ``meshing.simplify_voxel_size`` (default None = off; a
positive number, in the config's units, clusters the cleaned mesh's vertices per voxel cell before the colour query,
``mesh.simplify_vertex_clustering``) and ``meshing.simplify_contraction`` ('quadric' or 'average').  Vertex clustering by this
package's own rules (include/adfp.h, "mesh simplification"): open3d's function was never run against it.

``color_mesh_extraction_method: keyframe_projection`` (this package's own value of the reference's key) colours the vertices that a
keyframe sees from the keyframes' images (``mesh.project_colors``, csrc/adfp_meshcolor.h) and the rest by the direct point query;
``meshing.projection_depth_tol`` (default 0.05, in the config's units), ``projection_blend`` ('weighted' or 'best') and
``projection_border`` (pixels) steer it.

Deviations, both documented in INTEGRATION.md:
  * the mesh bound (``get_bound_from_frames``) is the convex hull of the keyframes' camera centres and back-projected valid
    depth pixels (scipy.spatial.ConvexHull, per frame, then over the union of the frames' hull vertices), scaled by
    ``clean_mesh_bound_scale`` about the mean of its vertices; the reference hulls the vertices of an open3d TSDF mesh of the
    same frames;
  * marching cubes resolves ambiguous faces by separating the inside corners (include/adfp.h), where scikit-image uses the
    Lewiner decider; the vertex set (every edge crossing) is the same.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import mesh as M
from .config import meshing_setting


# direct_point_query: the colour decoder at every vertex (the reference's default).  keyframe_projection: the keyframes' own
# images where a keyframe sees the vertex (mesh.project_colors), the decoder elsewhere.  The reference's render_ray is not offered.
COLOR_METHODS = ('direct_point_query', 'keyframe_projection')


class Mesher(object):

    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = slam.renderer
        self.scale = cfg['scale']
        self.occupancy = cfg['occupancy']

        self.resolution = cfg['meshing']['resolution']
        self.level_set = cfg['meshing']['level_set']
        self.clean_mesh_bound_scale = cfg['meshing']['clean_mesh_bound_scale']
        self.remove_small_geometry_threshold = cfg['meshing']['remove_small_geometry_threshold']
        self.color_mesh_extraction_method = cfg['meshing']['color_mesh_extraction_method']
        self.get_largest_components = cfg['meshing']['get_largest_components']
        self.depth_test = cfg['meshing']['depth_test']
        # this package's own keys (config.MESHING_DEFAULTS; the reference's configs have neither): a positive simplify_voxel_size
        # (in the config's units, like the bounds) clusters the cleaned mesh's vertices before the colour query
        self.simplify_voxel_size = meshing_setting(cfg, 'simplify_voxel_size')
        self.simplify_contraction = meshing_setting(cfg, 'simplify_contraction')
        if self.simplify_contraction not in M.SIMPLIFY_CONTRACTIONS:
            raise ValueError(f'meshing.simplify_contraction={self.simplify_contraction!r}: one of {sorted(M.SIMPLIFY_CONTRACTIONS)}')
        # color_mesh_extraction_method: keyframe_projection (this package's own; the rule is include/adfp.h's "mesh colours from the
        # keyframes"): depth_tol in the config's units (times `scale`, like the bounds), the blend and the border in pixels
        self.projection_depth_tol = float(meshing_setting(cfg, 'projection_depth_tol')) * self.scale
        self.projection_blend = meshing_setting(cfg, 'projection_blend')
        self.projection_border = int(meshing_setting(cfg, 'projection_border'))
        if self.projection_blend not in M.BLENDS:
            raise ValueError(f'meshing.projection_blend={self.projection_blend!r}: one of {sorted(M.BLENDS)}')
        if not (self.projection_depth_tol >= 0 and np.isfinite(self.projection_depth_tol)) or self.projection_border < 0:
            raise ValueError(f'meshing.projection_depth_tol={self.projection_depth_tol!r}, projection_border={self.projection_border!r}: '
                             'a finite tolerance and a border, neither negative')

        self.bound = slam.bound
        self.verbose = slam.verbose
        self.marching_cubes_bound = torch.from_numpy(np.array(cfg['mapping']['marching_cubes_bound']) * self.scale)
        # The reference builds a dataset reader here (frame_reader, n_img); get_mesh never reads it, so none is constructed.
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.sample_mode = 'bilinear'
        self.tsdf_bnds = slam.tsdf_bnds

    # ---- Mesher.py:58-217, line for line in torch -------------------------------------------------------------------------
    def _project(self, points, c2w, device):
        fx, fy, cx, cy = self.fx, self.fy, self.cx, self.cy
        w2c = np.linalg.inv(c2w)
        w2c = torch.from_numpy(w2c).to(device).float()
        ones = torch.ones_like(points[:, 0]).reshape(-1, 1).to(device)
        homo_points = torch.cat([points, ones], dim=1).reshape(-1, 4, 1).to(device).float()
        cam_cord_homo = w2c @ homo_points
        cam_cord = cam_cord_homo[:, :3]
        K = torch.from_numpy(np.array([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]]).reshape(3, 3)).to(device)
        cam_cord[:, 0] *= -1
        uv = K.float() @ cam_cord.float()
        z = uv[:, -1:] + 1e-8
        uv = uv[:, :2] / z
        uv = uv.float()
        H, W = self.H, self.W
        edge = 0
        cur_mask_seen = (uv[:, 0] < W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < H - edge) & (uv[:, 1] > edge)
        cur_mask_seen = cur_mask_seen & (z[:, :, 0] < 0)
        edge = -1000
        cur_mask_forecast = (uv[:, 0] < W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < H - edge) & (uv[:, 1] > edge)
        cur_mask_forecast = cur_mask_forecast & (z[:, :, 0] < 0)
        return cam_cord, uv, cur_mask_seen, cur_mask_forecast

    def point_masks(self, input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False):
        """(seen, forecast, unseen) boolean numpy masks of the points, as Mesher.py:58-217 computes them."""
        H, W = self.H, self.W
        if not isinstance(input_points, torch.Tensor):
            input_points = torch.from_numpy(input_points)
        input_points = input_points.clone().detach()
        seen_mask_list, forecast_mask_list, unseen_mask_list = [], [], []
        for pnts in torch.split(input_points, self.points_batch_size, dim=0):
            points = pnts.to(device).float()
            seen_mask = torch.zeros((points.shape[0])).bool().to(device)
            forecast_mask = torch.zeros((points.shape[0])).bool().to(device)
            if get_mask_use_all_frames:
                for i in range(0, idx + 1, 1):
                    c2w = estimate_c2w_list[i].cpu().numpy()
                    _, _, cur_mask_seen, cur_mask_forecast = self._project(points, c2w, device)
                    seen_mask |= cur_mask_seen.reshape(-1)
                    forecast_mask |= cur_mask_forecast.reshape(-1)
            else:
                for keyframe in keyframe_dict:
                    c2w = keyframe['est_c2w'].cpu().numpy()
                    cam_cord, uv, cur_mask_seen, cur_mask_forecast = self._project(points, c2w, device)
                    if self.depth_test:
                        gt_depth = keyframe['depth'].to(device).reshape(1, 1, H, W)
                        vgrid = uv.reshape(1, 1, -1, 2)
                        vgrid[..., 0] = (vgrid[..., 0] / (W - 1) * 2.0 - 1.0)
                        vgrid[..., 1] = (vgrid[..., 1] / (H - 1) * 2.0 - 1.0)
                        depth_sample = F.grid_sample(gt_depth, vgrid, padding_mode='zeros', align_corners=True)
                        depth_sample = depth_sample.reshape(-1)
                        max_depth = torch.max(depth_sample)
                        cur_mask_forecast = cur_mask_forecast.reshape(-1)
                        proj_depth_forecast = -cam_cord[cur_mask_forecast, 2].reshape(-1)
                        cur_mask_forecast[cur_mask_forecast.clone()] &= proj_depth_forecast < max_depth
                        cur_mask_seen = cur_mask_seen.reshape(-1)
                        proj_depth_seen = - cam_cord[cur_mask_seen, 2].reshape(-1)
                        cur_mask_seen[cur_mask_seen.clone()] &= \
                            (proj_depth_seen < depth_sample[cur_mask_seen] + 2.4) \
                            & (depth_sample[cur_mask_seen] - 2.4 < proj_depth_seen)
                    else:
                        max_depth = torch.max(keyframe['depth']) * 1.1
                        cur_mask_forecast = cur_mask_forecast.reshape(-1)
                        proj_depth_forecast = -cam_cord[cur_mask_forecast, 2].reshape(-1)
                        cur_mask_forecast[cur_mask_forecast.clone()] &= proj_depth_forecast < max_depth.to(device)
                        cur_mask_seen = cur_mask_seen.reshape(-1)
                        proj_depth_seen = - cam_cord[cur_mask_seen, 2].reshape(-1)
                        cur_mask_seen[cur_mask_seen.clone()] &= proj_depth_seen < max_depth.to(device)
                    seen_mask |= cur_mask_seen
                    forecast_mask |= cur_mask_forecast
            forecast_mask &= ~seen_mask
            unseen_mask = ~(seen_mask | forecast_mask)
            seen_mask_list.append(seen_mask.cpu().numpy())
            forecast_mask_list.append(forecast_mask.cpu().numpy())
            unseen_mask_list.append(unseen_mask.cpu().numpy())
        return (np.concatenate(seen_mask_list, axis=0), np.concatenate(forecast_mask_list, axis=0),
                np.concatenate(unseen_mask_list, axis=0))

    def seen_mask(self, verts, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False, keyframe_store=None):
        """The *seen* mask of point_masks as a bool device tensor [V], every pose in ONE launch (adfp_mesh_seen_mask): what
        get_mesh culls with.  The poses are inverted on the host exactly as _project does (np.linalg.inv in the pose's own dtype,
        then f32): one read-back of [K,4,4].  Depth images come from ``keyframe_store`` (a keyframes.KeyframeStore holding the
        same keyframes in the same order: its resident [K,H,W] block is read in place) or are stacked from ``keyframe_dict``
        once.  Agrees with point_masks(...)[0] except where the two f32 evaluations of the projection can round to different
        sides of a bound (rocBLAS's order for w2c @ p is not ours): points within rounding of an image edge, of z = 0 or of a
        depth bound."""
        H, W = self.H, self.W
        dev = torch.device(device)
        pts = verts if isinstance(verts, torch.Tensor) else torch.from_numpy(np.asarray(verts))
        pts = pts.detach().to(dev, torch.float32).reshape(-1, 3).contiguous()
        if get_mask_use_all_frames:
            mats = [estimate_c2w_list[i] for i in range(0, idx + 1, 1)]
        else:
            mats = [keyframe['est_c2w'] for keyframe in keyframe_dict]
        seen = torch.zeros(pts.shape[0], dtype=torch.uint8, device=dev)
        K = len(mats)
        if K == 0 or pts.shape[0] == 0:
            return seen.bool()
        c2w = torch.stack([m.detach() for m in mats]).cpu().numpy()
        w2c = M.w2c_rows_own_dtype(c2w, dev)
        depth = far = None
        rule = 'frustum'
        if not get_mask_use_all_frames:
            rule = 'depth_test' if self.depth_test else 'max_depth'
            if keyframe_store is not None:
                if len(keyframe_store) < K:
                    raise ValueError(f'seen_mask: the store holds {len(keyframe_store)} keyframes, keyframe_dict {K}')
                depth = keyframe_store.depths(K)
            else:
                depth = torch.stack([keyframe['depth'] for keyframe in keyframe_dict]).to(dev, torch.float32)
            depth = depth.reshape(K, H, W).contiguous()
            if not self.depth_test:
                far = (depth.reshape(K, -1).amax(1) * 1.1).contiguous()          # torch.max(depth) * 1.1, per keyframe
        with M._lib.on(dev) as L:
            L.adfp_mesh_seen_mask(pts, int(pts.shape[0]), w2c, K, M._lib.SEEN_RULE[rule], depth if self.depth_test else None, far,
                                  float(self.fx), float(self.fy), float(self.cx), float(self.cy), int(W), int(H), seen)
        return seen.bool()

    # ---- mesh bound ------------------------------------------------------------------------------------------------------
    def get_bound_planes(self, keyframe_dict, scale=1):
        """Facet planes [F,4] (n, d; inside: n . p + d <= 0) of the mesh bound: the convex hull of the keyframes' camera centres
        and back-projected valid depth pixels, scaled by clean_mesh_bound_scale about its vertices' mean (see the module
        docstring: the reference hulls an open3d TSDF mesh of the same frames instead)."""
        from scipy.spatial import ConvexHull
        H, W, fx, fy, cx, cy = self.H, self.W, self.fx, self.fy, self.cx, self.cy
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
        pts = []
        for keyframe in keyframe_dict:
            c2w = keyframe['est_c2w'].cpu().numpy().astype(np.float64)
            c2w[:3, 1] *= -1.0                                        # open3d / OpenCV camera, Mesher.py:247-249
            c2w[:3, 2] *= -1.0
            depth = keyframe['depth'].cpu().numpy().astype(np.float64)
            ok = (depth > 0) & (depth < 1000)                        # depth_trunc=1000 of Mesher.py:256-261
            d = depth[ok]
            cam = np.stack([(u[ok] - cx) / fx * d, (v[ok] - cy) / fy * d, d], 1)
            frame = np.concatenate([c2w[:3, 3][None], cam @ c2w[:3, :3].T + c2w[:3, 3]], 0)
            if len(frame) >= 4:
                try:
                    frame = frame[ConvexHull(frame).vertices]
                except Exception:                                    # a degenerate (planar) frame: keep its points
                    pass
            pts.append(frame)
        hull = ConvexHull(np.concatenate(pts, 0))
        verts = hull.points[hull.vertices]
        center = verts.mean(0)
        verts = center + self.clean_mesh_bound_scale * (verts - center)
        return ConvexHull(verts).equations

    def bound_planes(self, keyframe_dict, scale=1, device='cuda:0', keyframe_store=None):
        """get_bound_planes with the point work on the device (mesh.depth_hull: a quickhull in rounds over the resident depth
        block, csrc/adfp_bound.h): the same bound, facet planes [F,4].  Depths and poses come from ``keyframe_store`` (a
        keyframes.KeyframeStore of the same keyframes in the same order, read in place) or are stacked from ``keyframe_dict`` once.
        The tail is the host path's: the mean of the hull's vertices in id order (the order the per-frame-then-union hull yields
        them in), the scale by clean_mesh_bound_scale, Qhull's equations of the scaled vertices.  The vertex set is that of the
        hull over ALL points, which the per-frame-then-union route also yields; coordinates differ from get_bound_planes' within
        the rounding of its BLAS product (include/adfp.h fixes the order of operations here)."""
        from scipy.spatial import ConvexHull
        dev = torch.device(device)
        K = len(keyframe_dict)
        if K == 0:
            raise ValueError('bound_planes: need at least one keyframe')
        if keyframe_store is not None:
            if len(keyframe_store) < K:
                raise ValueError(f'bound_planes: the store holds {len(keyframe_store)} keyframes, keyframe_dict {K}')
            depth, poses = keyframe_store.depths(K), keyframe_store.poses(K)
        else:
            depth = torch.stack([keyframe['depth'] for keyframe in keyframe_dict]).to(dev, torch.float32)
            poses = torch.stack([keyframe['est_c2w'].detach() for keyframe in keyframe_dict]).to(dev, torch.float32)
        depth = depth.reshape(K, self.H, self.W)
        _, verts = M.depth_hull(depth, poses.reshape(K, 4, 4), self.fx, self.fy, self.cx, self.cy)
        center = verts.mean(0)
        verts = center + self.clean_mesh_bound_scale * (verts - center)
        return ConvexHull(verts).equations

    def get_grid_uniform(self, resolution):
        """The lattice axes of Mesher.py:365-393 (float64 np.linspace over the marching-cubes bound + 0.05).  The [P,3] point
        list is not formed on the host: get_mesh builds it on the device chunk by chunk."""
        bound = self.marching_cubes_bound
        padding = 0.05
        x = np.linspace(bound[0][0] - padding, bound[0][1] + padding, resolution)
        y = np.linspace(bound[1][0] - padding, bound[1][1] + padding, resolution)
        z = np.linspace(bound[2][0] - padding, bound[2][1] + padding, resolution)
        # np.linspace over torch scalars hands back float64 tensors; the values are the reference's, as numpy arrays
        return {"xyz": [np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64)]}

    @staticmethod
    def marching_cubes_geometry(xyz):
        """(spacing, origin) of the lattice as Mesher.py:464-486 hands them to marching cubes and adds to its vertices."""
        spacing = (xyz[0][2] - xyz[0][1], xyz[1][2] - xyz[1][1], xyz[2][2] - xyz[2][1])
        origin = (xyz[0][0], xyz[1][0], xyz[2][0])
        return spacing, origin

    def eval_points(self, p, decoders, tsdf_volume, tsdf_bnds, c=None, stage='color', device='cuda:0'):
        """Mesher.py:286-326: raw [P,4]; occupancy 100 outside ``bound``."""
        ret, _ = self.renderer.eval_points(p, decoders, tsdf_volume, tsdf_bnds, c, stage, device)
        return ret

    def lattice(self, c, decoders, tsdf_volume, axes, device):
        """Occupancy ('high') of every lattice point as a device tensor [X,Y,Z] (Mesher.py:437-455 before the hull mask).  The
        reference also samples the TSDF per chunk (eval_tsdf_mask, :441-442, :446) and never uses the result: skipped."""
        ax = [torch.from_numpy(np.asarray(a, dtype=np.float64).astype(np.float32)).to(device) for a in axes]
        X, Y, Z = (int(a.numel()) for a in ax)
        out = torch.empty(X * Y * Z, dtype=torch.float32, device=device)
        with torch.no_grad():
            for s in range(0, X * Y * Z, self.points_batch_size):
                lin = torch.arange(s, min(s + self.points_batch_size, X * Y * Z), device=device, dtype=torch.int64)
                k = lin % Z
                j = (lin // Z) % Y
                i = lin // (Y * Z)
                pts = torch.stack([ax[0][i], ax[1][j], ax[2][k]], 1)
                out[s:s + lin.numel()] = self.eval_points(pts, decoders, tsdf_volume, self.tsdf_bnds, c, 'high', device)[:, 3]
        return out.reshape(X, Y, Z), ax

    # ---- culling (Mesher.py:492-513) -------------------------------------------------------------------------------------
    def clean(self, vertices, faces, seen_mask):
        """Drop faces whose three vertices are unseen, split into components (trimesh.split), keep the largest
        (get_largest_components) or those above remove_small_geometry_threshold * scale^2 in area, keep referenced vertices.
        Components follow trimesh's face adjacency: two faces are joined only through an edge that EXACTLY two faces use
        (trimesh.graph.face_adjacency groups edges with require_count=2).  An edge with four faces -- the fan diagonal that
        both cells of an ambiguous face can draw (include/adfp.h) -- joins nothing, as it would in the reference."""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        faces = faces[~(~seen_mask)[faces].all(axis=1)]
        if len(faces) == 0:
            return vertices[:0], faces
        nf = len(faces)
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
        e = np.sort(e, 1)
        fid = np.tile(np.arange(nf), 3)
        key = e[:, 0].astype(np.int64) * (len(vertices) + 1) + e[:, 1]
        order = np.argsort(key, kind='stable')
        ks, fs = key[order], fid[order]
        _, start, count = np.unique(ks, return_index=True, return_counts=True)
        two = start[count == 2]                        # edges of exactly two faces: those two faces are adjacent
        adj = coo_matrix((np.ones(len(two)), (fs[two], fs[two + 1])), shape=(nf, nf))
        ncomp, label = connected_components(adj, directed=False)
        v = vertices.astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]]), axis=1)
        comp_area = np.bincount(label, weights=area, minlength=ncomp)
        if self.get_largest_components:
            keep = label == comp_area.argmax()
        else:
            keep = (comp_area > self.remove_small_geometry_threshold * self.scale * self.scale)[label]
        faces = faces[keep]
        used = np.unique(faces)
        remap = np.full(len(vertices), -1, np.int64)
        remap[used] = np.arange(len(used))
        return vertices[used], remap[faces].astype(np.int32)

    def projected_colors(self, verts, faces, keyframe_dict, device='cuda:0', keyframe_store=None):
        """(rgb f32 [V,3], count int32 [V]) of the mesh's vertices from the keyframes' images (mesh.project_colors with the
        mesh's own vertex normals and this Mesher's projection_* settings): count = 0 where no keyframe sees the vertex.  Depth,
        colour and poses come from ``keyframe_store`` (a keyframes.KeyframeStore of the same keyframes in the same order: its
        resident blocks are read in place) or are stacked from ``keyframe_dict`` once, as seen_mask stacks the depths."""
        dev = torch.device(device)
        K = len(keyframe_dict)
        if keyframe_store is not None:
            if len(keyframe_store) < K:
                raise ValueError(f'projected_colors: the store holds {len(keyframe_store)} keyframes, keyframe_dict {K}')
            depth, image, poses = keyframe_store.depths(K), keyframe_store.colors(K), keyframe_store.poses(K)
        elif K:
            depth = torch.stack([keyframe['depth'] for keyframe in keyframe_dict]).to(dev, torch.float32)
            image = torch.stack([keyframe['color'] for keyframe in keyframe_dict]).to(dev, torch.float32)
            poses = torch.stack([keyframe['est_c2w'].detach() for keyframe in keyframe_dict]).to(torch.float32)
        else:
            depth = torch.zeros((0, self.H, self.W), dtype=torch.float32, device=dev)
            image = torch.zeros((0, self.H, self.W, 3), dtype=torch.float32, device=dev)
            poses = torch.zeros((0, 4, 4), dtype=torch.float32)
        normals = M.vertex_normals(verts, faces)
        rgb, _, count, _ = M.project_colors(verts, normals, depth.reshape(K, self.H, self.W), image.reshape(K, self.H, self.W, 3),
                                            poses.reshape(K, 4, 4), self.fx, self.fy, self.cx, self.cy, self.projection_depth_tol,
                                            self.projection_border, self.projection_blend)
        return rgb, count

    def mesh_arrays(self, verts, faces, c, decoders, keyframe_dict, estimate_c2w_list, idx, tsdf_volume, device='cuda:0',
                    color=True, clean_mesh=True, get_mask_use_all_frames=False, keyframe_store=None):
        """get_mesh from the marching-cubes output (device verts f32 [V,3], faces int32 [F,3]) to the arrays write_ply takes
        (numpy vertices / scale, faces, uint8 colours or None): culling, colour query and bytes, vertex merge on the device, then
        one copy of each array."""
        with torch.no_grad():
            if clean_mesh:
                seen = self.seen_mask(verts, keyframe_dict, estimate_c2w_list, idx, device,
                                      get_mask_use_all_frames=get_mask_use_all_frames, keyframe_store=keyframe_store)
                verts, faces = M._clean_components(verts, faces, seen.to(torch.uint8),
                                                   self.remove_small_geometry_threshold * self.scale * self.scale,
                                                   bool(self.get_largest_components))
            if self.simplify_voxel_size is not None and self.simplify_voxel_size > 0:
                verts, faces, _ = M._simplify_vertex_clustering(verts, faces, float(self.simplify_voxel_size) * self.scale,
                                                                self.simplify_contraction, None)
            vertex_colors = None
            if color:
                vc = [M.color_bytes(self.eval_points(pnts, decoders, tsdf_volume, self.tsdf_bnds, c, 'color', device))
                      for pnts in torch.split(verts, self.points_batch_size, dim=0)]
                vertex_colors = torch.cat(vc, 0) if vc else torch.zeros((0, 3), dtype=torch.uint8, device=verts.device)
                if self.color_mesh_extraction_method == 'keyframe_projection' and verts.shape[0]:
                    # the keyframes' colour where a keyframe sees the vertex, the decoder's elsewhere
                    rgb, count = self.projected_colors(verts, faces, keyframe_dict, device, keyframe_store)
                    vertex_colors = torch.where((count > 0)[:, None], M.color_bytes(rgb), vertex_colors)
            verts, faces, vertex_colors = M._merge_coincident(verts, faces, vertex_colors)
            vertices = verts.cpu().numpy() / np.float32(self.scale)
            return vertices, faces.cpu().numpy(), (vertex_colors.cpu().numpy() if vertex_colors is not None else None)

    def get_mesh(self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, tsdf_volume, device='cuda:0',
                 color=True, clean_mesh=True, get_mask_use_all_frames=False, keyframe_store=None):
        """Extract the mesh of the scene representation and write it to mesh_out_file (.ply); returns z_uni_m (Mesher.py:395-544).
        From marching cubes to the file everything stays on the device (seen_mask, mesh.clean_components' kernels, the colour
        query and bytes, mesh.merge_coincident's kernels); the host receives the final vertices, faces and colours, one copy each.
        keyframe_store: a keyframes.KeyframeStore of the same keyframes, whose resident depth block bound_planes and seen_mask
        then read."""
        if not str(mesh_out_file).lower().endswith('.ply'):
            raise NotImplementedError(f'{mesh_out_file}: only .ply output is supported')
        if color and self.color_mesh_extraction_method not in COLOR_METHODS:
            raise NotImplementedError(f'color_mesh_extraction_method={self.color_mesh_extraction_method!r}: one of {COLOR_METHODS}')
        with torch.no_grad():
            xyz = self.get_grid_uniform(self.resolution)['xyz']
            z, ax = self.lattice(c, decoders, tsdf_volume, xyz, device)
            planes = self.bound_planes(keyframe_dict, self.scale, device, keyframe_store)
            M.hull_fill(z, ax, planes, 100.)
            z_uni_m = z.cpu().numpy()
            spacing, origin = self.marching_cubes_geometry(xyz)
            verts, faces, _ = M.marching_cubes(z, level=self.level_set, spacing=spacing, origin=origin, outward='lower')
            if faces.shape[0] == 0:
                print('marching_cubes error. Possibly no surface extracted from the level set.')
                return
            vertices, faces, vertex_colors = self.mesh_arrays(verts, faces, c, decoders, keyframe_dict, estimate_c2w_list, idx,
                                                              tsdf_volume, device, color, clean_mesh, get_mask_use_all_frames,
                                                              keyframe_store)
            os.makedirs(os.path.dirname(os.path.abspath(mesh_out_file)), exist_ok=True)
            M.write_ply(mesh_out_file, vertices, faces, colors=vertex_colors)
            if self.verbose:
                print('Saved mesh at', mesh_out_file)
            return z_uni_m


def merge_coincident(vertices, faces, colors=None):
    """Merge bitwise-equal vertex positions (what trimesh.Trimesh(process=True) does to the coincident vertices marching cubes
    leaves at exactly-level corners); the first occurrence survives, in order."""
    if len(vertices) == 0:
        return vertices, faces, colors
    bits = np.ascontiguousarray(vertices.astype(np.float32)).view(np.int32).reshape(-1, 3)
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    if len(first) == len(vertices):
        return vertices, faces, colors
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(len(first))
    keep = np.sort(first)
    new_of_old = rank[inv]
    return vertices[keep], new_of_old[faces].astype(np.int32), (colors[keep] if colors is not None else None)
