"""Drop-in for the reference's src/tools/evaluate_scannet.py on the MI355X: the ScanNet mesh metrics (Acc, Comp, Chamfer, Prec,
Recal, F-score) without open3d, pyrender, trimesh, sklearn or an OpenGL context.

    python -m attentive_dfprior_amd.evaluate_scannet configs/ScanNet/scene0050.yaml [--input_folder ..] [--output ..] [--space ..]

The reference renders the predicted mesh (faces inverted, back faces culled) from every 10th ground-truth pose, fuses the depths
into open3d's ScalableTSDFVolume, extracts a mesh again, writes it, reads it back, voxel-downsamples it and the ground truth and
compares nearest-neighbour distances.  Here every step of that runs on the device (raycast.MeshBVH with a cull mode, refusion.py,
recon.NNIndex); the readings of open3d and pyrender this rests on are listed in INTEGRATION.md section 2b.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch
import yaml

from . import mesh as _mesh
from . import raycast, recon, refusion

VOXEL = 0.01                 # refuse(): ScalableTSDFVolume(voxel_length=0.01, sdf_trunc=3 * 0.01)
SDF_TRUNC = 3 * 0.01
DEPTH_TRUNC = 5.0            # create_from_color_and_depth(depth_scale=1.0, depth_trunc=5.0)
DEPTH_STRIDE = 4             # ScalableTSDFVolume's depth_sampling_stride (open3d's default)
ZNEAR = 0.05                 # pyrender IntrinsicsCamera's default znear
# pyrender's IntrinsicsCamera projection, as we read it, puts pixel (i, j)'s ray through ((j + 0.5 - cx) / fx, (i + 0.5 - cy) / fy):
# the port renders with principal point (cx - PIXEL_CENTRE, cy - PIXEL_CENTRE).  Unverified: pyrender is not installed here.
PIXEL_CENTRE = 0.5
FRAME_SPACE = 10             # get_pose keeps every 10th frame
UNIT_VOXELS = refusion.UNIT ** 3


def nn_correspondance(verts1, verts2):
    """For each point of verts2 the distance to its nearest point of verts1 (f64 numpy [len(verts2)]); ([], []) when either is
    empty, as the reference returns."""
    if len(verts1) == 0 or len(verts2) == 0:
        return [], []
    d, _ = recon.NNIndex(verts1).query(verts2)
    return d.cpu().numpy()


def _points(x, dev):
    v = x.vertices if hasattr(x, 'vertices') else x
    return recon.as_points(np.asarray(v)[:, :3] if not torch.is_tensor(v) else v[:, :3], dev)


def evaluate(mesh_pred, mesh_trgt, threshold=.05, down_sample=.02):
    """The reference's six metrics over the vertices of two meshes (objects with .vertices, or [N,3] arrays), each cloud voxel-
    downsampled first when down_sample is set; nearest neighbours by recon.NNIndex, the sums on the device.  Python floats."""
    dev = recon.device_of(getattr(mesh_pred, 'vertices', mesh_pred), getattr(mesh_trgt, 'vertices', mesh_trgt))
    pred, trgt = _points(mesh_pred, dev), _points(mesh_trgt, dev)
    if down_sample:
        pred, _ = refusion.voxel_down_sample(pred, down_sample, dev)
        trgt, _ = refusion.voxel_down_sample(trgt, down_sample, dev)
    if pred.shape[0] == 0 or trgt.shape[0] == 0:
        raise ValueError('evaluate: a point cloud is empty')
    dist1, _ = recon.NNIndex(pred).query(trgt)          # nn_correspondance(verts_pred, verts_trgt)
    dist2, _ = recon.NNIndex(trgt).query(pred)          # nn_correspondance(verts_trgt, verts_pred)
    s1, c1 = recon.metric_sums(dist1, threshold)
    s2, c2 = recon.metric_sums(dist2, threshold)
    n1, n2 = int(dist1.numel()), int(dist2.numel())
    precision, recal = c2 / n2, c1 / n1
    fscore = 2 * precision * recal / (precision + recal) if precision + recal > 0 else float('nan')
    return {'Acc': s2 / n2, 'Comp': s1 / n1, 'Chamfer': (s1 / n1 + s2 / n2) / 2, 'Prec': precision, 'Recal': recal, 'F-score': fscore}


def update_cam(cfg):
    """Camera intrinsics after the pre-processing of the config (resize to crop_size, then crop_edge): (H, W, fx, fy, cx, cy)."""
    H, W, fx, fy, cx, cy = cfg['cam']['H'], cfg['cam']['W'], cfg['cam']['fx'], cfg['cam']['fy'], cfg['cam']['cx'], cfg['cam']['cy']
    if 'crop_size' in cfg['cam']:
        crop_size = cfg['cam']['crop_size']
        sx = crop_size[1] / W
        sy = crop_size[0] / H
        fx = sx * fx
        fy = sy * fy
        cx = sx * cx
        cy = sy * cy
        W = crop_size[1]
        H = crop_size[0]
    if cfg['cam']['crop_edge'] > 0:
        H -= cfg['cam']['crop_edge'] * 2
        W -= cfg['cam']['crop_edge'] * 2
        cx -= cfg['cam']['crop_edge']
        cy -= cfg['cam']['crop_edge']
    return H, W, fx, fy, cx, cy


def update_recursive(dict1, dict2):
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def load_config(path, default_path=None):
    """src/config.py's load_config with yaml alone: `inherit_from` first (recursively), else default_path, then the file itself
    merged over it key by key."""
    with open(path, 'r') as f:
        cfg_special = yaml.full_load(f)
    inherit_from = cfg_special.get('inherit_from')
    if inherit_from is not None:
        cfg = load_config(inherit_from, default_path)
    elif default_path is not None:
        with open(default_path, 'r') as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    update_recursive(cfg, cfg_special)
    return cfg


def _stem_key(path):
    return int(os.path.basename(path)[:-4])


def scannet_poses(input_folder, scale):
    """(number of frames, f32 poses) of a ScanNet scene as the reference's ScanNet dataset yields them: frames = the count of
    frames/color/*.jpg; each frames/pose/*.txt (sorted by integer stem) read in f64, columns 1 and 2 negated, rounded to f32, the
    translation multiplied by scale in f32.  No image is read."""
    folder = os.path.join(input_folder, 'frames')
    n_img = len(glob.glob(os.path.join(folder, 'color', '*.jpg')))
    poses = []
    for p in sorted(glob.glob(os.path.join(folder, 'pose', '*.txt')), key=_stem_key):
        with open(p, 'r') as f:
            c2w = np.array([list(map(float, line.split(' '))) for line in f.readlines()]).reshape(4, 4)
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        c2w = c2w.astype(np.float32)
        c2w[:3, 3] *= np.float32(scale)
        poses.append(c2w)
    return n_img, poses


def get_pose(cfg, args):
    """Every FRAME_SPACE-th ground-truth pose (f32 [4,4], OpenCV axes: the dataset's negation of columns 1 and 2 undone) whose
    matrix holds SOME finite entry (the reference's np.isfinite(c2w).any()), the intrinsic matrix K, H and W."""
    scale = cfg['scale']
    H, W, fx, fy, cx, cy = update_cam(cfg)
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)
    if cfg['dataset'] != 'scannet':
        raise NotImplementedError(f"get_pose: dataset {cfg['dataset']!r} (only 'scannet' is read without its images)")
    input_folder = args.input_folder if getattr(args, 'input_folder', None) is not None else cfg['data']['input_folder']
    n_img, poses = scannet_poses(input_folder, scale)
    pose_ls = []
    for idx in range(n_img):
        if idx % FRAME_SPACE != 0:
            continue
        c2w = poses[idx].copy()
        if np.isfinite(c2w).any():
            c2w[:3, 1] *= -1.0
            c2w[:3, 2] *= -1.0
            pose_ls.append(c2w)
    return pose_ls, K, H, W


class RefusedMesh(object):
    """What refuse() returns: vertices f32 [V,3] and faces int32 [F,3] device tensors of the extracted surface."""

    def __init__(self, vertices, faces):
        self.vertices = vertices
        self.faces = faces


def refuse(mesh, poses, K, H, W, cfg):
    """Render `mesh` (vertices, faces; its faces inverted, as the reference's mesh.invert() leaves them before this call) with back
    faces culled from each pose, fuse the depths (cut at DEPTH_TRUNC) into a dense box of units, and extract the observed surface.
    Returns a RefusedMesh on the device."""
    return refuse_chunked(mesh, poses, K, cfg)


def refuse_chunked(mesh, poses, K, cfg, chunk=None, leaf=None, timings=None):
    """refuse() with the views per integration chunk (default refusion.chunk_views), the BVH leaf size, and optionally a dict that
    collects per-stage device times in ms (render, touch, integrate, extract)."""
    H, W, fx, fy, cx, cy = update_cam(cfg)
    verts = np.asarray(mesh.vertices, np.float64)
    faces = np.asarray(mesh.faces, np.int64)
    dev = recon.device_of()
    bvh = raycast.MeshBVH(verts, faces, dev, **({'leaf': leaf} if leaf else {}))
    box = refusion.UnitBox.around(verts, VOXEL, SDF_TRUNC)
    tsdf = torch.zeros(box.shape, dtype=torch.float32, device=dev)
    weight = torch.zeros(box.shape, dtype=torch.float32, device=dev)
    outside = torch.zeros(1, dtype=torch.int32, device=dev)
    w2c_all = refusion.w2c_rows(poses)
    bp_all = refusion.backproject_rows(w2c_all)
    K = np.asarray(K, np.float64)
    kfx, kfy, kcx, kcy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    step = chunk or refusion.chunk_views(H, W)

    def lap(name, t0):
        if timings is None:
            return None
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if t0 is not None:
            timings[name] = timings.get(name, 0.0) + (t1 - t0) * 1e3
        return t1

    t = lap(None, None)
    for p0 in range(0, len(poses), step):
        c2w = np.stack([np.asarray(p, np.float64) for p in poses[p0:p0 + step]])
        depth = bvh.render_depth(c2w, H, W, kfx, kfy, kcx - PIXEL_CENTRE, kcy - PIXEL_CENTRE, ZNEAR, DEPTH_TRUNC, cull='back')
        t = lap('render', t)
        bp = torch.from_numpy(bp_all[p0:p0 + step]).to(dev).contiguous()
        touched = refusion.touch(depth, bp, box, fx, fy, cx, cy, DEPTH_STRIDE, DEPTH_TRUNC, SDF_TRUNC, outside)
        units = torch.nonzero(touched.any(0)).reshape(-1).to(torch.int32).contiguous()
        w2c = torch.from_numpy(w2c_all[p0:p0 + step]).to(dev).contiguous()
        t = lap('touch', t)
        refusion.integrate(tsdf, weight, box, units, depth, w2c, touched, fx, fy, cx, cy, SDF_TRUNC, DEPTH_TRUNC)
        t = lap('integrate', t)
        if timings is not None:
            timings['voxel_view_updates'] = timings.get('voxel_view_updates', 0) + int(touched.sum().item()) * UNIT_VOXELS
            timings['units_listed'] = timings.get('units_listed', 0) + int(units.numel())
    if int(outside.item()) != 0:
        raise RuntimeError(f'refuse: {int(outside.item())} depth points touched units outside the box')
    t = lap(None, None)
    v, f = refusion.extract(tsdf, weight, box)
    lap('extract', t)
    return RefusedMesh(v, f)


class LoadedMesh(object):
    """vertices f64 [V,3] and faces [F,3] as trimesh.load(process=True) hands them on, as we read it: only vertices some face
    references, exact-duplicate positions merged into their first occurrence (trimesh rounds before merging; we do not)."""

    def __init__(self, verts, faces):
        v = np.asarray(verts, np.float64).reshape(-1, 3)
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        ref = np.zeros(len(v), bool)
        ok = ((f >= 0) & (f < len(v))).all(1)
        f = f[ok]
        ref[f.reshape(-1)] = True
        keep = np.nonzero(ref)[0]
        uniq, first, inv = np.unique(v[keep], axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first, kind='stable')                  # merged vertices in order of first occurrence
        rank = np.empty(len(order), np.int64)
        rank[order] = np.arange(len(order))
        remap = np.full(len(v), -1, np.int64)
        remap[keep] = rank[inv.reshape(-1)]
        self.vertices = uniq[order]
        self.faces = remap[f]


def load_mesh(path):
    """A .ply or .obj mesh file as LoadedMesh."""
    m = _mesh.read_obj(path) if path.lower().endswith('.obj') else _mesh.read_ply(path)
    return LoadedMesh(m.verts, m.faces)


def _require(path, what):
    if not os.path.isfile(path):
        sys.stderr.write(f'evaluate_scannet: {what} {path} does not exist\n')
        raise SystemExit(2)


def evaluate_mesh():
    """The reference's command line: refuse the predicted mesh, write it, read it back and print the metrics (also returned)."""
    parser = argparse.ArgumentParser(description='Arguments for running the code.')
    parser.add_argument('config', type=str, help='Path to config file.')
    parser.add_argument('--input_folder', type=str,
                        help='input folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--output', type=str,
                        help='output folder, this have higher priority, can overwrite the one in config file')
    parser.add_argument('--space', type=int, default=10, help='the space between frames to integrate into the TSDF volume.')
    parser.add_argument('--rec_mesh', type=str, help='predicted mesh (default: the reference\'s final_mesh.ply path)')
    parser.add_argument('--gt_mesh', type=str, help='ground-truth mesh (default: the reference\'s GTmesh_lowres path)')
    parser.add_argument('--out_mesh', type=str, help='refused mesh to write (default: final_mesh_refused.ply next to the input)')
    args = parser.parse_args()
    _require(args.config, 'config')
    cfg = load_config(args.config, 'configs/df_prior.yaml')
    scene_id = cfg['data']['id']
    input_file = args.rec_mesh or f"output/scannet/scans/scene{scene_id:04d}_00/mesh/final_mesh.ply"
    out_mesh_path = args.out_mesh or f"output/scannet/scans/scene{scene_id:04d}_00/mesh/final_mesh_refused.ply"
    gt_path = args.gt_mesh or os.path.join("./Datasets/scannet/GTmesh_lowres", f"{scene_id:04d}_00.obj")
    _require(input_file, 'predicted mesh')
    _require(gt_path, 'ground-truth mesh')
    m = load_mesh(input_file)
    m.faces = m.faces[:, ::-1].copy()                 # mesh.invert()
    poses, K, H, W = get_pose(cfg, args)
    refused = refuse(m, poses, K, H, W, cfg)
    _mesh.write_ply(out_mesh_path, refused.vertices, refused.faces)
    mesh_pred = load_mesh(out_mesh_path)
    gt_mesh = load_mesh(gt_path)
    metrics = evaluate(mesh_pred, gt_mesh)
    print(metrics)
    return metrics


if __name__ == "__main__":
    evaluate_mesh()
