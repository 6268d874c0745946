"""Recolour a mesh file of a finished run from the run's keyframes, on the MI355X: every vertex takes the colour the keyframes'
images show at it, wherever a keyframe's own depth image confirms that it sees the vertex.

    python -m attentive_dfprior_amd.color_mesh CONFIG --input_mesh M.ply [--ckpt PATH] [--output_mesh OUT.ply]
                                                      [--blend weighted|best] [--depth_tol M] [--border N] [--output ..]

The keyframes (colour, depth, estimated pose) are the ``keyframe_dict`` of a checkpoint, by default the newest under
{output}/ckpts; they go into a keyframes.KeyframeStore.  The mesh is read with mesh.read_ply; the run's meshes hold vertices
divided by the config's ``scale``, which is undone before the projection.  mesh.project_colors (include/adfp.h, "mesh colours from
the keyframes") does the work with the mesh's own vertex normals: --depth_tol is in the config's units (default
meshing.projection_depth_tol, else 0.05), --blend and --border default to meshing.projection_blend / projection_border.  A vertex
that no keyframe sees keeps the file's colour, or grey 128 if the file has none.  The output (default: the input's name with
_projected before .ply) has the input's vertices and faces; the covered share is printed."""
import argparse
import os

import numpy as np
import torch

from . import mesh
from .config import meshing_setting
from .keyframes import KeyframeStore

GREY = 128


def color_mesh_file(path_in, path_out, keyframe_dict, H, W, fx, fy, cx, cy, scale=1.0, depth_tol=0.05, border=0, blend='weighted',
                    device='cuda:0'):
    """Writes path_out and returns (covered vertices, vertices).  depth_tol is in the units of the keyframes' depth."""
    m = mesh.read_ply(path_in)
    file_verts = m.verts.astype(np.float32)
    v = torch.from_numpy(file_verts * np.float32(scale)).to(device)
    f = torch.from_numpy(np.ascontiguousarray(m.faces).astype(np.int32)).reshape(-1, 3).to(device)
    V = int(v.shape[0])
    if m.colors is not None:
        old = torch.from_numpy(np.ascontiguousarray(m.colors[:, :3])).to(device)
    else:
        old = torch.full((V, 3), GREY, dtype=torch.uint8, device=device)
    covered = 0
    colors = old
    if V and len(keyframe_dict):
        store = KeyframeStore.from_keyframe_dict(keyframe_dict, H, W, device)
        K = len(store)
        rgb, _, count, _ = mesh.project_colors(v, mesh.vertex_normals(v, f), store.depths(K), store.colors(K), store.poses(K), fx, fy, cx,
                                               cy, depth_tol, border, blend)
        seen = count > 0
        colors = torch.where(seen[:, None], mesh.color_bytes(rgb), old)
        covered = int(seen.sum())
    mesh.write_ply(path_out, file_verts, f, colors=colors)
    return covered, V


def main(argv=None):
    from .get_tsdf import load_config, update_cam
    from .render_eval import newest_checkpoint
    parser = argparse.ArgumentParser(description="Recolour a run's mesh from its keyframes' images on the GPU.")
    parser.add_argument('config', type=str, help='YAML config of the scene')
    parser.add_argument('--input_mesh', type=str, required=True, help='the mesh to recolour (.ply)')
    parser.add_argument('--ckpt', type=str, help='checkpoint file (default: the newest {output}/ckpts/*.tar)')
    parser.add_argument('--output_mesh', type=str, help='where the recoloured mesh goes (default: <input>_projected.ply)')
    parser.add_argument('--blend', choices=sorted(mesh.BLENDS), help="'weighted': every view by cos / depth^2; 'best': the best view alone")
    parser.add_argument('--depth_tol', type=float, help="how far a keyframe's depth may lie from the vertex, in the config's units")
    parser.add_argument('--border', type=int, help="pixels kept clear of the images' edge")
    parser.add_argument('--output', type=str, help="output directory of the run; replaces the config's data.output")
    parser.add_argument('--default_config', type=str, default='configs/df_prior.yaml', help='the config every other one inherits from')
    parser.add_argument('--device', type=str, default='cuda:0')
    args = parser.parse_args(argv)
    cfg = load_config(args.config, args.default_config if os.path.exists(args.default_config) else None)
    output = args.output or cfg['data']['output']
    ckpt = args.ckpt or newest_checkpoint(output)
    keyframe_dict = torch.load(ckpt, map_location='cpu', weights_only=False)['keyframe_dict']
    H, W, fx, fy, cx, cy = update_cam(cfg)
    scale = cfg['scale']
    tol = (args.depth_tol if args.depth_tol is not None else float(meshing_setting(cfg, 'projection_depth_tol'))) * scale
    blend = args.blend or meshing_setting(cfg, 'projection_blend')
    border = args.border if args.border is not None else int(meshing_setting(cfg, 'projection_border'))
    out = args.output_mesh or (os.path.splitext(args.input_mesh)[0] + '_projected.ply')
    covered, V = color_mesh_file(args.input_mesh, out, keyframe_dict, H, W, fx, fy, cx, cy, scale, tol, border, blend, args.device)
    print(f'{out}: {covered} of {V} vertices coloured from {len(keyframe_dict)} keyframes of {ckpt} ({100.0 * covered / max(V, 1):.1f} % covered)')
    return covered, V


if __name__ == '__main__':
    main()
