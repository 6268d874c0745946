"""Make a mesh file smaller by vertex clustering, on the MI355X (what an open3d user does with simplify_vertex_clustering).

    python -m attentive_dfprior_amd.simplify_mesh IN.ply OUT.ply --voxel_size M [--contraction average|quadric] [--normals]

The mesh is read with mesh.read_ply (vertices rounded to float32), simplified by mesh.simplify_vertex_clustering on the device --
one vertex per occupied cell of an M-sized lattice, at the cell's average or placed by the quadric of its faces -- and written with
mesh.write_ply.  Vertex colours follow when the input has them (per-cell averages, an alpha channel is not kept); --normals
recomputes area-weighted vertex normals on the simplified mesh (mesh.vertex_normals) and writes them; input normals are not carried
over.  The rules are this package's own statement of vertex clustering (include/adfp.h, "mesh simplification"): open3d is not
installed here and its function was never run against this one.
"""
import argparse

import numpy as np
import torch

from . import mesh


def simplify_file(path_in, path_out, voxel_size, contraction='quadric', normals=False, device='cuda:0'):
    """Returns ((V, F) before, (V', F') after)."""
    m = mesh.read_ply(path_in)
    v = torch.from_numpy(m.verts.astype(np.float32)).to(device)
    f = torch.from_numpy(np.ascontiguousarray(m.faces).astype(np.int32)).reshape(-1, 3).to(device)
    c = torch.from_numpy(np.ascontiguousarray(m.colors[:, :3])).to(device) if m.colors is not None else None
    vo, fo, co = mesh.simplify_vertex_clustering(v, f, voxel_size, contraction=contraction, colors=c)
    no = mesh.vertex_normals(vo, fo) if normals else None
    mesh.write_ply(path_out, vo, fo, colors=co, normals=no)
    return (int(v.shape[0]), int(f.shape[0])), (int(vo.shape[0]), int(fo.shape[0]))


def main(argv=None):
    parser = argparse.ArgumentParser(description='Simplify a PLY mesh by vertex clustering on the GPU.')
    parser.add_argument('input_mesh', type=str, help='path to the mesh to simplify (.ply)')
    parser.add_argument('output_mesh', type=str, help='path to the simplified mesh (.ply)')
    parser.add_argument('--voxel_size', type=float, required=True, help='edge of a clustering cell, in the units of the mesh')
    parser.add_argument('--contraction', choices=sorted(mesh.SIMPLIFY_CONTRACTIONS), default='quadric',
                        help="where a cell's vertex goes: its vertices' average, or the quadric placement")
    parser.add_argument('--normals', action='store_true', help='write vertex normals recomputed on the simplified mesh')
    parser.add_argument('--device', type=str, default='cuda:0')
    args = parser.parse_args(argv)
    before, after = simplify_file(args.input_mesh, args.output_mesh, args.voxel_size, args.contraction, args.normals, args.device)
    print(f'{args.input_mesh}: {before[0]} vertices, {before[1]} faces')
    print(f'{args.output_mesh}: {after[0]} vertices, {after[1]} faces')
    return before, after


if __name__ == '__main__':
    main()
