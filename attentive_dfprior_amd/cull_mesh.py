"""Drop-in for the reference's src/tools/cull_mesh.py, on the MI355X.

The reference tests every vertex against every pose in a Python loop (cull_mesh.py:49-71: one projection and one device-to-host
copy per pose) and needs trimesh to load and save the mesh.  Here one launch tests every vertex against every pose
(adfp_cull_vertices, the poses staged through LDS), a second one marks the faces to keep (adfp_cull_faces), and mesh.read_ply /
mesh.write_ply do the files.  The arithmetic is the reference's, in f32: w2c = inv(c2w) (numpy: f64, rounded to f32),
cam = w2c [p, 1], cam.x *= -1, uv = K cam, z = uv.z + 1e-5, uv /= z, seen iff 0 <= -z and 0 < u < W and 0 < v < H.  A face is
dropped iff all three of its vertices are unseen in every pose.  Like trimesh's update_faces, the output keeps every vertex and
its properties and only the kept faces.

    python -m attentive_dfprior_amd.cull_mesh --input_mesh MESH.ply --traj traj.txt --output_mesh CULLED.ply [--remove_occlusion]

--remove_occlusion (not in the reference) is the occlusion-aware cull: a vertex counts as seen only where a pose also sees it
unoccluded by the mesh itself (visibility.points_visible), so a face behind a wall goes although it lies inside a frustum.
"""
import argparse

import numpy as np
import torch

from . import mesh, visibility
from .raycast import MeshBVH
from .recon import device_of, frustum_seen, faces_kept

H, W = 680, 1200                      # cull_mesh.py:31-37 (Replica)
FX, FY, CX, CY = 600.0, 600.0, 599.5, 339.5


def load_poses(path):
    """Camera-to-world poses of a Replica traj.txt (one row-major 4x4 per line), columns 1 and 2 negated, as float32 tensors
    (cull_mesh.py:9-19)."""
    poses = []
    with open(path, 'r') as f:
        lines = f.readlines()
    for line in lines:
        c2w = np.array(list(map(float, line.split()))).reshape(4, 4)
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        c2w = torch.from_numpy(c2w).float()
        poses.append(c2w)
    return poses


def cull_mesh(verts, faces, c2w_list, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, occlusion=False, eps=visibility.OCCLUSION_EPS):
    """Boolean numpy mask [F] of the faces to keep: a face goes iff none of its vertices lies in any pose's viewing frustum.
    occlusion=True (not in the reference): a vertex also has to be seen unoccluded by the mesh itself from such a pose, no face
    nearer to the camera than the vertex by more than `eps` metres (visibility.points_visible against the mesh's own BVH)."""
    dev = device_of(verts, faces)
    if occlusion:
        seen = visibility.points_visible(MeshBVH(verts, faces, dev), verts, c2w_list, H, W, fx, fy, cx, cy, eps=eps)
    else:
        seen = frustum_seen(verts, c2w_list, H, W, fx, fy, cx, cy, device=dev)
    return faces_kept(seen, faces).cpu().numpy().astype(bool)


_PLY_NAMES = {'i1': 'char', 'u1': 'uchar', 'i2': 'short', 'u2': 'ushort', 'i4': 'int', 'u4': 'uint', 'f4': 'float', 'f8': 'double'}


def _write_like(path, m, faces):
    """Binary little-endian PLY of every vertex of `m` with all its properties, in their types, and the triangles `faces`."""
    names = m.vertex.dtype.names
    dt = np.dtype([(n, '<' + m.vertex.dtype[n].str[1:]) for n in names])
    rec = np.empty(len(m.vertex), dtype=dt)
    for n in names:
        rec[n] = m.vertex[n]
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(rec)}']
    head += [f'property {_PLY_NAMES[dt[n].str[1:]]} {n}' for n in names]
    head += [f'element face {len(faces)}', 'property list uchar int vertex_indices', 'end_header']
    fr = np.empty(len(faces), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    fr['n'] = 3
    fr['i'] = faces
    with open(path, 'wb') as out:
        out.write(('\n'.join(head) + '\n').encode('ascii'))
        out.write(rec.tobytes())
        out.write(fr.tobytes())


def main(argv=None):
    parser = argparse.ArgumentParser(description='Arguments to cull the mesh.')
    parser.add_argument('--input_mesh', type=str, help='path to the mesh to be culled')
    parser.add_argument('--traj', type=str, help='path to the trajectory')
    parser.add_argument('--output_mesh', type=str, help='path to the output mesh')
    parser.add_argument('--remove_occlusion', action='store_true',
                        help='also drop faces whose vertices the mesh itself hides from every pose (not in the reference)')
    parser.add_argument('--eps', type=float, default=visibility.OCCLUSION_EPS, help='occlusion margin in metres')
    args = parser.parse_args(argv)
    poses = load_poses(args.traj)
    m = mesh.read_ply(args.input_mesh)
    keep = cull_mesh(m.verts, m.faces, poses, occlusion=args.remove_occlusion, eps=args.eps)
    _write_like(args.output_mesh, m, m.faces[keep])
    return keep


if __name__ == '__main__':
    main()
