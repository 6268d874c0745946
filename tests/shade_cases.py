"""The meshes, vertex colours and views of the shading tests (test_hits_host.py checks the oracle on them, test_gpu_mesh_shade.py
the kernels): two triangle soups of tests/soup_meshes.py and depth_ref's box room with a box standing in it, colours from a seeded
generator.  Chosen so that the shading oracle's half-integer mask stays within its cap (test_hits_host.py asserts it)."""
import collections
import functools

import numpy as np

import depth_ref as D
import soup_meshes as S

Case = collections.namedtuple('Case', 'label verts faces colors c2w cam')       # cam = (H, W, fx, fy, cx, cy, near, far)
AMBIENT = 0.3


def colors_of(n, seed):
    return S.frozen(np.random.default_rng(seed).integers(0, 256, (n, 3)).astype(np.uint8))


def rolled(c2w, angle):
    """The pose turned by `angle` about its own viewing axis.  depth_ref.viewmatrix keeps the camera's x axis horizontal, so a
    horizontal surface (a sheet, the room's floor) has a camera-space normal with x = 0 exactly, and the normal map's red channel
    sits on the half-integer 127.5 over the whole surface: the mask cap is a condition on the inputs, and a roll meets it."""
    m = np.array(c2w, np.float64)
    c, s = np.cos(angle), np.sin(angle)
    m[:3, :3] = m[:3, :3] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for seed, (name, k) in enumerate((('sheets', 2), ('uniform', 0))):           # obliquely between two clip planes; from inside
        verts, faces = S.mesh(name)
        v = S.views(name)[k]
        out.append(Case(name, verts, faces, colors_of(len(verts), 20250401 + seed), S.frozen(rolled(S.c2w_of(v), 0.3)), S.camera(v)))
    verts, faces = D.box_room(inner=((-0.6, -0.4, -1.2), (0.3, 0.5, 0.2)))
    c2w = rolled(S.look((1.0, 0.35, -0.25), (-1.5, -0.8, 0.6)), 0.2)
    out.append(Case('room', S.frozen(verts), S.frozen(faces), colors_of(len(verts), 20250403), S.frozen(c2w),
                    (24, 32, 20.0, 20.0, 15.5, 11.5, D.near_of(verts), 20.0)))
    return tuple(out)
