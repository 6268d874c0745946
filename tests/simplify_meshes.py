"""Meshes of the simplification tests (tests/test_simplify_host.py on the oracle, tests/test_gpu_simplify.py on the device): numpy
(verts f32 [V,3], faces int32 [F,3]) and the voxel each is used with."""
import numpy as np


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def triangle():
    return _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32), 0.3


def collapsing():
    """vertices 1 and 2 share a cell of the 0.3 lattice: the face collapses"""
    return _f32([[0, 0, 0], [1, 0, 0], [1.02, 0.02, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 3]], np.int32), 0.3


def negative_coordinates():
    """x = -0.9, -0.1, 0.3 under voxel 1: vmin = -1.4, the cells are [-1.4, -0.4), [-0.4, 0.6): -0.1 shares 0.3's cell (floor of
    the offset from vmin); int(x / voxel), truncation toward zero, would put all three into one."""
    v = _f32([[-0.9, 0, 0], [-0.1, 0, 0], [0.3, 0, 0], [-0.9, 3, 0], [0.3, 3, 0]])
    return v, np.array([[0, 1, 3], [1, 2, 4], [0, 2, 4]], np.int32), 1.0


def boundary():
    """x = 0, 0.4, 0.5, 1.4 under voxel 1: vmin = -0.5, the boundary between cells 0 and 1 is x = 0.5 exactly"""
    v = _f32([[0, 0, 0], [0.4, 0, 0], [0.5, 0, 0], [1.4, 0, 0], [0, 3, 0]])
    return v, np.array([[0, 1, 4], [1, 2, 4], [2, 3, 4]], np.int32), 1.0


def cube_corner(n=4, h=0.25):
    """Three quads of the planes x = 0, y = 0, z = 0 meeting at the origin, each sampled at the points (i + 0.5) h, i < n, of
    its own plane (so no vertex lies at the corner or on an edge), triangulated; binary fractions, exact in f32.  With voxel
    2 n h the cell of the corner holds all of them."""
    t = (np.arange(n) + 0.5) * h
    a, b = np.meshgrid(t, t, indexing='ij')
    a, b, z = a.ravel(), b.ravel(), np.zeros(n * n)
    planes = [np.stack([z, a, b], 1), np.stack([b, z, a], 1), np.stack([a, b, z], 1)]
    quad = np.array([[i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j, (i + 1) * n + j + 1, i * n + j + 1]
                     for i in range(n - 1) for j in range(n - 1)]).reshape(-1, 3)
    faces = np.concatenate([quad + k * n * n for k in range(3)])
    # anchors far outside the corner's cell keep the corner's faces alive: every plane gets a fan to two outer vertices
    verts = np.concatenate(planes + [np.array([[0, 8., 8.], [8., 0, 8.], [8., 8., 0], [0, 8., -8.], [-8., 0, 8.], [8., -8., 0]])])
    base = 3 * n * n
    fans = np.array([[k * n * n, base + k, base + 3 + k] for k in range(3)])
    return _f32(verts), np.concatenate([faces, fans]).astype(np.int32), 2 * n * h


def duplicates():
    """faces 0 and 2 map to the same rotated triple (2 is a rotation of 0 through coincident-cell vertices); 1 is 0 reversed"""
    v = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.01, 0.01, 0], [1.01, 0.01, 0], [0.01, 1.01, 0]])
    return v, np.array([[0, 1, 2], [2, 1, 0], [4, 5, 3], [0, 4, 2]], np.int32), 0.3


def dropped_cluster():
    """cluster of vertex 0 (the lowest key) is used only by a face that collapses: it is dropped and the rest renumbered"""
    v = _f32([[-2, -2, -2], [1, 0, 0], [1.02, 0.01, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]])
    return v, np.array([[0, 1, 2], [1, 3, 4], [3, 5, 4]], np.int32), 0.3


def uv_sphere(rings=48, segs=96, radius=0.5, centre=(0.1, -0.2, 0.3)):
    """poles + (rings - 1) x segs vertices: 4 514 vertices, 9 024 faces at 48 x 96"""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2 * np.pi * np.arange(segs) / segs
    x = np.outer(np.sin(th), np.cos(ph)).ravel()
    y = np.outer(np.sin(th), np.sin(ph)).ravel()
    z = np.repeat(np.cos(th), segs)
    v = np.concatenate([[[0, 0, 1.]], np.stack([x, y, z], 1), [[0, 0, -1.]]]) * radius + np.asarray(centre)
    f = []
    last = 1 + (rings - 1) * segs
    for j in range(segs):
        f.append([0, 1 + j, 1 + (j + 1) % segs])
        f.append([last, 1 + (rings - 2) * segs + (j + 1) % segs, 1 + (rings - 2) * segs + j])
    for i in range(rings - 2):
        for j in range(segs):
            a, b = 1 + i * segs + j, 1 + i * segs + (j + 1) % segs
            c, d = a + segs, b + segs
            f += [[a, c, b], [b, c, d]]
    return _f32(v), np.asarray(f, np.int32), 0.06


def cube_surface(n=13, lo=(-0.3, 0.1, 0.2), hi=(0.7, 0.9, 1.3)):
    """every face of the box has its own n x n vertices (edge vertices are duplicated across faces): 1 014 vertices, 1 728 faces"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    t = np.linspace(0., 1., n)
    a, b = np.meshgrid(t, t, indexing='ij')
    a, b = a.ravel(), b.ravel()
    quad = np.array([[i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j, (i + 1) * n + j + 1, i * n + j + 1]
                     for i in range(n - 1) for j in range(n - 1)]).reshape(-1, 3)
    vs, fs = [], []
    for axis in range(3):
        for side in (0, 1):
            u = np.zeros((n * n, 3))
            u[:, axis] = side
            u[:, (axis + 1) % 3] = a
            u[:, (axis + 2) % 3] = b
            fs.append((quad if side else quad[:, ::-1]) + len(vs) * n * n)
            vs.append(lo + u * (hi - lo))
    return _f32(np.concatenate(vs)), np.concatenate(fs).astype(np.int32), 0.11


def colours(n, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.int64).astype(np.uint8)


HAND_MADE = {'triangle': triangle, 'collapsing': collapsing, 'negative_coordinates': negative_coordinates, 'boundary': boundary,
             'cube_corner': cube_corner,
             'duplicates': duplicates, 'dropped_cluster': dropped_cluster}
