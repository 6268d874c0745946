"""GPU: libadfp.so's marching cubes (adfp_mc_count / adfp_mc_emit through mesh.marching_cubes), hull fill and the TSDFVolume
mesh against the numpy oracle tests/mesh_ref.py: identical faces, vertices to 1e-6 of the extent, normals to 1e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_ref as R
from attentive_dfprior_amd import _lib, mesh, synthetic
from attentive_dfprior_amd.fusion import TSDFVolume

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def sphere(shape, r=0.6):
    axes = [np.linspace(-1, 1, n).astype(np.float32) for n in shape]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    return (r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), [float(a[1] - a[0]) for a in axes]


def random_field(shape, seed):
    f = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return f


def compare(values, level=0., spacing=(1., 1., 1.), origin=(0., 0., 0.), outward='lower'):
    v, f, n = mesh.marching_cubes(torch.from_numpy(values).to(DEV), level, spacing, origin, normals=True, outward=outward)
    rv, rf, rn = R.marching_cubes(values, level, spacing, origin, normals=True, outward=outward)
    v, f, n = v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(f, rf)
    if len(rv):
        extent = max(float(np.ptp(rv, 0).max()), 1e-30)
        assert np.abs(v - rv).max() <= 1e-6 * extent
        fin = np.isfinite(rn)                             # normals next to a non-finite value are non-finite on both sides
        assert np.array_equal(np.isfinite(n), fin)
        assert np.abs(n[fin] - rn[fin]).max(initial=0.0) <= 1e-5
    return v, f, n


@pytest.mark.parametrize('outward', ['lower', 'higher'])
def test_sphere(outward):
    s, h = sphere((64, 64, 64))
    v, f, _ = compare(s, 0., h, (-1, -1, -1), outward)
    assert R.is_watertight_oriented(f) and R.euler(v, f) == 2


@pytest.mark.parametrize('shape', [(2, 2, 2), (37, 64, 129), (21, 33, 70), (1, 5, 7), (5, 1, 3)])
@pytest.mark.parametrize('seed', [0, 1])
def test_random_fields(shape, seed):
    vals = random_field(shape, seed)
    compare(vals, 0.1, (0.5, 1.0, 2.0), (1.0, -2.0, 3.0), 'lower')
    compare(vals, -0.2, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), 'higher')


def test_all_inside_all_outside_and_nan():
    for fill in (1.0, -1.0):
        v, f, n = mesh.marching_cubes(torch.full((9, 10, 11), fill, device=DEV), 0., normals=True)
        assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)
    vals = random_field((12, 13, 14), 3)
    vals[4, 5, 6] = np.nan
    vals[7, 0, 2] = np.inf
    compare(vals, 0.0)


def test_exactly_level_corners():
    vals = np.random.default_rng(5).integers(-2, 3, size=(19, 20, 21)).astype(np.float32)
    compare(vals, 0.0)
    compare(vals, 1.0, outward='higher')


def test_bit_identical_runs():
    vals = torch.from_numpy(random_field((50, 60, 70), 7)).to(DEV)
    a = mesh.marching_cubes(vals, 0.3, normals=True)
    b = mesh.marching_cubes(vals, 0.3, normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_small_capacity_is_refused_and_nothing_is_written():
    vals = torch.from_numpy(random_field((16, 17, 18), 2)).to(DEV)
    X, Y, Z = vals.shape
    L = _lib.lib()
    nb = L.adfp_mc_workspace_bytes(X, Y, Z)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tot = torch.zeros(2, dtype=torch.int64, device=DEV)
    st = _lib.current_stream(torch.device(DEV))
    assert L.adfp_mc_count(_lib.ptr(vals), X, Y, Z, 0.0, _lib.ptr(ws), nb, _lib.ptr(tot), st) == 0
    nv, nf = tot.tolist()
    guard = 64
    verts = torch.full(((nv + guard) * 3,), 7.0, device=DEV)
    keys = torch.full((nv + guard,), -5, dtype=torch.int64, device=DEV)
    faces = torch.full(((nf + guard) * 3,), -9, dtype=torch.int32, device=DEV)
    org = (C.c_float * 3)(0, 0, 0)
    sp = (C.c_float * 3)(1, 1, 1)
    rc = L.adfp_mc_emit(_lib.ptr(vals), X, Y, Z, 0.0, C.byref(org), C.byref(sp), 0, _lib.ptr(ws), nb, nv, nf, _lib.ptr(verts), None,
                        _lib.ptr(keys), nv - 1, _lib.ptr(faces), nf, st)
    assert rc == -3
    rc = L.adfp_mc_emit(_lib.ptr(vals), X, Y, Z, 0.0, C.byref(org), C.byref(sp), 0, _lib.ptr(ws), nb, nv, nf, _lib.ptr(verts), None,
                        _lib.ptr(keys), nv, _lib.ptr(faces), nf - 1, st)
    assert rc == -3
    torch.cuda.synchronize()
    assert (verts == 7.0).all() and (keys == -5).all() and (faces == -9).all()
    rc = L.adfp_mc_emit(_lib.ptr(vals), X, Y, Z, 0.0, C.byref(org), C.byref(sp), 0, _lib.ptr(ws), nb, nv, nf, _lib.ptr(verts), None,
                        _lib.ptr(keys), nv, _lib.ptr(faces), nf, st)
    assert rc == 0
    torch.cuda.synchronize()
    assert (verts[3 * nv:] == 7.0).all() and (keys[nv:] == -5).all() and (faces[3 * nf:] == -9).all()
    rv, rf, _ = R.marching_cubes(vals.cpu().numpy(), 0.0)
    assert np.array_equal(faces[:3 * nf].cpu().numpy().reshape(-1, 3), rf)


def test_hull_fill():
    rng = np.random.default_rng(0)
    axes = [np.linspace(-1.05, 1.05, n).astype(np.float32) for n in (33, 40, 47)]
    pts = rng.standard_normal((60, 3))
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    from scipy.spatial import ConvexHull
    hull = ConvexHull(pts * 0.9)
    planes = hull.equations                                                              # [F,4]: n . p + d <= 0 inside
    vals = torch.zeros(tuple(len(a) for a in axes), device=DEV)
    mesh.hull_fill(vals, axes, planes, 100.)
    P = np.stack(np.meshgrid(*[a.astype(np.float64) for a in axes], indexing='ij'), -1).reshape(-1, 3)
    s = (P @ planes[:, :3].T + planes[:, 3]).max(1)
    ref = np.where(s > 0, 100.0, 0.0).reshape(vals.shape)
    got = vals.cpu().numpy()
    near = (np.abs(s) < 1e-9).reshape(vals.shape)
    assert ((got == ref) | near).all()
    assert (ref == 100).any() and (ref == 0).any()


def test_tsdf_volume_get_mesh():
    sc = synthetic.mini_scene(device=DEV)
    vol = TSDFVolume(sc.bound.numpy(), 0.04, device=DEV)
    for k in range(3):
        c2w = sc.default_c2w(offset=(0.05 * k, -0.04 * k, 0.02), yaw=0.9 * k, pitch=0.1 * k - 0.1)
        depth = sc.depth_image(c2w, zero_band=0.08).cpu().numpy().astype(np.float32)
        color = np.random.default_rng(k).integers(0, 256, size=(sc.H, sc.W, 3)).astype(np.uint8)
        pose = c2w.cpu().numpy().astype(np.float64).copy()
        pose[:3, 1] *= -1.0
        pose[:3, 2] *= -1.0
        K = np.array([[sc.fx, 0, sc.cx], [0, sc.fy, sc.cy], [0, 0, 1]], dtype=np.float64)
        vol.integrate(color, depth, K, pose, obs_weight=1.0)
    verts, faces, norms, colors = vol.get_mesh()
    tsdf, cvol, _ = vol.get_volume()
    rv, rf, rn = R.marching_cubes(tsdf, 0., normals=True, outward='higher')
    assert len(rf) > 100
    assert np.array_equal(faces, rf)
    world = rv * np.float32(vol._voxel_size) + vol._vol_origin
    assert np.abs(verts - world).max() <= 1e-6 * float(np.ptp(world, 0).max())
    assert np.abs(norms - rn).max() <= 1e-5
    # src/fusion.py:329-336 on the oracle's index-space vertices
    ind = np.round(rv).astype(int)
    rgb = cvol[ind[:, 0], ind[:, 1], ind[:, 2]]
    b = np.floor(rgb / 65536)
    g = np.floor((rgb - b * 65536) / 256)
    r = rgb - b * 65536 - g * 256
    ref_col = np.floor(np.asarray([r, g, b])).T.astype(np.uint8)
    assert np.array_equal(colors, ref_col)
    pc = vol.get_point_cloud()
    assert pc.shape == (len(verts), 6)
    assert np.array_equal(pc[:, 3:], ref_col.astype(pc.dtype))


def test_hull_fill_without_planes_and_unpack_colors_without_vertices():
    """max over no planes is not > 0: nothing is outside, nothing is filled.  No vertices: no colours."""
    vals = torch.arange(24, dtype=torch.float32, device=DEV).reshape(2, 3, 4).contiguous()
    before = vals.clone()
    axes = [np.linspace(0, 1, n, dtype=np.float32) for n in (2, 3, 4)]
    assert mesh.hull_fill(vals, axes, np.zeros((0, 4)), 100.) is vals and torch.equal(vals, before)
    out = mesh.unpack_colors(torch.zeros((0, 3), dtype=torch.float32, device=DEV), torch.zeros((2, 3, 4), dtype=torch.float32, device=DEV))
    assert out.shape == (0, 3) and out.dtype == torch.uint8
