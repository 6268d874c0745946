"""CPU: properties of the marching-cubes oracle (tests/mesh_ref.py) that the device kernel is later held to bit for bit:
closed, consistently oriented surfaces with the right topology, area and volume, and the edge cases of the conventions."""
import numpy as np
import pytest

import mesh_ref as R


def sphere(n=64, r=0.6):
    x = np.linspace(-1, 1, n).astype(np.float32)
    h = float(x[1] - x[0])
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    return (r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), h


@pytest.mark.parametrize('outward', ['lower', 'higher'])
def test_sphere_watertight_area_volume_orientation(outward):
    r = 0.6
    sdf, h = sphere(64, r)
    v, f, n = R.marching_cubes(sdf, 0., (h, h, h), (-1, -1, -1), normals=True, outward=outward)
    assert R.is_watertight_oriented(f)
    assert R.euler(v, f) == 2
    assert abs(R.area(v, f) / (4 * np.pi * r * r) - 1) < 0.01
    sgn = 1 if outward == 'lower' else -1                                       # inside = higher values = the ball
    assert abs(sgn * R.volume(v, f) / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
    fn = R.face_normals(v, f)
    cen = v[f].mean(1)
    assert (sgn * np.einsum('ij,ij->i', fn, cen) > 0).all()
    assert (sgn * np.einsum('ij,ij->i', n, v) > 0).all()


def test_torus_genus_one():
    n = 72
    x = np.linspace(-1, 1, n).astype(np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    q = np.sqrt(X * X + Y * Y) - 0.55
    sdf = (0.22 - np.sqrt(q * q + Z * Z)).astype(np.float32)
    v, f, _ = R.marching_cubes(sdf, 0.)
    assert R.is_watertight_oriented(f)
    assert R.euler(v, f) == 0


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_random_fields_watertight(seed):
    rng = np.random.default_rng(seed)
    f0 = rng.standard_normal((12, 13, 14)).astype(np.float32)
    f0[0], f0[-1], f0[:, 0], f0[:, -1], f0[:, :, 0], f0[:, :, -1] = -1, -1, -1, -1, -1, -1      # inside-free border
    for outward in ('lower', 'higher'):
        v, f, _ = R.marching_cubes(f0, 0.2, outward=outward)
        assert len(f) > 0
        # closed and oriented; a fan diagonal across an ambiguous face may be shared by the two cells (R.is_closed_oriented)
        assert R.is_closed_oriented(f)


def test_exactly_level_corners():
    rng = np.random.default_rng(5)
    v0 = rng.integers(-2, 3, size=(9, 10, 11)).astype(np.float32)
    v0[0], v0[-1], v0[:, 0], v0[:, -1], v0[:, :, 0], v0[:, :, -1] = -2, -2, -2, -2, -2, -2
    assert (v0 == 0).any()
    v, f, _ = R.marching_cubes(v0, 0.)
    assert R.is_closed_oriented(f)
    # a corner exactly at the level is outside: vertices land exactly on it (t = 0 or 1), several edges can give the same point
    on_lattice = (v == np.round(v)).all(1)
    assert on_lattice.any()
    assert len(np.unique(v, axis=0)) < len(v)


def test_nan_corner_emits_no_faces():
    v0 = -np.ones((2, 2, 2), np.float32)
    v0[0, 0, 0] = 1.0
    v, f, _ = R.marching_cubes(v0, 0.)
    assert len(f) == 1 and len(v) == 3
    v0[1, 1, 1] = np.nan
    v, f, _ = R.marching_cubes(v0, 0.)
    assert len(f) == 0
    assert len(v) == 3                                                          # the finite edges still carry their vertices
