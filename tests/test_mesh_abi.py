"""CPU: the mesh-extraction entries of the C ABI without a GPU -- the case table in the library equals the oracle's
independently built one, argument errors come back as negative codes before any launch, the workspace stays O(cells / tile) --
and mesh.write_ply round-trips."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as R
from attentive_dfprior_amd import _lib, mesh


def test_table_equals_oracle():
    L = _lib.lib()
    buf = (C.c_byte * (3 * _lib.MC_MAX_TRI))()
    assert R.MAX_TRI == _lib.MC_MAX_TRI
    for case in range(256):
        n = L.adfp_mc_table(case, buf)
        got = [tuple(buf[3 * m:3 * m + 3]) for m in range(n)]
        assert got == R.TABLE[case], case
        assert all(b == -1 for b in buf[3 * n:])
    assert L.adfp_mc_table(256, buf) == -1
    assert L.adfp_mc_table(-1, buf) == -1
    assert L.adfp_mc_table(0, None) == -1


def test_workspace_is_per_tile():
    L = _lib.lib()
    assert L.adfp_mc_workspace_bytes(512, 512, 512) <= 64 * 2 ** 20
    assert L.adfp_mc_workspace_bytes(1024, 1024, 1024) <= 64 * 2 ** 20
    assert L.adfp_mc_workspace_bytes(2, 2, 2) > 0
    assert L.adfp_mc_workspace_bytes(0, 2, 2) == 0


def test_argument_errors_need_no_gpu():
    L = _lib.lib()
    dummy = C.c_void_p(16)                         # never dereferenced: every call below fails its host-side checks first
    org = (C.c_float * 3)(0, 0, 0)
    sp = (C.c_float * 3)(1, 1, 1)
    ws = L.adfp_mc_workspace_bytes(4, 4, 4)
    assert L.adfp_mc_count(None, 4, 4, 4, 0.0, dummy, ws, dummy, None) == -1
    assert L.adfp_mc_count(dummy, 0, 4, 4, 0.0, dummy, ws, dummy, None) == -1
    assert L.adfp_mc_count(dummy, 4, 4, 4, 0.0, None, ws, dummy, None) == -1
    assert L.adfp_mc_count(dummy, 4, 4, 4, 0.0, dummy, ws, None, None) == -1
    assert L.adfp_mc_count(dummy, 4, 4, 4, 0.0, dummy, ws - 1, dummy, None) == -3

    def emit(values=dummy, nx=4, origin=org, outward=0, wsp=dummy, wsb=ws, nv=10, nf=10, verts=dummy, keys=dummy, vcap=10,
             faces=dummy, fcap=10):
        return L.adfp_mc_emit(values, nx, 4, 4, 0.0, origin, C.byref(sp), outward, wsp, wsb, nv, nf, verts, None, keys, vcap,
                              faces, fcap, None)
    assert emit(values=None) == -1
    assert emit(nx=-1) == -1
    assert emit(origin=None) == -1
    assert emit(outward=2) == -1
    assert emit(wsp=None) == -1
    assert emit(verts=None) == -1
    assert emit(keys=None) == -1
    assert emit(faces=None) == -1
    assert emit(nv=-1) == -1
    assert emit(wsb=ws - 1) == -3
    assert emit(vcap=9) == -3
    assert emit(fcap=9) == -3
    assert emit(nv=2 ** 31, vcap=2 ** 31) == -2
    assert emit(nv=0, nf=0, verts=None, keys=None, faces=None, vcap=0, fcap=0) == 0        # empty surface: nothing to launch

    assert L.adfp_lattice_hull_fill(None, dummy, dummy, dummy, 4, 4, 4, dummy, 1, 100.0, None) == -1
    assert L.adfp_lattice_hull_fill(dummy, None, dummy, dummy, 4, 4, 4, dummy, 1, 100.0, None) == -1
    assert L.adfp_lattice_hull_fill(dummy, dummy, dummy, dummy, 4, 0, 4, dummy, 1, 100.0, None) == -1
    assert L.adfp_lattice_hull_fill(dummy, dummy, dummy, dummy, 4, 4, 4, None, 1, 100.0, None) == -1
    assert L.adfp_lattice_hull_fill(dummy, dummy, dummy, dummy, 4, 4, 4, dummy, -1, 100.0, None) == -1
    assert L.adfp_lattice_hull_fill(dummy, dummy, dummy, dummy, 4, 4, 4, None, 0, 100.0, None) == 0
    assert L.adfp_mesh_unpack_colors(None, 5, dummy, 4, 4, 4, dummy, None) == -1
    assert L.adfp_mesh_unpack_colors(dummy, 5, None, 4, 4, 4, dummy, None) == -1
    assert L.adfp_mesh_unpack_colors(dummy, 5, dummy, 4, 4, 4, None, None) == -1
    assert L.adfp_mesh_unpack_colors(dummy, -1, dummy, 4, 4, 4, dummy, None) == -1
    assert L.adfp_mesh_unpack_colors(None, 0, dummy, 4, 4, 4, None, None) == 0


@pytest.mark.parametrize('ascii', [False, True])
def test_write_ply_round_trip(tmp_path, ascii):
    x = np.linspace(-1, 1, 12).astype(np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing='ij')
    v, f, n = R.marching_cubes((0.7 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), 0., normals=True)
    rng = np.random.default_rng(0)
    col = rng.integers(0, 256, size=(len(v), 3)).astype(np.uint8)
    p = tmp_path / ('m_ascii.ply' if ascii else 'm.ply')
    mesh.write_ply(str(p), v, f, colors=col, normals=n, ascii=ascii)
    rec, faces = R.read_ply(str(p))
    assert rec.dtype.names == ('x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue')
    got = np.stack([rec['x'], rec['y'], rec['z']], 1)
    gn = np.stack([rec['nx'], rec['ny'], rec['nz']], 1)
    tol = 1e-6 if ascii else 0                                      # ascii: '%f' (six decimals, as src/fusion.py:meshwrite)
    assert np.abs(got - v).max() <= tol
    assert np.abs(gn - n).max() <= tol
    assert (np.stack([rec['red'], rec['green'], rec['blue']], 1) == col).all()
    assert (faces == f).all()
    mesh.write_ply(str(p), v, f)                                     # geometry only
    rec, faces = R.read_ply(str(p))
    assert rec.dtype.names == ('x', 'y', 'z') and (faces == f).all()
