"""CPU: the mesh simplification entries of the C ABI without a GPU -- the exports are bound in _lib's table, the version is what it
was, and every argument error of the contract (include/adfp.h, "mesh simplification") comes back as a negative code before any
launch."""
import ctypes as C

from attentive_dfprior_amd import _lib

NEW = ['adfp_mesh_simplify_workspace_bytes', 'adfp_mesh_simplify_plan', 'adfp_mesh_simplify_emit']
ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
TOO_MANY_VERTS = 2 ** 31 - 1024            # one above 2^31 - 1025
TOO_MANY_FACES = (2 ** 31 - 1025) // 3 + 1   # 3 F above 2^31 - 1025
d = C.c_void_p(16)                         # never dereferenced: every call below fails its host-side checks first
NAN, INF = float('nan'), float('inf')


def vec(*x):
    return C.byref((C.c_double * 3)(*x))


def test_exports_are_bound_and_version_is_unchanged():
    names = [n for n, _, _ in _lib.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1, n
    L = _lib.lib()
    for n in NEW:
        assert getattr(L, n) is not None
    assert L.adfp_version() == _lib.ABI_VERSION == 134
    assert _lib.SIMPLIFY == {'average': 0, 'quadric': 1}


def test_workspace_bytes():
    L = _lib.lib()
    wb = L.adfp_mesh_simplify_workspace_bytes
    assert wb(50, 100) > 0 and wb(50, 100) % 256 == 0
    assert wb(0, 100) == 0 and wb(50, 0) == 0 and wb(-1, 100) == 0 and wb(50, -1) == 0
    assert wb(TOO_MANY_VERTS, 100) == 0 and wb(50, TOO_MANY_FACES) == 0
    assert wb(TOO_MANY_VERTS - 1, 1) > 0 and wb(1, TOO_MANY_FACES - 1) > 0
    assert wb(51, 100) >= wb(50, 100) and wb(50, 200) > wb(50, 100)
    # it holds the compaction's workspace and the sort's table for the 3 F contributions
    assert wb(50, 100) > L.adfp_mesh_compact_workspace_bytes(50, 100) + L.adfp_sort_workspace_bytes(300)


def test_plan_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_simplify_workspace_bytes(50, 100)

    def plan(verts=d, nv=50, faces=d, nf=100, colors=None, vs=0.1, contraction=1, lo=vec(0, 0, 0), hi=vec(1, 1, 1), wsp=d, wsb=ws,
             totals=d):
        return L.adfp_mesh_simplify_plan(verts, nv, faces, nf, colors, vs, contraction, lo, hi, wsp, wsb, totals, None)
    assert plan(verts=None) == ARG
    assert plan(faces=None) == ARG
    assert plan(wsp=None) == ARG
    assert plan(totals=None) == ARG
    assert plan(lo=None) == ARG
    assert plan(hi=None) == ARG
    assert plan(nv=-1) == ARG
    assert plan(nf=-1) == ARG
    for bad in (0.0, -0.1, NAN, INF):
        assert plan(vs=bad) == ARG, bad
    assert plan(contraction=2) == ARG
    assert plan(contraction=-1) == ARG
    assert plan(lo=vec(0, NAN, 0)) == ARG
    assert plan(hi=vec(1, 1, INF)) == ARG
    assert plan(lo=vec(0, 2, 0)) == ARG                       # min_bound above max_bound
    assert plan(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert plan(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert plan(vs=1e-7) == UNSUPPORTED                       # 10^7 cells on an axis: more than 2^21
    assert plan(vs=1.0 / 2 ** 21, hi=vec(1, 0, 0)) == UNSUPPORTED       # floor(2^21 + 0.5) + 1 cells
    assert plan(wsb=ws - 1) == WORKSPACE
    assert plan(wsb=0) == WORKSPACE
    assert plan(colors=d, wsb=ws - 1) == WORKSPACE
    # bad arguments come before the empty mesh's shortcut
    assert plan(nv=0, vs=0.0) == ARG
    assert plan(nf=0, contraction=3) == ARG
    assert plan(nv=0, totals=None) == ARG


def test_empty_meshes_launch_nothing():
    """V = 0 or F = 0: no pointer but totals is looked at, no kernel runs -- the call only zeroes the two totals with a memset on
    the stream, so without a device it returns the runtime's own (positive) error or 0, never an ADFP_E_* code."""
    L = _lib.lib()
    for nv, nf in ((0, 100), (50, 0), (0, 0)):
        rc = L.adfp_mesh_simplify_plan(None, nv, None, nf, None, 0.1, 0, None, None, None, 0, d, None)
        assert rc >= 0, (nv, nf, rc)
    assert L.adfp_mesh_simplify_emit(0, 0, None, 0, None, None, 0, None, 0, None) == 0
    assert L.adfp_mesh_simplify_emit(50, 100, d, 0, None, None, 0, None, 0, None) == 0         # nothing survived: nothing to write


def test_emit_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_simplify_workspace_bytes(50, 100)

    def emit(nv=50, nf=100, wsp=d, wsb=ws, vo=d, co=None, nvo=10, fo=d, nfo=10):
        return L.adfp_mesh_simplify_emit(nv, nf, wsp, wsb, vo, co, nvo, fo, nfo, None)
    assert emit(wsp=None) == ARG
    assert emit(vo=None) == ARG
    assert emit(fo=None) == ARG
    assert emit(nv=-1) == ARG
    assert emit(nf=-1) == ARG
    assert emit(nvo=-1) == ARG
    assert emit(nfo=-1) == ARG
    assert emit(nvo=51) == ARG                                # more out than in
    assert emit(nfo=101) == ARG
    assert emit(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert emit(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert emit(wsb=ws - 1) == WORKSPACE
    assert emit(co=d, wsb=ws - 1) == WORKSPACE
