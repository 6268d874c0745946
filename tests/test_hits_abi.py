"""CPU: the mesh-view entries of the C ABI without a GPU -- adfp_render_hits, adfp_vertex_normals and adfp_shade_hits return their
argument errors as negative codes before any launch, empty inputs return 0 as include/adfp.h defines them, and the vertex-normal
workspace follows its formula."""
import ctypes as C

from attentive_dfprior_amd import _lib

D = C.c_void_p(16)                                  # never dereferenced: every call below fails (or returns) before any launch
BIG = 2 ** 31
ALBEDO = (C.c_float * 3)(0.8, 0.8, 0.8)
BG = (C.c_ubyte * 3)(255, 255, 255)
NAN, INF = float('nan'), float('inf')


def al256(b):
    return (b + 255) // 256 * 256


def test_abi_version_and_symbols():
    assert _lib.ABI_VERSION == 134 == _lib.lib().adfp_version()          # additive: the version stays
    names = [n for n, _, _ in _lib.SYMBOLS]
    for n in ('adfp_render_hits', 'adfp_vertex_normals_workspace_bytes', 'adfp_vertex_normals', 'adfp_shade_hits'):
        assert n in names and hasattr(_lib.lib(), n)
    assert _lib.SHADE_MODE == {'color': 0, 'shaded': 1, 'normal': 2}


def test_render_hits_argument_errors():
    L = _lib.lib()
    bb = L.adfp_tri_bvh_bytes(100, 8)

    def r(bvh=D, bvhb=bb, nf=100, leaf=8, c2w=D, near=D, far=20.0, views=3, H=64, W=48, fx=300.0, fy=300.0, cx=24.0, cy=32.0,
          cull=0, depth=D, face=D, bary=D):
        return L.adfp_render_hits(bvh, bvhb, nf, leaf, c2w, near, far, views, H, W, fx, fy, cx, cy, cull, depth, face, bary, None)
    assert r(bvh=None) == -1
    assert r(c2w=None) == -1
    assert r(near=None) == -1
    assert r(depth=None, face=None, bary=None) == -1                      # all three outputs NULL
    assert r(nf=0, bvh=None, c2w=None, near=None, depth=None, face=None, bary=None) == -1
    assert r(nf=-1) == -1
    assert r(views=-1) == -1
    assert r(leaf=12) == -1
    assert r(H=0) == -1 and r(W=-2) == -1
    assert r(far=0.0) == -1 and r(far=-1.0) == -1 and r(far=NAN) == -1 and r(far=INF) == -1
    assert r(fx=0.0) == -1 and r(fy=NAN) == -1 and r(cx=INF) == -1
    assert r(cull=3) == -1 and r(cull=-1) == -1
    assert r(H=40000) == -2
    assert r(nf=BIG) == -2
    assert r(bvhb=bb - 1) == -3
    for cull in (0, 1, 2):
        assert r(views=0, bvh=None, c2w=None, near=None, depth=None, face=None, bary=None, cull=cull) == 0   # no views
    # the checks are adfp_render_depth_cull's, in its order: the same code for the same bad call
    def d(**kw):
        a = dict(bvh=D, bvhb=bb, nf=100, leaf=8, c2w=D, near=D, far=20.0, views=3, H=64, W=48, fx=300.0, fy=300.0, cx=24.0,
                 cy=32.0, cull=0)
        a.update(kw)
        return (L.adfp_render_depth_cull(*a.values(), D, None), L.adfp_render_hits(*a.values(), D, D, D, None))
    for kw in (dict(nf=-1, H=40000), dict(nf=BIG, bvhb=0), dict(cull=7, H=40000), dict(far=NAN, nf=BIG), dict(bvh=None, nf=BIG),
               dict(H=40000, bvhb=0)):
        a, b = d(**kw)
        assert a == b < 0, kw


def test_vertex_normals_workspace_and_errors():
    L = _lib.lib()
    for n in (1, 3, 1000, 1234567):
        assert L.adfp_vertex_normals_workspace_bytes(n) == al256(24 * n) + 4 * al256(12 * n) + al256(L.adfp_sort_workspace_bytes(3 * n))
    limit = (2 ** 31 - 1 - 1024) // 3                                    # 3 F within the int32 sort
    assert L.adfp_vertex_normals_workspace_bytes(limit) > 0 and L.adfp_vertex_normals_workspace_bytes(limit + 1) == 0
    assert L.adfp_vertex_normals_workspace_bytes(0) == 0 and L.adfp_vertex_normals_workspace_bytes(-1) == 0
    wb = L.adfp_vertex_normals_workspace_bytes(100)

    def n(v=D, nv=50, f=D, nf=100, ws=D, wsb=wb, out=D):
        return L.adfp_vertex_normals(v, nv, f, nf, ws, wsb, out, None)
    assert n(v=None) == -1 and n(f=None) == -1 and n(ws=None) == -1 and n(out=None) == -1
    assert n(nv=-1) == -1 and n(nf=-1) == -1
    assert n(nv=BIG) == -2
    assert n(nf=limit + 1, wsb=2 ** 40) == -2
    assert n(wsb=wb - 1) == -3
    assert n(nv=0, v=None, f=None, nf=0, ws=None, wsb=0, out=None) == 0   # no vertices: nothing to do
    assert n(nv=0) == 0


def test_shade_hits_argument_errors():
    L = _lib.lib()

    def s(face=D, bary=D, views=2, H=24, W=32, v=D, nv=50, f=D, nf=100, c2w=D, fx=40.0, fy=40.0, cx=15.5, cy=11.5, vn=D, vc=D,
          albedo=ALBEDO, ambient=0.3, bg=BG, mode=1, normal=D, rgb=D):
        return L.adfp_shade_hits(face, bary, views, H, W, v, nv, f, nf, c2w, fx, fy, cx, cy, vn, vc, albedo, ambient, bg, mode,
                                 normal, rgb, None)
    assert s(face=None) == -1 and s(bary=None) == -1 and s(c2w=None) == -1
    assert s(v=None) == -1 and s(f=None) == -1
    assert s(bg=None) == -1
    assert s(albedo=None, vc=None) == -1
    assert s(views=-1) == -1 and s(nv=-1) == -1 and s(nf=-1) == -1
    assert s(H=0) == -1 and s(W=-3) == -1
    assert s(mode=3) == -1 and s(mode=-1) == -1                          # a bad mode
    for bad in (-0.01, 1.01, NAN, INF, -INF):                             # ambient outside [0, 1] or not finite
        assert s(ambient=bad) == -1
    assert s(fx=0.0) == -1 and s(fy=NAN) == -1 and s(cx=INF) == -1 and s(cy=NAN) == -1
    assert s(H=40000) == -2
    assert s(nv=BIG) == -2 and s(nf=BIG) == -2 and s(views=BIG) == -2
    assert s(views=2 ** 30, H=32768, W=32768) == -2                       # more pixels than one grid takes
    assert s(views=0, face=None, bary=None, c2w=None, normal=None, rgb=None) == 0        # no views: nothing to do
    assert s(normal=None, rgb=None) == 0                                  # nothing asked for
    assert s(views=0, mode=9) == -1                                       # a bad mode is an error even with nothing to do
