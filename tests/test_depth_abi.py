"""CPU: the mesh depth rendering entries of the C ABI without a GPU -- argument errors come back as negative codes before any
launch, empty inputs return 0 as include/adfp.h defines them, and the BVH and workspace sizes follow their formulas."""
import ctypes as C

from attentive_dfprior_amd import _lib

D = C.c_void_p(16)                                  # never dereferenced: every call below fails (or returns) before any launch
BIG = 2 ** 31


def al256(b):
    return (b + 255) // 256 * 256


def test_abi_version():
    assert _lib.ABI_VERSION == 134 == _lib.lib().adfp_version()
    assert _lib.TRI_LEAF_DEFAULT in _lib.TRI_LEAVES == (4, 8, 16)


def test_bvh_and_workspace_formulas():
    L = _lib.lib()
    for n in (1, 3, 4, 5, 16, 17, 1000, 1234567):
        for leaf in (4, 8, 16):
            leaves = -(-n // leaf)
            P = 1
            while P < leaves:
                P *= 2
            assert L.adfp_tri_bvh_bytes(n, leaf) == al256(72 * n) + al256(4 * n) + 96 * P
        assert L.adfp_tri_bvh_build_workspace_bytes(n) == al256(24 * n) + L.adfp_nn_build_workspace_bytes(n)
        for views in (1, 7):
            assert L.adfp_depth_l1_workspace_bytes(views, n) == 8 * views * min(max(-(-n // 256), 1), 1024)
    for leaf in (0, 2, 5, 32, -8):
        assert L.adfp_tri_bvh_bytes(100, leaf) == 0
    assert L.adfp_tri_bvh_bytes(0, 8) == 0 and L.adfp_tri_bvh_bytes(-1, 8) == 0 and L.adfp_tri_bvh_bytes(BIG, 8) == 0
    assert L.adfp_tri_bvh_build_workspace_bytes(0) == 0 and L.adfp_tri_bvh_build_workspace_bytes(BIG) == 0
    assert L.adfp_depth_l1_workspace_bytes(0, 100) == 0 and L.adfp_depth_l1_workspace_bytes(3, 0) == 8 * 3
    assert L.adfp_depth_l1_workspace_bytes(-1, 5) == 0 and L.adfp_depth_l1_workspace_bytes(2, BIG) == 0


def test_bvh_build_argument_errors():
    L = _lib.lib()
    bb, wb = L.adfp_tri_bvh_bytes(100, 8), L.adfp_tri_bvh_build_workspace_bytes(100)

    def b(v=D, nv=50, f=D, nf=100, leaf=8, bvh=D, bvhb=bb, ws=D, wsb=wb):
        return L.adfp_tri_bvh_build(v, nv, f, nf, leaf, bvh, bvhb, ws, wsb, None)
    assert b(v=None) == -1
    assert b(f=None) == -1
    assert b(bvh=None) == -1
    assert b(ws=None) == -1
    assert b(nv=-1) == -1
    assert b(nf=-1) == -1
    assert b(leaf=32) == -1
    assert b(nf=BIG) == -2
    assert b(bvhb=bb - 1) == -3
    assert b(wsb=wb - 1) == -3
    assert b(v=None, f=None, nf=0, bvh=None, bvhb=0, ws=None, wsb=0) == 0        # no faces: nothing to build


def test_render_argument_errors():
    L = _lib.lib()
    bb = L.adfp_tri_bvh_bytes(100, 8)

    def r(bvh=D, bvhb=bb, nf=100, leaf=8, c2w=D, near=D, far=20.0, views=3, H=64, W=48, fx=300.0, fy=300.0, cx=24.0, cy=32.0,
          depth=D):
        return L.adfp_render_depth(bvh, bvhb, nf, leaf, c2w, near, far, views, H, W, fx, fy, cx, cy, depth, None)
    assert r(bvh=None) == -1
    assert r(c2w=None) == -1
    assert r(near=None) == -1
    assert r(depth=None) == -1
    assert r(nf=-1) == -1
    assert r(views=-1) == -1
    assert r(leaf=12) == -1
    assert r(H=0) == -1 and r(W=-2) == -1
    assert r(far=0.0) == -1 and r(far=-1.0) == -1 and r(far=float('nan')) == -1 and r(far=float('inf')) == -1
    assert r(fx=0.0) == -1 and r(fy=float('nan')) == -1 and r(cx=float('inf')) == -1
    assert r(H=40000) == -2
    assert r(nf=BIG) == -2
    assert r(bvhb=bb - 1) == -3
    assert r(views=0, bvh=None, c2w=None, near=None, depth=None) == 0                 # no views: nothing to do


def test_views_in_sight_argument_errors():
    L = _lib.lib()

    def s(pts=D, n=10, w2c=D, poses=4, out=D):
        return L.adfp_views_in_sight(pts, n, w2c, poses, 300.0, 300.0, 249.5, 249.5, 500, 500, out, None)
    assert s(pts=None) == -1
    assert s(w2c=None) == -1
    assert s(out=None) == -1
    assert s(n=-1) == -1 and s(poses=-1) == -1
    assert s(n=BIG) == -2
    assert s(poses=0, pts=None, w2c=None, out=None) == 0                             # no poses: nothing to do


def test_depth_l1_argument_errors():
    L = _lib.lib()
    wb = L.adfp_depth_l1_workspace_bytes(3, 1000)

    def l1(a=D, b=D, views=3, n=1000, ws=D, wsb=wb, out=D):
        return L.adfp_depth_l1_sums(a, b, views, n, ws, wsb, out, None)
    assert l1(a=None) == -1 and l1(b=None) == -1 and l1(ws=None) == -1 and l1(out=None) == -1
    assert l1(views=-1) == -1 and l1(n=-1) == -1
    assert l1(n=BIG) == -2
    assert l1(wsb=wb - 1) == -3
    assert l1(views=0, a=None, b=None, ws=None, out=None) == 0
