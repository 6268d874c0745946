"""CPU: adfp_points_visible of the C ABI without a GPU -- the symbol is exported and bound, argument errors come back as negative
codes before any launch, and the empty inputs that need no launch return 0 as include/adfp.h defines them."""
import ctypes as C
import math

from attentive_dfprior_amd import _lib

D = C.c_void_p(16)                                  # never dereferenced: every call below fails (or returns) before any launch
BIG = 2 ** 31


def test_symbol_is_exported_and_bound():
    assert 'adfp_points_visible' in [name for name, _, _ in _lib.SYMBOLS]
    fn = _lib.lib().adfp_points_visible
    assert fn.restype is C.c_int and len(fn.argtypes) == 19
    assert _lib.ABI_VERSION == 134 == _lib.lib().adfp_version()           # additive: the version stays


def test_points_visible_argument_errors():
    L = _lib.lib()
    bb = L.adfp_tri_bvh_bytes(100, 8)

    def pv(bvh=D, bvhb=bb, nf=100, leaf=8, pts=D, n=10, w2c=D, c2w=D, poses=4, fx=300.0, fy=300.0, near=0.0, eps=0.03, seen=D):
        return L.adfp_points_visible(bvh, bvhb, nf, leaf, pts, n, w2c, c2w, poses, fx, fy, 249.5, 249.5, 500, 500, near, eps, seen,
                                     None)
    for k in ('bvh', 'pts', 'w2c', 'c2w', 'seen'):
        assert pv(**{k: None}) == -1, k
    assert pv(nf=-1) == -1 and pv(n=-1) == -1 and pv(poses=-1) == -1
    assert pv(leaf=12) == -1 and pv(leaf=0) == -1
    assert pv(eps=-1e-9) == -1 and pv(eps=math.nan) == -1 and pv(eps=math.inf) == -1
    assert pv(near=-0.5) == -1 and pv(near=math.nan) == -1 and pv(near=math.inf) == -1
    assert pv(fx=0.0) == -1 and pv(fy=0.0) == -1
    assert pv(nf=0, bvh=None, bvhb=0, c2w=None, pts=None) == -1           # no faces: bvh and c2w may be null, the points may not
    assert pv(nf=0, bvh=None, bvhb=0, c2w=None, seen=None) == -1
    assert pv(nf=0, bvh=None, bvhb=0, c2w=None, w2c=None) == -1
    assert pv(n=BIG) == -2 and pv(nf=BIG) == -2 and pv(poses=BIG) == -2
    assert pv(bvhb=bb - 1) == -3


def test_points_visible_empty_inputs():
    L = _lib.lib()

    def pv(bvh, bvhb, nf, pts, n, w2c, c2w, poses, seen):
        return L.adfp_points_visible(bvh, bvhb, nf, 8, pts, n, w2c, c2w, poses, 300.0, 300.0, 249.5, 249.5, 500, 500, 0.0, 0.03,
                                     seen, None)
    assert pv(None, 0, 100, None, 0, None, None, 4, None) == 0             # no points: nothing to do, whatever else is null
    assert pv(None, 0, 0, None, 0, None, None, 0, None) == 0              # no points and no poses
    assert pv(None, 0, 100, None, 0, None, None, -1, None) == -1          # the counts are checked before that early return
