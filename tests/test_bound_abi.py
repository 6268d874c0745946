"""CPU: the mesh-bound entries of the C ABI without a GPU: argument errors come back as negative codes before any launch, the
workspaces stay small beside the depth block, and the ABI version is unchanged (the entries are additions)."""
import ctypes as C

from attentive_dfprior_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
DUMMY = C.c_void_p(16)                             # never dereferenced: every call below fails its host-side checks first


def scene(depth=DUMMY, poses=DUMMY, K=2, H=4, W=4, fx=5.0, fy=5.0, cx=1.5, cy=1.5):
    return (depth, poses, K, H, W, fx, fy, cx, cy)


def bad_scenes():
    nan, inf = float('nan'), float('inf')
    return [(scene(depth=None), ARG), (scene(poses=None), ARG), (scene(K=-1), ARG), (scene(H=0), ARG), (scene(W=0), ARG),
            (scene(fx=0.0), ARG), (scene(fy=nan), ARG), (scene(fx=inf), ARG), (scene(cx=nan), ARG), (scene(cy=inf), ARG),
            (scene(H=32769), UNSUPPORTED), (scene(K=2 ** 40), UNSUPPORTED)]


def test_version_is_unchanged():
    assert _lib.lib().adfp_version() == 134 == _lib.ABI_VERSION


def test_support_argument_errors_need_no_gpu():
    L = _lib.lib()
    ws = L.adfp_bound_support_workspace_bytes(2, 4, 4, 64)
    assert ws > 0

    def call(sc=scene(), dirs=DUMMY, D=64, wsp=DUMMY, wsb=ws, best=DUMMY, aabb=DUMMY, counts=DUMMY):
        return L.adfp_bound_support(*sc, dirs, D, wsp, wsb, best, aabb, counts, None)
    for sc, code in bad_scenes():
        assert call(sc=sc) == code, sc
    assert call(dirs=None) == ARG
    assert call(D=0) == ARG
    assert call(D=_lib.BOUND_MAX_DIRECTIONS + 1) == ARG
    assert call(wsp=None) == ARG
    assert call(best=None) == ARG
    assert call(aabb=None) == ARG
    assert call(counts=None) == ARG
    assert call(wsb=ws - 1) == WORKSPACE
    assert call(sc=scene(depth=None, poses=None, K=0), wsp=None, wsb=0) == 0          # no keyframes: nothing to launch
    assert L.adfp_bound_support_workspace_bytes(0, 4, 4, 64) == 0
    assert L.adfp_bound_support_workspace_bytes(2, 4, 4, 0) == 0
    # per-workgroup partials only: the ScanNet end of a run (1 000 keyframes of 480 x 640) at the largest D stays under 64 MiB
    assert L.adfp_bound_support_workspace_bytes(1000, 480, 640, _lib.BOUND_MAX_DIRECTIONS) <= 64 * 2 ** 20


def test_classify_argument_errors_need_no_gpu():
    L = _lib.lib()
    n_all = 2 * (4 * 4 + 1)
    ws = L.adfp_bound_classify_workspace_bytes(n_all)
    assert ws > 0

    def call(sc=scene(), ids=None, n=n_all, planes=DUMMY, F=8, eps=1e-12, wsp=DUMMY, wsb=ws, out=DUMMY, cap=n_all, count=DUMMY,
             far_id=DUMMY, far_dist=DUMMY):
        return L.adfp_bound_classify(*sc, ids, n, planes, F, eps, wsp, wsb, out, cap, count, far_id, far_dist, None)
    for sc, code in bad_scenes():
        assert call(sc=sc) == code, sc
    assert call(n=n_all - 1) == ARG                  # NULL ids mean ALL ids
    assert call(ids=DUMMY, n=-1) == ARG
    assert call(planes=None) == ARG
    assert call(F=0) == ARG
    assert call(eps=-1.0) == ARG
    assert call(eps=float('nan')) == ARG
    assert call(eps=float('inf')) == ARG
    assert call(wsp=None) == ARG
    assert call(out=None) == ARG
    assert call(cap=-1) == ARG
    assert call(count=None) == ARG
    assert call(far_id=None) == ARG
    assert call(far_dist=None) == ARG
    assert call(wsb=ws - 1) == WORKSPACE
    assert call(ids=DUMMY, n=2 ** 40 + 1, wsb=2 ** 50) == UNSUPPORTED
    assert L.adfp_bound_classify_workspace_bytes(0) == 0
    # one bit per candidate and 12 bytes per tile of 1024: 300 M candidates need under 64 MiB
    assert L.adfp_bound_classify_workspace_bytes(300 * 10 ** 6) <= 64 * 2 ** 20


def test_points_argument_errors_need_no_gpu():
    L = _lib.lib()

    def call(sc=scene(), ids=DUMMY, n=5, out=DUMMY):
        return L.adfp_bound_points(*sc, ids, n, out, None)
    for sc, code in bad_scenes():
        assert call(sc=sc) == code, sc
    assert call(ids=None) == ARG
    assert call(out=None) == ARG
    assert call(n=-1) == ARG
    assert call(n=2 ** 40 + 1) == UNSUPPORTED
    assert call(ids=None, out=None, n=0) == 0         # nothing to launch
