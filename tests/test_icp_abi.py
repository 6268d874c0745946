"""CPU: the depth-ICP entries of the C ABI (adfp_depth_normals, adfp_icp_begin, adfp_icp_step, adfp_icp_end) return their error code
before any launch, as include/adfp.h states, and adfp_icp_workspace_bytes is 0 for a bad size.  No GPU: nothing is dereferenced on an
argument error, so any non-null aligned address stands in for device memory; every call here is an error case, so nothing is ever
launched (the suite also runs on machines with a GPU)."""
import ctypes as C

from attentive_dfprior_amd import _lib

P = 4096                                         # any non-null, 8-byte aligned address
NAN = float('nan')
NAMES = ('adfp_icp_workspace_bytes', 'adfp_depth_normals', 'adfp_icp_begin', 'adfp_icp_step', 'adfp_icp_end')


def test_symbols_and_constants():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert all(n in names for n in NAMES)
    assert (_lib.ICP_SUMS, _lib.ICP_STATS, _lib.ICP_STATE_BYTES) == (29, 6, 272)
    assert _lib.ICP_STATUS == {'ok': 0, 'few_pairs': 1, 'degenerate': 2, 'rejected': 3}
    assert _lib.lib().adfp_version() == _lib.ABI_VERSION              # additive: the version stays


def test_workspace_bytes():
    f = _lib.lib().adfp_icp_workspace_bytes
    assert f(0, 64) == 0 and f(48, 0) == 0 and f(-1, 64) == 0 and f(32769, 64) == 0 and f(48, 32769) == 0
    assert f(1, 1) == 29 * 8 and f(48, 64) == 12 * 29 * 8 and f(16, 16) == 29 * 8 and f(16, 17) == 2 * 29 * 8
    assert f(680, 1200) == 1024 * 29 * 8 == f(32768, 32768)           # capped: the grid is sized to the compute units


def normals(**kw):
    a = dict(depth=P, V=2, H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5, max_jump=0.0, normals=P, stream=None)
    a.update(kw)
    return _lib.lib().adfp_depth_normals(a['depth'], a['V'], a['H'], a['W'], a['fx'], a['fy'], a['cx'], a['cy'], a['max_jump'], a['normals'], a['stream'])


def test_depth_normals_argument_errors():
    for bad in (dict(depth=None), dict(normals=None), dict(V=0), dict(H=0), dict(W=0), dict(W=-3), dict(fx=NAN), dict(fy=0.0), dict(cx=NAN),
                dict(cy=NAN), dict(max_jump=NAN)):
        assert normals(**bad) == -1, bad
    for bad in (dict(H=32769), dict(W=32769), dict(V=65536)):
        assert normals(**bad) == -2, bad


def step(**kw):
    a = dict(depth_s=P, normals_s=P, depth_m=P, normals_m=P, p_ref=P, H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5, stride=1, dist_tol=0.1,
             cos_tol=0.8, min_pivot=1e-6, min_pairs=100.0, state=P, stats=P, stats_rows=4, row=0, sums=None, workspace=P,
             workspace_bytes=12 * 29 * 8, stream=None)
    a.update(kw)
    return _lib.lib().adfp_icp_step(a['depth_s'], a['normals_s'], a['depth_m'], a['normals_m'], a['p_ref'], a['H'], a['W'], a['fx'], a['fy'],
                                    a['cx'], a['cy'], a['stride'], a['dist_tol'], a['cos_tol'], a['min_pivot'], a['min_pairs'], a['state'],
                                    a['stats'], a['stats_rows'], a['row'], a['sums'], a['workspace'], a['workspace_bytes'], a['stream'])


def test_icp_step_argument_errors():
    for name in ('depth_s', 'normals_s', 'depth_m', 'normals_m', 'p_ref', 'state', 'stats', 'workspace'):
        assert step(**{name: None}) == -1, name
    for bad in (dict(H=0), dict(W=0), dict(H=-1), dict(stride=0), dict(stride=-2), dict(dist_tol=NAN), dict(cos_tol=NAN), dict(min_pivot=NAN),
                dict(min_pairs=NAN), dict(fx=NAN), dict(fx=0.0), dict(cy=NAN), dict(workspace_bytes=12 * 29 * 8 - 1), dict(workspace_bytes=0),
                dict(row=-1), dict(row=4), dict(stats_rows=0), dict(state=P + 4), dict(workspace=P + 4), dict(stats=P + 2)):
        assert step(**bad) == -1, bad
    for bad in (dict(H=32769), dict(W=32769)):
        assert step(**bad) == -2, bad


def test_icp_begin_and_end_argument_errors():
    L = _lib.lib()
    assert L.adfp_icp_begin(None, P, None) == -1 and L.adfp_icp_begin(P, None, None) == -1 and L.adfp_icp_begin(P, P + 4, None) == -1
    e = L.adfp_icp_end
    assert e(None, 0.5, 0.5, P, P, P, 4, 3, None) == -1 and e(P, 0.5, 0.5, None, P, P, 4, 3, None) == -1
    assert e(P, 0.5, 0.5, P, None, P, 4, 3, None) == -1 and e(P + 4, 0.5, 0.5, P, P, P, 4, 3, None) == -1
    assert e(P, NAN, 0.5, P, P, P, 4, 3, None) == -1 and e(P, 0.5, NAN, P, P, P, 4, 3, None) == -1
    assert e(P, 0.5, 0.5, P, P, P, 4, 4, None) == -1 and e(P, 0.5, 0.5, P, P, P, 4, -1, None) == -1 and e(P, 0.5, 0.5, P, P, P, 0, 0, None) == -1
