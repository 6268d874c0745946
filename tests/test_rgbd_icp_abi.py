"""CPU: the RGB-D ICP entries of the C ABI (adfp_rgbd_workspace_bytes, adfp_rgbd_frame_map, adfp_rgbd_step) return their error code
before any launch, as include/adfp.h states.  No GPU: nothing is dereferenced on an argument error, so any non-null aligned address
stands in for device memory; every call here is an error case, so nothing is ever launched (the suite also runs on machines with a
GPU)."""
from attentive_dfprior_amd import _lib

P = 4096                                         # any non-null, 16-byte aligned address
NAN = float('nan')
NAMES = ('adfp_rgbd_workspace_bytes', 'adfp_rgbd_frame_map', 'adfp_rgbd_step')


def test_symbols_and_constants():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert all(n in names for n in NAMES)
    assert (_lib.RGBD_SUMS, _lib.RGBD_STATS) == (31, 2)
    assert (_lib.ICP_SUMS, _lib.ICP_STATS, _lib.ICP_STATE_BYTES) == (29, 6, 272)
    assert _lib.lib().adfp_version() == _lib.ABI_VERSION              # additive: the version stays


def test_workspace_bytes():
    f, g = _lib.lib().adfp_rgbd_workspace_bytes, _lib.lib().adfp_icp_workspace_bytes
    assert f(0, 64) == 0 and f(48, 0) == 0 and f(-1, 64) == 0 and f(32769, 64) == 0 and f(48, 32769) == 0
    assert f(1, 1) == 31 * 8 and f(48, 64) == 12 * 31 * 8 and f(16, 16) == 31 * 8 and f(16, 17) == 2 * 31 * 8
    assert f(680, 1200) == 1024 * 31 * 8 == f(32768, 32768)
    for H, W in ((1, 1), (48, 64), (16, 17), (680, 1200)):            # the workgroups of the depth ICP's workspace
        assert f(H, W) * 29 == g(H, W) * 31


def frame_map(**kw):
    a = dict(color=P, depth=P, H=48, W=64, map=P, stream=None)
    a.update(kw)
    return _lib.lib().adfp_rgbd_frame_map(a['color'], a['depth'], a['H'], a['W'], a['map'], a['stream'])


def test_frame_map_argument_errors():
    for bad in (dict(color=None), dict(depth=None), dict(map=None), dict(H=0), dict(W=0), dict(W=-3), dict(map=P + 8), dict(map=P + 4)):
        assert frame_map(**bad) == -1, bad
    for bad in (dict(H=32769), dict(W=32769)):
        assert frame_map(**bad) == -2, bad


def step(**kw):
    a = dict(cur_map=P, normals_s=P, depth_m=P, normals_m=P, p_ref=P, key_map=P, p_key=P, H=48, W=64, fx=50.0, fy=50.0, cx=31.5, cy=23.5,
             stride=1, dist_tol=0.1, cos_tol=0.8, rgb_weight=1.0, rgb_tol=0.25, min_pivot=1e-6, min_pairs=100.0, state=P, stats=P,
             rgb_stats=P, stats_rows=4, row=0, sums=None, workspace=P, workspace_bytes=12 * 31 * 8, stream=None)
    a.update(kw)
    return _lib.lib().adfp_rgbd_step(a['cur_map'], a['normals_s'], a['depth_m'], a['normals_m'], a['p_ref'], a['key_map'], a['p_key'], a['H'],
                                     a['W'], a['fx'], a['fy'], a['cx'], a['cy'], a['stride'], a['dist_tol'], a['cos_tol'], a['rgb_weight'],
                                     a['rgb_tol'], a['min_pivot'], a['min_pairs'], a['state'], a['stats'], a['rgb_stats'], a['stats_rows'],
                                     a['row'], a['sums'], a['workspace'], a['workspace_bytes'], a['stream'])


def test_rgbd_step_argument_errors():
    for name in ('cur_map', 'normals_s', 'depth_m', 'normals_m', 'p_ref', 'state', 'stats', 'rgb_stats', 'workspace'):
        assert step(**{name: None}) == -1, name
    for bad in (dict(key_map=None), dict(p_key=None),                                        # both or neither
                dict(cur_map=P + 8), dict(key_map=P + 8), dict(cur_map=P + 4),                # maps: 16 bytes
                dict(rgb_weight=NAN), dict(rgb_weight=-1.0), dict(rgb_weight=-1e-300), dict(rgb_tol=NAN),
                dict(H=0), dict(W=0), dict(H=-1), dict(stride=0), dict(stride=-2), dict(dist_tol=NAN), dict(cos_tol=NAN), dict(min_pivot=NAN),
                dict(min_pairs=NAN), dict(fx=NAN), dict(fx=0.0), dict(cy=NAN), dict(workspace_bytes=12 * 31 * 8 - 1),
                dict(workspace_bytes=12 * 29 * 8), dict(workspace_bytes=0), dict(row=-1), dict(row=4), dict(stats_rows=0), dict(state=P + 4),
                dict(workspace=P + 4), dict(stats=P + 2), dict(rgb_stats=P + 4)):
        assert step(**bad) == -1, bad
    for bad in (dict(H=32769), dict(W=32769)):
        assert step(**bad) == -2, bad
    # the same checks with no keyframe given
    assert step(key_map=None, p_key=None, workspace_bytes=0) == -1 and step(key_map=None, p_key=None, H=32769) == -2
