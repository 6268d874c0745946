"""CPU: adfp_mesh_project_colors of the C ABI without a GPU -- the export is bound in _lib's table, the version is what it was, and
every argument error of the contract (include/adfp.h, "mesh colours from the keyframes") comes back as a negative code before
any launch."""
import ctypes as C

from attentive_dfprior_amd import _lib

ARG, UNSUPPORTED = -1, -2
d = C.c_void_p(16)                         # never dereferenced: every call below fails its host-side checks first
NAN, INF = float('nan'), float('inf')


def call(verts=d, normals=d, nv=50, w2c=d, center=d, depth=d, color=d, K=4, fx=40.0, fy=40.0, cx=31.5, cy=23.5, W=64, H=48, tol=0.05,
         border=0, blend=0, rgb=d, wsum=d, count=d, best=d):
    return _lib.lib().adfp_mesh_project_colors(verts, normals, nv, w2c, center, depth, color, K, fx, fy, cx, cy, W, H, tol, border, blend,
                                               rgb, wsum, count, best, None)


def test_export_is_bound_and_version_is_unchanged():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert names.count('adfp_mesh_project_colors') == 1
    L = _lib.lib()
    assert L.adfp_mesh_project_colors is not None
    assert L.adfp_version() == _lib.ABI_VERSION == 134          # additive: the version stays
    assert _lib.BLEND == {'weighted': 0, 'best': 1}


def test_null_pointers():
    for name in ('verts', 'w2c', 'center', 'depth', 'color', 'rgb', 'wsum', 'count', 'best'):
        assert call(**{name: None}) == ARG, name
    # the keyframe arrays may be NULL only without keyframes; the outputs never
    for name in ('verts', 'rgb', 'wsum', 'count', 'best'):
        assert call(K=0, w2c=None, center=None, depth=None, color=None, **{name: None}) == ARG, name


def test_argument_errors():
    assert call(nv=-1) == ARG
    assert call(K=-1) == ARG
    for bad in (2, -1, 7):
        assert call(blend=bad) == ARG, bad
    for bad in (-0.01, NAN, INF, -INF):
        assert call(tol=bad) == ARG, bad
    assert call(border=-1) == ARG
    assert call(border=24) == ARG                             # 2 * 24 > min(64, 48) - 2
    assert call(W=13, H=9, border=4) == ARG                   # 8 > 7
    assert call(W=0) == ARG and call(H=0) == ARG and call(W=-5) == ARG
    # bad arguments come before the empty mesh's shortcut
    assert call(nv=0, blend=2) == ARG
    assert call(nv=0, tol=NAN) == ARG
    assert call(nv=0, border=24) == ARG
    assert call(nv=0, K=-1) == ARG


def test_unsupported():
    assert call(W=1) == UNSUPPORTED and call(H=1) == UNSUPPORTED
    assert call(W=32769) == UNSUPPORTED and call(H=32769) == UNSUPPORTED
    assert call(K=32769) == UNSUPPORTED
    assert call(nv=2 ** 31 - 1024) == UNSUPPORTED             # one above 2^31 - 1025
    # a null pointer is reported before a size that is not served
    assert call(W=1, rgb=None) == ARG


def test_mesher_settings_without_a_gpu():
    """The three projection_* keys: absent keys give the defaults, a config that names one wins, a wrong value is refused when
    the Mesher is built; the simplification defaults are what they were."""
    from types import SimpleNamespace
    import numpy as np
    import pytest
    from attentive_dfprior_amd import config, mesh, mesher
    assert config.MESHING_DEFAULTS == {'simplify_voxel_size': None, 'simplify_contraction': 'quadric'}
    assert config.PROJECTION_DEFAULTS == {'projection_depth_tol': 0.05, 'projection_blend': 'weighted', 'projection_border': 0}
    assert config.meshing_setting({}, 'projection_depth_tol') == 0.05 and config.meshing_setting({'meshing': None}, 'projection_blend') == 'weighted'
    assert config.meshing_setting({'meshing': {'projection_border': 3}}, 'projection_border') == 3
    assert config.meshing_setting({}, 'simplify_contraction') == 'quadric'
    assert mesher.COLOR_METHODS == ('direct_point_query', 'keyframe_projection') and mesh.BLENDS == _lib.BLEND

    def build(scale=1, **meshing):
        cfg = {'scale': scale, 'occupancy': True, 'mapping': {'marching_cubes_bound': [[0, 1]] * 3},
               'meshing': dict({'resolution': 16, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02, 'remove_small_geometry_threshold': 0.2,
                                'color_mesh_extraction_method': 'keyframe_projection', 'get_largest_components': False, 'depth_test': False},
                               **meshing)}
        slam = SimpleNamespace(renderer=None, bound=None, verbose=False, H=48, W=64, fx=40., fy=40., cx=31.5, cy=23.5, tsdf_bnds=None)
        return mesher.Mesher(cfg, None, slam)
    m = build()
    assert (m.projection_depth_tol, m.projection_blend, m.projection_border) == (0.05, 'weighted', 0)
    m = build(scale=2, projection_depth_tol=0.1, projection_blend='best', projection_border=2)
    assert np.isclose(m.projection_depth_tol, 0.2) and (m.projection_blend, m.projection_border) == ('best', 2)      # times `scale`
    for bad in (dict(projection_blend='mean'), dict(projection_depth_tol=-1.0), dict(projection_depth_tol=float('nan')), dict(projection_border=-1)):
        with pytest.raises(ValueError, match='projection'):
            build(**bad)


def test_no_vertices_launch_nothing():
    """V = 0 returns 0 whatever the pointers: nothing is looked at, no kernel runs."""
    L = _lib.lib()
    assert L.adfp_mesh_project_colors(None, None, 0, None, None, None, None, 4, 40.0, 40.0, 31.5, 23.5, 64, 48, 0.05, 0, 0, None, None, None,
                                      None, None) == 0
    assert call(nv=0, K=0) == 0 and call(nv=0, blend=1, border=23) == 0       # 2 * 23 = 46 = min(W, H) - 2: the last legal border
