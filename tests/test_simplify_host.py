"""CPU: the properties of vertex clustering as include/adfp.h states it ("mesh simplification"), on the numpy oracle
tests/simplify_ref.py and hand-made meshes -- the statement the device kernels are compared against in tests/test_gpu_simplify.py
-- and the two config keys.  (The import of the package's names at the top is what ties this file to the feature: the oracle alone
would pass anywhere.)"""
import numpy as np
import pytest

import simplify_meshes as SM
import simplify_ref as R
from attentive_dfprior_amd import config
from attentive_dfprior_amd.mesh import SIMPLIFY_CONTRACTIONS


def test_contractions_are_the_packages():
    assert tuple(sorted(SIMPLIFY_CONTRACTIONS)) == tuple(sorted(R.CONTRACTIONS))
    assert SIMPLIFY_CONTRACTIONS == {'average': 0, 'quadric': 1}


@pytest.mark.parametrize('contraction', R.CONTRACTIONS)
def test_a_triangle_stays_a_triangle(contraction):
    v, f, vs = SM.triangle()
    vo, fo, co = R.simplify(v, f, vs, contraction)
    assert co is None and vo.dtype == np.float32 and fo.dtype == np.int32
    assert vo.shape == (3, 3) and fo.shape == (1, 3)
    # ascending key order: (0,0,0), (0,1,0), (1,0,0); the face starts at its smallest index and keeps its orientation
    assert np.array_equal(vo, v[[0, 2, 1]]) and fo.tolist() == [[0, 2, 1]]


def test_two_vertices_in_one_cell_collapse_the_face():
    v, f, vs = SM.collapsing()
    vo, fo, _ = R.simplify(v, f, vs, 'average')
    assert vo.shape == (3, 3) and fo.shape == (1, 3)
    merged = ((v[1].astype(np.float64) + v[2].astype(np.float64)) / 2).astype(np.float32)
    assert any(np.array_equal(row, merged) for row in vo)


def test_negative_coordinates_use_floor():
    v, f, vs = SM.negative_coordinates()
    _, cl, K = R.clusters(v, vs)
    assert cl[1] == cl[2] and cl[0] != cl[1] and K == 4


def test_a_boundary_vertex_belongs_to_the_upper_cell():
    v, f, vs = SM.boundary()
    _, cl, _ = R.clusters(v, vs)
    assert cl[0] == cl[1] and cl[2] == cl[3] and cl[1] != cl[2]


def test_corner_recovery():
    v, f, vs = SM.cube_corner()
    vq, fq, _, q = R.simplify(v, f, vs, 'quadric', detail=True)
    va, fa, _ = R.simplify(v, f, vs, 'average')
    assert np.array_equal(fq, fa) and vq.shape == (7, 3) and fq.shape == (3, 3)
    k = q['cl'][0]                                           # the corner's cluster holds every vertex of the three quads
    assert (q['cl'][:48] == k).all() and q['ok'][k]
    corner = q['m'][k] + q['x'][k]
    assert np.abs(corner).max() <= 1e-12 * vs
    row = int(np.flatnonzero(q['used'] == k)[0])
    assert np.abs(vq[row]).max() <= 1e-12 * vs
    assert np.abs(va[row]).min() > 0.1 * vs                  # the average lies inside the octant, a third of a metre from every plane
    assert not R.ambiguous(v, f, vs).any()


def test_duplicate_faces_leave_the_earliest_and_opposite_orientations_both_stay():
    v, f, vs = SM.duplicates()
    vo, fo, _ = R.simplify(v, f, vs, 'average')
    assert vo.shape == (3, 3)
    assert fo.tolist() == [[0, 2, 1], [0, 1, 2]]             # face 0 and its reversal; faces 2 and 3 repeat face 0's triple


def test_a_cluster_whose_faces_collapsed_is_dropped():
    v, f, vs = SM.dropped_cluster()
    vo, fo, _, q = R.simplify(v, f, vs, 'average', detail=True)
    assert q['K'] == 5 and vo.shape == (4, 3) and fo.shape == (2, 3)
    assert 0 not in q['used'] and q['cl'][0] == 0            # the lowest key is the dropped one: every index moves down
    assert fo.min() == 0 and fo.max() == 3
    assert not any(np.array_equal(row, v[0]) for row in vo)


@pytest.mark.parametrize('contraction', R.CONTRACTIONS)
def test_a_voxel_larger_than_the_model_gives_nothing(contraction):
    v, f, _ = SM.cube_surface(n=5)
    vo, fo, co = R.simplify(v, f, 8.0, contraction, colors=SM.colours(len(v)))
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and co.shape == (0, 3)


def test_a_tiny_voxel_is_the_identity_in_key_order():
    v, f, _ = SM.uv_sphere(rings=8, segs=12)
    vs = 1e-4                                                # the edges are ~0.1; 10^4 cells per axis: keys beyond 31 bits
    p, cl, K = R.clusters(v, vs)
    assert K == len(v)
    order = np.argsort(cl)
    vo, fo, co = R.simplify(v, f, vs, 'average', colors=SM.colours(len(v)))
    assert np.array_equal(vo, v[order]) and np.array_equal(co, SM.colours(len(v))[order]) and len(fo) == len(f)
    # every face is its input face, re-indexed and rotated
    back = order[fo]
    assert all(sorted(a) == sorted(b) for a, b in zip(back.tolist(), f.tolist()))
    vq, fq, _ = R.simplify(v, f, vs, 'quadric')
    assert np.array_equal(fq, fo) and np.abs(vq - vo).max() <= 2.4e-7 * np.abs(v).max()


def test_colours_round_half_up():
    v, f, vs = SM.collapsing()
    c = np.array([[0, 0, 0], [1, 2, 255], [2, 5, 254], [9, 9, 9]], np.uint8)
    vo, fo, co = R.simplify(v, f, vs, 'average', colors=c)
    assert [2, 4, 255] in co.tolist()                        # (1 + 2) / 2 = 1.5 -> 2, 3.5 -> 4, 254.5 -> 255


def test_config_defaults_and_meshing_setting():
    assert config.MESHING_DEFAULTS == {'simplify_voxel_size': None, 'simplify_contraction': 'quadric'}
    assert config.meshing_setting({}, 'simplify_voxel_size') is None
    assert config.meshing_setting({'meshing': {'resolution': 256}}, 'simplify_contraction') == 'quadric'
    assert config.meshing_setting({'meshing': None}, 'simplify_voxel_size') is None
    cfg = {'meshing': {'simplify_voxel_size': 0.04, 'simplify_contraction': 'average'}}
    assert config.meshing_setting(cfg, 'simplify_voxel_size') == 0.04 and config.meshing_setting(cfg, 'simplify_contraction') == 'average'
    assert config.meshing_setting({'meshing': {'simplify_voxel_size': 0}}, 'simplify_voxel_size') == 0      # a named key wins
    with pytest.raises(KeyError):
        config.meshing_setting({}, 'resolution')             # the reference's keys have no default here
