"""CPU: the numpy statement of the keyframe-projection colour rule (tests/project_colors_ref.py; include/adfp.h, "mesh colours from
the keyframes") against itself -- f32 against f64 on the cube scene, against the analytic texture, and on the cases by
construction.  These are conditions the reference statement alone must meet before a kernel is held to it; the caps are the
issue's, not measurements of the kernel.  The statement itself gives: 39.5 % covered, 0.06 % ambiguous, equal counts and best
views in f32 and f64 on every vertex, largest f32-f64 colour difference 1.4e-7, largest texture error 0.0009."""
import functools

import numpy as np
import pytest

import project_colors_ref as R

TOL = 0.1


@functools.lru_cache(maxsize=None)
def scene():
    return R.cube_scene()


@functools.lru_cache(maxsize=None)
def statement(blend, dtype):
    return R.project_colors_ref(*R.scene_args(scene()), TOL, 0, blend, dtype)


def test_scene_shape():
    s = scene()
    assert s['verts'].shape == (3456, 3) and s['normals'].shape == (3456, 3)
    assert s['depth'].shape == (4, 48, 64) and s['color'].shape == (4, 48, 64, 3) and s['fx'] == s['fy'] == 40.0
    assert (s['depth'] == 0).sum() == 100 and (s['depth'] >= 0).all()
    t = np.sort(np.unique(s['verts'][:576, 1]))
    assert np.allclose(t, -1 + 2 * (np.arange(24) + 0.37) / 24)
    assert (np.abs(s['verts']).max(1) == 1).all()                                   # on the walls
    assert ((s['verts'] * s['normals']).sum(1) == -1).all()                         # inward normals
    assert (np.abs(s['c2w'][:, :3, 3]) < 1).all()                                   # cameras inside


@pytest.mark.parametrize('blend', R.BLENDS)
def test_statement_f32_against_f64(blend):
    s = scene()
    rgb32, w32, n32, b32 = statement(blend, np.float32)
    rgb64, w64, n64, b64 = statement(blend, np.float64)
    covered = n64 > 0
    share = covered.mean()
    amb = R.ambiguity_mask(*R.scene_args(s), TOL, 0, blend)
    diff = np.abs(rgb32.astype(np.float64) - rgb64)[~amb].max()
    tex = np.abs(rgb64[covered] - R.texture(s['verts'][covered].astype(np.float64))).max()
    print(f'{blend}: covered {share:.4f}, ambiguous {amb.mean():.5f}, count differs at {(n32 != n64).sum()}, best at {(b32 != b64).sum()}, '
          f'f32-f64 colour {diff:.2e}, texture {tex:.4f}')
    assert 0.30 <= share <= 0.50
    assert amb.mean() <= 0.005
    assert (n32[~amb] == n64[~amb]).all() and (b32[~amb] == b64[~amb]).all()
    assert diff <= 2e-6
    assert tex <= 0.01
    assert (n64 >= 2).sum() >= 100                                                  # the blends have something to blend
    assert ((b64 >= 0) == covered).all() and (rgb64[~covered] == 0).all() and (w64[~covered] == 0).all()
    assert rgb32.dtype == np.float32 and w32.dtype == np.float32


def test_blends_differ_only_where_two_views_meet():
    (rw, ww, nw, bw), (rb, wb, nb, bb) = statement('weighted', np.float32), statement('best', np.float32)
    assert (nw == nb).all() and (bw == bb).all()
    one = nw == 1
    assert np.array_equal(rw[one], rb[one]) or np.abs(rw[one] - rb[one]).max() <= 2e-7     # (w c) / w rounds twice
    two = nw >= 2
    assert (ww[two] > wb[two]).all() and np.abs(rw[two] - rb[two]).max() < 0.01


def test_hole_drops_views():
    """The 10 x 10 block of zero depth: the vertices whose footprint touches it lose that keyframe."""
    s = scene()
    full = dict(s)
    full['depth'] = s['depth'].copy()
    k, r, c = R.SCENE_HOLE
    full['depth'][k] = R.render_cube(s['c2w'][k], s['H'], s['W'], s['fx'], s['fy'], s['cx'], s['cy'])[0]
    n_hole = statement('weighted', np.float32)[2]
    n_full = R.project_colors_ref(*R.scene_args(full), TOL, 0, 'weighted', np.float32)[2]
    lost = n_full - n_hole
    assert lost.min() == 0 and lost.max() == 1 and 2 <= lost.sum() <= 60


@pytest.mark.parametrize('blend', R.BLENDS)
@pytest.mark.parametrize('border', [0, 2])
@pytest.mark.parametrize('normals', [True, False])
def test_cases_by_construction(blend, border, normals):
    """In f32 only: zz = -2 + 1e-8 is -2 there, which is what puts the on-bound vertices exactly on their bounds."""
    s, dtype = R.constructed_scene(), np.float32
    rgb, wsum, count, best = R.project_colors_ref(*R.scene_args(s, normals='scene' if normals else None), R.CASE_TOL, border, blend, dtype)
    want = R.case_counts(border, normals)
    for i, case in enumerate(R.CASES):
        assert count[i] == want[i], (i, case[4], int(count[i]))
    assert (best == np.where(want > 0, 0, -1)).all()
    seen = want > 0
    assert (rgb[~seen] == 0).all() and (wsum[~seen] == 0).all()
    # the colour image is linear in the pixel: the bilinear sample is (u / 16, v / 12, 0.25)
    v = s['verts'][seen].astype(np.float64)
    u_px, v_px = 7.5 + 8.0 * v[:, 0] / -v[:, 2], 5.5 - 8.0 * v[:, 1] / -v[:, 2]
    assert np.abs(rgb[seen] - np.stack([u_px / 16, v_px / 12, np.full(len(v), 0.25)], 1)).max() <= 1e-6
    # weights: cos / z^2
    to = -v
    cos = np.abs(to[:, 2]) / np.linalg.norm(to, axis=1) if normals else np.ones(len(v))
    ok = np.isfinite(cos)
    assert np.allclose(wsum[seen][ok], (cos / v[:, 2] ** 2)[ok], rtol=1e-6)


@pytest.mark.parametrize('blend', R.BLENDS)
def test_two_identical_keyframes(blend):
    one, two = R.constructed_scene(1), R.constructed_scene(2)
    a = R.project_colors_ref(*R.scene_args(one), R.CASE_TOL, 0, blend)
    b = R.project_colors_ref(*R.scene_args(two), R.CASE_TOL, 0, blend)
    assert np.array_equal(a[0], b[0])                     # (w c + w c) / (w + w) = (w c) / w exactly: doubling is exact
    assert (b[2] == 2 * a[2]).all()
    assert (b[3] == a[3]).all() and set(b[3].tolist()) == {-1, 0}          # index 0 wins the tie
    assert np.array_equal(b[1], a[1] * (2 if blend == 'weighted' else 1))


@pytest.mark.parametrize('blend', R.BLENDS)
def test_no_keyframes_and_no_vertices(blend):
    s = R.constructed_scene()
    none = dict(s, w2c=s['w2c'][:0], center=s['center'][:0], depth=s['depth'][:0], color=s['color'][:0])
    rgb, wsum, count, best = R.project_colors_ref(*R.scene_args(none), R.CASE_TOL, 0, blend)
    V = len(s['verts'])
    assert rgb.shape == (V, 3) and not rgb.any() and not wsum.any() and not count.any() and (best == -1).all()
    rgb, wsum, count, best = R.project_colors_ref(*R.scene_args(s, verts=s['verts'][:0], normals=s['normals'][:0]), R.CASE_TOL, 0, blend)
    assert rgb.shape == (0, 3) and wsum.shape == count.shape == best.shape == (0,)
    assert R.ambiguity_mask(*R.scene_args(none), R.CASE_TOL, 0, blend).shape == (V,)
