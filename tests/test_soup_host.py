"""CPU: the triangle soups of tests/soup_meshes.py are as hard as they claim and the oracles agree on them, before any kernel
sees them: many hits along a ray, leaf boxes that cover everything, more copies of a triangle than a leaf holds; the culled oracle
against the plain one; and an independent f64 Moeller-Trumbore renderer (soup_meshes.mt_render) against the watertight oracle."""
import numpy as np
import pytest

import depth_ref as D
import refuse_ref as RF
import soup_meshes as S

SKIP_CAP = 0.01                                        # of the covered pixels of a view
MIN_COVERED = 0.05                                     # of a view's pixels, unless it looks away: no view is all but empty
MARGIN_CAP = 0.005                                     # of the in-frustum (pose, point) pairs
SOUP_VIEWS = [(name, k) for name in S.NAMES for k in range(len(S.views(name)))]
CULLED = ('uniform', 'sheets', 'coincident')           # the soups whose culled renders the GPU suite checks


def check_against_mt(name, v):
    """The oracle's image within 1e-9 x extent of the independent renderer's, outside the capped set of unsure pixels."""
    want = S.reference(name, v)
    tol = 1e-9 * S.extent(name)
    z, hits, _, unsure = S.mt_of(name, v)
    covered = want > 0
    skipped = int((unsure & covered).sum())
    assert skipped <= SKIP_CAP * int(covered.sum()), (name, v.kind, skipped, int(covered.sum()))
    sure = ~unsure
    assert np.array_equal(covered[sure], np.isfinite(z)[sure]), (name, v.kind, np.argwhere((covered != np.isfinite(z)) & sure)[:5])
    both = sure & covered
    # the oracle rounds to f32 at the end, and rounding is monotone: its value lies between the roundings of z -+ tol
    lo, hi = (z[both] - tol).astype(np.float32), (z[both] + tol).astype(np.float32)
    bad = (want[both] < lo) | (want[both] > hi)
    assert not bad.any(), (name, v.kind, int(bad.sum()), want[both][bad][:5], z[both][bad][:5])
    return z, hits, covered


@pytest.mark.parametrize('name,k', SOUP_VIEWS)
def test_oracle_agrees_with_moeller_trumbore(name, k):
    v = S.views(name)[k]
    _, hits, covered = check_against_mt(name, v)
    if v.kind == 'away':
        assert not covered.any()
    else:
        assert (~covered).any() and covered.sum() >= MIN_COVERED * covered.size, (name, v.kind, int(covered.sum()))
    if (name, v.kind) == ('uniform', 'inside'):
        assert (hits >= 4).mean() >= 0.5, float((hits >= 4).mean())            # not the room: four or more surfaces along most rays
    if name == 'sheets' and v.kind.startswith('normal'):
        assert hits.max() >= 60, int(hits.max())


def test_counts_views_see_the_first_faces():
    for n in S.COUNTS:
        name = 'counts:%d' % n
        verts, faces = S.mesh(name)
        assert len(faces) == n and S.in_range(verts, faces).all()
        assert np.array_equal(faces, S.mesh('counts:1025')[1][:n])
        for v in S.views(name):
            _, _, covered = check_against_mt(name, v)
            assert not covered.any() if v.kind == 'away' else covered.any() and (~covered).any(), (n, v.kind)


def test_soups_are_what_they_claim():
    verts, faces = S.mesh('uniform')
    bad = ~S.in_range(verts, faces)
    a, b, c = (verts[np.where(bad[:, None], 0, faces)[:, k]] for k in range(3))
    flat = np.linalg.norm(np.cross(b - a, c - a), axis=1) <= 1e-12
    assert len(faces) == 3020 and bad.sum() == 10 and (flat & ~bad).sum() == 10
    assert np.ptp(np.flatnonzero(bad | flat)) > 1000                            # sprinkled in, not in one place
    edge = np.linalg.norm(b - a, axis=1)[~bad & ~flat]
    assert edge.min() < 0.02 and edge.max() > 1.0

    verts, faces = S.mesh('giants_and_dust')
    tri = verts[faces]
    cen = tri.mean(1)
    lo, hi = tri.min(1), tri.max(1)
    holds = ((cen[None] >= lo[:, None]) & (cen[None] <= hi[:, None])).all(2).sum(1)
    assert len(faces) == 4008 and holds.max() > len(faces) / 2, int(holds.max())  # a leaf box that covers most of the soup
    lattice = np.floor((cen - cen.min(0)) / np.ptp(cen, 0) * 1024).clip(0, 1023).astype(np.int64) >> 7
    cells = np.unique(lattice, axis=0, return_counts=True)[1]
    assert np.sort(cells)[-20:].sum() > len(faces) / 2                           # most centroids in a few cells of an 8^3 lattice

    verts, faces = S.mesh('sheets')
    assert len(faces) == S.SHEETS * 32 and len(np.unique(verts[:, 2])) == S.SHEETS
    assert S.c2w_of(S.views('sheets')[3])[2][3] in verts[:, 2]                    # the in-plane camera lies exactly in a sheet

    verts, faces = S.mesh('coincident')
    copies = np.unique(np.sort(faces, 1), axis=0, return_counts=True)[1]
    assert len(copies) == 200 and copies.max() == 40 and copies.min() == 1 and (copies > 16).sum() > 50
    assert len(np.unique(faces, axis=0)) > 200                                   # rotated and reversed copies among them

    v0, f0 = S.mesh('uniform')
    v1, f1 = S.mesh('far_offset')
    assert np.array_equal(f0, f1) and np.array_equal(v1, v0 + S.OFFSET)
    for a, b in zip(S.views('uniform'), S.views('far_offset')):
        assert np.array_equal(S.c2w_of(b)[:3, :3], S.c2w_of(a)[:3, :3]) and a[2:] == b[2:]
        assert np.abs(S.c2w_of(b)[:3, 3] - S.c2w_of(a)[:3, 3] - S.OFFSET).max() < 1e-9


def test_views_cover_the_cases():
    for name in S.NAMES:
        vs = S.views(name)
        assert 3 <= len(vs) <= 5
        assert any(v.H % 16 and v.W % 16 and (v.H, v.W) != (48, 64) for v in vs)      # an odd image: partial tiles in both axes
        whole = [v for v in vs if v.cx == int(v.cx) and v.cy == int(v.cy)]
        assert whole and all((np.abs(S.c2w_of(v)[:3, :3]) == np.round(np.abs(S.c2w_of(v)[:3, :3]))).all() for v in whole)
        assert any(v.near == 1.0 and v.far == 2.5 for v in vs)
        for v in vs:
            R = S.c2w_of(v)[:3, :3]
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0


@pytest.mark.parametrize('name,k', [(name, k) for name, k in SOUP_VIEWS if name in CULLED])
def test_culled_oracle_agrees_with_the_plain_one(name, k):
    verts, faces = S.mesh(name)
    v = S.views(name)[k]
    none = S.reference(name, v)
    assert np.array_equal(RF.render_depth_cull(verts, faces, S.c2w_of(v), *S.camera(v), cull='none'), none)
    back, front = S.reference(name, v, 'back'), S.reference(name, v, 'front')
    nearest = np.minimum(np.where(back > 0, back, np.inf), np.where(front > 0, front, np.inf))
    assert np.array_equal(np.where(np.isfinite(nearest), nearest, 0).astype(np.float32), none), (name, v.kind)
    assert np.array_equal(none == 0, (back == 0) & (front == 0))
    if v.kind != 'away':                                                         # both windings face every camera somewhere
        assert (back > 0).any() and (front > 0).any()
        assert name == 'coincident' or (back != front).any()                     # coincident: a reversed copy lies on most faces


@pytest.mark.parametrize('name', ['uniform', 'sheets'])
def test_visibility_fixture(name):
    """The points are what the GPU suite expects, both outcomes occur, and few decisions are marginal: a pair whose margin is at
    most 1e-12 x extent.  At eps = 0 a point ON the surface meets its own triangle at a margin of rounding size, so two thirds of
    the pairs are marginal by construction; the cap is checked there over the points that lie off the surface, and the GPU suite
    leaves no pair out of its comparison at either eps (kernel and oracle share every operation of the decision)."""
    pts = S.vis_points(name)
    n = len(S.views(name))
    assert len(pts) == 600 + 2 * n and len(S.vis_poses(name)) == 2 * n
    off_surface = np.arange(len(pts)) >= 400
    for eps in (0.03, 0.0):
        for near in (0.0, 0.5):
            fr, cl, mg = S.visible_reference(name, eps, near)
            assert fr.shape == (2 * n, len(pts))
            assert (fr & cl).any() and (fr & ~cl).any() and (~fr).any()
            marginal = fr & (mg <= 1e-12 * S.extent(name))
            if eps == 0.0:
                assert marginal[:, ~off_surface].sum() > 0.5 * fr[:, ~off_surface].sum()
                marginal, fr = marginal[:, off_surface], fr[:, off_surface]
            assert marginal.sum() <= MARGIN_CAP * fr.sum(), (name, eps, near, int(marginal.sum()), int(fr.sum()))
    a, b = S.visible_reference(name, 0.03, 0.0), S.visible_reference(name, 0.03, 0.5)
    assert (a[1] != b[1]).any()                                                  # near = 0.5 changes some decision
    seen = a[0] & a[1]
    for k in range(n):                                                           # no camera sees its own centre or the point behind it
        assert not seen[k, 600 + k] and not seen[k, 600 + n + k] and not seen[2 * n - 1 - k, 600 + k]
