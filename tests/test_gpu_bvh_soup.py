"""GPU: the two ray walks over the triangle BVH (bvh_walk under RtNearest and RtAny in csrc/adfp_raycast.h) on the triangle soups of
tests/soup_meshes.py, against the brute-force numpy oracles bit for bit: triangles of every size, leaf boxes that cover the whole
soup, dozens of surfaces along a ray, more copies of a triangle than a leaf holds, zero-thickness boxes seen edge on, a soup
3 000 units from the origin, and face counts around every full and nearly empty last level.  On the room meshes of the other tests
the first box a ray enters nearly always holds the nearest hit; here a walk that prunes or orders wrongly shows.  What makes the
soups hard, and that the oracles agree on them, is checked on the CPU in tests/test_soup_host.py."""
import functools

import numpy as np
import pytest
import torch

import depth_ref as D
import soup_meshes as S
from attentive_dfprior_amd import _lib, raycast, visibility
from test_gpu_visible import CULL_CHUNK, perturbed

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEAVES = _lib.TRI_LEAVES
SOUP_VIEWS = [(name, k) for name in S.NAMES for k in range(len(S.views(name)))]
CULLED = [(name, k) for name, k in SOUP_VIEWS if name in ('uniform', 'sheets', 'coincident')]


@functools.lru_cache(maxsize=None)
def bvh_of(name, leaf):
    return raycast.MeshBVH(*S.mesh(name), DEV, leaf=leaf)


def render(bvh, v, cull='none'):
    """One view, twice: the same bits both times."""
    got = bvh.render_depth(S.c2w_of(v), *S.camera(v), cull=cull)
    assert torch.equal(got, bvh.render_depth(S.c2w_of(v), *S.camera(v), cull=cull))
    assert got.shape == (1, v.H, v.W) and got.dtype == torch.float32
    return got[0].cpu().numpy()


def same(got, want, *what):
    bad = got != want
    assert not bad.any(), what + (int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


@pytest.mark.parametrize('leaf', LEAVES)
@pytest.mark.parametrize('name,k', SOUP_VIEWS)
def test_depth_equals_oracle(name, k, leaf):
    v = S.views(name)[k]
    same(render(bvh_of(name, leaf), v), S.reference(name, v), name, v.kind, leaf)


@pytest.mark.parametrize('name', S.NAMES)
def test_leaf_sizes_give_identical_images(name):
    for v in S.views(name):
        first = render(bvh_of(name, LEAVES[0]), v)
        for leaf in LEAVES[1:]:
            same(render(bvh_of(name, leaf), v), first, name, v.kind, leaf)


@pytest.mark.parametrize('leaf', LEAVES)
def test_face_counts_sweep(leaf):
    """1 .. 1025 faces: a tree of depth 0, last levels that are exactly full, and last levels that are nearly all padding leaves."""
    for n in S.COUNTS:
        name = 'counts:%d' % n
        bvh = raycast.MeshBVH(*S.mesh(name), DEV, leaf=leaf)
        for v in S.views(name):
            same(render(bvh, v), S.reference(name, v), n, v.kind, leaf)


@pytest.mark.parametrize('leaf', LEAVES)
@pytest.mark.parametrize('name,k', CULLED)
def test_culled_depth_equals_oracle(name, k, leaf):
    v = S.views(name)[k]
    bvh = bvh_of(name, leaf)
    for cull in ('back', 'front'):
        same(render(bvh, v, cull), S.reference(name, v, cull), name, v.kind, leaf, cull)
    plain = bvh.render_depth(S.c2w_of(v), *S.camera(v))
    assert torch.equal(bvh.render_depth(S.c2w_of(v), *S.camera(v), cull='none'), plain)


@pytest.mark.parametrize('leaf', LEAVES)
def test_per_view_near(leaf):
    """One launch, a near plane of its own per view: three of uniform's cameras over one image."""
    nears = (0.05, 0.9, 1.7)
    vs = [v._replace(near=nr, far=20.0, **{c: S.CAM[c] for c in ('H', 'W', 'fx', 'fy', 'cx', 'cy')})
          for v, nr in zip([S.views('uniform')[i] for i in (0, 3, 4)], nears)]
    bvh = bvh_of('uniform', leaf)
    got = bvh.render_depth(np.stack([S.c2w_of(v) for v in vs]), *S.camera(vs[0])[:6], np.array(nears), 20.0).cpu().numpy()
    for k, v in enumerate(vs):
        same(got[k], S.reference('uniform', v), v.kind, leaf, nears[k])
    assert (got[0] != got[1]).any()


# ---- sensitivity: one missing triangle shows ----
@functools.lru_cache(maxsize=None)
def front_faces(count=20):
    """Rows of `count` faces of uniform that are the nearest hit of some pixel of the inside view (seeded choice)."""
    v = S.views('uniform')[0]
    _, _, face, unsure = S.mt_of('uniform', v)
    ids = np.unique(face[(face >= 0) & ~unsure])
    return tuple(int(i) for i in np.random.default_rng(5).choice(ids, count, replace=False))


@functools.lru_cache(maxsize=None)
def without_face(j):
    verts, faces = S.mesh('uniform')
    reduced = np.delete(faces, front_faces()[j], axis=0)
    v = S.views('uniform')[0]
    return reduced, S.frozen(D.render_depth(verts, reduced, S.c2w_of(v), *S.camera(v)))


@pytest.mark.parametrize('leaf', LEAVES)
@pytest.mark.parametrize('j', range(20))
def test_one_missing_triangle_shows(j, leaf):
    v = S.views('uniform')[0]
    full = S.reference('uniform', v)
    reduced, want = without_face(j)
    assert len(reduced) == len(S.mesh('uniform')[1]) - 1 and (want != full).any()    # the oracle: the face is some pixel's nearest
    got = render(raycast.MeshBVH(S.mesh('uniform')[0], reduced, DEV, leaf=leaf), v)
    assert (got != full).any()
    same(got, want, j, leaf)


# ---- visibility ----
def visible(bvh, pts, poses, eps, near):
    return visibility.points_visible(bvh, pts, list(poses), *S.VIS_CAM, eps=eps, near=near).cpu().numpy()


def same_flags(got, want, *what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, what + (len(bad), bad[:8].tolist(), got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize('near', [0.0, 0.5])
@pytest.mark.parametrize('eps', [0.03, 0.0])
@pytest.mark.parametrize('leaf', LEAVES)
@pytest.mark.parametrize('name', ['uniform', 'sheets'])
def test_visibility_equals_oracle(name, leaf, eps, near):
    """Each pose alone and all together (the views, then the views reversed).  Every (pose, point) pair is compared: the margin
    exemption of marginal pairs is not needed, kernel and oracle decide z < z_p - eps on the same bits (tests/test_soup_host.py)."""
    pts, poses = S.vis_points(name), S.vis_poses(name)
    fr, cl, _ = S.visible_reference(name, eps, near)
    want = (fr & cl).astype(np.uint8)
    bvh = bvh_of(name, leaf)
    for k in range(len(S.views(name))):
        same_flags(visible(bvh, pts, [poses[k]], eps, near), want[k], name, leaf, eps, near, k)
    got = visible(bvh, pts, poses, eps, near)
    same_flags(got, want.any(0).astype(np.uint8), name, leaf, eps, near, 'all')
    same_flags(visible(bvh, pts, poses[::-1], eps, near), got, name, leaf, eps, near, 'reversed')


def test_visibility_more_poses_than_one_lds_stage():
    """The views repeated, moved by up to 5 cm, past one stage of poses.  The brute-force oracle takes 12 s for all 610 points
    against the 265 poses; every fourth of the 600 sampled points (50 of each kind), and every camera-centre and behind-camera
    point, keep it to 3 s."""
    name = 'uniform'
    verts, faces = S.mesh(name)
    pts = S.vis_points(name)
    pts = pts[np.r_[0:600:4, 600:len(pts)]]
    assert len(pts) == 150 + 2 * len(S.views(name))
    many = perturbed(list(S.vis_poses(name)), CULL_CHUNK + 9, np.random.default_rng(9))
    fr, cl, _ = S.per_pose_in_frustum(verts, faces, pts, many, 0.03, 0.0)
    want = (fr & cl).any(0).astype(np.uint8)
    assert want.any() and not want.all()
    for leaf in LEAVES:
        same_flags(visible(bvh_of(name, leaf), pts, many, 0.03, 0.0), want, leaf)
    tail = visible(bvh_of(name, 4), pts, many[CULL_CHUNK - 3:], 0.03, 0.0)      # the stage boundary at another place
    same_flags(tail, (fr & cl)[CULL_CHUNK - 3:].any(0).astype(np.uint8), 'tail')
