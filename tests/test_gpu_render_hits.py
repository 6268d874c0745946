"""GPU: the hit render (k_render_hits in csrc/adfp_raycast.h, MeshBVH.render_hits) on the triangle soups of tests/soup_meshes.py.
Its depth is render_depth's bit for bit, its face and barycentric images are the brute-force oracle's (tests/hits_ref.py) exactly,
ties between coincident faces included, for every soup, view and cull mode; the result does not depend on the leaf size, the run,
the launch chunk or which outputs are asked for.  The views cover partial tiles (47 x 61), rays with a zero component, 24 x 32
images and face counts around every leaf boundary; the oracle itself is checked on the CPU in tests/test_hits_host.py."""
import functools

import numpy as np
import pytest
import torch

import depth_ref as D
import hits_ref as HR
import soup_meshes as S
from attentive_dfprior_amd import _lib, raycast

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LEAVES = _lib.TRI_LEAVES


@functools.lru_cache(maxsize=None)
def bvh_of(name, leaf=_lib.TRI_LEAF_DEFAULT):
    return raycast.MeshBVH(*S.mesh(name), DEV, leaf=leaf)


def check_view(bvh, name, v, cull):
    got = bvh.render_hits(S.c2w_of(v), *S.camera(v), cull=cull)
    assert got['depth'].shape == (1, v.H, v.W) and got['face'].dtype == torch.int32 and got['bary'].shape == (1, v.H, v.W, 2)
    assert torch.equal(got['depth'], bvh.render_depth(S.c2w_of(v), *S.camera(v), cull=cull)), (name, v.kind, cull)
    depth, face, bary = HR.soup_hits(name, v)[cull]
    g = {k: t[0].cpu().numpy() for k, t in got.items()}
    bad = g['face'] != face
    assert not bad.any(), (name, v.kind, cull, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g['face'][bad][:5], face[bad][:5])
    bad = (g['bary'] != bary).any(-1)
    assert not bad.any(), (name, v.kind, cull, int(bad.sum()), np.argwhere(bad)[:5].tolist(), g['bary'][bad][:5], bary[bad][:5])
    assert np.array_equal(g['depth'], depth)
    return got


@pytest.mark.parametrize('name', S.NAMES)
def test_hits_equal_oracle(name):
    for v in S.views(name):
        for cull in HR.CULLS:
            check_view(bvh_of(name), name, v, cull)


def test_face_counts_sweep():
    """1 .. 1025 faces: a tree of depth 0, last levels that are exactly full, and last levels that are nearly all padding leaves."""
    for n in S.COUNTS:
        name = 'counts:%d' % n
        for v in S.views(name):
            for cull in HR.CULLS:
                check_view(bvh_of(name), name, v, cull)


def test_leaf_sizes_and_runs_give_identical_tensors():
    for name in S.NAMES:
        for v in S.views(name):
            first = bvh_of(name, LEAVES[0]).render_hits(S.c2w_of(v), *S.camera(v))
            for leaf in LEAVES:                                         # the first leaf again: two runs
                again = bvh_of(name, leaf).render_hits(S.c2w_of(v), *S.camera(v))
                for k in first:
                    assert torch.equal(first[k], again[k]), (name, v.kind, leaf, k)


def test_ties_go_to_the_smallest_index():
    """The room with one wall's two faces listed three times, then the same faces with the originals last."""
    verts, faces = D.box_room()
    wall = [i for i, f in enumerate(faces) if (verts[f][:, 2] == verts[:, 2].max()).all()]
    f = np.concatenate([faces, faces[wall], faces[wall][::-1]])
    cam = (24, 32, 20.0, 20.0, 15.5, 11.5, 0.05, 20.0)
    for ff in (f, f[np.r_[np.arange(12, len(f)), np.arange(12)]]):
        want = HR.render_hits(verts, ff, np.eye(4), *cam)['none']
        for leaf in LEAVES:
            got = raycast.MeshBVH(verts, ff, DEV, leaf=leaf).render_hits(np.eye(4), *cam)
            for k, w in zip(('depth', 'face', 'bary'), want):
                assert np.array_equal(got[k][0].cpu().numpy(), w), (leaf, k)
    # a hit at z = 0 with near = 0 has depth 0 and a face
    tri = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    got = raycast.MeshBVH(tri, [[0, 1, 2]], DEV).render_hits(np.eye(4), 3, 3, 10.0, 10.0, 1.0, 1.0, 0.0, 20.0)
    assert got['face'][0, 1, 1].item() == 0 and got['depth'][0, 1, 1].item() == 0.0


def test_views_cross_the_launch_chunk():
    """32 770 views of a 2 x 2 image: two launches; the first and the last view are their single-view renders."""
    name = 'counts:17'
    a, b = S.views(name)[0], S.views(name)[1]
    cam = (2, 2, 20.0, 20.0, 0.5, 0.5, a.near, a.far)                # four rays close about the face both views look at
    n = 32770
    poses = np.broadcast_to(S.c2w_of(a), (n, 4, 4)).copy()
    poses[-1] = S.c2w_of(b)
    poses[32768] = S.c2w_of(b)
    bvh = bvh_of(name)
    got = bvh.render_hits(poses, *cam)
    one_a, one_b = bvh.render_hits(S.c2w_of(a), *cam), bvh.render_hits(S.c2w_of(b), *cam)
    assert (one_a['face'] >= 0).any() and (one_b['face'] >= 0).any() and not torch.equal(one_a['bary'], one_b['bary'])
    for k in got:
        assert got[k].shape[0] == n
        assert torch.equal(got[k][:1], one_a[k]) and torch.equal(got[k][32767:32768], one_a[k]), k
        assert torch.equal(got[k][32768:32769], one_b[k]) and torch.equal(got[k][-1:], one_b[k]), k


def test_non_finite_pose():
    name = 'uniform'
    v = S.views(name)[0]
    bad = S.c2w_of(v)
    bad[1, 3] = np.nan
    poses = np.stack([S.c2w_of(v), bad])
    bvh = bvh_of(name)
    for cull in ('back', 'front'):
        got = bvh.render_hits(poses, *S.camera(v), cull=cull)
        assert (got['depth'][1] == 0).all() and (got['face'][1] == -1).all() and (got['bary'][1] == 0).all()
        assert (got['face'][0] >= 0).any()
    got = bvh.render_hits(poses, *S.camera(v))
    want = bvh.render_depth(poses, *S.camera(v))
    assert torch.equal(got['depth'].view(torch.int32), want.view(torch.int32))
    assert torch.equal(got['face'] >= 0, want != 0)


def test_each_output_alone_and_the_empty_cases():
    name = 'sheets'
    bvh = bvh_of(name)
    vs = S.views(name)[:1] + S.views(name)[3:4]                          # two views of one camera size
    poses = np.stack([S.c2w_of(v) for v in vs])
    full = bvh.render_hits(poses, *S.camera(vs[0]), cull='back')
    for k in ('depth', 'face', 'bary'):
        alone = bvh.render_hits(poses, *S.camera(vs[0]), cull='back', want=(k,))
        assert list(alone) == [k] and torch.equal(alone[k], full[k]), k
    pair = bvh.render_hits(poses, *S.camera(vs[0]), cull='back', want=('face', 'bary'))
    assert torch.equal(pair['face'], full['face']) and torch.equal(pair['bary'], full['bary'])
    with pytest.raises(ValueError):
        bvh.render_hits(poses, *S.camera(vs[0]), want=())
    with pytest.raises(ValueError):
        bvh.render_hits(poses, *S.camera(vs[0]), cull='both')
    # no faces: 0 / -1 / 0; no views: empty tensors
    empty = raycast.MeshBVH(np.zeros((0, 3)), np.zeros((0, 3), np.int64), DEV)
    got = empty.render_hits(poses, *S.camera(vs[0]))
    assert (got['depth'] == 0).all() and (got['face'] == -1).all() and (got['bary'] == 0).all() and got['face'].shape == (2, 48, 64)
    none = bvh.render_hits(np.zeros((0, 4, 4)), *S.camera(vs[0]))
    assert none['bary'].shape == (0, 48, 64, 2) and none['face'].numel() == 0
