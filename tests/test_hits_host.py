"""CPU: the oracles of tests/hits_ref.py before any kernel is compared with them.  The hit oracle's depth is the depth oracle's bit
for bit; its face is the face an independent f64 Moeller-Trumbore renderer finds (soup_meshes.mt_of) wherever that renderer is
sure, by index on the soups without coincident faces and by triangle on the one with them; exact ties go to the smallest index.
The vertex-normal oracle against closed forms, and the shading oracle's half-integer mask within its cap for the inputs the GPU
suite uses."""
import numpy as np
import pytest

import depth_ref as D
import hits_ref as HR
import soup_meshes as S

# a few 48 x 64 views of each soup: soup_meshes.mt_of is slow and cached per process (test_soup_host.py computes the same ones)
VIEWS = [('uniform', 0), ('uniform', 3), ('giants_and_dust', 0), ('giants_and_dust', 4), ('sheets', 0), ('sheets', 3),
         ('far_offset', 0), ('far_offset', 4)]
TIED = [('coincident', 0), ('coincident', 4)]
MASK_CAP = 0.005                                       # of a view's hit channels


@pytest.mark.parametrize('name,k', VIEWS + TIED)
def test_depth_is_the_depth_oracles(name, k):
    v = S.views(name)[k]
    h = HR.soup_hits(name, v)
    for cull in HR.CULLS if name in ('uniform', 'sheets', 'coincident') else ('none',):
        depth, face, bary = h[cull]
        assert np.array_equal(depth.view(np.uint32), S.reference(name, v, cull).view(np.uint32)), (name, k, cull)
        assert ((bary == 0).all(-1) | (face >= 0)).all()
    depth, face, _ = h['none']
    assert np.array_equal(face >= 0, depth > 0)        # near > 0 in every soup view: a hit has a positive depth


@pytest.mark.parametrize('name,k', VIEWS)
def test_face_is_the_independent_renderers(name, k):
    v = S.views(name)[k]
    _, face, bary = HR.soup_hits(name, v)['none']
    z, _, mt_face, unsure = S.mt_of(name, v)
    assert int(unsure.sum()) <= 8
    sure = ~unsure
    assert np.array_equal(face[sure], mt_face[sure]), (name, k, int((face != mt_face)[sure].sum()))
    hit = face >= 0
    b = bary[hit].astype(np.float64)
    assert (b >= -1e-6).all() and (b.sum(1) <= 1 + 1e-6).all()
    # the weights put the hit point on the ray at the oracle's depth
    verts, faces = S.mesh(name)
    t = verts[faces[face[hit]]]
    pt = t[:, 0] * (1 - b.sum(1))[:, None] + t[:, 1] * b[:, :1] + t[:, 2] * b[:, 1:]
    m = S.c2w_of(v)
    zc = (pt - m[:3, 3]) @ m[:3, 2]
    assert np.abs(zc - z[hit])[~unsure[hit]].max() <= 1e-5          # bary is f32: 2^-24 of a triangle's size, at most 6


@pytest.mark.parametrize('name,k', TIED)
def test_coincident_faces_agree_by_triangle(name, k):
    v = S.views(name)[k]
    _, face, _ = HR.soup_hits(name, v)['none']
    _, _, mt_face, unsure = S.mt_of(name, v)
    _, faces = S.mesh(name)
    ok = ~unsure & (face >= 0)
    assert np.array_equal(face >= 0, mt_face >= 0)
    assert np.array_equal(np.sort(faces[face[ok]], 1), np.sort(faces[mt_face[ok]], 1))
    # the rule is exercised: many pixels see an exact copy with a larger index (the same vertex order: the same z to the bit)
    same = {}
    for i, f in enumerate(map(tuple, faces.tolist())):
        same.setdefault(f, []).append(i)
    first = np.array([same[tuple(f)][0] for f in faces.tolist()])
    copies = np.array([len(same[tuple(f)]) for f in faces.tolist()])
    assert np.array_equal(first[face[ok]], face[ok])                   # never a later exact copy
    assert int((copies[face[ok]] > 1).sum()) >= 100


def test_exact_ties_go_to_the_smallest_index():
    verts, faces = D.box_room()
    near_wall = [i for i, f in enumerate(faces) if (verts[f][:, 2] == verts[:, 2].max()).all()]
    f = np.concatenate([faces, faces[near_wall], faces[near_wall][::-1]])          # copies listed after the originals
    c2w = np.eye(4)
    cam = (24, 32, 20.0, 20.0, 15.5, 11.5, 0.05, 20.0)
    want = HR.render_hits(verts, faces, c2w, *cam)['none']
    got = HR.render_hits(verts, f, c2w, *cam)['none']
    for a, b in zip(want, got):
        assert np.array_equal(a, b)
    assert set(np.unique(got[1])) <= set(near_wall) and len(np.unique(got[1])) == 2
    # the originals listed last: now the copies win
    perm = np.r_[np.arange(12, len(f)), np.arange(12)]
    got = HR.render_hits(verts, f[perm], c2w, *cam)['none']
    assert got[1].max() < len(f) - 12 and np.array_equal(got[0], want[0])
    # a hit at z = 0 with near = 0 has depth 0 and a face
    tri = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.0, 0.0]])
    d, fc, _ = HR.render_hits(tri, [[0, 1, 2]], c2w, 3, 3, 10.0, 10.0, 1.0, 1.0, 0.0, 20.0)['none']
    assert fc[1, 1] == 0 and d[1, 1] == 0.0
    assert HR.render_hits(tri, [[0, 1, 2]], c2w, 3, 3, 10.0, 10.0, 1.0, 1.0, 0.05, 20.0)['none'][1][1, 1] == -1
    # a pose with a NaN: nothing in the culled modes
    bad = np.eye(4)
    bad[0, 3] = np.nan
    for cull in ('back', 'front'):
        d, fc, b = HR.render_hits(verts, faces, bad, *cam)[cull]
        assert (d == 0).all() and (fc == -1).all() and (b == 0).all()


def test_vertex_normals_closed_forms():
    # an octahedron, outward faces: every vertex normal is its own direction
    v = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.75
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    n = HR.vertex_normals(v, f)
    assert np.array_equal(n, v / 0.75)
    # the box room: at every corner three faces' normals of equal length along the three axes, up to how many triangles meet there
    bv, bf = D.box_room()
    n = HR.vertex_normals(bv, bf)
    g, _ = HR.face_normals(bv, bf)
    want = np.zeros_like(bv)
    for i, tri in enumerate(bf):
        want[tri] += g[i]
    want /= np.linalg.norm(want, axis=1)[:, None]
    assert np.abs(n - want).max() <= 4 * np.finfo(np.float64).eps
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 4 * np.finfo(np.float64).eps
    centre = (bv.min(0) + bv.max(0)) / 2
    side = np.sign(n) * np.sign(bv - centre)                          # all three axes at every corner, all on one side of the walls
    assert (side != 0).all() and (side == side[0, 0]).all()
    # an unreferenced vertex, a degenerate face and a face with an index out of range give zeros / change nothing
    v2 = np.concatenate([v, [[5.0, 5.0, 5.0], [6.0, 6.0, 6.0]]])
    f2 = np.concatenate([f, [[6, 6, 7], [0, 1, 99], [-1, 2, 3]]])
    n2 = HR.vertex_normals(v2, f2)
    assert np.array_equal(n2[:6], v / 0.75) and (n2[6:] == 0).all()
    # a face listed twice counts twice
    f3 = np.concatenate([f, f[:1]])
    g3, _ = HR.face_normals(v, f3)
    s = sum(g3[i] for i in (0, 3, 4, 7, 8))                           # vertex 0's faces, in ascending index
    assert np.array_equal(HR.vertex_normals(v, f3)[0], s / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
    assert not np.array_equal(HR.vertex_normals(v, f3)[0], [1.0, 0.0, 0.0])
    assert HR.vertex_normals(np.zeros((0, 3)), np.zeros((0, 3), int)).shape == (0, 3)
    assert (HR.vertex_normals(v, np.zeros((0, 3), int)) == 0).all()


def test_shading_oracle_and_its_mask_cap():
    import shade_cases as SC
    for case in SC.cases():
        verts, faces, colors = case.verts, case.faces, case.colors
        vn = HR.vertex_normals(verts, faces)
        _, face, bary = HR.render_hits(verts, faces, case.c2w, *case.cam)['none']
        hit = face >= 0
        assert hit.sum() >= 0.05 * hit.size, case.label
        for mode in HR.MODES:
            for normals in (None, vn):
                nrm, rgb, unsure = HR.shade(face, bary, verts, faces, case.c2w, *case.cam[2:6], normals=normals, colors=colors,
                                            mode=mode, ambient=SC.AMBIENT)
                assert int(unsure.sum()) <= MASK_CAP * 3 * int(hit.sum()), (case.label, mode, int(unsure.sum()))
                assert (rgb[~hit] == 255).all() and (nrm[~hit] == 0).all()
                ln = np.linalg.norm(nrm[hit].astype(np.float64), axis=1)
                assert np.abs(ln - 1).max() <= 1e-6
                jj, ii = np.meshgrid(np.arange(case.cam[1]), np.arange(case.cam[0]))
                d = np.stack([(jj - case.cam[4]) / case.cam[2], (ii - case.cam[5]) / case.cam[3], np.ones_like(jj, float)], -1)
                assert ((nrm.astype(np.float64) * d).sum(-1)[hit] <= 1e-7).all()       # toward the camera
        # flat shading of the axis-aligned room: the normal map holds only axis colours
        if case.label == 'room':
            nrm, _, _ = HR.shade(face, bary, verts, faces, case.c2w, *case.cam[2:6], mode='normal')
            world = nrm[hit].astype(np.float64) @ np.asarray(case.c2w)[:3, :3].T
            assert np.abs(np.abs(world).max(1) - 1).max() <= 1e-6
