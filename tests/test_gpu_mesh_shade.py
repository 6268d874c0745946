"""GPU: vertex normals and the shading pass (csrc/adfp_meshshade.h: mesh.vertex_normals, render_mesh.MeshViews) against the numpy
oracle of tests/hits_ref.py.  Every operation of the two contracts is a single f64 operation that numpy rounds correctly, and the
kernels are built without contraction, so the normals are compared bit for bit and the bytes exactly, except on the few channels
whose value before rounding lies within 1e-6 of a half-integer (the oracle's mask, capped on the CPU in tests/test_hits_host.py),
where they may differ by one."""
import numpy as np
import pytest
import torch

import depth_ref as D
import hits_ref as HR
import shade_cases as SC
import soup_meshes as S
from attentive_dfprior_amd import mesh, render_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize('name', ['sheets', 'uniform', 'box_room'])
def test_vertex_normals_equal_oracle(name):
    verts, faces = D.box_room() if name == 'box_room' else S.mesh(name)      # uniform: out-of-range and degenerate faces
    want = HR.vertex_normals(verts, faces)
    got = mesh.vertex_normals(verts, faces, DEV)
    assert got.dtype == torch.float64 and got.shape == (len(verts), 3)
    g = got.cpu().numpy()
    bad = (bits(g) != bits(want)).any(1) & ~((g == 0) & (want == 0)).all(1)
    assert not bad.any(), (name, int(bad.sum()), g[bad][:3], want[bad][:3])
    assert torch.equal(got, mesh.vertex_normals(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)))
    assert (np.abs(np.linalg.norm(g, axis=1) - 1) < 1e-15).sum() + (g == 0).all(1).sum() == len(g)


def test_vertex_normals_small_cases():
    v = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]) * 0.75
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    assert np.array_equal(mesh.vertex_normals(v, f, DEV).cpu().numpy(), v / 0.75)
    v2 = np.concatenate([v, [[5.0, 5.0, 5.0], [6.0, 6.0, 6.0]]])
    f2 = np.concatenate([f, [[6, 6, 7], [0, 1, 99], [-1, 2, 3]]])                # degenerate, out of range: nothing changes
    n2 = mesh.vertex_normals(v2, f2, DEV).cpu().numpy()
    assert np.array_equal(n2[:6], v / 0.75) and (n2[6:] == 0).all()
    f3 = np.concatenate([f, f[:1]])                                             # a face listed twice counts twice
    assert np.array_equal(bits(mesh.vertex_normals(v, f3, DEV).cpu().numpy()), bits(HR.vertex_normals(v, f3)))
    assert (mesh.vertex_normals(v, np.zeros((0, 3), np.int64), DEV) == 0).all()
    assert mesh.vertex_normals(np.zeros((0, 3)), np.zeros((0, 3), np.int64), DEV).shape == (0, 3)


def oracle_hits(case):
    return HR.render_hits(case.verts, case.faces, case.c2w, *case.cam)['none']


@pytest.mark.parametrize('k', range(3))
def test_shading_equals_oracle(k):
    case = SC.cases()[k]
    depth, face, bary = oracle_hits(case)
    hit = face >= 0
    vn = HR.vertex_normals(case.verts, case.faces)
    for smooth in (False, True):
        mv = render_mesh.MeshViews(case.verts, case.faces, case.colors, DEV, smooth=smooth)
        if smooth:
            assert np.array_equal(mv.normals.cpu().numpy(), vn)
        for mode in HR.MODES:
            got = mv.render(case.c2w, *case.cam, mode=mode, ambient=SC.AMBIENT)
            assert np.array_equal(got['face'][0].cpu().numpy(), face) and np.array_equal(got['depth'][0].cpu().numpy(), depth)
            nrm, rgb, unsure = HR.shade(face, bary, case.verts, case.faces, case.c2w, *case.cam[2:6], normals=vn if smooth else None,
                                        colors=case.colors, mode=mode, ambient=SC.AMBIENT)
            assert int(unsure.sum()) <= 0.005 * 3 * int(hit.sum())
            gn, gc = got['normal'][0].cpu().numpy(), got['rgb'][0].cpu().numpy()
            assert gn.dtype == np.float32 and gc.dtype == np.uint8 and gc.shape == face.shape + (3,)
            bad = gn != nrm
            assert not bad.any(), (case.label, smooth, mode, int(bad.sum()), gn[bad][:5], nrm[bad][:5])
            diff = np.abs(gc.astype(np.int32) - rgb.astype(np.int32))
            assert (diff[~unsure] == 0).all(), (case.label, smooth, mode, int((diff[~unsure] != 0).sum()))
            assert diff.max() <= 1
            assert (gc[~hit] == 255).all() and (gn[~hit] == 0).all()


def test_albedo_background_and_ambient():
    case = SC.cases()[2]
    _, face, bary = oracle_hits(case)
    mv = render_mesh.MeshViews(case.verts, case.faces, None, DEV, smooth=False)
    for mode, ambient, albedo, bg in (('shaded', 0.0, (0.9, 0.5, 0.25), (0, 0, 0)), ('shaded', 1.0, (1.0, 0.2, 0.7), (1, 2, 3)),
                                      ('color', 0.5, (0.1, 2.0, -1.0), (9, 8, 7))):
        got = mv.render(case.c2w, *case.cam, mode=mode, ambient=ambient, albedo=albedo, background=bg)
        _, rgb, unsure = HR.shade(face, bary, case.verts, case.faces, case.c2w, *case.cam[2:6], mode=mode, ambient=ambient,
                                  albedo=albedo, background=bg)
        diff = np.abs(got['rgb'][0].cpu().numpy().astype(np.int32) - rgb.astype(np.int32))
        assert (diff[~unsure] == 0).all() and diff.max() <= 1, (mode, ambient)
    with pytest.raises(ValueError):
        mv.render(case.c2w, *case.cam, mode='lit')


def test_caller_made_face_image():
    """-1, F, a face with an out-of-range vertex and a negative index other than -1 give the background; a real face is shaded."""
    verts, faces = S.mesh('uniform')
    out_of_range = int(np.flatnonzero(~S.in_range(verts, faces))[0])
    good = int(np.flatnonzero(S.in_range(verts, faces))[0])
    face = np.array([[-1, len(faces), out_of_range, good, -7, 2 ** 31 - 1]], np.int32)
    bary = np.full((1, 6, 2), 0.25, np.float32)
    mv = render_mesh.MeshViews(verts, faces, SC.colors_of(len(verts), 7), DEV, smooth=True)
    cam = (1, 6, 5.0, 5.0, 2.5, 0.0)
    got = mv.shade(torch.from_numpy(face), torch.from_numpy(bary), np.eye(4), *cam[2:], mode='shaded', background=(1, 2, 3))
    nrm, rgb, unsure = HR.shade(face, bary, verts, faces, np.eye(4), *cam[2:], normals=HR.vertex_normals(verts, faces),
                                colors=SC.colors_of(len(verts), 7), mode='shaded', background=(1, 2, 3))
    gc, gn = got['rgb'][0].cpu().numpy(), got['normal'][0].cpu().numpy()
    for j in (0, 1, 2, 4, 5):
        assert gc[0, j].tolist() == [1, 2, 3] and (gn[0, j] == 0).all(), j
    assert np.array_equal(gn, nrm) and (gn[0, 3] != 0).any()
    assert (np.abs(gc.astype(int) - rgb.astype(int))[~unsure] == 0).all()
    only = mv.shade(torch.from_numpy(face), torch.from_numpy(bary), np.eye(4), *cam[2:], background=(1, 2, 3), want=('rgb',))
    assert list(only) == ['rgb'] and torch.equal(only['rgb'], got['rgb'])


def test_no_views_and_a_mesh_of_nothing():
    verts, faces = S.mesh('uniform')
    mv = render_mesh.MeshViews(verts, faces, None, DEV, smooth=True)
    none = mv.shade(torch.zeros((0, 4, 6), dtype=torch.int32), torch.zeros((0, 4, 6, 2)), np.zeros((0, 4, 4)), 5.0, 5.0, 2.5, 1.5)
    assert none['normal'].shape == (0, 4, 6, 3) and none['normal'].dtype == torch.float32
    assert none['rgb'].shape == (0, 4, 6, 3) and none['rgb'].dtype == torch.uint8
    r = mv.render(np.zeros((0, 4, 4)), 4, 6, 5.0, 5.0, 2.5, 1.5)
    assert r['depth'].shape == (0, 4, 6) and r['face'].shape == (0, 4, 6) and r['rgb'].shape == (0, 4, 6, 3)
    nothing = render_mesh.MeshViews(np.zeros((0, 3)), np.zeros((0, 3), np.int64), None, DEV, smooth=True)
    r = nothing.render(np.eye(4), 4, 6, 5.0, 5.0, 2.5, 1.5, background=(1, 2, 3))
    assert (r['depth'] == 0).all() and (r['face'] == -1).all() and (r['normal'] == 0).all()
    assert r['rgb'].shape == (1, 4, 6, 3) and (r['rgb'].reshape(-1, 3).cpu() == torch.tensor([1, 2, 3], dtype=torch.uint8)).all()
