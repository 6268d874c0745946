"""GPU: mesh.simplify_vertex_clustering (csrc/adfp_meshsimplify.h) against the numpy statement of the same rules
(tests/simplify_ref.py): faces, counts and colours element for element, average positions bit for bit, quadric positions within two
f32 ulps of the mesh's largest coordinate; the degenerate voxels; the Mesher's config keys; the command line.

Measured on the CPU with the oracle: the sphere comes out at 1 045 vertices and 2 086 faces, the cube at 448 and 892, neither has an
ambiguous cluster, a dropped cluster or a placement guard firing, and on the cube the quadric moves vertices by up to 0.24 voxel
(the tests assert what the oracle says, not these figures)."""
import functools

import numpy as np
import pytest
import torch

import simplify_meshes as SM
import simplify_ref as R
from attentive_dfprior_amd import mesh as M
from attentive_dfprior_amd import simplify_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BIG = {'sphere': SM.uv_sphere, 'cube': SM.cube_surface}
ULPS2 = 2.4e-7                              # two f32 ulps, relative: the one rounding of two f64 results that differ far below it


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts, faces, voxel, colours) and the oracle's results, computed once and shared: {(contraction, coloured): outputs}."""
    v, f, vs = (BIG.get(name) or SM.HAND_MADE[name])()
    c = SM.colours(len(v))
    ref = {}
    for contraction in R.CONTRACTIONS:
        ref[contraction] = R.simplify(v, f, vs, contraction, colors=c, detail=True)
    return v, f, vs, c, ref, R.ambiguous(v, f, vs)


def device_call(v, f, vs, contraction, c=None):
    vo, fo, co = M.simplify_vertex_clustering(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), vs, contraction=contraction,
                                              colors=torch.from_numpy(c).to(DEV) if c is not None else None)
    assert vo.is_cuda and vo.dtype == torch.float32 and fo.dtype == torch.int32 and (co is None) == (c is None)
    assert co is None or co.dtype == torch.uint8
    return vo.cpu().numpy(), fo.cpu().numpy(), (co.cpu().numpy() if co is not None else None)


def check_against_oracle(name, contraction, coloured):
    v, f, vs, c, ref, amb = case(name)
    rv, rf, rc, q = ref[contraction]
    assert amb.mean() <= 0.01                                # from the oracle alone: almost every cluster is compared in full
    gv, gf, gc = device_call(v, f, vs, contraction, c if coloured else None)
    print(f'{name} {contraction}: {len(v)} -> {len(gv)} vertices, {len(f)} -> {len(gf)} faces (oracle {len(rv)}, {len(rf)}), '
          f'{int(amb.sum())} ambiguous clusters')
    assert gv.shape == rv.shape and gf.shape == rf.shape
    assert np.array_equal(gf, rf)
    if coloured:
        assert np.array_equal(gc, rc)
    flagged = amb[q['used']]
    err = np.abs(gv.astype(np.float64) - rv.astype(np.float64))
    print(f'  max position difference {err.max() if err.size else 0.0:.3e}, bound {ULPS2 * np.abs(v).max():.3e}')
    if contraction == 'average':
        assert np.array_equal(gv.view(np.uint32), rv.view(np.uint32))
    else:
        assert (err[~flagged] <= ULPS2 * np.abs(v).max()).all()
        for row in np.flatnonzero(flagged):                  # one of the candidates, each rounded to f32
            cand = R.candidates(q, q['used'][row]).astype(np.float32).astype(np.float64)
            assert (np.abs(cand - gv[row].astype(np.float64)).max(1) <= ULPS2 * np.abs(v).max()).any()


@pytest.mark.parametrize('coloured', [False, True])
@pytest.mark.parametrize('contraction', R.CONTRACTIONS)
@pytest.mark.parametrize('name', sorted(BIG))
def test_sphere_and_cube_match_the_oracle(name, contraction, coloured):
    v, f, vs, c, ref, amb = case(name)
    assert len(ref[contraction][1]) > 0.1 * len(f) and len(ref[contraction][0]) < 0.5 * len(v)        # a real simplification
    check_against_oracle(name, contraction, coloured)


@pytest.mark.parametrize('contraction', R.CONTRACTIONS)
@pytest.mark.parametrize('name', sorted(SM.HAND_MADE))
def test_hand_made_meshes_match_the_oracle(name, contraction):
    check_against_oracle(name, contraction, True)


def test_the_quadric_moves_the_cube_and_not_only_by_rounding():
    """the two contractions are different functions on the device too: on the cube the quadric moves vertices by a good part of
    a voxel (the oracle says how far), toward the edges and corners"""
    v, f, vs, c, ref, _ = case('cube')
    ga, _, _ = device_call(v, f, vs, 'average')
    gq, _, _ = device_call(v, f, vs, 'quadric')
    moved = np.abs(gq.astype(np.float64) - ga).max()
    want = np.abs(ref['quadric'][0].astype(np.float64) - ref['average'][0]).max()
    assert want > 0.1 * vs and abs(moved - want) <= 2 * ULPS2 * np.abs(v).max()


@pytest.mark.parametrize('contraction', R.CONTRACTIONS)
def test_a_voxel_as_large_as_the_model_returns_nothing(contraction):
    """one cell holds all 4 514 vertices: its lane's run crosses every tile and workgroup boundary, every face collapses"""
    v, f, _, c, _, _ = case('sphere')
    assert R.clusters(v, 4.0)[2] == 1
    gv, gf, gc = device_call(v, f, 4.0, contraction, c)
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gc.shape == (0, 3)


def test_a_few_huge_cells_match_the_oracle():
    """voxel 0.7 on the sphere: eight cells of hundreds of vertices each, long runs whose sums are compared"""
    v, f, _, c, _, _ = case('sphere')
    for contraction in R.CONTRACTIONS:
        rv, rf, rc = R.simplify(v, f, 0.7, contraction, colors=c)
        gv, gf, gc = device_call(v, f, 0.7, contraction, c)
        assert len(rv) == 8 and np.array_equal(gf, rf) and np.array_equal(gc, rc)
        if contraction == 'average':
            assert np.array_equal(gv, rv)
        else:
            assert not R.ambiguous(v, f, 0.7).any() and np.abs(gv.astype(np.float64) - rv).max() <= ULPS2 * np.abs(v).max()


def test_a_tiny_voxel_is_the_identity_up_to_key_order():
    """voxel 1e-4: 10^4 cells per axis, keys of 40 bits (two 31-bit passes), every vertex its own cluster"""
    v, f, _, c, _, _ = case('sphere')
    _, cl, K = R.clusters(v, 1e-4)
    assert K == len(v)
    order = np.argsort(cl)
    gv, gf, gc = device_call(v, f, 1e-4, 'average', c)
    assert np.array_equal(gv, v[order]) and np.array_equal(gc, c[order])
    rv, rf, _ = R.simplify(v, f, 1e-4, 'average')
    assert len(gf) == len(f) and np.array_equal(gf, rf)
    qv, qf, _ = device_call(v, f, 1e-4, 'quadric')
    assert np.array_equal(qf, rf) and np.abs(qv.astype(np.float64) - gv).max() <= ULPS2 * np.abs(v).max()


def test_two_calls_give_the_same_bits():
    v, f, vs, c, _, _ = case('sphere')
    tv, tf, tc = (torch.from_numpy(a).to(DEV) for a in (v, f, c))
    a = M.simplify_vertex_clustering(tv, tf, vs, 'quadric', tc)
    b = M.simplify_vertex_clustering(tv, tf, vs, 'quadric', tc)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_corner_recovery_on_the_device():
    v, f, vs = SM.cube_corner()
    gq, gf, _ = device_call(v, f, vs, 'quadric')
    ga, _, _ = device_call(v, f, vs, 'average')
    rv, rf, _, q = R.simplify(v, f, vs, 'quadric', detail=True)
    row = int(np.flatnonzero(q['used'] == q['cl'][0])[0])
    assert np.array_equal(gf, rf)
    assert np.abs(gq[row]).max() <= 1e-12 * vs               # the corner itself (the origin), although no input vertex lies there
    assert np.abs(ga[row]).min() > 0.1 * vs


def test_argument_errors():
    v, f, vs = SM.triangle()
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            M.simplify_vertex_clustering(tv, tf, bad)
    with pytest.raises(ValueError):
        M.simplify_vertex_clustering(tv, tf, vs, contraction='median')
    with pytest.raises(ValueError):
        M.simplify_vertex_clustering(tv, tf, vs, colors=torch.zeros((2, 3), dtype=torch.uint8, device=DEV))
    for bad in (float('nan'), float('inf')):
        w = tv.clone()
        w[1, 2] = bad
        with pytest.raises(ValueError):
            M.simplify_vertex_clustering(w, tf, vs)
    with pytest.raises(ValueError):
        M.simplify_vertex_clustering(tv, torch.tensor([[0, 1, 3]], dtype=torch.int32, device=DEV), vs)
    vo, fo, co = M.simplify_vertex_clustering(tv, tf[:0], vs)          # no faces: nothing is referenced
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and co is None


def _cells(p, vmin, vs):
    return {tuple(r) for r in np.floor((p.astype(np.float64) - vmin) / vs).astype(np.int64).tolist()}


def test_mesher_config_keys(tmp_path, monkeypatch):
    import mesh_ref
    import test_gpu_mesher as TM
    from attentive_dfprior_amd.mesher import Mesher
    sc, sd, dec, cfg, slam, kfs, est, c = TM.setup(resolution=40)
    tsdf = sc.tsdf_volume.to(DEV)

    def run(name, **keys):
        cfg2 = dict(cfg, meshing=dict(cfg['meshing'], **keys))
        m = Mesher(cfg2, None, slam)
        out = tmp_path / name
        assert m.get_mesh(str(out), c, dec, kfs, est, 2, tsdf, DEV, color=True, clean_mesh=True) is not None
        return m, out

    # without the key, or with None or 0, the new code is never reached and the file is the same bytes
    def never(*a, **k):
        raise AssertionError('simplification ran without a positive simplify_voxel_size')
    with monkeypatch.context() as mp:
        mp.setattr(M, '_simplify_vertex_clustering', never)
        m, plain = run('plain.ply')
        assert m.simplify_voxel_size is None and m.simplify_contraction == 'quadric'
        for k, value in enumerate((None, 0, 0.0)):
            _, other = run(f'off{k}.ply', simplify_voxel_size=value)
            assert other.read_bytes() == plain.read_bytes()
    rec0, faces0 = mesh_ref.read_ply(str(plain))
    p0 = np.stack([rec0['x'], rec0['y'], rec0['z']], 1)

    xyz = m.get_grid_uniform(40)['xyz']
    vs = 2 * max(float(a[2] - a[1]) for a in xyz)             # twice the lattice spacing (scale is 1)
    vmin = p0.min(0).astype(np.float64) - vs / 2
    got = {}
    for contraction in ('average', 'quadric'):
        m, out = run(f'{contraction}.ply', simplify_voxel_size=vs, simplify_contraction=contraction)
        rec, faces = mesh_ref.read_ply(str(out))
        p = np.stack([rec['x'], rec['y'], rec['z']], 1)
        print(f'{contraction}: {len(p0)} -> {len(p)} vertices, {len(faces0)} -> {len(faces)} faces')
        assert 0 < len(faces) < len(faces0) and len(p) < len(p0) and faces.max() == len(p) - 1
        # the colours are the colour query at the file's own vertices
        col = M.color_bytes(m.eval_points(torch.from_numpy(p).to(DEV), dec, tsdf, m.tsdf_bnds, c, 'color', DEV)).cpu().numpy()
        assert np.array_equal(np.stack([rec['red'], rec['green'], rec['blue']], 1), col)
        got[contraction] = (p, faces)
    # the average of a cell's vertices lies in that cell: every vertex lies inside a cell some original vertex lies in
    assert _cells(got['average'][0], vmin, vs) <= _cells(p0, vmin, vs)
    # the quadric keeps the clusters and the faces, and moves a vertex by a voxel at the most
    assert np.array_equal(got['quadric'][1], got['average'][1])
    assert np.abs(got['quadric'][0].astype(np.float64) - got['average'][0]).max() <= vs * (1 + 1e-6)
    with pytest.raises(ValueError):
        Mesher(dict(cfg, meshing=dict(cfg['meshing'], simplify_contraction='median')), None, slam)


def test_command_line_round_trip(tmp_path, capsys):
    v, f, vs, c, ref, _ = case('cube')
    src, dst = tmp_path / 'in.ply', tmp_path / 'out.ply'
    M.write_ply(str(src), v, f, colors=c)
    simplify_mesh.main([str(src), str(dst), '--voxel_size', str(vs), '--normals'])
    rv, rf, rc, _ = ref['quadric']
    said = capsys.readouterr().out
    assert f'{len(v)} vertices, {len(f)} faces' in said and f'{len(rv)} vertices, {len(rf)} faces' in said
    m = M.read_ply(str(dst))
    assert np.array_equal(m.faces, rf) and np.array_equal(m.colors, rc)
    assert np.abs(m.verts - rv).max() <= ULPS2 * np.abs(v).max()
    nrm = M.vertex_normals(m.verts.astype(np.float32), m.faces, device=DEV).cpu().numpy()
    assert m.normals is not None and np.abs(m.normals - nrm).max() <= 1e-6
    assert np.abs(np.linalg.norm(m.normals, axis=1) - 1).max() <= 1e-5
    # the other contraction, no normals
    simplify_mesh.main([str(src), str(dst), '--voxel_size', str(vs), '--contraction', 'average'])
    m = M.read_ply(str(dst))
    assert m.normals is None and np.array_equal(m.verts.astype(np.float32), ref['average'][0]) and np.array_equal(m.colors, ref['average'][2])


def test_no_vertices():
    v0 = torch.zeros((0, 3), dtype=torch.float32, device=DEV)
    f0 = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    vo, fo, co = M.simplify_vertex_clustering(v0, f0, 0.1, colors=torch.zeros((0, 3), dtype=torch.uint8, device=DEV))
    assert vo.shape == (0, 3) and vo.dtype == torch.float32 and fo.shape == (0, 3) and fo.dtype == torch.int32
    assert co.shape == (0, 3) and co.dtype == torch.uint8
