"""GPU: ScanNet mesh evaluation on the MI355X against the numpy oracle tests/refuse_ref.py -- the culled depth render (bit for bit
at every leaf size, a hand-built triangle in both windings, a closed box seen from inside, non-finite poses), unit touch marks,
unit-gated integration (bit for bit, chunking never changes a bit, untouched units keep their values), extraction of the observed
surface, voxel downsampling (means, counts and order bit for bit, wide keys), and evaluate_mesh end to end on a synthetic ScanNet
tree."""
import os
import sys

import numpy as np
import pytest
import torch

import refuse_ref as R
from attentive_dfprior_amd import _lib, evaluate_scannet as E, mesh, raycast, refusion

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, W, FX, FY, CX, CY = 30, 40, 32.0, 32.0, 19.6, 14.7


def inverted_scene():
    v, f = R.scene()
    return v, f[:, ::-1].copy()


def poses32(n=20, seed=0):
    return [p.astype(np.float32) for p in R.orbit_poses(n, seed=seed)]


# ---- culled render ----
def test_facing_sign_of_a_hand_built_triangle():
    v = np.array([[-1.0, -1.0, 2.0], [1.0, -1.0, 2.0], [0.0, 1.0, 2.0]])
    away = np.array([[0, 1, 2]])                  # (v1 - v0) x (v2 - v0) = (0, 0, 4): away from a camera at 0 looking along +z
    toward = away[:, ::-1].copy()
    c2w = np.eye(4)
    for faces, front in ((away, False), (toward, True)):
        bvh = raycast.MeshBVH(v, faces, DEV)
        plain = bvh.render_depth(c2w, 9, 9, 10.0, 10.0, 4.0, 4.0, 0.1, 10.0)[0, 4, 4].item()
        back = bvh.render_depth(c2w, 9, 9, 10.0, 10.0, 4.0, 4.0, 0.1, 10.0, cull='back')[0, 4, 4].item()
        frnt = bvh.render_depth(c2w, 9, 9, 10.0, 10.0, 4.0, 4.0, 0.1, 10.0, cull='front')[0, 4, 4].item()
        assert plain == 2.0
        assert (back, frnt) == ((2.0, 0.0) if front else (0.0, 2.0))


@pytest.mark.parametrize('leaf', _lib.TRI_LEAVES)
def test_culled_render_matches_oracle(leaf):
    v, f = inverted_scene()
    c2ws = [p.astype(np.float64) for p in poses32(6, seed=3)]
    bvh = raycast.MeshBVH(v, f, DEV, leaf=leaf)
    plain = bvh.render_depth(np.stack(c2ws), H, W, FX, FY, CX, CY, 0.05, 5.0)
    none = bvh.render_depth(np.stack(c2ws), H, W, FX, FY, CX, CY, 0.05, 5.0, cull='none')
    assert torch.equal(plain, none)
    for cull in ('back', 'front'):
        got = bvh.render_depth(np.stack(c2ws), H, W, FX, FY, CX, CY, 0.05, 5.0, cull=cull)
        # the culled kernel's NONE path is adfp_render_depth itself: compare the culled entry at NONE too
        for k, c2w in enumerate(c2ws):
            want = R.render_depth_cull(v, f, c2w, H, W, FX, FY, CX, CY, 0.05, 5.0, cull)
            bad = got[k].cpu().numpy() != want
            assert not bad.any(), (cull, k, int(bad.sum()))
        assert torch.equal(got, bvh.render_depth(np.stack(c2ws), H, W, FX, FY, CX, CY, 0.05, 5.0, cull=cull))


def test_closed_box_from_inside_and_nonfinite_poses():
    v, f = R.grid_box((-1, -1, -1), (1, 1, 1), 0.5, toward_inside=False)       # outward normals: back faces from inside
    bvh = raycast.MeshBVH(v, f, DEV)
    c2ws = np.stack([R.look_at((0.1, 0.2, 0.0), (1.0, 0.5, 0.3)), R.look_at((0.0, 0.0, 0.2), (-0.3, 1.0, -0.8))])
    plain = bvh.render_depth(c2ws, H, W, FX, FY, CX, CY, 0.05, 10.0)
    assert (plain > 0).all()
    assert (bvh.render_depth(c2ws, H, W, FX, FY, CX, CY, 0.05, 10.0, cull='back') == 0).all()
    assert torch.equal(bvh.render_depth(c2ws, H, W, FX, FY, CX, CY, 0.05, 10.0, cull='front'), plain)
    bad = c2ws.copy()
    bad[0, 0, 3] = np.nan
    bad[1, 2, 1] = np.inf
    for cull in ('back', 'front'):
        assert (bvh.render_depth(bad, H, W, FX, FY, CX, CY, 0.05, 10.0, cull=cull) == 0).all()
    torch.cuda.synchronize()


# ---- touch marks ----
def test_touch_marks_match_oracle():
    rng = np.random.default_rng(5)
    P, h, w = 5, 23, 37
    depth = rng.uniform(0.2, 6.0, (P, h, w)).astype(np.float32)               # some beyond depth_trunc = 5
    depth[rng.random((P, h, w)) < 0.2] = 0.0
    depth[1, 0, 0], depth[1, 4, 8] = 5.0, np.float32(5.0000005)               # exactly at and just past the cut
    poses = [R.look_at(rng.uniform(-0.3, 0.3, 3), rng.uniform(-1, 1, 3) + 2.0) for _ in range(P)]
    poses[2][0, 3] = np.nan                                                    # a partly non-finite pose touches nothing
    poses[3][:3, 3] += 1e3                                                    # far outside the box: counted, marks nothing
    rows = np.stack([p[:3, :4].reshape(-1) for p in poses])
    box = refusion.UnitBox([-6, -6, -6], [14, 13, 12], 0.01)
    dev = torch.device(DEV)
    outside = torch.zeros(1, dtype=torch.int32, device=dev)
    got = refusion.touch(torch.from_numpy(depth).to(dev), torch.from_numpy(rows).to(dev), box, FX, FY, CX, CY, 4, 5.0, 0.03,
                         outside)
    want, n_out = R.touch(depth, rows, FX, FY, CX, CY, 4, 5.0, 0.03, box.unit_length, box.lo, box.dim)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(outside.item()) == n_out > 0
    assert want[2].sum() == 0 and want[3].sum() == 0 and want[0].sum() > 0
    # a box holding every point: nothing outside
    d2 = np.minimum(depth[[0, 1, 4]], np.float32(3.0))
    r2 = rows[[0, 1, 4]]
    big = refusion.UnitBox([-40, -40, -40], [80, 80, 80], 0.01)
    outside.zero_()
    got = refusion.touch(torch.from_numpy(d2).to(dev), torch.from_numpy(r2).to(dev), big, FX, FY, CX, CY, 4, 5.0, 0.03, outside)
    want, n_out = R.touch(d2, r2, FX, FY, CX, CY, 4, 5.0, 0.03, big.unit_length, big.lo, big.dim)
    assert n_out == 0 and int(outside.item()) == 0
    assert np.array_equal(got.cpu().numpy(), want)


# ---- integration ----
def fuse_on_device(depth, w2c, bp, box, tsdf0, weight0, chunk):
    dev = torch.device(DEV)
    tsdf = torch.from_numpy(tsdf0).to(dev)
    weight = torch.from_numpy(weight0).to(dev)
    outside = torch.zeros(1, dtype=torch.int32, device=dev)
    for p0 in range(0, len(depth), chunk):
        d = torch.from_numpy(depth[p0:p0 + chunk]).to(dev).contiguous()
        touched = refusion.touch(d, torch.from_numpy(bp[p0:p0 + chunk]).to(dev).contiguous(), box, FX, FY, CX, CY, 4, 5.0, 0.03,
                                 outside)
        units = torch.nonzero(touched.any(0)).reshape(-1).to(torch.int32).contiguous()
        refusion.integrate(tsdf, weight, box, units, d, torch.from_numpy(w2c[p0:p0 + chunk]).to(dev).contiguous(), touched, FX, FY,
                           CX, CY, 0.03, 5.0)
    assert int(outside.item()) == 0
    return tsdf.cpu().numpy(), weight.cpu().numpy()


@pytest.fixture(scope='module')
def fused():
    v, f = inverted_scene()
    poses = poses32(20)
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    lo, dim = R.unit_box(v, 0.01, 0.03)
    box = refusion.UnitBox(lo.tolist(), dim.tolist(), 0.01)
    w2c = R.w2c_rows(poses)
    bp = R.backproject_rows(w2c)
    depth = np.stack([R.render_depth_cull(v, f, p.astype(np.float64), H, W, FX, FY, CX - 0.5, CY - 0.5, 0.05, 5.0, 'back')
                      for p in poses])
    rng = np.random.default_rng(1)
    tsdf0 = rng.uniform(-1, 1, box.shape).astype(np.float32)
    weight0 = rng.integers(0, 3, box.shape).astype(np.float32)
    touched, _ = R.touch(depth, bp, FX, FY, CX, CY, 4, 5.0, 0.03, box.unit_length, box.lo, box.dim)
    tsdf, weight = tsdf0.copy(), weight0.copy()
    R.integrate(tsdf, weight, box.lo, box.dim, 0.01, depth, w2c, touched, FX, FY, CX, CY, 0.03, 5.0)
    return dict(v=v, f=f, poses=poses, K=K, box=box, w2c=w2c, bp=bp, depth=depth, tsdf0=tsdf0, weight0=weight0, touched=touched,
                tsdf=tsdf, weight=weight)


def test_integration_matches_oracle_and_chunking(fused):
    z = fused
    # the device render feeds the device pipeline in evaluate_scannet: it equals the oracle's depths
    bvh = raycast.MeshBVH(z['v'], z['f'], DEV)
    dd = bvh.render_depth(np.stack([p.astype(np.float64) for p in z['poses']]), H, W, FX, FY, CX - 0.5, CY - 0.5, 0.05, 5.0,
                          cull='back')
    assert np.array_equal(dd.cpu().numpy(), z['depth'])
    results = []
    for chunk in (20, 1, 3, 7):
        t, w = fuse_on_device(z['depth'], z['w2c'], z['bp'], z['box'], z['tsdf0'], z['weight0'], chunk)
        results.append((t, w))
    t, w = results[0]
    assert (w != z['weight0']).any()
    bad = (t.view(np.uint32) != z['tsdf'].view(np.uint32)) | (w != z['weight'])
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5])
    for t2, w2 in results[1:]:
        assert np.array_equal(t2.view(np.uint32), t.view(np.uint32)) and np.array_equal(w2, w)
    # voxels of units no view touched keep their initial values
    box = z['box']
    untouched = ~z['touched'].any(0).astype(bool)
    assert untouched.any()
    uid = np.arange(box.n_units).reshape(box.dim)
    full = np.repeat(np.repeat(np.repeat(uid, 16, 0), 16, 1), 16, 2)
    keep = untouched[full]
    assert np.array_equal(t[keep].view(np.uint32), z['tsdf0'][keep].view(np.uint32)) and np.array_equal(w[keep], z['weight0'][keep])


def test_extraction_vertex_set(fused):
    z = fused
    box = z['box']
    shape = box.shape
    tsdf, weight = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    R.integrate(tsdf, weight, box.lo, box.dim, 0.01, z['depth'], z['w2c'], z['touched'], FX, FY, CX, CY, 0.03, 5.0)
    v, f = refusion.extract(torch.from_numpy(tsdf).to(DEV), torch.from_numpy(weight).to(DEV), box)
    v, f = v.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    want = R.extract_vertices(tsdf, weight, box.lo, 0.01)
    assert len(want) > 1000 and v.shape == want.shape
    a = v[np.lexsort(v.T[::-1])]
    b = want[np.lexsort(want.T[::-1])]
    assert np.abs(a.astype(np.float64) - b).max() <= 1e-6 * 0.01
    used = np.zeros(len(v), bool)
    used[f.reshape(-1)] = True
    assert used.all()
    # every face lies in a cube whose 8 corners were all observed
    org = np.array([(16 * box.lo[c] + 0.5) * 0.01 for c in range(3)])
    idx = (v.astype(np.float64) - org) / 0.01
    snap = np.where(np.abs(idx - np.round(idx)) < 1e-3, np.round(idx), idx)
    tri = snap[f]                                                            # [F,3,3]
    lo_c = np.ceil(tri).max(1) - 1
    hi_c = np.floor(tri).min(1)
    obs = weight > 0
    for c in range(f.shape[0]):
        ok = False
        for i in range(int(lo_c[c, 0]), int(hi_c[c, 0]) + 1):
            for j in range(int(lo_c[c, 1]), int(hi_c[c, 1]) + 1):
                for k in range(int(lo_c[c, 2]), int(hi_c[c, 2]) + 1):
                    if 0 <= i < shape[0] - 1 and 0 <= j < shape[1] - 1 and 0 <= k < shape[2] - 1 and obs[i:i + 2, j:j + 2, k:k + 2].all():
                        ok = True
        assert ok, c


# ---- voxel downsample ----
@pytest.mark.parametrize('case', ['room', 'wide'])
def test_voxel_down_sample_matches_oracle(case):
    rng = np.random.default_rng(7)
    if case == 'room':
        p = rng.uniform(-1.0, 1.0, (20000, 3))
        p[::3] = np.round(p[::3] / 0.02) * 0.02                                # points on cell boundaries
        vs = 0.02
    else:
        p = np.concatenate([rng.uniform(-1.0, 1.0, (3000, 3)), rng.uniform(-900.0, 900.0, (3000, 3))])   # keys of > 31 bits
        vs = 0.02
    got, cnt = refusion.voxel_down_sample(p, vs, DEV)
    want, wcnt = R.voxel_down_sample(p, vs)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(cnt.cpu().numpy(), wcnt)
    again, cnt2 = refusion.voxel_down_sample(p, vs, DEV)
    assert torch.equal(again, got) and torch.equal(cnt2, cnt)


def test_voxel_down_sample_limits():
    with pytest.raises(RuntimeError, match='UNSUPPORTED'):
        refusion.voxel_down_sample(np.array([[0.0, 0, 0], [1e5, 0, 0]]), 0.02, DEV)           # 5e6 cells along x
    got, cnt = refusion.voxel_down_sample(np.zeros((0, 3)), 0.02, DEV)
    assert got.shape == (0, 3) and cnt.shape == (0,)
    got, cnt = refusion.voxel_down_sample(np.array([[0.5, 0.5, 0.5]] * 4), 0.02, DEV)
    assert got.shape == (1, 3) and cnt.tolist() == [4]


# ---- end to end ----
def write_tree(root, n_frames=200, nonfinite=True):
    """A synthetic ScanNet tree under root: configs, frames/color (empty .jpg), frames/pose, the predicted mesh (the room, a few cm
    off) and the ground-truth mesh (.obj)."""
    os.makedirs(os.path.join(root, 'configs', 'ScanNet'), exist_ok=True)
    with open(os.path.join(root, 'configs', 'df_prior.yaml'), 'w') as fh:
        fh.write('scale: 1\ndataset: replica\ncam:\n  crop_edge: 0\n')
    with open(os.path.join(root, 'configs', 'ScanNet', 'scannet.yaml'), 'w') as fh:
        fh.write(f'dataset: scannet\ncam:\n  H: {H + 4}\n  W: {W + 4}\n  fx: {FX}\n  fy: {FY}\n  cx: {CX + 2}\n  cy: {CY + 2}\n'
                 f'  png_depth_scale: 1000.\n  crop_edge: 2\n')
    with open(os.path.join(root, 'configs', 'ScanNet', 'scene0077.yaml'), 'w') as fh:
        fh.write('inherit_from: configs/ScanNet/scannet.yaml\ndata:\n  dataset: scannet\n'
                 '  input_folder: Datasets/scannet/scans/scene0077_00\n  output: output/scannet/scans/scene0077_00\n  id: 77\n')
    fr = os.path.join(root, 'Datasets', 'scannet', 'scans', 'scene0077_00', 'frames')
    os.makedirs(os.path.join(fr, 'color'), exist_ok=True)
    os.makedirs(os.path.join(fr, 'pose'), exist_ok=True)
    poses = R.orbit_poses(n_frames // 10 + 1, seed=2)
    for i in range(n_frames):
        open(os.path.join(fr, 'color', f'{i}.jpg'), 'wb').close()
        m = poses[i // 10] if i % 10 == 0 else R.look_at((0, 0, 0), (1, 0, 0))
        if nonfinite and i == 30:
            m = np.full((4, 4), -np.inf)
        with open(os.path.join(fr, 'pose', f'{i}.txt'), 'w') as fh:
            fh.write('\n'.join(' '.join(repr(float(x)) for x in row) for row in m) + '\n')
    md = os.path.join(root, 'output', 'scannet', 'scans', 'scene0077_00', 'mesh')
    os.makedirs(md, exist_ok=True)
    pv, pf = R.scene(step=0.05, shift=(0.02, -0.03, 0.0))
    mesh.write_ply(os.path.join(md, 'final_mesh.ply'), pv, pf)
    gv, gf = R.scene(step=0.025)
    gd = os.path.join(root, 'Datasets', 'scannet', 'GTmesh_lowres')
    os.makedirs(gd, exist_ok=True)
    with open(os.path.join(gd, '0077_00.obj'), 'w') as fh:
        fh.write(''.join(f'v {x!r} {y!r} {z!r}\n' for x, y, z in gv.tolist()))
        fh.write(''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in gf.tolist()))


def run_cli(root, monkeypatch, *extra):
    monkeypatch.chdir(root)
    monkeypatch.setattr(sys, 'argv', ['evaluate_scannet', 'configs/ScanNet/scene0077.yaml'] + list(extra))
    return E.evaluate_mesh()


def test_evaluate_mesh_end_to_end(tmp_path, monkeypatch, capsys):
    write_tree(str(tmp_path))
    got = run_cli(str(tmp_path), monkeypatch)
    printed = capsys.readouterr().out
    assert "'F-score'" in printed and "'Acc'" in printed
    out = tmp_path / 'output' / 'scannet' / 'scans' / 'scene0077_00' / 'mesh' / 'final_mesh_refused.ply'
    first = out.read_bytes()
    # the oracle pipeline: the same poses, oracle render / touch / integrate / extract, the vertices as written (f32), cKDTree
    cfg = E.load_config(str(tmp_path / 'configs' / 'ScanNet' / 'scene0077.yaml'), str(tmp_path / 'configs' / 'df_prior.yaml'))

    class A:
        input_folder = None
    poses, K, h, w = E.get_pose(cfg, A)
    assert len(poses) == 19                                   # 20 kept frames, the all -inf one dropped
    pm = E.load_mesh(str(tmp_path / 'output' / 'scannet' / 'scans' / 'scene0077_00' / 'mesh' / 'final_mesh.ply'))
    _, _, fx, fy, cx, cy = E.update_cam(cfg)
    ts, wt, lo, dim, _ = R.refuse_tsdf(pm.vertices, pm.faces[:, ::-1], poses, K, h, w, fx, fy, cx, cy)
    ov = R.extract_vertices(ts, wt, lo, 0.01).astype(np.float64)
    rv = E.load_mesh(str(out)).vertices
    assert len(rv) == len(ov)
    assert np.array_equal(rv[np.lexsort(rv.T[::-1])], ov[np.lexsort(ov.T[::-1])])
    gt = E.load_mesh(str(tmp_path / 'Datasets' / 'scannet' / 'GTmesh_lowres' / '0077_00.obj'))
    want = R.evaluate(rv, gt.vertices)
    n_pred, n_gt = len(R.voxel_down_sample(rv, 0.02)[0]), len(R.voxel_down_sample(gt.vertices, 0.02)[0])
    for k in ('Acc', 'Comp', 'Chamfer'):
        assert abs(got[k] - want[k]) <= 1e-6, (k, got[k], want[k])
    assert abs(got['Prec'] - want['Prec']) <= 1.0 / n_pred and abs(got['Recal'] - want['Recal']) <= 1.0 / n_gt
    assert 0.0 < got['F-score'] < 1.0 and got['Acc'] < 0.05
    assert set(got) == {'Acc', 'Comp', 'Chamfer', 'Prec', 'Recal', 'F-score'} and all(type(x) is float for x in got.values())
    # a rerun writes the same bytes; a mesh compared with itself scores 1
    run_cli(str(tmp_path), monkeypatch)
    assert out.read_bytes() == first
    self_m = E.evaluate(gt, gt)
    assert self_m['F-score'] == 1.0 and self_m['Acc'] == 0.0


def test_missing_input_names_the_file(tmp_path, monkeypatch, capsys):
    write_tree(str(tmp_path), n_frames=20, nonfinite=False)
    os.remove(tmp_path / 'Datasets' / 'scannet' / 'GTmesh_lowres' / '0077_00.obj')
    with pytest.raises(SystemExit) as e:
        run_cli(str(tmp_path), monkeypatch)
    assert e.value.code != 0
    assert '0077_00.obj' in capsys.readouterr().err


def test_touch_and_integrate_without_views_or_units():
    dev = torch.device(DEV)
    box = refusion.UnitBox([-6, -6, -6], [14, 13, 12], 0.01)
    outside = torch.zeros(1, dtype=torch.int32, device=dev)
    none = refusion.touch(torch.zeros((0, 6, 8), device=dev), torch.zeros((0, 12), dtype=torch.float64, device=dev), box, FX, FY, CX, CY,
                          4, 5.0, 0.03, outside)
    assert none.shape == (0, box.n_units) and none.dtype == torch.uint8 and int(outside.item()) == 0
    tsdf = torch.full((4, 4, 4), 0.25, device=dev)
    weight = torch.zeros((4, 4, 4), device=dev)
    d = torch.ones((1, 6, 8), device=dev)
    w2c = torch.zeros((1, 12), dtype=torch.float32, device=dev)
    touched = torch.zeros((1, box.n_units), dtype=torch.uint8, device=dev)
    refusion.integrate(tsdf, weight, box, torch.zeros(0, dtype=torch.int32, device=dev), d, w2c, touched, FX, FY, CX, CY, 0.03, 5.0)
    refusion.integrate(tsdf, weight, box, torch.zeros(1, dtype=torch.int32, device=dev), d[:0], w2c[:0], touched[:0], FX, FY, CX, CY, 0.03, 5.0)
    assert (tsdf == 0.25).all() and (weight == 0).all()
