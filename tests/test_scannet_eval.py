"""CPU: the host side of attentive_dfprior_amd.evaluate_scannet against golden values from the reference's own evaluate_scannet.py
(tests/golden/make_scannet_golden.py) -- signatures, update_cam, get_pose over a synthetic ScanNet folder, refuse's camera and
volume settings, evaluate's formulas (refuse_ref's numpy pipeline); read_obj, load_config inheritance, trimesh-style vertex
handling; and the new C-ABI entries' argument errors and workspace formulas without a launch."""
import ctypes as C
import inspect
import json
import os
import types

import numpy as np
import pytest

import refuse_ref as R
from attentive_dfprior_amd import _lib, evaluate_scannet as E, mesh
from conftest import GOLDEN, ROOT

D = C.c_void_p(16)                                  # never dereferenced: every call below fails (or returns) before any launch
BIG = 2 ** 31


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN, 'mini_scannet.npz'))
    return {k: z[k] for k in z.files}


def test_signatures_match_reference():
    want = json.load(open(os.path.join(GOLDEN, 'scannet_signatures.json')))
    for name, sig in want.items():
        assert str(inspect.signature(getattr(E, name))) == sig, name


def write_cfgs(root):
    os.makedirs(os.path.join(root, 'configs', 'ScanNet'))
    with open(os.path.join(root, 'configs', 'df_prior.yaml'), 'w') as fh:
        fh.write('scale: 1\ndataset: replica\ncam:\n  H: 680\n  W: 1200\n  crop_edge: 0\n  png_depth_scale: 6553.5\n'
                 'mapping:\n  bound: [[0, 1]]\n  iters: 3\n')
    with open(os.path.join(root, 'configs', 'ScanNet', 'scannet.yaml'), 'w') as fh:
        fh.write('dataset: scannet\ncam:\n  H: 480\n  W: 640\n  fx: 577.590698\n  fy: 578.729797\n  cx: 318.905426\n'
                 '  cy: 242.683609\n  png_depth_scale: 1000.\n  crop_edge: 10\nmapping:\n  iters: 60\n')
    with open(os.path.join(root, 'configs', 'ScanNet', 'scene0050.yaml'), 'w') as fh:
        fh.write('inherit_from: configs/ScanNet/scannet.yaml\nmapping:\n  bound: [[0.5,7.0],[0.0,4.5],[-0.5,3.0]]\n'
                 'data:\n  dataset: scannet\n  input_folder: Datasets/scannet/scans/scene0050_00\n  id: 50\n')


def test_load_config_inherits(tmp_path, monkeypatch):
    write_cfgs(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg = E.load_config('configs/ScanNet/scene0050.yaml', 'configs/df_prior.yaml')
    assert cfg['dataset'] == 'scannet' and cfg['scale'] == 1
    assert cfg['cam']['H'] == 480 and cfg['cam']['crop_edge'] == 10 and cfg['cam']['png_depth_scale'] == 1000.
    assert cfg['mapping'] == {'bound': [[0.5, 7.0], [0.0, 4.5], [-0.5, 3.0]], 'iters': 60}
    assert cfg['data']['id'] == 50
    assert E.load_config('configs/ScanNet/scannet.yaml')['cam']['W'] == 640          # no default: the file alone


def test_update_cam_and_get_pose_match_reference(gold, tmp_path, monkeypatch):
    write_cfgs(str(tmp_path))
    monkeypatch.chdir(tmp_path)
    cfg = E.load_config('configs/ScanNet/scene0050.yaml', 'configs/df_prior.yaml')
    assert np.array_equal(np.array(E.update_cam(cfg), np.float64), gold['cam'])
    crop = {'cam': dict(cfg['cam'], crop_size=[384, 512])}
    H, W, fx, fy, cx, cy = E.update_cam(crop)
    assert (H, W) == (364, 492) and fx == 512 / 640 * 577.590698 and cx == 512 / 640 * 318.905426 - 10
    fr = tmp_path / 'scene' / 'frames'
    for d in ('color', 'pose'):
        (fr / d).mkdir(parents=True)
    for i, m in enumerate(gold['tree_poses']):
        (fr / 'color' / f'{i}.jpg').write_bytes(b'')
        (fr / 'pose' / f'{i}.txt').write_text('\n'.join(' '.join(repr(float(x)) for x in row) for row in m) + '\n')
    poses, K, H, W = E.get_pose(cfg, types.SimpleNamespace(input_folder=str(tmp_path / 'scene')))
    assert len(poses) == len(gold['poses']) == 2                              # frame 10 (all -inf) dropped, frame 20 kept
    for p, q in zip(poses, gold['poses']):
        assert p.dtype == np.float32 and gold['pose_dtype_f32']
        assert np.array_equal(p, q, equal_nan=True)
    assert np.array_equal(K, gold['K']) and [H, W] == gold['HW'].tolist()
    with pytest.raises(NotImplementedError, match='replica'):
        E.get_pose(dict(cfg, dataset='replica'), types.SimpleNamespace(input_folder=None))


def test_refuse_settings_match_reference(gold):
    """What the reference hands pyrender and open3d, against the port's constants and arithmetic."""
    H, W = gold['HW'].tolist()
    assert (gold['refuse.viewport'] == [H, W]).all()
    K = gold['K']
    assert (gold['refuse.gl_cam'] == [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]).all()
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    for p, g in zip(gold['poses'], gold['refuse.gl_pose']):
        assert np.allclose(p.astype(np.float64) @ flip, g, equal_nan=True, atol=1e-15)   # fix_pose: OpenCV -> GL axes
    assert bool(gold['refuse.extrinsic_f32'])
    w2c = R.w2c_rows(list(gold['poses']))
    for k, e in enumerate(gold['refuse.extrinsic']):
        assert np.array_equal(w2c[k], e[:3, :4].astype(np.float32).reshape(-1), equal_nan=True)
    from attentive_dfprior_amd import refusion
    assert np.array_equal(refusion.w2c_rows(list(gold['poses'])), w2c, equal_nan=True)
    assert (gold['refuse.rgbd'] == [1.0, E.DEPTH_TRUNC, 0.0]).all()
    assert gold['refuse.volume'].tolist() == [E.VOXEL, E.SDF_TRUNC]
    cam = gold['cam']
    assert (gold['refuse.o3d_intrinsic'] == [cam[1], cam[0], cam[2], cam[3], cam[4], cam[5]]).all()


def test_evaluate_formulas_match_reference(gold):
    """refuse_ref.evaluate (the numpy pipeline the GPU tests hold the device to) against the reference's evaluate: the real KDTree
    without downsampling; with down_sample=0.02 the golden's stub called the same oracle, so this pins the formulas only."""
    a, b = gold['eval.a'], gold['eval.b']
    keys = ['Acc', 'Comp', 'Chamfer', 'Prec', 'Recal', 'F-score']
    for name, ds in (('none', None), ('ds02', 0.02)):
        m = R.evaluate(a, b, down_sample=ds)
        assert np.allclose([m[k] for k in keys], gold[f'eval.{name}'], rtol=1e-12, atol=0), name


def test_nn_correspondance_empty():
    assert E.nn_correspondance(np.zeros((0, 3)), np.ones((4, 3))) == ([], [])
    assert E.nn_correspondance(np.ones((4, 3)), []) == ([], [])


def test_read_obj_forms(tmp_path):
    p = tmp_path / 'm.obj'
    p.write_text('# comment\nmtllib x.mtl\no thing\n'
                 'v 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n'
                 'f 1 2 3\nf 1/1 3/1 4/1\ng part\nusemtl m\nf 1//1 2//1 3//1 4//1\nf -4/1/1 -3/1/1 -2/1/1\ns off\n'
                 'v 2 2 2\nf 1 2 3 4 -1\n')
    m = mesh.read_obj(str(p))
    assert m.verts.dtype == np.float64 and m.verts.shape == (5, 3) and m.verts[1].tolist() == [1, 0, 0]
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    empty = tmp_path / 'e.obj'
    empty.write_text('v 1 2 3\n')
    e = mesh.read_obj(str(empty))
    assert e.verts.shape == (1, 3) and e.faces.shape == (0, 3)


def test_loaded_mesh_keeps_referenced_and_merges_duplicates():
    v = np.array([[0, 0, 0], [9, 9, 9], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    f = np.array([[0, 2, 3], [4, 3, 5]])
    m = E.LoadedMesh(v, f)
    assert m.vertices.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    assert m.faces.tolist() == [[0, 1, 2], [1, 2, 3]]


def test_missing_config_exits_naming_it(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr('sys.argv', ['evaluate_scannet', 'configs/ScanNet/nope.yaml'])
    with pytest.raises(SystemExit) as e:
        E.evaluate_mesh()
    assert e.value.code != 0 and 'nope.yaml' in capsys.readouterr().err


# ---- C ABI, no launch ----
def al256(b):
    return (b + 255) // 256 * 256


def test_new_symbols_and_constants():
    L = _lib.lib()
    assert _lib.ABI_VERSION == 134 == L.adfp_version()
    for n in ('adfp_render_depth_cull', 'adfp_refuse_touch', 'adfp_refuse_integrate', 'adfp_voxel_down_sample',
              'adfp_voxel_down_sample_workspace_bytes'):
        assert hasattr(L, n) and n in {s[0] for s in _lib.SYMBOLS}
    src = open(os.path.join(ROOT, 'include', 'adfp.h')).read()
    for k, v in _lib.CULL.items():
        assert f'#define ADFP_CULL_{k.upper()} ' in src and f'ADFP_CULL_{k.upper()}' in src
        assert int(src.split(f'#define ADFP_CULL_{k.upper()}')[1].split()[0]) == v
    assert int(src.split('#define ADFP_UNIT_VOXELS')[1].split()[0]) == _lib.UNIT_VOXELS == 16


def test_voxel_down_sample_workspace_formula():
    L = _lib.lib()
    for n in (1, 5, 1023, 1024, 1025, 100000):
        T = -(-n // 1024)
        want = al256(8 * n) + 5 * al256(4 * n) + al256(4 * T) + al256(8 * T) + al256(L.adfp_sort_workspace_bytes(n))
        assert L.adfp_voxel_down_sample_workspace_bytes(n) == want
    assert L.adfp_voxel_down_sample_workspace_bytes(0) == 0 and L.adfp_voxel_down_sample_workspace_bytes(-3) == 0
    assert L.adfp_voxel_down_sample_workspace_bytes(BIG) == 0


def test_render_cull_argument_errors():
    L = _lib.lib()
    bb = L.adfp_tri_bvh_bytes(100, 8)

    def r(cull=1, bvh=D, bvhb=bb, nf=100, views=3, far=20.0, H=64, depth=D):
        return L.adfp_render_depth_cull(bvh, bvhb, nf, 8, D, D, far, views, H, 48, 300.0, 300.0, 24.0, 32.0, cull, depth, None)
    assert r(cull=3) == -1 and r(cull=-1) == -1
    assert r(bvh=None) == -1 and r(depth=None) == -1 and r(far=0.0) == -1
    assert r(H=40000) == -2
    assert r(bvhb=bb - 1) == -3
    assert r(views=0, bvh=None, depth=None) == 0


def test_touch_argument_errors():
    L = _lib.lib()
    lo, dim = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(4, 4, 4)

    def t(depth=D, n=2, H=8, W=8, c2w=D, fx=10.0, stride=4, dt=5.0, tr=0.03, unit=0.16, lo=lo, dim=dim, out=D, outside=D):
        return L.adfp_refuse_touch(depth, n, H, W, c2w, fx, 10.0, 4.0, 4.0, stride, dt, tr, unit, C.byref(lo), C.byref(dim), out,
                                   outside, None)
    assert t(depth=None) == -1 and t(c2w=None) == -1 and t(out=None) == -1 and t(outside=None) == -1
    assert t(n=-1) == -1 and t(H=0) == -1 and t(stride=0) == -1 and t(fx=0.0) == -1 and t(fx=float('nan')) == -1
    assert t(dt=0.0) == -1 and t(tr=-0.1) == -1 and t(unit=0.0) == -1 and t(unit=float('inf')) == -1
    assert t(dim=(C.c_int * 3)(4, 0, 4)) == -1
    assert t(dim=(C.c_int * 3)(2048, 2048, 1024)) == -2
    assert t(W=40000) == -2
    assert t(n=0, depth=None, c2w=None, out=None, outside=None) == 0


def test_integrate_argument_errors():
    L = _lib.lib()
    lo, dim = (C.c_int * 3)(0, 0, 0), (C.c_int * 3)(4, 4, 4)

    def g(ts=D, wt=D, voxel=0.01, units=D, nu=3, depth=D, w2c=D, touched=D, n=2, H=8, tr=0.03, dt=5.0, dim=dim):
        return L.adfp_refuse_integrate(ts, wt, C.byref(lo), C.byref(dim), voxel, units, nu, depth, w2c, touched, n, H, 8, 10.0, 10.0,
                                       4.0, 4.0, tr, dt, None)
    assert g(ts=None) == -1 and g(wt=None) == -1 and g(units=None) == -1 and g(depth=None) == -1
    assert g(w2c=None) == -1 and g(touched=None) == -1
    assert g(nu=-1) == -1 and g(n=-1) == -1 and g(H=0) == -1 and g(voxel=0.0) == -1 and g(tr=0.0) == -1 and g(dt=0.0) == -1
    assert g(dim=(C.c_int * 3)(0, 4, 4)) == -1
    assert g(nu=65) == -2 and g(n=65537) == -2
    assert g(nu=0, ts=None, wt=None, units=None) == 0 and g(n=0, depth=None, w2c=None, touched=None) == 0


def test_voxel_down_sample_argument_errors():
    L = _lib.lib()
    wb = L.adfp_voxel_down_sample_workspace_bytes(100)
    lo, hi = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)

    def v(p=D, n=100, vs=0.02, lo=lo, hi=hi, ws=D, wsb=wb, out=D, cnt=D, tot=D):
        return L.adfp_voxel_down_sample(p, n, vs, C.byref(lo) if lo is not None else None, C.byref(hi) if hi is not None else None,
                                        ws, wsb, out, cnt, tot, None)
    assert v(p=None) == -1 and v(ws=None) == -1 and v(out=None) == -1 and v(cnt=None) == -1 and v(tot=None) == -1
    assert v(lo=None) == -1 and v(n=-1) == -1 and v(vs=0.0) == -1 and v(vs=float('nan')) == -1
    assert v(lo=(C.c_double * 3)(2, 0, 0)) == -1 and v(hi=(C.c_double * 3)(1, float('inf'), 1)) == -1
    assert v(hi=(C.c_double * 3)(1e5, 1, 1)) == -2                                           # 5e6 cells along x
    assert v(wsb=wb - 1) == -3
