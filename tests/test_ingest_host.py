"""CPU: the host side of the dataset drop-ins (attentive_dfprior_amd/datasets.py, get_tsdf.py) on tiny Replica- and ScanNet-layout
directories written with PIL: attributes, file order, pose parsing, dispatch and refusals, update_cam, the config merge, and the
call signatures recorded from the reference (tests/golden/datasets_signatures.json, tests/golden/make_datasets_golden.py).
Constructing a dataset needs no GPU; the frames themselves are tests/test_gpu_ingest.py's."""
import inspect
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import ingest_ref
from conftest import GOLDEN
from attentive_dfprior_amd import datasets, get_tsdf

RNG = np.random.RandomState(7)


def _assert_compatible(mine, ref, what):
    """The reference's parameters (name, kind, default) come first and unchanged; anything after them has a default or is **kw."""
    pm = [(p.name, p.kind, p.default) for p in inspect.signature(mine).parameters.values()]
    pr = [(n, getattr(inspect.Parameter, k), d if has else inspect.Parameter.empty) for n, k, has, d in ref]
    assert pm[:len(pr)] == pr, f'{what}: {pm} against the reference\'s {pr}'
    for n, k, d in pm[len(pr):]:
        assert d is not inspect.Parameter.empty or k in (inspect.Parameter.VAR_KEYWORD, inspect.Parameter.VAR_POSITIONAL), \
            f'{what}: extra required parameter {n!r}'


def golden():
    with open(os.path.join(GOLDEN, 'datasets_signatures.json')) as f:
        return json.load(f)


def cam(H, W, **kw):
    return dict(dict(H=H, W=W, fx=30.0, fy=31.0, cx=W / 2 - 0.5, cy=H / 2 - 0.5, png_depth_scale=6553.5, crop_edge=0), **kw)


def pose_rows(k):
    m = np.eye(4)
    m[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]) if k % 2 else np.eye(3)
    m[:3, 3] = [0.1 * k, -0.2 * k, 0.3 + k]
    return m + np.arange(16).reshape(4, 4) * 1e-3


def write_replica(root, n=3, hw=(6, 8)):
    os.makedirs(os.path.join(root, 'results'))
    for k in range(n):
        Image.fromarray(RNG.randint(0, 256, hw + (3,), dtype=np.uint8)).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'))
        Image.fromarray(RNG.randint(0, 65536, hw).astype(np.uint16)).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        for k in range(n + 1):                          # one line more than frames: only the first n are read
            f.write(' '.join(repr(float(v)) for v in pose_rows(k).reshape(-1)) + '\n')
    return root


SCANNET_STEMS = [0, 1, 2, 9, 10, 100]


def write_scannet(root, color_hw=(9, 12), depth_hw=(6, 8), bad=9):
    for sub in ('color', 'depth', 'pose'):
        os.makedirs(os.path.join(root, 'frames', sub))
    for k in SCANNET_STEMS:
        Image.fromarray(RNG.randint(0, 256, color_hw + (3,), dtype=np.uint8)).save(os.path.join(root, 'frames', 'color', f'{k}.jpg'))
        Image.fromarray(RNG.randint(0, 65536, depth_hw).astype(np.uint16)).save(os.path.join(root, 'frames', 'depth', f'{k}.png'))
        with open(os.path.join(root, 'frames', 'pose', f'{k}.txt'), 'w') as f:
            for row in pose_rows(k):
                f.write(' '.join('-inf' if k == bad else repr(float(v)) for v in row) + '\n')
    return root


def replica_cfg(root, scale=1.0, **camkw):
    return {'dataset': 'replica', 'scale': scale, 'cam': cam(6, 8, **camkw), 'data': {'input_folder': root}}


def scannet_cfg(root, **camkw):
    return {'dataset': 'scannet', 'cam': cam(6, 8, png_depth_scale=1000.0, crop_edge=1, **camkw), 'data': {'input_folder': root}}


ARGS = SimpleNamespace(input_folder=None)


def expected_pose(k):
    m = pose_rows(k)
    m[:3, 1] *= -1
    m[:3, 2] *= -1
    return torch.from_numpy(m).float()


def test_replica_attributes_paths_and_poses(tmp_path):
    root = write_replica(str(tmp_path / 'room'))
    ds = datasets.get_dataset(replica_cfg(root), ARGS, 1.0)
    assert type(ds) is datasets.Replica and isinstance(ds, datasets.BaseDataset) and isinstance(ds, torch.utils.data.Dataset)
    g = golden()['attributes']
    for name in g['BaseDataset'] + g['Replica']:
        assert hasattr(ds, name), name
    assert (ds.n_img, len(ds), len(ds.poses)) == (3, 3, 3)
    assert (ds.H, ds.W, ds.fx, ds.fy, ds.cx, ds.cy) == (6, 8, 30.0, 31.0, 3.5, 2.5)
    assert (ds.png_depth_scale, ds.crop_size, ds.crop_edge, ds.distortion, ds.input_folder) == (6553.5, None, 0, None, root)
    assert (ds.name, ds.scale, ds.device) == ('replica', 1.0, 'cuda:0')
    assert [os.path.basename(p) for p in ds.color_paths] == [f'frame{k:06d}.jpg' for k in range(3)]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f'depth{k:06d}.png' for k in range(3)]
    for k in range(3):
        assert ds.poses[k].dtype == torch.float32 and torch.equal(ds.poses[k], expected_pose(k))
    # --input_folder has priority over the config's
    other = write_replica(str(tmp_path / 'other'), n=2)
    assert datasets.get_dataset(replica_cfg(root), SimpleNamespace(input_folder=other), 1.0).n_img == 2


def test_scannet_sorts_by_integer_stem_and_reads_poses(tmp_path):
    root = write_scannet(str(tmp_path / 'scene'))
    ds = datasets.get_dataset(scannet_cfg(root), ARGS, 1.0, device='cuda:0')
    assert type(ds) is datasets.ScanNet
    for name in golden()['attributes']['ScanNet']:
        assert hasattr(ds, name), name
    assert ds.input_folder == os.path.join(root, 'frames')
    assert [os.path.basename(p) for p in ds.color_paths] == [f'{k}.jpg' for k in SCANNET_STEMS]        # 10.jpg after 9.jpg
    assert [os.path.basename(p) for p in ds.depth_paths] == [f'{k}.png' for k in SCANNET_STEMS]
    assert ds.n_img == len(ds) == len(ds.poses) == len(SCANNET_STEMS)
    for i, k in enumerate(SCANNET_STEMS):
        if k == 9:
            assert not torch.isfinite(ds.poses[i]).any()
        else:
            assert torch.equal(ds.poses[i], expected_pose(k))
    assert (ds.crop_edge, ds.png_depth_scale) == (1, 1000.0)


def test_pose_is_scaled_once_on_a_copy(tmp_path):
    root = write_replica(str(tmp_path / 'room'))
    ds = datasets.get_dataset(replica_cfg(root, scale=2.5), ARGS, 2.5)
    want = expected_pose(1)
    want[:3, 3] *= 2.5
    for _ in range(3):                                   # every access gives the same pose: the stored one is not touched
        assert torch.equal(ds.pose(1), want)
    assert torch.equal(ds.poses[1], expected_pose(1))
    one = datasets.get_dataset(replica_cfg(root), ARGS, 1)
    assert torch.equal(one.pose(2), expected_pose(2))   # scale 1: what the reference returns


def test_dispatch_and_refusals(tmp_path):
    assert golden()['dataset_dict'] == {k: v.__name__ for k, v in datasets.dataset_dict.items()}
    assert datasets.dataset_dict['replica'] is datasets.Replica and datasets.dataset_dict['scannet'] is datasets.ScanNet
    root = write_replica(str(tmp_path / 'room'))
    for name in ('azure', 'cofusion', 'tumrgbd'):
        with pytest.raises(NotImplementedError, match='EXR|undistortion'):
            datasets.get_dataset(dict(replica_cfg(root), dataset=name), ARGS, 1.0)
    with pytest.raises(NotImplementedError, match='distortion'):
        datasets.get_dataset(replica_cfg(root, distortion=[0.1, 0.0, 0.0, 0.0, 0.0]), ARGS, 1.0)
    seen = []
    ds = datasets.get_dataset(replica_cfg(root, distortion=[0.1, 0.0, 0.0, 0.0, 0.0]), ARGS, 1.0,
                              undistort=lambda img, K, dist: seen.append((K, dist)) or img)
    color, depth = ds._decode(0)
    assert color.shape == (6, 8, 3) and color.dtype == np.uint8 and depth.shape == (6, 8) and depth.dtype == np.uint16
    assert np.array_equal(seen[0][0], [[30.0, 0, 3.5], [0, 31.0, 2.5], [0, 0, 1]]) and seen[0][1][0] == 0.1


def test_decoding_goes_through_the_imread_hook(tmp_path):
    root = write_replica(str(tmp_path / 'room'))
    calls = []

    def imread(path, unchanged=False):
        calls.append((os.path.basename(path), unchanged))
        return np.zeros((6, 8), np.uint16) if unchanged else np.zeros((6, 8, 3), np.uint8)
    ds = datasets.get_dataset(replica_cfg(root), ARGS, 1.0, imread=imread, color_order='bgr')
    ds._decode(1)
    assert calls == [('frame000001.jpg', False), ('depth000001.png', True)] and ds.color_order == 'bgr'
    # the default decoder returns the PNG's 16-bit values as they are
    ds = datasets.get_dataset(replica_cfg(root), ARGS, 1.0)
    with Image.open(ds.depth_paths[2]) as im:
        assert np.array_equal(ds._decode(2)[1], np.asarray(im).astype(np.uint16))


def test_imread_hook_needs_its_color_order(tmp_path):
    root = write_replica(str(tmp_path / 'room'))
    with pytest.raises(ValueError, match='color_order'):
        datasets.get_dataset(replica_cfg(root), ARGS, 1.0, imread=datasets.imread_pil)
    with pytest.raises(ValueError, match='color_order'):
        datasets.get_dataset(replica_cfg(root), ARGS, 1.0, imread=datasets.imread_pil, color_order='gbr')
    assert datasets.get_dataset(replica_cfg(root), ARGS, 1.0, imread=datasets.imread_pil, color_order='rgb').color_order == 'rgb'


class _StandIn(object):
    """What a used dataset holds in _ingest, as far as pickle is concerned: something that cannot travel."""

    def __reduce__(self):
        raise TypeError('a FrameIngest does not pickle')


@pytest.mark.parametrize('layout', ['replica', 'scannet'])
def test_dataset_pickles_for_the_processes_of_a_run(tmp_path, layout):
    """The reference hands its frame_reader to spawned Tracker / Mapper processes and to a DataLoader worker (src/DF_Prior.py:305-307,
    src/Tracker.py:65-69): the dataset round-trips through pickle, before and after its FrameIngest exists, and still decodes."""
    if layout == 'replica':
        ds = datasets.get_dataset(replica_cfg(write_replica(str(tmp_path / 'room')), scale=2.5), ARGS, 2.5)
    else:
        ds = datasets.get_dataset(scannet_cfg(write_scannet(str(tmp_path / 'scene'))), ARGS, 1.0)
    color, depth = ds._decode(1)
    for used in (False, True):
        if used:
            ds._ingest = _StandIn()
        back = pickle.loads(pickle.dumps(ds))
        assert type(back) is type(ds) and back._ingest is None and (ds._ingest is not None) == used
        assert (back.n_img, back.color_paths, back.depth_paths, back.input_folder) == (ds.n_img, ds.color_paths, ds.depth_paths, ds.input_folder)
        assert (back.color_order, back.color_dtype, back.crop_edge, back.scale, back.device) == (ds.color_order, ds.color_dtype, ds.crop_edge, ds.scale, ds.device)
        assert all(torch.equal(a, b) or not torch.isfinite(a).any() for a, b in zip(back.poses, ds.poses)) and len(back.poses) == len(ds.poses)
        c, d = back._decode(1)
        assert np.array_equal(c, color) and np.array_equal(d, depth)
        assert torch.equal(back.pose(1), ds.pose(1)) or not torch.isfinite(ds.pose(1)).any()


def test_cpu_dataset_has_its_length_but_no_frames(tmp_path):
    """src/utils/Mesher.py:48 builds a device='cpu' dataset and asks its length."""
    ds = datasets.get_dataset(replica_cfg(write_replica(str(tmp_path / 'room'))), ARGS, 1.0, device='cpu')
    assert len(ds) == 3 and ds.device == 'cpu'
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds[0]


def test_update_cam(tmp_path):
    cfg = {'cam': cam(480, 640, fx=577.6, fy=578.7, cx=318.9, cy=242.7, crop_edge=10)}
    assert get_tsdf.update_cam(cfg) == (460, 620, 577.6, 578.7, 318.9 - 10, 242.7 - 10)
    cfg['cam']['crop_size'] = [384, 512]
    sx, sy = 512 / 640, 384 / 480
    assert get_tsdf.update_cam(cfg) == (364, 492, sx * 577.6, sy * 578.7, sx * 318.9 - 10, sy * 242.7 - 10)
    cfg['cam']['crop_edge'] = 0
    assert get_tsdf.update_cam(cfg) == (384, 512, sx * 577.6, sy * 578.7, sx * 318.9, sy * 242.7)
    # the shapes agree with the chain's
    assert ingest_ref.out_shape((480, 640), (384, 512), 10) == (364, 492)


def test_config_merge_follows_inherit_from(tmp_path):
    base, mid, top = tmp_path / 'base.yaml', tmp_path / 'mid.yaml', tmp_path / 'top.yaml'
    base.write_text('scale: 1\ncam:\n  H: 480\n  W: 640\n  crop_edge: 0\nmapping:\n  bound: [[0, 1], [0, 1], [0, 1]]\n')
    mid.write_text(f'inherit_from: {base}\ncam:\n  crop_edge: 10\ndata:\n  dataset: scannet\n')
    top.write_text(f'inherit_from: {mid}\ncam:\n  W: 320\ndata:\n  id: 59\n')
    cfg = get_tsdf.load_config(str(top))
    assert cfg['cam'] == {'H': 480, 'W': 320, 'crop_edge': 10} and cfg['data'] == {'dataset': 'scannet', 'id': 59}
    assert cfg['scale'] == 1 and cfg['mapping']['bound'] == [[0, 1], [0, 1], [0, 1]] and cfg['inherit_from'] == str(mid)
    # without inherit_from the default is the parent; with it the default is the root's parent
    lone = tmp_path / 'lone.yaml'
    lone.write_text('cam:\n  H: 48\n')
    assert get_tsdf.load_config(str(lone), str(base))['cam'] == {'H': 48, 'W': 640, 'crop_edge': 0}
    assert get_tsdf.load_config(str(lone)) == {'cam': {'H': 48}}


def test_signatures_match_the_reference():
    ref = golden()['signatures']
    _assert_compatible(datasets.get_dataset, ref['get_dataset'], 'get_dataset')
    _assert_compatible(datasets.BaseDataset.__init__, ref['BaseDataset.__init__'], 'BaseDataset.__init__')
    _assert_compatible(datasets.Replica.__init__, ref['Replica.__init__'], 'Replica.__init__')
    _assert_compatible(datasets.ScanNet.__init__, ref['ScanNet.__init__'], 'ScanNet.__init__')
    _assert_compatible(datasets.BaseDataset.__getitem__, ref['BaseDataset.__getitem__'], 'BaseDataset.__getitem__')
    _assert_compatible(get_tsdf.update_cam, ref['update_cam'], 'update_cam')
    _assert_compatible(get_tsdf.init_tsdf_volume, ref['init_tsdf_volume'], 'init_tsdf_volume')
    assert [p.name for p in inspect.signature(get_tsdf.init_tsdf_volume).parameters.values()] == ['cfg', 'args', 'space']
    assert len(ref) == 7


def test_resize_restatement_against_cv2():
    """ingest_ref's step B against cv2.resize on doubles, for whoever has cv2 (it is not a dependency of this package)."""
    cv2 = pytest.importorskip('cv2')
    rng = np.random.RandomState(3)
    for (h, w), (H, W) in (((11, 13), (5, 7)), ((4, 5), (9, 11)), ((968, 1296), (480, 640)), ((7, 200), (1, 70))):
        img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8) / 255.
        assert np.abs(ingest_ref.cv_resize_f64(img, (H, W)) - cv2.resize(img, (W, H))).max() <= 1e-12, ((h, w), (H, W))
