"""CPU: the TUM RGB-D and Azure loaders and the undistortion route of attentive_dfprior_amd/datasets.py, on trees this file writes.
Constructing a dataset needs no GPU; the frames are tests/test_gpu_undistort.py's.

The TUM tree holds every case of the association (src/utils/datasets.py:248-312): list files with comment lines and timestamps
offset from one another, an image whose nearest depth is exactly max_dt = 0.08 s away (dropped: the test is strict), one with no
depth and one with no pose within 0.08 s, and images closer than 1 / 32 s to the last kept one (thinned).  The expected
association is stated twice: by hand, and by a brute-force search written here.

Pose bound: the loader forms inv(first) @ c2w in float64 and rounds to float32; the expectation is formed from Rodrigues' formula
instead of the quaternion formula, so the two differ by float64 rounding (~1e-15) before the float32 rounding: at most one float32
ulp of the largest entry (|t| < 8: 4.8e-7), bound 1e-6."""
import inspect
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from attentive_dfprior_amd import datasets

ARGS = SimpleNamespace(input_folder=None)
POSE_TOL = 1e-6

# (timestamp, file): image 0 has its nearest depth at exactly 0.08; 2 and 3 are closer than 1/32 s to image 1; 5 has no depth and
# 6 no pose within 0.08
RGB = [(0.0, 'rgb/a0.png'), (1.0, 'rgb/a1.png'), (1.02, 'rgb/a2.png'), (1.031, 'rgb/a3.png'), (1.04, 'rgb/a4.png'),
       (2.0, 'rgb/a5.png'), (3.0, 'rgb/a6.png'), (4.0, 'rgb/a7.png'), (4.5, 'rgb/a8.png')]
DEPTH = [(0.08, 'depth/d0.png'), (1.013, 'depth/d1.png'), (1.05, 'depth/d2.png'), (2.1, 'depth/d3.png'), (3.01, 'depth/d4.png'),
         (4.02, 'depth/d5.png'), (4.47, 'depth/d6.png')]
# (timestamp, translation, rotation axis, angle, quaternion scale): the quaternions are written un-normalised
POSE = [(0.01, (0.0, 0.0, 0.0), (0, 0, 1), 0.0, 1.0), (1.005, (1.0, -2.0, 0.5), (0, 0, 1), np.pi / 2, 0.5),
        (1.045, (1.5, -2.5, 0.25), (1, 0, 0), np.pi / 2, 2.0), (2.0, (3.0, 0.0, 0.0), (0, 1, 0), 0.3, 1.0),
        (3.2, (0.0, 3.0, 0.0), (0, 1, 0), -0.7, 1.0), (3.99, (-1.0, 4.0, 2.0), (1, 2, 3), 1.1, 1.0),
        (4.55, (2.0, 2.0, -3.0), (-2, 1, 0.5), -2.4, 3.0)]
KEPT = [(1, 1, 1), (4, 2, 2), (7, 5, 5), (8, 6, 6)]          # (image, depth, pose) rows, by hand


def rodrigues(axis, angle):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quaternion(axis, angle, scale):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    return np.concatenate([k * np.sin(angle / 2), [np.cos(angle / 2)]]) * scale


def pose_matrix(k):
    _, t, axis, angle, _ = POSE[k]
    m = np.eye(4)
    m[:3, :3] = rodrigues(axis, angle)
    m[:3, 3] = t
    return m


def write_tum(root, pose_file='groundtruth.txt'):
    os.makedirs(root)
    with open(os.path.join(root, 'rgb.txt'), 'w') as f:
        f.write('# color images\n# file: \'mini.bag\'\n# timestamp filename\n')
        for t, name in RGB:
            f.write(f'{t!r} {name}\n')
    with open(os.path.join(root, 'depth.txt'), 'w') as f:
        f.write('# depth maps\n\n# timestamp filename\n')
        for t, name in DEPTH:
            f.write(f'{t!r} {name}\n')
        f.write('\n')
    with open(os.path.join(root, pose_file), 'w') as f:
        f.write('# ground truth trajectory\n# file: \'mini.bag\'\n# timestamp tx ty tz qx qy qz qw\n')
        for t, trans, axis, angle, scale in POSE:
            f.write(' '.join(repr(float(v)) for v in (t,) + tuple(trans) + tuple(quaternion(axis, angle, scale))) + '\n')
    return root


def cam(**kw):
    return dict(dict(H=6, W=8, fx=30.0, fy=31.0, cx=3.5, cy=2.5, png_depth_scale=5000.0, crop_edge=0), **kw)


def tum_cfg(root, **camkw):
    return {'dataset': 'tumrgbd', 'cam': cam(**camkw), 'data': {'input_folder': root}}


def brute_force():
    """The association and thinning, searched: every image's nearest depth and pose, both strictly within 0.08 s; then the images
    more than 1 / 32 s after the last kept one."""
    rows = []
    for i, (t, _) in enumerate(RGB):
        j = min(range(len(DEPTH)), key=lambda n: abs(DEPTH[n][0] - t))
        k = min(range(len(POSE)), key=lambda n: abs(POSE[n][0] - t))
        if abs(DEPTH[j][0] - t) < 0.08 and abs(POSE[k][0] - t) < 0.08:
            rows.append((i, j, k))
    kept = [rows[0]]
    for r in rows[1:]:
        if RGB[r[0]][0] - RGB[kept[-1][0]][0] > 1.0 / 32:
            kept.append(r)
    return rows, kept


def expected_poses(kept):
    first = np.linalg.inv(pose_matrix(kept[0][2]))
    out = []
    for n, (_, _, k) in enumerate(kept):
        m = np.eye(4) if n == 0 else first @ pose_matrix(k)
        m[:3, 1] *= -1
        m[:3, 2] *= -1
        out.append(m)
    return out


def test_the_tree_holds_every_case():
    rows, kept = brute_force()
    assert abs(DEPTH[0][0] - RGB[0][0]) == 0.08 and abs(POSE[0][0] - RGB[0][0]) < 0.08          # dropped by the strict test alone
    assert [r[0] for r in rows] == [1, 2, 3, 4, 7, 8] and kept == KEPT
    assert RGB[3][0] - RGB[1][0] < 1.0 / 32 < RGB[4][0] - RGB[1][0]


@pytest.mark.parametrize('pose_file', ['groundtruth.txt', 'pose.txt'])
def test_tum_paths_count_and_poses(tmp_path, pose_file):
    root = write_tum(str(tmp_path / 'fr1'), pose_file)
    ds = datasets.get_dataset(tum_cfg(root, undistort='device', distortion=[0.2624, -0.9531, -0.0054, 0.0026, 1.1633]), ARGS, 1.0)
    assert type(ds) is datasets.TUM_RGBD and isinstance(ds, datasets.BaseDataset)
    assert ds.n_img == len(ds) == len(ds.poses) == len(KEPT) == 4
    assert ds.color_paths == [os.path.join(root, RGB[i][1]) for i, _, _ in KEPT]
    assert ds.depth_paths == [os.path.join(root, DEPTH[j][1]) for _, j, _ in KEPT]
    want = expected_poses(KEPT)
    assert torch.equal(ds.poses[0], torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])))           # identity, y and z columns negated
    for n, pose in enumerate(ds.poses):
        assert pose.dtype == torch.float32 and tuple(pose.shape) == (4, 4)
        err = np.abs(pose.numpy().astype(np.float64) - want[n]).max()
        print(f'{pose_file} pose {n}: max |diff| {err:.3e} (bound {POSE_TOL:g})')
        assert err <= POSE_TOL
    assert ds.distortion.tolist() == [0.2624, -0.9531, -0.0054, 0.0026, 1.1633] and ds.undistort == 'device'


def test_groundtruth_is_preferred_and_a_missing_list_is_an_error(tmp_path):
    root = write_tum(str(tmp_path / 'both'))
    with open(os.path.join(root, 'pose.txt'), 'w') as f:
        f.write('# no poses near any image\n9.0 0 0 0 0 0 0 1\n')
    assert datasets.get_dataset(tum_cfg(root, undistort='device'), ARGS, 1.0).n_img == 4
    os.remove(os.path.join(root, 'groundtruth.txt'))
    assert datasets.get_dataset(tum_cfg(root, undistort='device'), ARGS, 1.0).n_img == 0
    os.remove(os.path.join(root, 'pose.txt'))
    with pytest.raises(FileNotFoundError):
        datasets.get_dataset(tum_cfg(root, undistort='device'), ARGS, 1.0)


def test_parse_list_and_associate_frames(tmp_path):
    root = write_tum(str(tmp_path / 'fr1'))
    ds = datasets.get_dataset(tum_cfg(root, undistort='device'), ARGS, 1.0)
    rgb = ds.parse_list(os.path.join(root, 'rgb.txt'))
    assert rgb.shape == (9, 2) and rgb.dtype.kind == 'U' and rgb[4].tolist() == ['1.04', 'rgb/a4.png']
    gt = ds.parse_list(os.path.join(root, 'groundtruth.txt'), skiprows=1)
    assert gt.shape == (7, 8) and gt[:, 0].astype(np.float64).tolist() == [p[0] for p in POSE]
    assert ds.parse_list(os.path.join(root, 'depth.txt'), skiprows=4).shape == (6, 2)        # the rows skipped come first
    ti, td, tp = (np.array([r[0] for r in rows]) for rows in (RGB, DEPTH, POSE))
    rows, _ = brute_force()
    got = ds.associate_frames(ti, td, tp)
    assert [tuple(int(v) for v in r) for r in got] == rows
    # without poses: pairs, the strict test on the depth alone
    pairs = ds.associate_frames(ti, td, None)
    assert [tuple(int(v) for v in r) for r in pairs] == [(1, 1), (2, 1), (3, 1), (4, 2), (6, 4), (7, 5), (8, 6)]
    assert ds.associate_frames(ti, td, None, max_dt=0.081)[0] == (0, 0)
    images, depths, poses = ds.loadtum(root)                 # frame_rate = -1: nothing is thinned
    assert len(images) == len(depths) == len(poses) == len(rows)


def test_quaternion_matrix():
    ds = datasets.TUM_RGBD.__new__(datasets.TUM_RGBD)
    s = np.sqrt(0.5)
    known = [((0, 0, 0, 1), np.eye(3)), ((0, 0, 0, -2), np.eye(3)),
             ((0, 0, s, s), [[0, -1, 0], [1, 0, 0], [0, 0, 1]]), ((s, 0, 0, s), [[1, 0, 0], [0, 0, -1], [0, 1, 0]]),
             ((0, s, 0, s), [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]), ((3, 0, 0, 0), [[1, 0, 0], [0, -1, 0], [0, 0, -1]]),
             ((0.5, 0.5, 0.5, 0.5), [[0, 0, 1], [1, 0, 0], [0, 1, 0]])]
    for q, R in known:
        m = ds.pose_matrix_from_quaternion(np.array((1.0, 2.0, 3.0) + tuple(q), dtype=np.float64))
        assert m.shape == (4, 4) and m.dtype == np.float64 and m[3].tolist() == [0, 0, 0, 1] and m[:3, 3].tolist() == [1, 2, 3]
        assert np.abs(m[:3, :3] - np.array(R, dtype=np.float64)).max() <= 4e-16, q
    rng = np.random.RandomState(5)
    quats = rng.standard_normal((64, 4)) * rng.uniform(0.1, 10.0, (64, 1))
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:
        Rotation = None
    worst = 0.0
    for q in quats:
        R = ds.pose_matrix_from_quaternion(np.concatenate([np.zeros(3), q]))[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
        if Rotation is not None:
            worst = max(worst, np.abs(R - Rotation.from_quat(q).as_matrix()).max())
    print(f'against scipy: max |diff| {worst:.3e} (bound 1e-15)' if Rotation is not None else 'scipy is not installed')
    assert worst <= 1e-15


def touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'wb').close()


AZURE_STEMS = ['10', '2', '0001', '0003']                    # sorted by NAME: 0001 0003 10 2


def write_azure(root, log=True):
    for s in AZURE_STEMS:
        touch(os.path.join(root, 'color', f'{s}.jpg'))
        touch(os.path.join(root, 'depth', f'{s}.png'))
    touch(os.path.join(root, 'color', 'notes.txt'))
    if log:
        os.makedirs(os.path.join(root, 'scene'))
        with open(os.path.join(root, 'scene', 'trajectory.log'), 'w') as f:
            for k in range(4):
                f.write(f'{k} {k} {k + 1}\n')
                for row in azure_pose(k):
                    f.write(' '.join(f'{v:.8f}' for v in row) + '\n')
    return root


def azure_pose(k):
    m = np.eye(4)
    m[:3, :3] = rodrigues((1, k, 2), 0.4 * k)
    m[:3, 3] = [0.5 * k, -k, 2.0]
    return m


def azure_cfg(root, **camkw):
    return {'dataset': 'azure', 'cam': cam(**camkw), 'data': {'input_folder': root}}


def test_azure_with_and_without_its_log(tmp_path):
    root = write_azure(str(tmp_path / 'apartment'))
    ds = datasets.get_dataset(azure_cfg(root, undistort='device', distortion=[0.1, 0.01, 0.0, 0.0]), ARGS, 1.0)
    assert type(ds) is datasets.Azure and ds.n_img == len(ds) == 4
    assert [os.path.basename(p) for p in ds.color_paths] == ['0001.jpg', '0003.jpg', '10.jpg', '2.jpg']
    assert [os.path.basename(p) for p in ds.depth_paths] == ['0001.png', '0003.png', '10.png', '2.png']
    assert len(ds.poses) == 4
    for k, pose in enumerate(ds.poses):
        want = np.array([[float(f'{v:.8f}') for v in row] for row in azure_pose(k)])
        want[:3, 1] *= -1
        want[:3, 2] *= -1
        assert pose.dtype == torch.float32 and torch.equal(pose, torch.from_numpy(want).float())
    bare = datasets.get_dataset(azure_cfg(write_azure(str(tmp_path / 'bare'), log=False), undistort='device'), ARGS, 1.0)
    assert bare.n_img == 4 and len(bare.poses) == 4
    assert all(p.dtype == torch.float32 and torch.equal(p, torch.eye(4)) for p in bare.poses)


def test_the_route_is_stated_by_key_or_keyword_and_the_keyword_wins(tmp_path):
    root = write_tum(str(tmp_path / 'fr1'))
    dist = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
    hook = lambda img, K, d: img + 1
    by_key = datasets.get_dataset(tum_cfg(root, undistort='device', distortion=dist), ARGS, 1.0)
    by_word = datasets.get_dataset(tum_cfg(root, distortion=dist), ARGS, 1.0, undistort='device')
    both = datasets.get_dataset(tum_cfg(root, undistort='device', distortion=dist), ARGS, 1.0, undistort=hook)
    assert by_key.undistort == 'device' and by_word.undistort == 'device' and both.undistort is hook
    for bad in ('host', 'cv2', True, 1):
        with pytest.raises(ValueError, match='undistort'):
            datasets.get_dataset(tum_cfg(root, undistort=bad, distortion=dist), ARGS, 1.0)
        with pytest.raises(ValueError, match='undistort'):
            datasets.get_dataset(tum_cfg(root, distortion=dist), ARGS, 1.0, undistort=bad)
    for n in (3, 6, 12, 14):
        with pytest.raises(ValueError, match='coefficients'):
            datasets.get_dataset(tum_cfg(root, undistort='device', distortion=[0.1] * n), ARGS, 1.0)
    # the device route leaves the decoded bytes alone (the launch undistorts); the host route applies the callable
    img = np.arange(6 * 8 * 3, dtype=np.uint8).reshape(6, 8, 3)
    depth = np.zeros((6, 8), np.uint16)
    imread = lambda path, unchanged=False: depth if unchanged else img
    on_device = datasets.get_dataset(tum_cfg(root, distortion=dist), ARGS, 1.0, undistort='device', imread=imread, color_order='rgb')
    on_host = datasets.get_dataset(tum_cfg(root, undistort='device', distortion=dist), ARGS, 1.0, undistort=hook, imread=imread, color_order='rgb')
    assert np.array_equal(on_device._decode(0)[0], img) and np.array_equal(on_host._decode(0)[0], img + 1)
    # the FrameIngest a dataset builds: constructing one launches nothing
    assert on_device.ingest._lens[:4] == (30.0, 31.0, 3.5, 2.5) and on_device.ingest._lens[4].tolist() == dist
    assert on_host.ingest._lens is None
    # a route without a distortion undistorts nothing
    plain = datasets.get_dataset(tum_cfg(root, undistort='device'), ARGS, 1.0, imread=imread, color_order='rgb')
    assert plain.distortion is None and plain.ingest._lens is None and np.array_equal(plain._decode(0)[0], img)
    # FrameIngest itself: the key, the keyword, neither
    c = cam(distortion=dist)
    assert datasets.FrameIngest(c, 1.0, 'cuda:0')._lens is None
    assert datasets.FrameIngest(c, 1.0, 'cuda:0', undistort='device')._lens is not None
    assert datasets.FrameIngest(dict(c, undistort='device'), 1.0, 'cuda:0')._lens is not None
    assert datasets.FrameIngest(cam(undistort='device'), 1.0, 'cuda:0')._lens is None
    with pytest.raises(ValueError, match='undistort'):
        datasets.FrameIngest(c, 1.0, 'cuda:0', undistort=hook)
    with pytest.raises(ValueError, match='coefficients'):
        datasets.FrameIngest(cam(distortion=[0.1] * 6), 1.0, 'cuda:0', undistort='device')
    with pytest.raises(ValueError, match='no distortion'):
        datasets.FrameIngest(cam(), 1.0, 'cuda:0').undistort(img)


def test_refusals_without_a_route_name_the_key(tmp_path):
    root = write_tum(str(tmp_path / 'fr1'))
    named = r"undistortion.*cfg\['cam'\]\['undistort'\] = 'device'"
    with pytest.raises(NotImplementedError, match=named):
        datasets.get_dataset(tum_cfg(root, distortion=[0.1, 0.0, 0.0, 0.0, 0.0]), ARGS, 1.0)
    with pytest.raises(NotImplementedError, match=named):
        datasets.get_dataset(tum_cfg(root), ARGS, 1.0)
    with pytest.raises(NotImplementedError, match=named):
        datasets.get_dataset(azure_cfg(write_azure(str(tmp_path / 'apartment'))), ARGS, 1.0)
    with pytest.raises(NotImplementedError, match=named):
        datasets.get_dataset(dict(tum_cfg(root, distortion=[0.1, 0.0, 0.0, 0.0]), dataset='replica'), ARGS, 1.0)
    with pytest.raises(NotImplementedError, match='EXR'):
        datasets.get_dataset(dict(tum_cfg(root, undistort='device'), dataset='cofusion'), ARGS, 1.0)
    assert datasets.dataset_dict['tumrgbd'] is datasets.TUM_RGBD and datasets.dataset_dict['azure'] is datasets.Azure
    assert (datasets.TUM_RGBD.__name__, datasets.Azure.__name__, datasets.CoFusion.__name__) == ('TUM_RGBD', 'Azure', 'CoFusion')


class _StandIn(object):
    """What a used FrameIngest holds, as far as pickle is concerned: something that cannot travel."""

    def __reduce__(self):
        raise TypeError('device memory does not pickle')


def test_a_dataset_with_the_device_route_pickles(tmp_path):
    root = write_tum(str(tmp_path / 'fr1'))
    dist = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]
    ds = datasets.get_dataset(tum_cfg(root, undistort='device', distortion=dist), ARGS, 1.0)
    for used in (False, True):
        if used:
            ds.ingest._maps[(6, 8)] = _StandIn()
            ds.ingest._staging[0] = _StandIn()
        back = pickle.loads(pickle.dumps(ds))
        assert type(back) is datasets.TUM_RGBD and back._ingest is None and back.undistort == 'device'
        assert (back.n_img, back.color_paths, back.depth_paths) == (ds.n_img, ds.color_paths, ds.depth_paths)
        assert back.distortion.tolist() == dist and all(torch.equal(a, b) for a, b in zip(back.poses, ds.poses))
        assert back.ingest._lens[4].tolist() == dist and back.ingest._maps == {}
    # a FrameIngest on its own travels without its map and staging buffers
    ing = pickle.loads(pickle.dumps(ds.ingest))
    assert ing._maps == {} and ing._staging == [None, None] and ing._events == [None, None] and ing._lens[4].tolist() == dist
    assert ds.ingest._maps != {}


def _assert_compatible(mine, ref, what):
    """The reference's parameters (name, kind, default) come first and unchanged; anything after them has a default or is **kw."""
    pm = [(p.name, p.kind, p.default) for p in inspect.signature(mine).parameters.values()]
    pr = [(n, getattr(inspect.Parameter, k), d if has else inspect.Parameter.empty) for n, k, has, d in ref]
    assert pm[:len(pr)] == pr, f'{what}: {pm} against the reference\'s {pr}'
    for n, k, d in pm[len(pr):]:
        assert d is not inspect.Parameter.empty or k in (inspect.Parameter.VAR_KEYWORD, inspect.Parameter.VAR_POSITIONAL), \
            f'{what}: extra required parameter {n!r}'


def test_signatures_and_attributes_match_the_reference(tmp_path):
    with open(os.path.join(GOLDEN, 'datasets_more_signatures.json')) as f:
        g = json.load(f)
    assert sorted(g['signatures']) == ['Azure.__init__', 'Azure.load_poses', 'TUM_RGBD.__init__', 'TUM_RGBD.associate_frames',
                                       'TUM_RGBD.loadtum', 'TUM_RGBD.parse_list', 'TUM_RGBD.pose_matrix_from_quaternion']
    for name, ref in g['signatures'].items():
        cls, method = name.split('.')
        _assert_compatible(getattr(getattr(datasets, cls), method), ref, name)
    tum = datasets.get_dataset(tum_cfg(write_tum(str(tmp_path / 'fr1')), undistort='device'), ARGS, 1.0)
    azure = datasets.get_dataset(azure_cfg(write_azure(str(tmp_path / 'apartment')), undistort='device'), ARGS, 1.0)
    assert g['attributes']['TUM_RGBD'] and g['attributes']['Azure']
    for name in g['attributes']['TUM_RGBD']:
        assert hasattr(tum, name), name
    for name in g['attributes']['Azure']:
        assert hasattr(azure, name), name
