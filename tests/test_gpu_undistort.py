"""GPU: lens undistortion on the device (adfp_undistort_image, adfp_ingest_frames_undistort, datasets.FrameIngest, TUM_RGBD) against
the numpy statement of the rule (tests/undistort_ref.py).

Bounds, none tuned:
  the undistorted uint8 image   byte for byte: the remap is integer arithmetic on both sides.
  the ingest launch             tests/test_gpu_ingest.py's own comparison (hold(), imported from there: float64 colour 1e-12,
                                float32 colour one ulp at 1.0, depth bit for bit) against tests/ingest_ref.py applied to the
                                statement's undistorted image: the byte that enters stage A is exact, the stages behind it are
                                the plain launch's.
  zero distortion, null map     torch.equal to the plain launch: the same bytes enter the same code."""
import ctypes as C
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ingest_ref
import undistort_ref
from test_gpu_ingest import TORCH_DTYPE, cam, e2e_scene, frame, hold
from attentive_dfprior_amd import _lib, datasets, fusion, get_tsdf
from attentive_dfprior_amd.datasets import FrameIngest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
I32 = np.iinfo(np.int32)
_MAPS = {}


def ref_map(k):
    """The statement's map of undistort_ref.GEOMETRIES[k], computed once."""
    if k not in _MAPS:
        _MAPS[k] = undistort_ref.undistort_map(*undistort_ref.GEOMETRIES[k])
    return _MAPS[k]


def lens_cam(k, depth_hw, png=6553.5, crop=None, edge=0, **kw):
    _, fx, fy, cx, cy, dist = undistort_ref.GEOMETRIES[k]
    return dict(cam(depth_hw, png, crop, edge), fx=fx, fy=fy, cx=cx, cy=cy, distortion=dist, **kw)


def image(seed, hw):
    return np.random.RandomState(seed).randint(0, 256, tuple(hw) + (3,), dtype=np.uint8)


def hand_maps(hw):
    """Maps [h,w,2] that between them hold every pair of these coordinates in x and y: taps at -2 .. 1 and n - 2 .. n + 1 with
    fractions 0, 13 and 31 (none, one, two and four taps inside), the sentinel value, the ends of int32 and of the clamp, and a
    million pixels out on both sides."""
    h, w = hw

    def axis(n):
        near = [32 * s + f for s in (-2, -1, 0, 1, n - 2, n - 1, n, n + 1) for f in (0, 13, 31)]
        return near + [I32.min, I32.min + 1, I32.max, -2 ** 30, 2 ** 30, -32 * 10 ** 6, 32 * 10 ** 6]
    pairs = np.array(list(itertools.product(axis(w), axis(h))), dtype=np.int64)
    assert len(pairs) == 31 * 31 and (pairs == I32.min).all(axis=1).any()
    n = h * w
    pairs = np.resize(pairs, (-(-len(pairs) // n) * n, 2))       # the last map is filled by starting over
    return [m.reshape(h, w, 2).astype(np.int32) for m in pairs.reshape(-1, n, 2)]


def undistort_on_device(ing, img, m):
    out = ing.undistort(img, map=torch.from_numpy(np.ascontiguousarray(m)).to(DEV))
    assert out.dtype == torch.uint8 and tuple(out.shape) == img.shape and out.device == torch.device(DEV)
    return out.cpu().numpy()


@pytest.mark.parametrize('hw', [(6, 8), (37, 53)])
def test_image_byte_for_byte(hw):
    ing = FrameIngest(cam(hw), 1.0, DEV)
    maps = [('lens map %d' % k, ref_map(k)) for k, g in enumerate(undistort_ref.GEOMETRIES) if g[0] == hw]
    maps += [('hand-built map %d' % k, m) for k, m in enumerate(hand_maps(hw))]
    maps.append(('identity', undistort_ref.identity_map(hw)))
    assert len(maps) >= 3
    images = [('random bytes', image(3, hw)), ('all 255', np.full(hw + (3,), 255, np.uint8))]
    worst = 0
    for (mname, m), (iname, img) in itertools.product(maps, images):
        got, want = undistort_on_device(ing, img, m), undistort_ref.remap(img, m)
        differ = int((got != want).sum())
        worst = max(worst, differ)
        assert differ == 0, (hw, mname, iname, differ, got[got != want][:4], want[got != want][:4])
    print(f'{hw}: {len(maps)} maps x {len(images)} images, bytes that differ: {worst}')
    # what the hand-built maps are for: an all-255 image comes back with every value the weights can make, 255 included
    white = np.stack([undistort_ref.remap(images[1][1], m) for _, m in maps[:-1]])
    assert white.max() == 255 and white.min() == 0 and ((white > 0) & (white < 255)).any()
    # device and host inputs, and the configured lens's own map
    k = 0 if hw == (6, 8) else 1
    lens = FrameIngest(lens_cam(k, hw), 1.0, DEV, undistort='device')
    img = images[0][1]
    want = undistort_ref.remap(img, ref_map(k))
    assert np.array_equal(lens.undistort(img).cpu().numpy(), want)
    assert np.array_equal(lens.undistort(torch.from_numpy(img).to(DEV)).cpu().numpy(), want)
    assert np.array_equal(lens._maps[hw].cpu().numpy(), ref_map(k))
    with pytest.raises(ValueError):
        lens.undistort(img, map=torch.zeros(hw + (2,), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        lens.undistort(img, map=torch.zeros((hw[0], hw[1] + 1, 2), dtype=torch.int32, device=DEV))


# colour 37 x 53 through lens 1; depth at the colour's size (no resize) and at 20 x 31 (resize); crop_size (17, 23)
LAUNCH_CASES = {'copy': ((37, 53), None), 'resize': ((20, 31), None), 'crop_size': ((37, 53), (17, 23)),
                'resize and crop_size': ((20, 31), (17, 23))}


@pytest.mark.parametrize('case', list(LAUNCH_CASES))
def test_ingest_launch_with_a_map(case):
    depth_hw, crop = LAUNCH_CASES[case]
    n = 0
    for edge, order, out in itertools.product((0, 2), ('bgr', 'rgb'), ('f32', 'f64')):
        color, depth = frame(300 + n, (37, 53), depth_hw)
        ing = FrameIngest(lens_cam(1, depth_hw, crop=crop, edge=edge), 1.0, DEV, color_order=order, color_dtype=TORCH_DTYPE[out],
                          undistort='device')
        c, d = ing(color, depth)
        assert tuple(d.shape) == ing.out_shape == ingest_ref.out_shape(depth_hw, crop, edge) and c.dtype == TORCH_DTYPE[out]
        flat = undistort_ref.remap(color, ref_map(1))
        assert (flat != color).mean() > 0.5                  # the lens does move the image
        hold(c, d, ingest_ref.ingest(flat, depth, 6553.5, 1.0, crop, edge, order), f'{case}, edge {edge}, {order}, out {out}')
        n += 1
    assert n == 8


def raw_launch(ing, color, depth, map_ptr):
    """adfp_ingest_frames_undistort called as it is, map_ptr None included."""
    geom = ing._geom(color.shape[:2], depth.shape, False)
    H, W = ing.out_shape_for(depth.shape)
    dc, dd = torch.from_numpy(color).to(DEV), torch.from_numpy(depth.view(np.int16)).to(DEV)
    co = torch.empty((H, W, 3), dtype=ing.color_dtype, device=DEV)
    do = torch.empty((H, W), dtype=torch.float32, device=DEV)
    jobs = (_lib.AdfpIngestJob * 1)(_lib.AdfpIngestJob(dc.data_ptr(), dd.data_ptr(), co.data_ptr(), do.data_ptr()))
    _lib.check(_lib.lib().adfp_ingest_frames_undistort(C.byref(geom), map_ptr, 1, jobs, _lib.current_stream(torch.device(DEV))), 'launch')
    torch.cuda.synchronize()
    return co, do


@pytest.mark.parametrize('case', list(LAUNCH_CASES))
def test_zero_distortion_and_null_map_equal_the_plain_launch(case):
    depth_hw, crop = LAUNCH_CASES[case]
    for out in ('f32', 'f64'):
        color, depth = frame(320, (37, 53), depth_hw)
        plain = FrameIngest(cam(depth_hw, crop=crop, edge=2), 1.0, DEV, color_dtype=TORCH_DTYPE[out])
        zero = FrameIngest(dict(lens_cam(1, depth_hw, crop=crop, edge=2), distortion=[0.0] * 5), 1.0, DEV, color_dtype=TORCH_DTYPE[out],
                           undistort='device')
        pc, pd = plain(color, depth)
        zc, zd = zero(color, depth)
        assert zero._maps and np.array_equal(zero._maps[(37, 53)].cpu().numpy(), undistort_ref.identity_map((37, 53)))
        assert torch.equal(zc, pc) and torch.equal(zd, pd)
        nc, nd = raw_launch(plain, color, depth, None)
        assert torch.equal(nc, pc) and torch.equal(nd, pd)
        mc, md = raw_launch(plain, color, depth, zero._maps[(37, 53)].data_ptr())
        assert torch.equal(mc, pc) and torch.equal(md, pd)
    # no route, or no distortion: the plain launch, no map built
    for ing in (FrameIngest(lens_cam(1, depth_hw, crop=crop, edge=2), 1.0, DEV),
                FrameIngest(cam(depth_hw, crop=crop, edge=2), 1.0, DEV, undistort='device')):
        c, d = ing(color, depth)
        assert not ing._maps and torch.equal(c, pc.float()) and torch.equal(d, pd)


def test_batch_equals_single_launches_and_writes_nothing_else():
    geometry = dict(crop=(17, 23), edge=2)
    frames = [frame(340 + k, (37, 53), (20, 31)) for k in range(3)]
    ing = FrameIngest(lens_cam(1, (20, 31), **geometry), 1.0, DEV, undistort='device')
    singles = [ing(c, d) for c, d in frames]
    H, W = ing.out_shape
    for k, (c, d) in enumerate(frames):
        hold(*singles[k], ingest_ref.ingest(undistort_ref.remap(c, ref_map(1)), d, 6553.5, 1.0, (17, 23), 2), f'single {k}')
    SENT = -123.0
    block_c = torch.full((5, H, W, 3), SENT, dtype=torch.float32, device=DEV)
    block_d = torch.full((5, H, W), SENT, dtype=torch.float32, device=DEV)
    rc, rd = ing.batch([c for c, _ in frames], [d for _, d in frames], out=(block_c[1:4], block_d[1:4]))
    assert rc.data_ptr() == block_c[1].data_ptr() and len(ing._maps) == 1
    for k in range(3):
        assert torch.equal(block_c[1 + k], singles[k][0]) and torch.equal(block_d[1 + k], singles[k][1])
    assert not torch.equal(block_c[1], block_c[2])
    for guard in (block_c[0], block_c[4], block_d[0], block_d[4]):
        assert (guard == SENT).all()
    # more frames than one launch carries, in scattered destinations
    many = [frames[k % 3] for k in range(_lib.INGEST_MAX_JOBS + 3)]
    big_c = torch.full((len(many) + 2, H, W, 3), SENT, dtype=torch.float32, device=DEV)
    big_d = torch.full((len(many) + 2, H, W), SENT, dtype=torch.float32, device=DEV)
    ing.batch([c for c, _ in many], [d for _, d in many], out=(big_c[1:-1], big_d[1:-1]))
    for k in range(len(many)):
        assert torch.equal(big_c[1 + k], singles[k % 3][0]) and torch.equal(big_d[1 + k], singles[k % 3][1])
    for guard in (big_c[0], big_c[-1], big_d[0], big_d[-1]):
        assert (guard == SENT).all()


def test_tum_geometry():
    """480 x 640 colour and depth, crop_size [384, 512], crop_edge 8, freiburg1's calibration: 368 x 496 out.  A full-size frame,
    once for both colour types."""
    hw, fx, fy, cx, cy, dist = undistort_ref.FREIBURG1
    color, depth = frame(31, hw, hw)
    flat = undistort_ref.remap(color, ref_map(4))
    black = float((flat == 0).all(axis=-1).mean())
    print(f'freiburg1: {black:.3f} of the undistorted pixels are black')
    assert 0.01 < black < 0.15
    ref = ingest_ref.ingest(flat, depth, 5000.0, 1.0, (384, 512), 8, 'rgb')
    for out in ('f64', 'f32'):
        ing = FrameIngest(lens_cam(4, hw, png=5000.0, crop=(384, 512), edge=8), 1.0, DEV, color_dtype=TORCH_DTYPE[out], undistort='device')
        assert ing.out_shape == (368, 496)
        c, d = ing(color, depth)
        hold(c, d, ref, f'TUM geometry, out {out}')
        assert np.array_equal(ing.undistort(color).cpu().numpy(), flat)


# ---- end to end: a TUM-layout directory of PNGs through the dataset classes, a DataLoader worker and init_tsdf_volume
E2E_HW = (24, 32)
E2E_PNG = 5000.0
E2E_DIST = [0.2, -0.1, 0.005, -0.004, 0.02]


def quaternion_of(R):
    """x y z w of a rotation matrix (the branch with the largest divisor)."""
    t = np.trace(R)
    cand = [np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1 + t]),
            np.array([1 + 2 * R[0, 0] - t, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]),
            np.array([R[0, 1] + R[1, 0], 1 + 2 * R[1, 1] - t, R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]),
            np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 + 2 * R[2, 2] - t, R[1, 0] - R[0, 1]])]
    q = cand[int(np.argmax([t, R[0, 0], R[1, 1], R[2, 2]]))]
    return q / np.linalg.norm(q)


def write_tum_e2e(root, sc, n=5):
    """Frame 0 sees the room from the origin with the file's identity pose, so that the loader's first-frame-relative poses are
    the scene's own; rgb, depth and pose timestamps are offset from one another."""
    from PIL import Image
    os.makedirs(os.path.join(root, 'rgb'))
    os.makedirs(os.path.join(root, 'depth'))
    lists = {'rgb.txt': ['# color images', '# timestamp filename'], 'depth.txt': ['# depth maps', '# timestamp filename'],
             'groundtruth.txt': ['# ground truth trajectory', '# timestamp tx ty tz qx qy qz qw']}
    for k in range(n):
        c2w = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])) if k == 0 else \
            sc.default_c2w(offset=(0.05 * k, -0.04 * k, 0.02), yaw=0.9 * k, pitch=0.1 * k - 0.1)
        depth = sc.depth_image(c2w, zero_band=0.08).numpy()
        raw = np.clip(np.rint(depth.astype(np.float64) * E2E_PNG), 0, 65535).astype(np.uint16)
        Image.fromarray(image(70 + k, E2E_HW)).save(os.path.join(root, 'rgb', f'{k}.png'))
        Image.fromarray(raw).save(os.path.join(root, 'depth', f'{k}.png'))
        pose = c2w.numpy().astype(np.float64)
        pose[:3, 1] *= -1.0                            # the file holds the OpenCV camera; the loader flips to the renderer's
        pose[:3, 2] *= -1.0
        lists['rgb.txt'].append(f'{0.1 * k:.4f} rgb/{k}.png')
        lists['depth.txt'].append(f'{0.1 * k + 0.011:.4f} depth/{k}.png')
        lists['groundtruth.txt'].append(' '.join(f'{v:.10f}' for v in [0.1 * k - 0.004] + pose[:3, 3].tolist() + quaternion_of(pose[:3, :3]).tolist()))
    for name, lines in lists.items():
        with open(os.path.join(root, name), 'w') as f:
            f.write('\n'.join(lines) + '\n')


def e2e_cfg(root, sc):
    return {'dataset': 'tumrgbd', 'scale': 1, 'data': {'input_folder': root, 'dataset': 'tumrgbd', 'id': 'mini'},
            'cam': dict(cam(E2E_HW, png=E2E_PNG), fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, distortion=E2E_DIST, undistort='device'),
            'mapping': {'bound': sc.bound.tolist()}, 'grid_len': {'bound_divisible': 0.32}}


def test_tum_dataset_and_init_tsdf_volume_end_to_end(tmp_path):
    sc = e2e_scene()
    imread, order = datasets._default_imread()
    root = str(tmp_path / 'mini')
    write_tum_e2e(root, sc)
    cfg = e2e_cfg(root, sc)
    args = SimpleNamespace(input_folder=None)
    lens = undistort_ref.undistort_map(E2E_HW, sc.fx, sc.fy, sc.cx, sc.cy, E2E_DIST)

    def reference(k):
        color, depth = imread(os.path.join(root, 'rgb', f'{k}.png')), imread(os.path.join(root, 'depth', f'{k}.png'), unchanged=True)
        assert np.array_equal(color if order == 'rgb' else color[..., ::-1], image(70 + k, E2E_HW))      # PNG: the bytes written
        return ingest_ref.ingest(undistort_ref.remap(color, lens), depth, E2E_PNG, 1, color_order=order)

    ds = datasets.get_dataset(cfg, args, 1, device=DEV)
    assert type(ds) is datasets.TUM_RGBD and len(ds) == 5 and ds.undistort == 'device'
    assert torch.equal(ds.poses[0], torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0])))
    idx, color, depth, pose = ds[3]
    assert idx == 3 and pose.device == torch.device(DEV) and torch.equal(pose.cpu(), ds.poses[3])
    hold(color, depth, reference(3), 'dataset frame 3')
    plain = datasets.get_dataset(dict(cfg, cam={k: v for k, v in cfg['cam'].items() if k != 'distortion'}), args, 1, device=DEV)[3]
    assert not torch.equal(plain[1], color) and torch.equal(plain[2], depth)       # the lens moved the colour, not the depth
    colors, depths, poses = ds.frames([4, 0, 3])
    assert tuple(poses.shape) == (3, 4, 4) and torch.equal(colors[2], color) and torch.equal(depths[2], depth)
    hold(colors[1], depths[1], reference(0), 'dataset frames()[1]')
    assert np.array_equal(ds.ingest._maps[E2E_HW].cpu().numpy(), lens) and len(ds.ingest._maps) == 1

    # the prior volume, against the same frames integrated here
    tsdf_volume, bounds, verts, faces, norms, vcolors = get_tsdf.init_tsdf_volume(cfg, args, space=2)
    bound = np.array(sc.bound.tolist(), dtype=np.float64)
    bound[:, 1] = (((bound[:, 1] - bound[:, 0]) / 0.32).astype(np.int32) + 1) * 0.32 + bound[:, 0]
    vol = fusion.TSDFVolume(bound, voxel_size=4.0 / 256, device=DEV)
    H, W, fx, fy, cx, cy = get_tsdf.update_cam(cfg)
    K = np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])
    for k in (0, 2, 4):
        ref_c, ref_d = reference(k)
        c2w = ds.pose(k).numpy()
        c2w[:3, 1] *= -1.0
        c2w[:3, 2] *= -1.0
        vol.integrate(torch.floor(torch.from_numpy(ref_c.astype(np.float32)) * 255), ref_d, K, c2w, obs_weight=1.)
    want, _, want_bounds = vol.get_volume()
    X, Y, Z = want.shape
    assert tuple(tsdf_volume.shape) == (1, 1, Z, Y, X) and tsdf_volume.dtype == torch.float32
    got = tsdf_volume[0, 0].permute(2, 1, 0).contiguous().numpy()
    assert (want != -1.0).mean() > 0.05                  # the frames did reach the volume
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bounds, want_bounds)
    assert verts.shape[0] > 0 and faces.shape[1] == 3 and norms.shape == verts.shape and vcolors.shape == verts.shape


def test_tum_dataset_through_a_dataloader_worker(tmp_path):
    """The Tracker's pattern: the dataset is pickled into a spawned worker, which builds its own FrameIngest and map."""
    from torch.utils.data import DataLoader
    sc = e2e_scene()
    root = str(tmp_path / 'mini')
    write_tum_e2e(root, sc, n=2)
    ds = datasets.get_dataset(e2e_cfg(root, sc), SimpleNamespace(input_folder=None), 1, device=DEV)
    here = [ds[k] for k in range(2)]
    assert ds._ingest is not None and ds._ingest._maps
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=1, multiprocessing_context='spawn')
    got = [[t.clone() for t in item] for item in loader]
    del loader
    assert len(got) == 2
    for k, (idx, color, depth, pose) in enumerate(got):
        assert int(idx[0]) == k and color.device == torch.device(DEV)
        assert torch.equal(color[0], here[k][1]) and torch.equal(depth[0], here[k][2]) and torch.equal(pose[0], here[k][3])
