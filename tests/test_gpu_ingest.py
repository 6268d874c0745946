"""GPU: frame ingestion (adfp_ingest_frames, attentive_dfprior_amd/datasets.py, get_tsdf.py) against the host statement of the
reference's chain (tests/ingest_ref.py: numpy for the byte conversion, the cv2.resize rule and the crops, torch's own
F.interpolate on the CPU for crop_size).  All inputs are seeded random bytes.

Bounds, derived and not tuned:
  float64 colour   1e-12 absolute.  Steps A and B are the same f64 operations on both sides; torch's CPU bilinear kernel forms its
                   coefficient dst * (in - 1) / (out - 1) and its four-term sum in an order of its own (vectorised, possibly
                   contracted), which a restatement follows to 1.1e-13 at worst on values in [0, 1] with indices up to ~1e3.
  float32 colour   within one float32 ulp at 1.0 (6e-8) of the reference's value rounded to float32: a 1e-13 difference may flip
                   that rounding, never more.
  depth            bit for bit: the same two f32 roundings, and nearest is an index rule."""
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ingest_ref
from attentive_dfprior_amd import datasets, fusion, get_tsdf, synthetic
from attentive_dfprior_amd.datasets import FrameIngest

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64_TOL = 1e-12
F32_TOL = 6e-8
TORCH_DTYPE = {'f32': torch.float32, 'f64': torch.float64}


def frame(seed, color_hw, depth_hw, kind='u16'):
    rng = np.random.RandomState(seed)
    color = rng.randint(0, 256, tuple(color_hw) + (3,), dtype=np.uint8)
    if kind == 'u16':
        depth = rng.randint(0, 65536, tuple(depth_hw)).astype(np.uint16)
        depth.reshape(-1)[:3] = np.array([0, 1, 65535], np.uint16)[:depth.size]
    else:
        depth = (rng.random_sample(tuple(depth_hw)) * 65535.0).astype(np.float32)
    return color, depth


def cam(depth_hw, png=6553.5, crop=None, edge=0):
    c = {'H': depth_hw[0], 'W': depth_hw[1], 'png_depth_scale': png, 'crop_edge': edge}
    if crop:
        c['crop_size'] = list(crop)
    return c


def hold(c, d, ref, what):
    """Holds device tensors to a reference pair at the bounds of the module docstring."""
    ref_c, ref_d = ref
    got_c, got_d = c.cpu().numpy(), d.cpu().numpy()
    assert got_c.shape == ref_c.shape and got_d.shape == ref_d.shape, (what, got_c.shape, ref_c.shape, got_d.shape, ref_d.shape)
    assert got_d.dtype == np.float32 and ref_c.dtype == np.float64
    same = got_d.view(np.uint32) == ref_d.view(np.uint32)
    if got_c.dtype == np.float64:
        err, tol = np.abs(got_c - ref_c).max(), F64_TOL
    else:
        assert got_c.dtype == np.float32
        err, tol = np.abs(got_c.astype(np.float64) - ref_c.astype(np.float32).astype(np.float64)).max(), F32_TOL
    print(f'{what}: colour {got_c.dtype} max |diff| {err:.3e} (bound {tol:g}); depth bits differ at {int((~same).sum())} of {same.size}')
    assert same.all(), (what, got_d[~same][:4], ref_d[~same][:4])
    assert err <= tol, (what, err)


def compare(got_c, got_d, color, depth, what, png=6553.5, scale=1.0, crop=None, edge=0, order='rgb'):
    """hold() against the host chain of these inputs; returns the reference pair."""
    ref = ingest_ref.ingest(color, depth, png, scale, crop, edge, order)
    hold(got_c, got_d, ref, what)
    return ref


def run(color, depth, png=6553.5, scale=1.0, crop=None, edge=0, order='rgb', out='f32', what=''):
    ing = FrameIngest(cam(depth.shape, png, crop, edge), scale, DEV, color_order=order, color_dtype=TORCH_DTYPE[out])
    c, d = ing(color, depth)
    assert tuple(d.shape) == ing.out_shape == ingest_ref.out_shape(depth.shape, crop, edge) and c.dtype == TORCH_DTYPE[out]
    assert c.device == torch.device(DEV) and c.is_contiguous() and d.is_contiguous()
    return compare(c, d, color, depth, what, png, scale, crop, edge, order)


# the smallest shapes that reach every branch: colour 11 x 13, depth 5 x 7, crop_size (6, 9), edge 1
STAGES = {'same size, no crop': ((5, 7), None), 'resize only': ((11, 13), None), 'crop_size only': ((5, 7), (6, 9)),
          'resize and crop_size': ((11, 13), (6, 9))}


@pytest.mark.parametrize('stage', list(STAGES))
def test_every_stage_combination(stage):
    color_hw, crop = STAGES[stage]
    n = 0
    for edge, order, kind, out in itertools.product((0, 1), ('bgr', 'rgb'), ('u16', 'f32'), ('f32', 'f64')):
        color, depth = frame(100 + n, color_hw, (5, 7), kind)
        run(color, depth, crop=crop, edge=edge, order=order, out=out, what=f'{stage}, edge {edge}, {order}, depth {kind}, out {out}')
        n += 1
    assert n == 16


@pytest.mark.parametrize('out', ['f32', 'f64'])
def test_resize_edges_of_the_coefficient_rule(out):
    # upscaling: sx < 0 on the left and sx >= w - 1 on the right clamp, and rows above / below the image are clamped
    run(*frame(1, (4, 5), (9, 11)), out=out, what='upscale 4x5 -> 9x11')
    run(*frame(2, (4, 5), (9, 11)), crop=(6, 9), edge=1, out=out, what='upscale 4x5 -> 9x11, crop_size, edge')
    # an exact 2 x downscale: OpenCV takes its area path there, and the bilinear rule (weights .5, .5) equals it to rounding
    run(*frame(3, (10, 14), (5, 7)), out=out, what='downscale 10x14 -> 5x7')
    # crop_size that shrinks, and one that keeps a side (torch copies an equal side)
    run(*frame(4, (7, 5), (7, 5)), crop=(3, 4), out=out, what='crop_size 7x5 -> 3x4')
    run(*frame(5, (5, 7), (5, 7)), crop=(5, 9), out=out, what='crop_size 5x7 -> 5x9')
    run(*frame(6, (5, 7), (5, 7)), crop=(10, 14), out=out, what='crop_size 5x7 -> 10x14 (nearest at exactly 2 x)')


@pytest.mark.parametrize('out', ['f32', 'f64'])
def test_row_and_block_boundaries(out):
    # a width that is no multiple of 64 over more than one workgroup (3 x 333 = 999 pixels, 4 workgroups of 256), with and without resize
    run(*frame(7, (3, 333), (3, 333)), out=out, what='3x333')
    run(*frame(8, (5, 400), (3, 333)), edge=1, out=out, what='5x400 -> 3x333, edge 1')
    # one-row images
    run(*frame(9, (1, 70), (1, 70)), out=out, what='1x70')
    run(*frame(10, (3, 150), (1, 70)), out=out, what='3x150 -> 1x70')
    run(*frame(11, (1, 150), (1, 70)), crop=(1, 33), out=out, what='1x150 -> 1x70 -> crop_size 1x33')
    run(*frame(12, (6, 1), (3, 1)), out=out, what='6x1 -> 3x1')


def test_depth_values_and_scales():
    color, _ = frame(13, (2, 3), (2, 3))
    depth = np.array([[0, 1, 65535], [6553, 6554, 1000]], np.uint16)
    for png, scale in itertools.product((6553.5, 1000.0), (1, 2.5)):
        _, ref_d = run(color, depth, png=png, scale=scale, what=f'depth values, png_depth_scale {png}, scale {scale}')
        assert ref_d[0, 0] == 0.0 and ref_d[0, 2] == np.float32(np.float32(65535.0) / np.float32(png)) * np.float32(scale)
        run(color, depth.astype(np.float32) + np.float32(0.25), png=png, scale=scale, what=f'float32 depth, png_depth_scale {png}, scale {scale}')


def test_batch_equals_single_launches_and_writes_nothing_else():
    geometry = dict(crop=(6, 9), edge=1)
    frames = [frame(20 + k, (11, 13), (5, 7)) for k in range(3)]
    ing = FrameIngest(cam((5, 7), **geometry), 1.0, DEV)
    singles = [ing(c, d) for c, d in frames]
    bc, bd = ing.batch([c for c, _ in frames], [d for _, d in frames])
    H, W = ing.out_shape
    assert tuple(bc.shape) == (3, H, W, 3) and tuple(bd.shape) == (3, H, W)
    for k, (c, d) in enumerate(frames):
        compare(bc[k], bd[k], c, d, f'batch frame {k}', **geometry)
        assert torch.equal(bc[k], singles[k][0]) and torch.equal(bd[k], singles[k][1])
    assert not torch.equal(bc[0], bc[1]) and not torch.equal(bd[0], bd[1])
    # out= into frames 2, 0 and 1 of a KeyframeStore-shaped block of 5: nothing outside them is touched
    SENT = -123.0
    block_c = torch.full((5, H, W, 3), SENT, dtype=torch.float32, device=DEV)
    block_d = torch.full((5, H, W), SENT, dtype=torch.float32, device=DEV)
    order = (2, 0, 1)
    ing.batch(np.stack([c for c, _ in frames]), np.stack([d for _, d in frames]), out=([block_c[s] for s in order], [block_d[s] for s in order]))
    for k, s in enumerate(order):
        assert torch.equal(block_c[s], singles[k][0]) and torch.equal(block_d[s], singles[k][1])
    assert (block_c[3:] == SENT).all() and (block_d[3:] == SENT).all()
    # and as whole tensors, more frames than one launch carries
    many = [frame(40 + k, (11, 13), (5, 7)) for k in range(19)]
    guard_c = torch.full((21, H, W, 3), SENT, dtype=torch.float32, device=DEV)
    guard_d = torch.full((21, H, W), SENT, dtype=torch.float32, device=DEV)
    rc, rd = ing.batch([c for c, _ in many], [d for _, d in many], out=(guard_c[1:20], guard_d[1:20]))
    assert rc.data_ptr() == guard_c[1].data_ptr() and rd.data_ptr() == guard_d[1].data_ptr()
    for k in (0, 15, 16, 18):
        compare(guard_c[1 + k], guard_d[1 + k], *many[k], f'batch of 19, frame {k}', **geometry)
    assert (guard_c[0] == SENT).all() and (guard_c[20] == SENT).all() and (guard_d[0] == SENT).all() and (guard_d[20] == SENT).all()


def test_scannet_geometry():
    """968 x 1296 colour resized to the 480 x 640 depth frame, edge 10: 460 x 620 out.  Full-size frames, once."""
    color, depth = frame(30, (968, 1296), (480, 640))
    ref = None
    for out in ('f64', 'f32'):
        ing = FrameIngest(cam((480, 640), png=1000.0, edge=10), 1.0, DEV, color_order='bgr', color_dtype=TORCH_DTYPE[out])
        assert ing.out_shape == (460, 620)
        c, d = ing(color, depth)
        ref = ref or ingest_ref.ingest(color, depth, 1000.0, 1.0, None, 10, 'bgr')
        hold(c, d, ref, f'ScanNet geometry, out {out}')


def test_replica_geometry():
    """680 x 1200, same size, no crop.  Full-size frames, once."""
    color, depth = frame(31, (680, 1200), (680, 1200))
    ref = None
    for out in ('f64', 'f32'):
        ing = FrameIngest(cam((680, 1200), png=6553.5), 1.0, DEV, color_order='bgr', color_dtype=TORCH_DTYPE[out])
        assert ing.out_shape == (680, 1200)
        c, d = ing(color, depth)
        ref = ref or ingest_ref.ingest(color, depth, 6553.5, 1.0, None, 0, 'bgr')
        hold(c, d, ref, f'Replica geometry, out {out}')


def test_frame_ingest_inputs_staging_and_out_checks():
    geometry = dict(crop=None, edge=1)
    ing = FrameIngest(cam((5, 7), edge=1), 2.5, DEV)
    color, depth = frame(50, (11, 13), (5, 7))
    a = ing(color, depth)
    compare(*a, color, depth, 'numpy inputs', scale=2.5, **geometry)
    b = ing(torch.from_numpy(color), torch.from_numpy(depth))
    c = ing(torch.from_numpy(color).to(DEV), torch.from_numpy(depth.view(np.int16)).to(DEV))        # device inputs; int16 storage of uint16
    d = ing(torch.from_numpy(color).to(DEV), depth)                                                 # mixed
    for other in (b, c, d):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
    # four consecutive calls with different host inputs: both staging buffers are reused, nothing is synchronised in between
    inputs = [frame(60 + k, (11, 13), (5, 7)) for k in range(4)]
    outs = [ing(ci, di) for ci, di in inputs]
    for k, (ci, di) in enumerate(inputs):
        compare(*outs[k], ci, di, f'consecutive call {k}', scale=2.5, **geometry)
    # out=: the destinations are written in place and returned; wrong shape, dtype, device or layout raises
    H, W = ing.out_shape
    oc, od = torch.zeros((H, W, 3), device=DEV), torch.zeros((H, W), device=DEV)
    rc, rd = ing(color, depth, out=(oc, od))
    assert rc is oc and rd is od and torch.equal(oc, a[0]) and torch.equal(od, a[1])
    bad = [(torch.zeros((H, W + 1, 3), device=DEV), od), (oc, torch.zeros((H + 1, W), device=DEV)),
           (torch.zeros((H, W, 3), dtype=torch.float64, device=DEV), od), (oc, torch.zeros((H, W), dtype=torch.float64, device=DEV)),
           (torch.zeros((H, W, 3)), od), (oc, torch.zeros((H, W))),
           (torch.zeros((H, W, 6), device=DEV)[..., ::2], od), (oc, torch.zeros((W, H), device=DEV).t())]
    for pair in bad:
        with pytest.raises(ValueError):
            ing(color, depth, out=pair)
    with pytest.raises(ValueError):
        ing.batch([color, color], [depth, depth], out=(torch.zeros((3, H, W, 3), device=DEV), torch.zeros((3, H, W), device=DEV)))
    with pytest.raises(ValueError):
        ing(color.astype(np.float32), depth)
    with pytest.raises(ValueError):
        ing(color, depth.astype(np.float64))
    with pytest.raises(ValueError):
        ing.batch([color, color[:5]], [depth, depth])


# ---- end to end: a Replica-layout directory through the dataset classes and init_tsdf_volume
E2E_HW = (24, 32)
E2E_PNG = 6553.5


def e2e_scene():
    sc = synthetic.mini_scene()
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = E2E_HW[0], E2E_HW[1], 28.88, 28.88, 15.5, 11.5
    return sc


def write_e2e_dataset(root, sc, n=6):
    from PIL import Image
    os.makedirs(os.path.join(root, 'results'))
    lines = []
    for k in range(n):
        c2w = sc.default_c2w(offset=(0.05 * k, -0.04 * k, 0.02), yaw=0.9 * k, pitch=0.1 * k - 0.1)
        depth = sc.depth_image(c2w, zero_band=0.08).numpy()
        raw = np.clip(np.rint(depth.astype(np.float64) * E2E_PNG), 0, 65535).astype(np.uint16)
        color = np.random.RandomState(70 + k).randint(0, 256, E2E_HW + (3,), dtype=np.uint8)
        Image.fromarray(color).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(raw).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
        pose = c2w.numpy().astype(np.float64)
        pose[:3, 1] *= -1.0                            # the file holds the OpenCV camera; the loader flips to the renderer's
        pose[:3, 2] *= -1.0
        lines.append(' '.join(repr(float(v)) for v in pose.reshape(-1)))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return lines


def test_dataset_and_init_tsdf_volume_end_to_end(tmp_path):
    sc = e2e_scene()
    imread, order = datasets._default_imread()          # parity starts at the decoded bytes, whichever decoder is installed
    root = str(tmp_path / 'mini')
    lines = write_e2e_dataset(root, sc)
    cfg = {'dataset': 'replica', 'scale': 1, 'data': {'input_folder': root, 'dataset': 'replica', 'id': 'mini'},
           'cam': dict(cam(E2E_HW, png=E2E_PNG), fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy),
           'mapping': {'bound': sc.bound.tolist()}, 'grid_len': {'bound_divisible': 0.32}}
    args = SimpleNamespace(input_folder=None)

    def decoded(k):
        return (imread(os.path.join(root, 'results', f'frame{k:06d}.jpg')),
                imread(os.path.join(root, 'results', f'depth{k:06d}.png'), unchanged=True))

    # the dataset: one frame, and a batch
    ds = datasets.get_dataset(cfg, args, 1, device=DEV)
    assert len(ds) == 6
    idx, color, depth, pose = ds[3]
    assert idx == 3 and pose.device == torch.device(DEV) and torch.equal(pose.cpu(), ds.poses[3])
    compare(color, depth, *decoded(3), 'dataset frame 3', png=E2E_PNG, order=order)
    colors, depths, poses = ds.frames([4, 0, 3])
    assert tuple(poses.shape) == (3, 4, 4) and torch.equal(colors[2], color) and torch.equal(depths[2], depth)
    compare(colors[1], depths[1], *decoded(0), 'dataset frames()[1]', png=E2E_PNG, order=order)

    # the prior volume
    tsdf_volume, bounds, verts, faces, norms, vcolors = get_tsdf.init_tsdf_volume(cfg, args, space=2)
    bound = np.array(sc.bound.tolist(), dtype=np.float64)
    bound[:, 1] = (((bound[:, 1] - bound[:, 0]) / 0.32).astype(np.int32) + 1) * 0.32 + bound[:, 0]
    vol = fusion.TSDFVolume(bound, voxel_size=4.0 / 256, device=DEV)
    H, W, fx, fy, cx, cy = get_tsdf.update_cam(cfg)
    assert (H, W) == E2E_HW
    K = np.array([[fx, 0., cx], [0., fy, cy], [0., 0., 1.]])
    for k in (0, 2, 4):
        ref_c, ref_d = ingest_ref.ingest(*decoded(k), E2E_PNG, 1, color_order=order)
        c2w = np.array([float(v) for v in lines[k].split()]).reshape(4, 4).astype(np.float32)
        vol.integrate(torch.floor(torch.from_numpy(ref_c.astype(np.float32)) * 255), ref_d, K, c2w, obs_weight=1.)
    want, _, want_bounds = vol.get_volume()
    X, Y, Z = want.shape
    assert tuple(tsdf_volume.shape) == (1, 1, Z, Y, X) and tsdf_volume.dtype == torch.float32
    got = tsdf_volume[0, 0].permute(2, 1, 0).contiguous().numpy()
    assert (want != -1.0).mean() > 0.05                  # the frames did reach the volume
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bounds, want_bounds) and np.array_equal(bounds[:, 0], bound[:, 0])
    assert verts.shape[0] > 0 and faces.shape[1] == 3 and norms.shape == verts.shape and vcolors.shape == verts.shape


def test_dataset_through_a_dataloader_worker(tmp_path):
    """The Tracker's pattern (src/Tracker.py:65-69): DataLoader(frame_reader, batch_size=1, num_workers=1).  The dataset is pickled
    into a spawned worker, which builds its own FrameIngest; a dataset that was already used in this process travels too."""
    from torch.utils.data import DataLoader
    sc = e2e_scene()
    root = str(tmp_path / 'mini')
    write_e2e_dataset(root, sc, n=2)
    cfg = {'dataset': 'replica', 'data': {'input_folder': root},
           'cam': dict(cam(E2E_HW, png=E2E_PNG), fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy)}
    ds = datasets.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device=DEV)
    here = [ds[k] for k in range(2)]
    assert ds._ingest is not None
    loader = DataLoader(ds, batch_size=1, shuffle=False, num_workers=1, multiprocessing_context='spawn')
    got = [[t.clone() for t in item] for item in loader]
    del loader
    assert len(got) == 2
    for k, (idx, color, depth, pose) in enumerate(got):
        assert int(idx[0]) == k and color.device == torch.device(DEV)
        assert torch.equal(color[0], here[k][1]) and torch.equal(depth[0], here[k][2]) and torch.equal(pose[0], here[k][3])

