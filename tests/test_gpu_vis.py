"""GPU: the Visualizer's device route (adfp_vis_panels, attentive_dfprior_amd/visualizer.py) against the host statement of the pixel
contract (tests/vis_ref.py, itself held to matplotlib byte for byte by tests/test_vis_host.py).

Bounds, derived and not tuned:
  canvas         byte for byte, no pixel exempt: every operation of the contract is exactly rounded (IEEE division, products by 256
                 and 255, truncation), so the reference alone decides every byte.
  vmax, counts   exact: a maximum and whole numbers.
  the f64 sums   1e-10 relative to numpy's f64 sums: N 2^-53 for N <= 816 000 non-negative terms summed in another order
                 (9.1e-11 at Replica's frame); an empty sum is exactly 0."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import vis_ref
from attentive_dfprior_amd import common, synthetic
from attentive_dfprior_amd.visualizer import Visualizer
import attentive_dfprior_amd as A
from conftest import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SUM_TOL = 1e-10
DTYPES = {'f32': np.float32, 'f64': np.float64}


def to_dev(inputs):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in inputs]          # a copy: the shared cases are read-only


def hold_stats(got, inputs, what):
    ref = vis_ref.stats(*inputs)
    print(f'{what}: stats {got}')
    for k in ('vmax', 'n_valid', 'n_nonfinite', 'n_color'):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ('depth_abs_sum', 'color_sq_sum'):
        err = abs(got[k] - ref[k])
        print(f'{what}: {k} {got[k]!r} against numpy {ref[k]!r}: relative {err / ref[k] if ref[k] else 0.0:.2e} (bound {SUM_TOL:g})')
        assert err <= SUM_TOL * abs(ref[k]), (what, k, got[k], ref[k])
    for k in ('depth_l1', 'psnr'):
        assert (np.isnan(got[k]) and np.isnan(ref[k])) or got[k] == ref[k] or abs(got[k] - ref[k]) <= 2 * SUM_TOL * abs(ref[k]), (what, k, got[k], ref[k])


def hold(vis, inputs, what):
    canvas, stats = vis.panels(*to_dev(inputs))
    want = vis_ref.canvas(*inputs, stride=vis.stride, gap=vis.gap)
    assert canvas.dtype == torch.uint8 and canvas.device == torch.device(DEV) and canvas.is_contiguous()
    got = canvas.cpu().numpy()
    assert got.shape == want.shape == vis.canvas_shape(*inputs[0].shape) + (3,), (what, got.shape, want.shape)
    diff = (got != want).any(-1)
    print(f'{what}: canvas {got.shape}, {int(diff.sum())} of {diff.size} pixels differ')
    assert not diff.any(), (what, np.argwhere(diff)[:4].tolist(), got[diff][:4].tolist(), want[diff][:4].tolist())
    hold_stats(stats, inputs, what)


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', vis_ref.CASES)
def test_case_list(tmp_path, name, dt):
    inputs = vis_ref.cases(name, DTYPES[dt])
    for stride, gap in vis_ref.LAYOUTS:
        hold(Visualizer(1, 1, str(tmp_path), None, False, DEV, stride=stride, gap=gap), inputs, f'{name} {dt} stride {stride} gap {gap}')


def test_replica_frame_and_determinism(tmp_path):
    """680 x 1200, stride 1: the grid-size arithmetic (1024 partials with a grid-stride loop, 4.9 million canvas pixels), and two
    calls on the same inputs give the same bits."""
    inputs = vis_ref.frame(7, (680, 1200), np.float32, top=6.0)
    vis = Visualizer(1, 1, str(tmp_path), None, False, DEV)
    hold(vis, inputs, 'replica frame')
    dev = to_dev(inputs)
    c1, s1 = vis.panels(*dev)
    c1 = c1.clone()
    c2, s2 = vis.panels(*dev)
    assert torch.equal(c1, c2)
    assert np.array([s1[k] for k in s1]).tobytes() == np.array([s2[k] for k in s2]).tobytes()
    # per shape, not per call: the same buffers serve both calls
    assert c2.data_ptr() == vis.panels(*dev)[0].data_ptr() and len(vis._buffers) == 1


def test_stride_two_of_an_even_frame_and_input_conversion(tmp_path):
    """An even frame (rows of whole dwords, h = H / stride exactly) and inputs that are not in the kernel's dtypes or not
    contiguous: converted, not misread."""
    gd, gc, d, c = vis_ref.frame(9, (40, 64), np.float64)
    vis = Visualizer(1, 1, str(tmp_path), None, False, DEV, stride=2, gap=4)
    hold(vis, (gd, gc, d, c), 'even frame, stride 2')
    want = vis_ref.canvas(gd, gc, d, c, stride=2, gap=4)
    tgd, tgc, td, tc = to_dev((gd, gc, d, c))
    wide = torch.zeros((40, 128), dtype=torch.float32, device=DEV)
    wide[:, ::2] = tgd
    got, _ = vis.panels(wide[:, ::2], tgc, td, tc)                      # a strided view of the sensor depth
    assert np.array_equal(got.cpu().numpy(), want)
    d32 = d.astype(np.float32)                                         # a float32 rendered depth is widened, as the reference's numpy does
    got, _ = vis.panels(tgd, tgc, torch.from_numpy(d32).to(DEV), tc)
    assert np.array_equal(got.cpu().numpy(), vis_ref.canvas(gd, gc, d32.astype(np.float64), c, stride=2, gap=4))
    with pytest.raises(ValueError):
        vis.panels(tgd, tgc, td[:-1], tc)


def test_canvas_off_the_dword_grid(tmp_path):
    """The C entry with a canvas whose base is not dword-aligned (no torch allocation is): the byte path writes the same canvas
    and not a byte beside it."""
    import ctypes as C
    from attentive_dfprior_amd import _lib
    inputs = vis_ref.cases('random')
    gd, gc, d, c = to_dev(inputs)
    for stride, gap in vis_ref.LAYOUTS:
        want = vis_ref.canvas(*inputs, stride=stride, gap=gap)
        geom = _lib.AdfpVisGeom(gd.shape[0], gd.shape[1], stride, gap, 0)
        nbytes = _lib.lib().adfp_vis_workspace_bytes(C.byref(geom))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
        stats = torch.empty(_lib.VIS_STATS, dtype=torch.float64, device=DEV)
        for off in (1, 2, 3):
            buf = torch.full((want.size + 8,), 7, dtype=torch.uint8, device=DEV)
            rc = _lib.lib().adfp_vis_panels(C.byref(geom), _lib.ptr(gd), _lib.ptr(gc), _lib.ptr(d), _lib.ptr(c), C.c_void_p(buf.data_ptr() + off),
                                            _lib.ptr(stats), _lib.ptr(ws), nbytes, _lib.current_stream(torch.device(DEV)))
            assert rc == 0
            got = buf.cpu().numpy()
            assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), (stride, gap, off)
            assert (got[:off] == 7).all() and (got[off + want.size:] == 7).all()
        assert stats.cpu().numpy()[1] == vis_ref.stats(*inputs)['n_valid']


@pytest.fixture(scope='module')
def scene():
    sc = synthetic.mini_scene(device=DEV)
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    rend = A.Renderer(make_cfg(32, 16), None, sc)
    c2w = sc.default_c2w()
    gt_depth = sc.depth_image(c2w)
    gt_color = torch.rand((sc.H, sc.W, 3), generator=torch.Generator().manual_seed(3)).to(DEV)
    return sc, dec, rend, c2w, gt_depth, gt_color


def test_vis_end_to_end_on_the_mini_scene(tmp_path, scene, capsys):
    sc, dec, rend, c2w, gt_depth, gt_color = scene
    out = str(tmp_path / 'vis')
    vis = Visualizer(2, 1, out, rend, True, DEV, ext='png')
    assert vis.vis(0, 0, gt_depth, gt_color, c2w, sc.c, dec, sc.tsdf_volume, sc.tsdf_bnds) is None
    assert os.listdir(out) == ['00000_0000.png']
    assert capsys.readouterr().out.strip() == f'Saved rendering visualization of color/depth image at {out}/00000_0000.png'
    depth, _, color = rend.render_img(sc.c, dec, c2w, DEV, sc.tsdf_volume, sc.tsdf_bnds, stage='color', gt_depth=gt_depth)
    canvas, stats = vis.panels(gt_depth, gt_color, depth, color)
    want = canvas.cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, '00000_0000.png'))), want)
    assert want.shape == vis_ref.canvas_shape(sc.H, sc.W, 1, 8) + (3,)
    assert np.array_equal(want, vis_ref.canvas(gt_depth.cpu().numpy(), gt_color.cpu().numpy(), depth.cpu().numpy(), color.cpu().numpy()))
    assert vis.last_stats == stats and stats['n_valid'] > 0 and stats['n_color'] == sc.H * sc.W and np.isfinite(stats['psnr'])
    assert (gt_depth == 0).any()                                       # the scene's band of invalid pixels: the residual mask is in play
    # off the frequency: nothing rendered, nothing written
    assert vis.vis(1, 0, gt_depth, gt_color, c2w, sc.c, dec, sc.tsdf_volume, sc.tsdf_bnds) is None
    quiet = Visualizer(2, 3, out, rend, False, DEV, ext='png')
    quiet.vis(0, 1, gt_depth, gt_color, c2w, sc.c, dec, sc.tsdf_volume, sc.tsdf_bnds)
    assert os.listdir(out) == ['00000_0000.png'] and quiet.last_stats is None and capsys.readouterr().out == ''
    # a [7] camera tensor of the same pose: the canvas of the 4 x 4 pose it converts to
    cam = common.get_tensor_from_camera(c2w)
    assert tuple(cam.shape) == (7,) and cam.is_cuda
    quiet.vis(4, 3, gt_depth, gt_color, cam, sc.c, dec, sc.tsdf_volume, sc.tsdf_bnds)
    bottom = torch.tensor([[0., 0., 0., 1.]], device=DEV)
    c2w7 = torch.cat([common.get_camera_from_tensor(cam.clone()), bottom], dim=0)
    d7, _, c7 = rend.render_img(sc.c, dec, c2w7, DEV, sc.tsdf_volume, sc.tsdf_bnds, stage='color', gt_depth=gt_depth)
    want7 = quiet.panels(gt_depth, gt_color, d7, c7)[0].cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(os.path.join(out, '00004_0003.png'))), want7)
    # jpg, the reference's file type
    jpg = Visualizer(1, 1, str(tmp_path / 'jpg'), rend, False, DEV)
    jpg.vis(3, 2, gt_depth, gt_color, c2w, sc.c, dec, sc.tsdf_volume, sc.tsdf_bnds)
    with Image.open(str(tmp_path / 'jpg' / '00003_0002.jpg')) as im:
        assert im.format == 'JPEG' and np.asarray(im).shape == want.shape
