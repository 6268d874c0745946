"""GPU: the rendering metrics on the device (adfp_frame_metrics, attentive_dfprior_amd/render_eval.py) against their host statement
(tests/render_ref.py, itself held to an independent torch f64 restatement by tests/test_render_ref_host.py).

Bounds, derived and not tuned:
  row[0], [3], [4]   exact: whole numbers.
  row[1], [2]        1e-10 relative to numpy's f64 sums: N 2^-53 for N <= 816 000 non-negative terms summed in another order
                     (9.1e-11 at Replica's frame) -- the bound and reasoning of tests/test_gpu_vis.py; an empty sum is exactly 0.
  SSIM and CS sums   each sum divided by its window count is within 1e-10 ABSOLUTE of the statement's.  A moment is a 121-term sum
                     of products of magnitude <= 1 with positive weights, so another order of summation (the kernel's row pass
                     then column pass against numpy's, or the pooling's four-term sum) moves it by <= 121 x 2^-53 = 1.3e-14.  The
                     variances are differences of such moments and the two quotients divide by at least C2 = 9e-4 and
                     C1 = 1e-4, where numerator and denominator carry a handful of those terms: a few 1e-14 / 9e-4 = a few 1e-11
                     per window at the very worst (both images flat), and the mean over windows is no worse than its worst
                     window.  No case and no window is exempt.
  levels >= `levels` exactly 0.

The kernel's tile of window positions is 16 rows x 32 columns (ADFP_MET_TH, ADFP_MET_TW in csrc/adfp_metrics.h) with a 10-pixel
apron below and to the right; the seam test's pixel positions follow from those two numbers."""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render_ref
import vis_ref
from attentive_dfprior_amd import _lib, render_eval, synthetic
from attentive_dfprior_amd.render_eval import FrameMetrics
from attentive_dfprior_amd.visualizer import Visualizer
import attentive_dfprior_amd as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SUM_TOL = 1e-10                                    # relative, row[1] and row[2]
MEAN_TOL = 1e-10                                   # absolute, every SSIM / CS sum over its window count
TORCH_DTYPE = {'f32': torch.float32, 'f64': torch.float64}
TILE_H, TILE_W, APRON = 16, 32, 10


def to_dev(inputs):
    return [torch.from_numpy(np.array(a)).to(DEV) for a in inputs]          # a copy: the shared cases are read-only


def device_row(inputs, levels):
    dev = to_dev(inputs)
    H, W = inputs[0].shape
    fm = FrameMetrics(1, H, W, levels, DEV, dev[1].dtype)
    assert fm.add(*dev) == 0
    t = fm.table()
    assert t.shape == (1, 35) and t.dtype == np.float64
    return t[0]


def hold_row(got, ref, hw, levels, what):
    n = render_ref.windows(hw[0], hw[1], levels)
    for k in (0, 3, 4):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in (1, 2):
        err = abs(got[k] - ref[k])
        print(f'{what}: row[{k}] {got[k]!r} against numpy {ref[k]!r}: relative {err / ref[k] if ref[k] else 0.0:.2e} (bound {SUM_TOL:g})')
        assert err <= SUM_TOL * abs(ref[k]), (what, k, got[k], ref[k])
    worst = 0.0
    for k in range(levels):
        for j in range(6):
            e = 5 + 6 * k + j
            err = abs(got[e] / n[k] - ref[e] / n[k])
            worst = max(worst, err)
            assert err <= MEAN_TOL, (what, f'level {k} channel {j // 2} {"cs" if j % 2 else "ssim"}', got[e] / n[k], ref[e] / n[k], err)
    print(f'{what}: levels {levels}, worst |mean - statement| over the SSIM and CS sums {worst:.2e} (bound {MEAN_TOL:g})')
    tail = got[5 + 6 * levels:]
    assert tail.tobytes() == np.zeros_like(tail).tobytes(), (what, tail)     # +0.0 exactly
    assert np.isfinite(got).all(), (what, got)


@pytest.mark.parametrize('dt', list(TORCH_DTYPE))
@pytest.mark.parametrize('name', list(render_ref.CASES))
def test_case_list(name, dt):
    inputs = render_ref.cases(name, render_ref.DTYPES[dt])
    hw = inputs[0].shape
    top = render_ref.max_levels(*hw)
    assert top == render_eval.max_levels(*hw) >= 1
    for levels in range(top + 1):
        got = device_row(inputs, levels)
        hold_row(got, render_ref.case_rows(name, render_ref.DTYPES[dt], levels), hw, levels, f'{name} {dt}')
    # what render_eval makes of the row
    want = render_ref.per_frame(render_ref.case_rows(name, render_ref.DTYPES[dt], top), hw[0], hw[1], top)
    got = render_eval.frame_metrics(*to_dev(inputs))
    assert set(got) == set(render_eval.PER_FRAME) and np.isnan(got['ms_ssim'])
    assert got['n_valid'] == want['n_valid'] and got['n_nonfinite'] == want['n_nonfinite']
    assert abs(got['ssim'] - want['ssim']) <= MEAN_TOL
    for k in ('psnr', 'depth_l1'):
        assert (np.isnan(got[k]) and np.isnan(want[k])) or got[k] == want[k] or abs(got[k] - want[k]) <= 2 * SUM_TOL * abs(want[k]), (k, got[k], want[k])


@pytest.mark.parametrize('dt', list(TORCH_DTYPE))
def test_entries_0_to_4_are_the_visualizer_s_bit_for_bit(tmp_path, dt):
    """adfp_frame_metrics launches the Visualizer's own k_vis_reduce over the same grid (min(ceil(H W / 256), 1024) workgroups) and
    folds its partials in k_vis_panels' fixed order: the two share their reduction grid, so the five entries are the Visualizer's
    stats bit for bit, not merely within 1e-10."""
    vis = Visualizer(1, 1, str(tmp_path), None, False, DEV)
    for name in ('nonfinite_47x53', 'out_of_range_47x53', 'gt_depth_zero_24x32', 'one_window_11x11'):
        inputs = render_ref.cases(name, render_ref.DTYPES[dt])
        _, stats = vis.panels_async(*to_dev(inputs))
        s = stats.cpu().numpy()
        got = device_row(inputs, 1)
        # the row: n_valid, depth_abs_sum, color_sq_sum, n_color, n_nonfinite; the stats: vmax, then [1] [2] [3] n_nonfinite n_color
        assert got[:5].tobytes() == s[[1, 2, 3, 5, 4]].tobytes(), (name, got[:5], s)


def bright(inputs, r, c):
    gd, gc, d, col = [np.array(a) for a in inputs]
    col[r, c] = 1.0
    gc[r, c] = 0.0
    return gd, gc, d, col


@pytest.mark.parametrize('hw', [(75, 140), (109, 173)])
def test_tile_seams(hw):
    """levels = 3 with tiles of 16 x 32 window positions.  75 x 140 (levels 75 x 140, 38 x 70, 19 x 35: 65 x 130, 28 x 60 and
    9 x 25 positions) has tile edges inside levels 0 and 1 and a last tile that is partial in both axes at every level; its
    level 2 is a single partial tile, so 109 x 173 (109 x 173, 55 x 87, 28 x 44: 99 x 163, 45 x 77 and 18 x 34 positions) adds a
    frame whose tile edges fall inside all three levels, odd at levels 0 and 1.  A single bright pixel at each of: the frame's
    corners; the first and last window position of tile (1, 1) (pixels (16, 32) and (31, 63)); the last apron pixel of that tile
    (41, 73), ten pixels outside its positions; the pixel just before the tile, which only the tiles above and to the left read;
    and the first column of the last, partial tile column.  Each must move the sums as the statement says."""
    H, W = hw
    base = vis_ref.frame(11, hw, np.float32)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
             (TILE_H, TILE_W), (2 * TILE_H - 1, 2 * TILE_W - 1), (2 * TILE_H - 1 + APRON, 2 * TILE_W - 1 + APRON), (TILE_H - 1, TILE_W - 1),
             (H // 2, (W - APRON) // TILE_W * TILE_W), ((H - APRON) // TILE_H * TILE_H, W // 2)]
    assert render_ref.max_levels(H, W) >= 3
    ref0 = render_ref.rows(*base, 3)
    hold_row(device_row(base, 3), ref0, hw, 3, f'{H}x{W} base')
    for r, c in spots:
        inputs = bright(base, r, c)
        ref = render_ref.rows(*inputs, 3)
        assert not np.array_equal(ref[5:11], ref0[5:11])          # the pixel does move level 0's sums
        hold_row(device_row(inputs, 3), ref, hw, 3, f'{H}x{W} bright pixel at ({r}, {c})')


def test_table_discipline():
    SENT = -123.25
    frames = [render_ref.cases(n) for n in ('noise_47x53', 'constant_47x53', 'nonfinite_47x53')]
    dev = [to_dev(f) for f in frames]

    def run():
        fm = FrameMetrics(4, 47, 53, 3, DEV)
        fm._table.fill_(SENT)
        assert fm.add(*dev[0]) == 0 and fm.add(*dev[1]) == 1 and fm.count == 2
        return fm

    fm = run()
    full = fm._table.cpu().numpy()
    assert (full[2:] == SENT).all() and not (full[:2] == SENT).any()
    t = fm.table()
    assert t.shape == (2, 35)
    for k in range(2):
        hold_row(t[k], render_ref.case_rows(('noise_47x53', 'constant_47x53')[k], np.float32, 3), (47, 53), 3, f'table row {k}')
    s = fm.summary()
    pf = fm.per_frame()
    assert s['n_frames'] == 2 and s['ssim'] == float(np.mean(pf['ssim'])) and s['psnr'] == float(np.mean(pf['psnr']))
    # two runs over the same frames: the same bytes
    assert run()._table.cpu().numpy().tobytes() == full.tobytes()
    # a full table raises
    assert fm.add(*dev[2]) == 2 and fm.add(*dev[0]) == 3
    with pytest.raises(IndexError):
        fm.add(*dev[1])
    assert fm.count == 4 and fm.table()[3].tobytes() == full[0].tobytes()
    # inputs that are not one frame of the object's shape or dtype
    with pytest.raises(ValueError):
        fm2 = FrameMetrics(1, 47, 53, 3, DEV)
        fm2.add(dev[0][0][:-1], dev[0][1][:-1], dev[0][2][:-1], dev[0][3][:-1])
    with pytest.raises(ValueError):
        FrameMetrics(1, 47, 53, 3, DEV).add(dev[0][0], dev[0][1].double(), dev[0][2], dev[0][3])
    with pytest.raises(RuntimeError):
        FrameMetrics(1, 47, 53, 4, DEV)                            # 47 -> 24 -> 12 -> 6: no fourth level
    # the C entry between guard words: nothing outside the row and the workspace it was given is written
    geom = _lib.AdfpMetricsGeom(47, 53, 3, 0)
    nbytes = _lib.lib().adfp_frame_metrics_workspace_bytes(C.byref(geom))
    G = 64
    ws = torch.full((nbytes // 8 + 2 * G,), SENT, dtype=torch.float64, device=DEV)
    rows = torch.full((2 * G + 35,), SENT, dtype=torch.float64, device=DEV)
    rc = _lib.lib().adfp_frame_metrics(C.byref(geom), *[_lib.ptr(x) for x in dev[0]], C.c_void_p(rows.data_ptr() + 8 * G),
                                       C.c_void_p(ws.data_ptr() + 8 * G), nbytes, _lib.current_stream(torch.device(DEV)))
    assert rc == 0
    rows, ws = rows.cpu().numpy(), ws.cpu().numpy()
    assert rows[G:G + 35].tobytes() == full[0].tobytes()
    assert (rows[:G] == SENT).all() and (rows[G + 35:] == SENT).all() and (ws[:G] == SENT).all() and (ws[-G:] == SENT).all()


def test_replica_frame_once_and_add_does_not_wait(tmp_path):
    """680 x 1200 with levels = 5: the grid arithmetic (1024 stats partials with a grid-stride loop, 42 x 38 tiles at level 0, odd
    sizes at levels 3 and 4) and the workspace at the real size, against the statement, once.  Then the same frame 40 more times
    into one table: an event recorded after the last add has not completed when add returns -- the stream is busy with the
    frames queued before it, and add waited for none of them -- and all 41 rows hold the same bytes."""
    hw = (680, 1200)
    inputs = vis_ref.frame(7, hw, np.float32, top=6.0)
    dev = to_dev(inputs)
    n = 41
    fm = FrameMetrics(n, hw[0], hw[1], 5, DEV)
    assert fm.windows == [670 * 1190, 330 * 590, 160 * 290, 75 * 140, 33 * 65]
    fm.add(*dev)
    first = fm.table()[0]
    ref = render_ref.rows(*inputs, 5)
    hold_row(first, ref, hw, 5, 'replica frame')
    vis_stats = Visualizer(1, 1, str(tmp_path), None, False, DEV).panels_async(*dev)[1].cpu().numpy()
    assert first[:5].tobytes() == vis_stats[[1, 2, 3, 5, 4]].tobytes()
    got, want = fm.per_frame(), render_ref.per_frame(ref, hw[0], hw[1], 5)
    print(f'replica frame: ssim {got["ssim"][0]!r} ms_ssim {got["ms_ssim"][0]!r} psnr {got["psnr"][0]!r}')
    assert abs(got['ssim'][0] - want['ssim']) <= MEAN_TOL and 0.0 < want['ms_ssim'] < 1.0
    # five factors m^w with |dm| <= 1e-10, w <= 0.3 and m >= 0.1 here: d(ms_ssim) <= sum_k w_k dm_k / m_k <= 1e-9
    assert abs(got['ms_ssim'][0] - want['ms_ssim']) <= 1e-9
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    for _ in range(n - 1):
        fm.add(*dev)
    done.record()
    pending = not done.query()
    t = fm.table()
    assert pending, 'add waited for the device'
    assert t.shape == (n, 35) and all(t[k].tobytes() == first.tobytes() for k in range(n))


def test_add_is_capturable_in_a_graph():
    """The launches of one add captured once and replayed: nothing is read back or allocated in between, so a replay scores whatever
    the captured input buffers hold by then."""
    names = ('noise_47x53', 'constant_47x53')
    dev = to_dev(render_ref.cases(names[0]))
    fm = FrameMetrics(1, 47, 53, 3, DEV)
    fm.add(*dev)                                                   # first launches outside the capture
    torch.cuda.synchronize()
    fm.count = 0
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fm.add(*dev)
    for name in names:
        for t, a in zip(dev, render_ref.cases(name)):
            t.copy_(torch.from_numpy(np.array(a)))
        fm._table.fill_(-1.0)
        graph.replay()
        hold_row(fm.table()[0], render_ref.case_rows(name, np.float32, 3), (47, 53), 3, f'graph replay, {name}')


# ---- end to end: a Replica-layout directory and a checkpoint through render_eval.main
E2E_HW = (24, 32)
E2E_PNG = 6553.5
E2E_BAD = 2                                        # the frame whose ground-truth pose is not finite


def e2e_scene():
    sc = synthetic.mini_scene()
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = E2E_HW[0], E2E_HW[1], 28.88, 28.88, 15.5, 11.5
    return sc


def write_e2e_dataset(root, sc, n=6):
    """tests/test_gpu_ingest.py's dataset: n frames of the mini scene in Replica's layout; returns the poses (renderer's
    convention, what the loader hands out)."""
    from PIL import Image
    os.makedirs(os.path.join(root, 'results'))
    lines, poses = [], []
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
        poses.append(c2w)
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return torch.stack(poses)


def test_render_eval_end_to_end(tmp_path, capsys):
    import yaml
    sc = e2e_scene()
    root, out = str(tmp_path / 'mini'), str(tmp_path / 'out')
    gt = write_e2e_dataset(root, sc)
    est = gt.clone()
    est[:, :3, 3] += torch.tensor([0.03, -0.02, 0.01])             # the run's estimate: off by a few centimetres
    gt_list = gt.clone()
    gt_list[E2E_BAD, 0, 3] = float('nan')
    cfg = {'dataset': 'replica', 'scale': 1, 'occupancy': True,
           'data': {'input_folder': root, 'output': out, 'dataset': 'replica', 'id': 'mini', 'dim': 3},
           'cam': {'H': E2E_HW[0], 'W': E2E_HW[1], 'fx': sc.fx, 'fy': sc.fy, 'cx': sc.cx, 'cy': sc.cy, 'png_depth_scale': E2E_PNG, 'crop_edge': 0},
           'mapping': {'bound': synthetic.SCENE_BOUNDS['mini']},
           'grid_len': {'low': 0.32, 'high': 0.16, 'color': 0.16, 'bound_divisible': 0.32},
           'model': {'c_dim': 32, 'pos_embedding_method': 'fourier'},
           'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
           'meshing': {'resolution': 256}}
    cfg_path = str(tmp_path / 'mini.yaml')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    sd = synthetic.seeded_state_dict(0)
    os.makedirs(os.path.join(out, 'ckpts'))
    ckpt = {'c': sc.c, 'decoder_state_dict': sd, 'gt_c2w_list': gt_list, 'estimate_c2w_list': est, 'keyframe_list': [0], 'keyframe_dict': [],
            'selected_keyframes': None, 'idx': 5, 'tsdf_volume': sc.tsdf_volume}
    torch.save(dict(ckpt, idx=1), os.path.join(out, 'ckpts', '00001.tar'), _use_new_zipfile_serialization=False)      # an older one
    torch.save(ckpt, os.path.join(out, 'ckpts', '00005.tar'), _use_new_zipfile_serialization=False)
    bounds_path = str(tmp_path / 'mini_bounds.pt')
    torch.save(sc.tsdf_bnds.numpy(), bounds_path)

    argv = [cfg_path, '--every', '2', '--tsdf_bounds', bounds_path, '--default_config', str(tmp_path / 'none.yaml')]
    summary = render_eval.main(argv)
    printed = capsys.readouterr().out
    with open(os.path.join(out, 'eval_render.json')) as f:
        res = json.load(f)
    assert res['frame_indices'] == [0, 4] and res['checkpoint'] == '00005.tar' and res['every'] == 2 and res['gt_pose'] is False
    assert render_eval.max_levels(*E2E_HW) == 2 == res['levels']
    assert str(summary['n_frames']) in printed and 'psnr' in printed and summary['n_frames'] == 2

    # the same frames by hand
    dec = A.get_model(cfg)
    dec.load_state_dict(sd)
    dec.bound = sc.bound
    dec = dec.to(DEV)
    sc.vol_bnds = sc.tsdf_bnds.to(DEV)
    rend = A.Renderer(cfg, None, sc)
    c = {k: v.to(DEV) for k, v in sc.c.items()}
    from attentive_dfprior_amd import datasets
    ds = datasets.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device=DEV)

    def by_hand(poses, indices):
        rows = []
        for i in indices:
            _, gt_color, gt_depth, _ = ds[i]
            depth, _, color = rend.render_img(c, dec, poses[i].to(DEV), DEV, sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV), stage='color', gt_depth=gt_depth)
            rows.append(render_eval.frame_metrics(gt_depth, gt_color, depth, color))
        return rows

    def same(a, b):
        return a == b or (np.isnan(a) and np.isnan(b))

    want = by_hand(est, [0, 4])
    for k in render_eval.PER_FRAME:
        assert all(same(res['frames'][k][j], want[j][k]) for j in range(2)), (k, res['frames'][k], [w[k] for w in want])
        mean = float(np.mean([w[k] for w in want]))
        assert same(res['summary'][k], mean) and same(summary[k], mean), (k, res['summary'][k], mean)
    assert all(np.isnan(v) for v in res['frames']['ms_ssim']) and np.isnan(res['summary']['ms_ssim'])      # two levels only
    assert all(np.isfinite(res['frames'][k]).all() for k in ('psnr', 'depth_l1', 'ssim')) and min(res['frames']['n_valid']) > 0

    # --gt_pose: the ground-truth poses of the same frames (the non-finite one is skipped either way)
    render_eval.main(argv + ['--gt_pose'])
    with open(os.path.join(out, 'eval_render.json')) as f:
        res_gt = json.load(f)
    assert res_gt['frame_indices'] == [0, 4] and res_gt['gt_pose'] is True
    want_gt = by_hand(gt, [0, 4])
    for k in ('psnr', 'depth_l1', 'ssim'):
        assert res_gt['frames'][k] == [w[k] for w in want_gt]
    assert res_gt['frames']['depth_l1'] != res['frames']['depth_l1']
    # --ckpt names a checkpoint: idx 1 ends the walk at frame 0
    render_eval.main(argv + ['--ckpt', os.path.join(out, 'ckpts', '00001.tar')])
    with open(os.path.join(out, 'eval_render.json')) as f:
        assert json.load(f)['frame_indices'] == [0]
