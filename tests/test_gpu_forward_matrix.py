"""GPU (MI355X): every cell of the forward's network-to-kernel selection (csrc/adfp_kernels.hip: launch_decoder, launch_low_color,
launch_attention) against the oracle at the north-star bar, and one backward cell per stage (run_decoder_bwd) under the tight
gradient criterion.

  entry   render_batch_ray, eval_points, adfp_decode_single LOW / HIGH / COLOR, adfp_attention_rows, adfp_decode_stage LOW / COLOR /
          LOW_COLOR
  math    f16x3 (the f16-split kernels), ADFP_MATH=f32 (the exact ones)
  stage   low, high, color where the entry has one
  call    inference, training forward with layer inputs (parameters want gradients), training forward with masks only (grids do)
  points  rays, f32 points, f64 points where the entry takes points

Shapes: 33 rays x 13 samples = 429 points -- 14 tiles: not a multiple of 32 points, more than one 768-thread workgroup, 262 points
inside the TSDF band and 20 outside the bound; no points at all; and, for the fused low + colour training launch alone, the far side
of its one-network-per-wave rule (2 x tiles <= compute units x 8): 520 rays x 64 samples = 1 040 tiles on a 256-CU part."""
import ctypes as C

import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import synthetic, _lib
from oracle import adfp_oracle as O
from conftest import make_cfg, to_dev, assert_close
from test_gpu_parity import build
from test_gpu_subnets import make
from test_gpu_grad import check_tight

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4
MODES = ['f16x3', 'f32']
CALLS = ['inference', 'train_act', 'train_masks']
N_RAYS, NS, NF = 33, 8, 5
S = NS + NF


@pytest.fixture(scope='module')
def ref(mini):
    """The oracle on the 429 points, once: per stage the render's outputs and raw; the points themselves (f64) and their f32 rounding."""
    class R(object):
        pass
    r = R()
    r.rays = tuple(t[:N_RAYS].contiguous() for t in (mini.rays_o, mini.rays_d, mini.gt_depth, mini.gt_color))
    ro, rd, gd, _ = r.rays
    r.render, r.pts_raw = {}, {}
    for stage in O.STAGES:
        d, u, c, w, aux = O.render_batch_ray(mini.sd, mini.c, rd, ro, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, stage, gd, NS, NF, return_aux=True)
        r.render[stage] = (d, u, c, w, aux['raw'].reshape(-1, 4))
    r.z = aux['z_vals']
    r.band = aux['band']
    r.pts = (ro[..., None, :] + rd[..., None, :] * r.z[..., :, None]).reshape(-1, 3)                # f64 (z_vals are)
    assert r.pts.dtype == torch.float64 and r.pts.shape[0] == N_RAYS * S == 429
    assert 0 < int(r.band.sum()) < 429 and int((r.render['color'][4][:, 3] == 100).sum()) > 0
    for dt in (torch.float64, torch.float32):
        for stage in O.STAGES:
            r.pts_raw[dt, stage] = O.eval_points(mini.sd, r.pts.to(dt), mini.c, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, stage)
    return r


def scene_on_gpu(mini, call):
    """A fresh DF + Renderer and the grids; `call` decides what wants a gradient (and so what the training forward leaves)."""
    dec, rend = build(mini, mini.sd, NS, NF)
    for p in dec.parameters():
        p.requires_grad_(call == 'train_act')
    c = {k: v.to(DEV).clone().requires_grad_(call != 'inference') for k, v in mini.c.items()}
    return dec, rend, c


@pytest.mark.parametrize('call', CALLS)
@pytest.mark.parametrize('stage', O.STAGES)
@pytest.mark.parametrize('mode', MODES)
def test_render_batch_ray_cells(mini, ref, mode, stage, call, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    dec, rend, c = scene_on_gpu(mini, call)
    ro, rd, gd, _ = (t.to(DEV) for t in ref.rays)
    with torch.set_grad_enabled(call != 'inference'):
        d, u, col, w = rend.render_batch_ray(c, dec, rd, ro, DEV, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), stage, gt_depth=gd)
    assert d.requires_grad == (call != 'inference')
    od, ou, oc, ow, _ = ref.render[stage]
    assert_close(d.detach(), od, TOL, f'{stage} {call} depth')
    assert_close(u.detach(), ou, TOL, f'{stage} {call} uncertainty')
    assert_close(col.detach(), oc, TOL, f'{stage} {call} color')
    assert_close(w.detach(), ow, TOL, f'{stage} {call} weight')
    with torch.no_grad():                                                                        # no rays
        e = rend.render_batch_ray(c, dec, rd[:0], ro[:0], DEV, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), stage, gt_depth=gd[:0])
    assert e[0].shape == (0,) and e[3].shape == (0, S, 1)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('call', CALLS)
@pytest.mark.parametrize('stage', O.STAGES)
@pytest.mark.parametrize('mode', MODES)
def test_eval_points_cells(mini, ref, mode, stage, call, dtype, monkeypatch):
    monkeypatch.setenv('ADFP_MATH', mode)
    dec, rend, c = scene_on_gpu(mini, call)
    pts = ref.pts.to(dtype).to(DEV)
    with torch.set_grad_enabled(call != 'inference'):
        raw, w = rend.eval_points(pts, dec, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), c, stage, DEV)
    assert raw.requires_grad == (call != 'inference')
    oraw, ow = ref.pts_raw[dtype, stage]
    assert torch.equal(raw[:, 3].detach().cpu() == 100, oraw[:, 3] == 100)
    assert_close(raw.detach(), oraw, TOL, f'{stage} {call} raw')
    assert_close(w.detach(), ow, TOL, f'{stage} {call} w')
    with torch.no_grad():
        e, _ = rend.eval_points(pts[:0], dec, mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV), c, stage, DEV)
    assert e.shape == (0, 4)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('mode', MODES)
def test_sub_network_cells(mini, ref, mode, dtype, monkeypatch):
    """adfp_decode_single LOW / HIGH / COLOR and adfp_attention_rows: one network alone, no bound rule, no band."""
    monkeypatch.setenv('ADFP_MATH', mode)
    dec = make(mini)
    c = to_dev(mini.c, DEV)
    p_cpu = ref.pts.to(dtype)
    p = p_cpu.to(DEV).unsqueeze(0)
    tsdf, tb = mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV)
    occ = ref.pts_raw[dtype, 'low'][0][:, 3].clone()
    occ[occ == 100] = 0.25
    t = O.trilerp(mini.tsdf_volume, p_cpu, mini.tsdf_bnds).reshape(-1)
    # the attention network sees in-band points only (decoder.py:329): at a saturated TSDF value inv_tsdf's logarithm turns the last
    # bit of the trilinear sample into percents of its output
    band = (t > -1.0 + 1e-4) & (t < 1.0 - 1e-4)
    assert 32 < int(band.sum()) < 429 and int(band.sum()) % 32
    with torch.no_grad():
        for name in ('low', 'high', 'color'):
            out = getattr(dec, name + '_decoder')(p, c)
            assert_close(out.reshape(429, -1), O.mlp_forward(mini.sd, name, p_cpu, mini.c, mini.bound).reshape(429, -1), TOL, f'{name}_decoder alone')
            assert getattr(dec, name + '_decoder')(p[:, :0], c).numel() == 0
        fused, w = dec.mlp(p[:, band.to(DEV)], occ[band].to(DEV), tsdf, tb)
        assert dec.mlp(p[:, :0], occ[:0].to(DEV), tsdf, tb)[0].numel() == 0
    ofused, ow = O.mlp_tsdf_forward(mini.sd, occ[band], t[band])
    assert_close(fused.reshape(-1), ofused, TOL, 'mlp_tsdf fused occupancy')
    assert_close(w.reshape(-1), ow, TOL, 'mlp_tsdf attention weight')


@pytest.mark.parametrize('pmode', ['rays', 'f32', 'f64'])
@pytest.mark.parametrize('mode', MODES)
def test_decode_stage_cells(mini, ref, mode, pmode, monkeypatch):
    """adfp_decode_stage LOW / COLOR / LOW_COLOR (the bench hook): each is the launch stage colour makes for that network -- LOW_COLOR bit
    for bit what the stage's inference call leaves in raw outside the TSDF band (inside it the call's attention pass rewrites the occupancy)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    dec, rend = build(mini, mini.sd, NS, NF)
    eng = rend._engine
    c = to_dev(mini.c, DEV)
    tsdf, tb = mini.tsdf_volume.to(DEV), mini.tsdf_bnds.to(DEV)
    ro, rd, gd, _ = (t.to(DEV) for t in ref.rays)
    with torch.no_grad():
        out = eng.render_forward(dec, c, ro, rd, gd, tsdf, tb, mini.bound, 'color', NS, NF, want_aux=True)
    z, frame_raw = out[4]['z_vals'].contiguous(), out[4]['raw'].reshape(-1, 4)
    dtype = torch.float32 if pmode == 'f32' else torch.float64
    pts = ref.pts.to(dtype).to(DEV).contiguous()
    ap = _lib.AdfpPoints()
    ap.n_points = 429
    if pmode == 'rays':
        ap.mode, ap.rays_o, ap.rays_d, ap.z_vals, ap.S = _lib.PTS_RAYS, ro.data_ptr(), rd.data_ptr(), z.data_ptr(), S
    else:
        ap.mode, ap.pts = (_lib.PTS_F32 if pmode == 'f32' else _lib.PTS_F64), pts.data_ptr()
    scn, keep = eng.scene(dec, c, tsdf, tb, mini.bound, 'color', images='hg')
    L, st = _lib.lib(), _lib.current_stream(torch.device(DEV))
    res = {}
    for kind in (0, 2, 3):                                                  # ADFP_DEC_LOW, ADFP_DEC_COLOR, ADFP_DEC_LOW_COLOR
        raw = torch.full((429, 4), float('nan'), dtype=torch.float32, device=DEV)
        w = torch.full((429,), float('nan'), dtype=torch.float32, device=DEV)
        cnt = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
        rc = L.adfp_decode_stage(C.byref(scn), C.byref(ap), kind, _lib.ptr(raw), _lib.ptr(w), _lib.ptr(cnt), st)
        if kind == 3 and mode == 'f32':
            assert rc < 0                                                   # the fused launch exists for the f16-split images only
            continue
        _lib.check(rc, 'adfp_decode_stage')
        res[kind] = (raw.cpu(), w.cpu())
        ap0 = _lib.AdfpPoints()
        ap0.mode, ap0.n_points, ap0.pts = _lib.PTS_F64, 0, pts.data_ptr()
        assert L.adfp_decode_stage(C.byref(scn), C.byref(ap0), kind, _lib.ptr(raw), _lib.ptr(w), _lib.ptr(cnt), st) == 0
    torch.cuda.synchronize()
    p_cpu = ref.pts.to(dtype)
    occ = O.eval_points(mini.sd, p_cpu, mini.c, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'low')[0][:, 3]      # LOW with the bound rule
    rgb = O.mlp_forward(mini.sd, 'color', p_cpu, mini.c, mini.bound)[:, :3]
    for kind, (raw, w) in res.items():
        if kind in (0, 3):
            assert_close(raw[:, 3], occ, TOL, f'decode_stage({kind}) occupancy')
            assert torch.equal(w, torch.ones(429))
        if kind in (2, 3):
            assert_close(raw[:, :3], rgb, TOL, f'decode_stage({kind}) rgb')
    if mode == 'f16x3' and pmode == 'rays':
        out_band = ~ref.band
        assert torch.equal(res[3][0][out_band].view(torch.int32), frame_raw.cpu()[out_band].view(torch.int32))
        assert torch.equal(res[3][0][:, :3].view(torch.int32), frame_raw.cpu()[:, :3].view(torch.int32))      # colour: every point


@pytest.fixture(scope='module')
def big():
    """520 rays x 64 samples on the synthetic mini scene: 1 040 tiles, beyond the fused training launch's one-network-per-wave rule."""
    sc = synthetic.mini_scene()
    sd = O.random_state_dict(seed=3)
    rays = synthetic.make_ray_batch(sc, 520, seed=5)
    ro, rd, gd, _ = rays
    return sc, sd, rays, O.render_batch_ray(sd, sc.c, rd, ro, sc.tsdf_volume, sc.tsdf_bnds, sc.bound, 'color', gd, 48, 16)


@pytest.mark.parametrize('call', ['train_act', 'train_masks'])
def test_fused_training_launch_beyond_the_split_rule(big, call, monkeypatch):
    """k_decode_lc16_train with both networks per wave (the 429-point cells above run it one network per wave)."""
    monkeypatch.setenv('ADFP_MATH', 'f16x3')
    sc, sd, (ro, rd, gd, _), (od, ou, oc, ow) = big
    assert 2 * (520 * 64 // 32) > torch.cuda.get_device_properties(0).multi_processor_count * 8
    dec, rend = build(sc, sd, 48, 16)
    for p in dec.parameters():
        p.requires_grad_(call == 'train_act')
    c = {k: v.to(DEV).clone().requires_grad_(True) for k, v in sc.c.items()}
    d, u, col, w = rend.render_batch_ray(c, dec, rd.to(DEV), ro.to(DEV), DEV, sc.tsdf_volume.to(DEV), sc.tsdf_bnds.to(DEV), 'color', gt_depth=gd.to(DEV))
    assert d.requires_grad
    assert_close(d.detach(), od, TOL, 'depth')
    assert_close(col.detach(), oc, TOL, 'color')
    assert_close(w.detach(), ow, TOL, 'weight')
    assert_close(u.detach(), ou, TOL, 'uncertainty')


@pytest.mark.parametrize('stage', O.STAGES)
@pytest.mark.parametrize('mode', MODES)
def test_backward_cell_per_stage(mini, ref, mode, stage, monkeypatch):
    """The three decoders' backward behind the forward cells above: every grid and parameter gradient of the 429-point batch under
    conftest.assert_grad_tight (the oracle's autograd along the kernels' own ReLU decisions)."""
    monkeypatch.setenv('ADFP_MATH', mode)
    check_tight(mini, stage, False, mode, n_samples=NS, n_surface=NF, rays=ref.rays, what='forward matrix, ')
