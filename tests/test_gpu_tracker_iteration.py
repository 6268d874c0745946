"""GPU: the fused Tracker iteration (tracking.TrackerIteration; reference src/Tracker.py:75-134 and the loop at :236-263).
Piece by piece against torch / the oracle, then the whole iteration against the reference-shaped sequence of calls
(get_samples -> pre-filter -> render_batch_ray -> loss -> backward -> torch.optim.Adam) on the same pixel draws."""
import ctypes as C

import numpy as np
import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import _lib, common, synthetic
from attentive_dfprior_amd._lib import lib, ptr, check
from attentive_dfprior_amd.tracking import TrackerIteration
from oracle import adfp_oracle as O
from conftest import make_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EDGE = 4


def stream():
    return _lib.current_stream(torch.device(DEV))


def test_camera_from_tensor_and_its_backward_match_torch_autograd():
    g = torch.Generator().manual_seed(0)
    for k in range(8):
        cam = torch.randn(7, generator=g)
        if k % 2:
            cam[:4] /= cam[:4].norm()                        # unit quaternions, what the Tracker starts from
        cam_t = cam.clone().requires_grad_(True)
        RT = common.get_camera_from_tensor(cam_t)            # [3,4]
        G = torch.randn(3, 4, generator=g)
        (RT * G).sum().backward()
        d_cam, d_c2w, d_g = cam.to(DEV), torch.empty(16, device=DEV), torch.empty(7, device=DEV)
        g_c2w = torch.zeros(4, 4)
        g_c2w[:3] = G
        g_c2w[3] = 7.0                                       # the bottom row carries no gradient
        check(lib().adfp_camera_from_tensor(ptr(d_cam), ptr(d_c2w), stream()), 'fwd')
        check(lib().adfp_camera_from_tensor_backward(ptr(d_cam), ptr(g_c2w.to(DEV)), ptr(d_g), stream()), 'bwd')
        got = d_c2w.cpu().reshape(4, 4)
        assert torch.equal(got[3], torch.tensor([0., 0., 0., 1.]))
        assert (got[:3] - RT.detach()).abs().max() <= 2e-6 * max(1.0, RT.detach().abs().max().item())
        ref = cam_t.grad
        assert (d_g.cpu() - ref).abs().max() <= 1e-5 * max(1.0, ref.abs().max().item()), (d_g.cpu(), ref)


def test_get_camera_from_tensor_on_the_gpu_is_one_kernel_each_way_with_the_torch_values():
    """common.get_camera_from_tensor(cuda camera tensor) = adfp_camera_from_tensor under autograd: same [3,4] matrix and the same
    gradient as the torch composition (quad2rotation, what a CPU tensor takes), through a further torch op like the Tracker's."""
    g = torch.Generator().manual_seed(3)
    for k in range(6):
        cam = torch.randn(7, generator=g)
        G = torch.randn(3, 4, generator=g)
        ref_in = cam.clone().requires_grad_(True)
        ref = common.get_camera_from_tensor(ref_in)
        (ref * G).sum().backward()
        dev_in = cam.to(DEV).requires_grad_(True)
        got = common.get_camera_from_tensor(dev_in)
        assert got.shape == (3, 4) and got.is_cuda and got.grad_fn is not None
        (got * G.to(DEV)).sum().backward()
        assert (got.detach().cpu() - ref.detach()).abs().max() <= 2e-6 * max(1.0, ref.detach().abs().max().item())
        assert (dev_in.grad.cpu() - ref_in.grad).abs().max() <= 1e-5 * max(1.0, ref_in.grad.abs().max().item())
    # a batch of camera tensors (bundle adjustment) keeps the torch composition
    batch = torch.randn(3, 7, generator=g).to(DEV)
    assert common.get_camera_from_tensor(batch).shape == (3, 3, 4)


def test_camera_kernels_match_the_reference_golden():
    """adfp_camera_from_tensor and its backward against the reference's own get_camera_from_tensor + autograd
    (tests/golden/mini_pose.npz, made by tests/golden/make_pose_golden.py from src/common.py:139-178)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mini_pose.npz'))
    for k in range(g['cam'].shape[0]):
        d_cam = torch.from_numpy(g['cam'][k]).to(DEV)
        d_c2w, d_g = torch.empty(16, device=DEV), torch.empty(7, device=DEV)
        g_c2w = torch.zeros(4, 4)
        g_c2w[:3] = torch.from_numpy(g['cot'][k])
        check(lib().adfp_camera_from_tensor(ptr(d_cam), ptr(d_c2w), stream()), 'fwd')
        check(lib().adfp_camera_from_tensor_backward(ptr(d_cam), ptr(g_c2w.to(DEV)), ptr(d_g), stream()), 'bwd')
        ref, ref_g = g['c2w'][k], g['g_cam'][k]
        assert np.abs(d_c2w.cpu().numpy().reshape(4, 4)[:3] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max())
        assert np.abs(d_g.cpu().numpy() - ref_g).max() <= 2e-5 * max(1.0, np.abs(ref_g).max())


def test_get_tensor_from_camera_round_trip():
    g = torch.Generator().manual_seed(5)
    for _ in range(12):
        cam = torch.randn(7, generator=g)
        RT = common.get_camera_from_tensor(cam)
        t = common.get_tensor_from_camera(RT)
        assert t.dtype == torch.float32 and t.shape == (7,) and abs(t[:4].norm().item() - 1) < 1e-5 and t[0] >= 0
        assert (common.get_camera_from_tensor(t) - RT).abs().max() < 1e-5
        tq = common.get_tensor_from_camera(RT, Tquad=True)
        assert torch.equal(tq[:3], t[4:]) and torch.equal(tq[3:], t[:4])


def test_select_pixels_is_get_sample_uv_on_the_same_draw():
    H, W = 48, 64
    g = torch.Generator().manual_seed(1)
    depth, color = torch.rand(H, W, generator=g).to(DEV), torch.rand(H, W, 3, generator=g).to(DEV)
    H0, H1, W0, W1 = 5, H - 3, 7, W - 9
    n = 333
    torch.manual_seed(11)
    i, j, d, c = common.get_sample_uv(H0, H1, W0, W1, n, depth, color, device=DEV)
    torch.manual_seed(11)
    pick = torch.randint((H1 - H0) * (W1 - W0), (n,), device=DEV)
    pi, pj, gd = (torch.empty(n, device=DEV) for _ in range(3))
    gc = torch.empty(n, 3, device=DEV)
    check(lib().adfp_select_pixels(ptr(pick), n, H0, H1, W0, W1, H, W, ptr(depth), ptr(color), ptr(pi), ptr(pj), ptr(gd), ptr(gc), stream()), 'select')
    assert torch.equal(pi, i) and torch.equal(pj, j) and torch.equal(gd, d) and torch.equal(gc, c)
    assert lib().adfp_select_pixels(ptr(pick), n, H0, H + 1, W0, W1, H, W, ptr(depth), ptr(color), ptr(pi), ptr(pj), ptr(gd), ptr(gc), stream()) == -1


def test_get_samples_fast_path_equals_the_reference_composition():
    """common.get_samples on the GPU (one draw + adfp_select_pixels + the ray kernel) against get_sample_uv + get_rays_from_uv,
    the reference's own composition (src/common.py:127-136), on the same generator state."""
    sc = synthetic.mini_scene(device=DEV)
    H, W = sc.H, sc.W
    g = torch.Generator().manual_seed(4)
    depth, color = torch.rand(H, W, generator=g).to(DEV), torch.rand(H, W, 3, generator=g).to(DEV)
    c2w = sc.default_c2w()
    for (H0, H1, W0, W1) in ((0, H, 0, W), (EDGE, H - EDGE, EDGE, W - EDGE)):
        torch.manual_seed(5)
        ro, rd, gd, gc = common.get_samples(H0, H1, W0, W1, 500, H, W, sc.fx, sc.fy, sc.cx, sc.cy, c2w, depth, color, DEV)
        torch.manual_seed(5)
        i, j, d2, c2 = common.get_sample_uv(H0, H1, W0, W1, 500, depth, color, device=DEV)
        ro2, rd2 = common.get_rays_from_uv(i, j, c2w, H, W, sc.fx, sc.fy, sc.cx, sc.cy, DEV)
        assert torch.equal(ro, ro2) and torch.equal(rd, rd2) and torch.equal(gd, d2) and torch.equal(gc, c2)
    # the generic path (here: a float64 depth image) still works
    torch.manual_seed(5)
    ro3, rd3, gd3, gc3 = common.get_samples(0, H, 0, W, 500, H, W, sc.fx, sc.fy, sc.cx, sc.cy, c2w, depth.double(), color, DEV)
    assert gd3.dtype == torch.float64 and ro3.shape == (500, 3)


def test_get_samples_multi_equals_the_sequential_calls():
    """common.get_samples_multi (the per-frame draws + ONE adfp_sample_keyframes launch) against get_samples per keyframe and the four
    torch.cat of src/Mapper.py:421-436, on the same generator state: bit for bit; poses on the device ([4,4] and [3,4]), on the host
    (tensor, numpy), filling caller-owned buffers, and the per-frame fallback (a float64 depth image)."""
    import numpy as np
    sc = synthetic.mini_scene(device=DEV)
    H, W = sc.H, sc.W
    g = torch.Generator().manual_seed(11)
    frames = []
    for k in range(5):
        c2w = sc.default_c2w(yaw=0.3 * k, pitch=0.05 * k, offset=(0.1 * k, 0.0, 0.05 * k))
        c2w = (c2w.to(DEV), c2w.to(DEV)[:3].contiguous(), c2w.cpu(), c2w.cpu().numpy(), c2w.to(DEV))[k]
        frames.append((c2w, torch.rand(H, W, generator=g).to(DEV), torch.rand(H, W, 3, generator=g).to(DEV)))
    args = (H, W, sc.fx, sc.fy, sc.cx, sc.cy)
    for (H0, H1, W0, W1) in ((0, H, 0, W), (EDGE, H - EDGE, EDGE, W - EDGE)):
        torch.manual_seed(7)
        parts = [common.get_samples(H0, H1, W0, W1, 333, *args, c2w if not isinstance(c2w, np.ndarray) else c2w, d, c, DEV) for c2w, d, c in frames]
        want = [torch.cat([p[k].float() for p in parts]) for k in range(4)]
        torch.manual_seed(7)
        got = common.get_samples_multi(H0, H1, W0, W1, 333, *args, frames, DEV)
        for a, b, name in zip(got, want, ('rays_o', 'rays_d', 'gt_depth', 'gt_color')):
            assert a.shape == b.shape and torch.equal(a, b), name
        out = tuple(torch.full_like(t, float('nan')) for t in want)
        torch.manual_seed(7)
        res = common.get_samples_multi(H0, H1, W0, W1, 333, *args, frames, DEV, out=out)
        assert all(r is o for r, o in zip(res, out)) and all(torch.equal(a, b) for a, b in zip(out, want))
    # the next draw continues the stream where the sequential calls would
    torch.manual_seed(7)
    for c2w, d, c in frames:
        common.get_samples(0, H, 0, W, 333, *args, c2w, d, c, DEV)
    nxt = torch.randint(1000, (4,), device=DEV)
    torch.manual_seed(7)
    common.get_samples_multi(0, H, 0, W, 333, *args, frames, DEV)
    assert torch.equal(torch.randint(1000, (4,), device=DEV), nxt)
    # per-frame fallback
    torch.manual_seed(7)
    slow = common.get_samples_multi(0, H, 0, W, 50, *args, [(frames[0][0], frames[0][1].double(), frames[0][2])], DEV)
    assert slow[0].shape == (50, 3) and slow[2].dtype == torch.float32
    with pytest.raises(ValueError):
        common.get_samples_multi(0, H, 0, W, 50, *args, frames, DEV, out=tuple(t[:10] for t in want))


def run_loss(depth, unc, color, gd, gc, keep, handle_dynamic, w_color):
    n = depth.shape[0]
    la = _lib.AdfpTrackLossArgs()
    d, u, c, g1, g2 = depth.to(DEV), unc.to(DEV), color.to(DEV), gd.to(DEV), gc.to(DEV)
    k = None if keep is None else keep.to(DEV, torch.uint8)
    loss = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    g_d, g_c = torch.empty(n, dtype=torch.float64, device=DEV), torch.empty(n, 3, device=DEV)
    la.n_rays, la.handle_dynamic, la.w_color_loss = n, int(handle_dynamic), w_color
    la.depth, la.uncertainty, la.color, la.gt_depth, la.gt_color = d.data_ptr(), u.data_ptr(), c.data_ptr(), g1.data_ptr(), g2.data_ptr()
    la.keep = None if k is None else k.data_ptr()
    la.loss, la.g_depth, la.g_color = loss.data_ptr(), g_d.data_ptr(), g_c.data_ptr()
    check(lib().adfp_tracker_loss(C.byref(la), stream()), 'adfp_tracker_loss')
    return loss.cpu(), g_d.cpu(), g_c.cpu()


@pytest.mark.parametrize('n', [1, 2, 199, 200, 1000, 5000])
@pytest.mark.parametrize('handle_dynamic', [True, False])
def test_tracker_loss_matches_the_reference_formula(n, handle_dynamic):
    g = torch.Generator().manual_seed(n)
    depth = (torch.rand(n, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    unc = torch.rand(n, generator=g, dtype=torch.float64) * 0.1
    color = torch.rand(n, 3, generator=g).requires_grad_(True)
    gd = torch.rand(n, generator=g) * 3
    gd[torch.rand(n, generator=g) < 0.1] = 0.0
    out = torch.rand(n, generator=g) < 0.05
    gd = torch.where(out, gd + 40.0, gd)                       # outliers the median mask removes
    gc = torch.rand(n, 3, generator=g)
    keep = torch.rand(n, generator=g) < 0.8
    if n <= 2:
        keep[:] = True
    for kp in (None, keep):
        depth.grad = color.grad = None
        sel = slice(None) if kp is None else kp
        ref = O.tracker_loss(depth[sel], unc[sel], color[sel], gd[sel], gc[sel], handle_dynamic=handle_dynamic, w_color_loss=0.5)
        ref.backward()
        loss, g_d, g_c = run_loss(depth.detach(), unc, color.detach(), gd, gc, kp, handle_dynamic, 0.5)
        assert abs(loss.item() - ref.item()) <= 1e-6 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
        assert (g_d - depth.grad).abs().max() <= 4e-16 * depth.grad.abs().max(), (g_d - depth.grad).abs().max()     # 1 ulp: host vs device sqrt / divide
        assert torch.equal(g_d == 0, depth.grad == 0)
        assert torch.equal(g_c, color.grad)


def test_tracker_loss_edge_cases():
    # all rays dropped: zero loss, zero cotangents; NaN depth poisons the median like torch.median (mask all False -> loss 0)
    n = 64
    z = torch.zeros(n, dtype=torch.float64)
    loss, g_d, g_c = run_loss(z + 1, z + 0.01, torch.zeros(n, 3), torch.ones(n) * 2, torch.zeros(n, 3), torch.zeros(n, dtype=torch.bool), True, 0.5)
    assert loss.item() == 0 and not g_d.any() and not g_c.any()
    d = z + 1
    d[3] = float('nan')
    ref = O.tracker_loss(d, z + 0.01, torch.zeros(n, 3), torch.ones(n) * 2, torch.ones(n, 3), handle_dynamic=True)
    loss, g_d, g_c = run_loss(d, z + 0.01, torch.zeros(n, 3), torch.ones(n) * 2, torch.ones(n, 3), None, True, 0.5)
    assert ref.item() == 0 and loss.item() == 0 and not g_d.any()
    la = _lib.AdfpTrackLossArgs()
    la.n_rays = 8193
    la.depth = la.uncertainty = la.color = la.gt_depth = la.gt_color = la.g_depth = la.g_color = la.loss = 8
    assert lib().adfp_tracker_loss(C.byref(la), stream()) == -2


def test_keep_best_follows_the_reference_comparison():
    best_l = torch.full((1,), float('inf'), dtype=torch.float64, device=DEV)
    best_c = torch.zeros(7, device=DEV)
    seen = []
    for l in (5.0, 7.0, float('nan'), 3.0, 3.0, 4.0):
        cam = torch.full((7,), float(len(seen)), device=DEV)
        seen.append(l)
        check(lib().adfp_track_keep_best(ptr(torch.tensor([l], dtype=torch.float64, device=DEV)), ptr(cam), ptr(best_l), ptr(best_c), stream()), 'keep_best')
    assert best_l.item() == 3.0 and torch.equal(best_c.cpu(), torch.full((7,), 3.0))


@pytest.mark.parametrize('n', [1, 64, 257, 777, 1025])
@pytest.mark.parametrize('n_groups', [1, 2])
def test_tracker_head_and_tail_equal_the_entries_they_merge(n_groups, n):
    """adfp_tracker_head = adfp_camera_from_tensor + adfp_select_pixels + adfp_rays_from_uv + adfp_prefilter_mask and
    adfp_tracker_tail = adfp_rays_from_uv_backward + adfp_camera_from_tensor_backward + adfp_adam_prep + adfp_masked_adam_multi +
    adfp_track_keep_best (before the step with two parameter groups, after it with one): every output bit for bit, over three steps.
    n: the smallest batch, one full wave, one past the tail's 256-thread stride, a few strides, one past the head's 1 024-thread stride."""
    L = lib()
    st = stream()
    g = torch.Generator().manual_seed(21)
    H, W = 60, 80
    H0, H1, W0, W1 = 5, 55, 7, 73
    fx, fy, cx, cy = 70.0, 71.0, 39.5, 29.5
    depth = (torch.rand(H, W, generator=g) * 4).to(DEV)
    color = torch.rand(H, W, 3, generator=g).to(DEV)
    bound = torch.tensor([-1.5, 2.0, -2.0, 1.0, -0.5, 2.5], dtype=torch.float64, device=DEV)
    cam = torch.tensor([0.9, 0.1, -0.2, 0.3, 0.2, -0.1, 0.4]).to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)

    def state():
        return dict(cam=cam.clone(), m=torch.zeros(7, **f32), v=torch.zeros(7, **f32), steps=torch.zeros(n_groups, dtype=torch.int32, device=DEV),
                    derived=torch.zeros((n_groups, 2), **f32), best_l=torch.full((1,), float('inf'), dtype=torch.float64, device=DEV),
                    best_c=torch.zeros(7, **f32))
    A_, B_ = state(), state()
    lrs = [1e-2, 2e-3][:n_groups] if n_groups == 2 else [1e-2]
    for it in range(3):
        pick = torch.randint((H1 - H0) * (W1 - W0), (n,), generator=g).to(DEV)
        g_ro, g_rd = torch.randn(n, 3, generator=g).to(DEV), torch.randn(n, 3, generator=g).to(DEV)
        loss = torch.tensor([5.0 - it if it != 1 else 9.0], dtype=torch.float64, device=DEV)       # better, worse, better
        outs = []
        for merged, S in ((False, A_), (True, B_)):
            c2w = torch.empty(16, **f32)
            pi, pj, gd = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **f32)
            gc, ro, rd = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
            keep, dmax = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(1, **f32)
            g_c2w, g_cam = torch.empty(16, **f32), torch.empty(7, **f32)
            if not merged:
                check(L.adfp_camera_from_tensor(ptr(S['cam']), ptr(c2w), st), 'cam')
                check(L.adfp_select_pixels(ptr(pick), n, H0, H1, W0, W1, H, W, ptr(depth), ptr(color), ptr(pi), ptr(pj), ptr(gd), ptr(gc), st), 'sel')
                check(L.adfp_rays_from_uv(ptr(pi), ptr(pj), n, fx, fy, cx, cy, ptr(c2w), ptr(ro), ptr(rd), st), 'rays')
                check(L.adfp_prefilter_mask(ptr(ro), ptr(rd), ptr(gd), n, ptr(bound), ptr(keep), ptr(dmax), st), 'pre')
                check(L.adfp_rays_from_uv_backward(ptr(pi), ptr(pj), n, fx, fy, cx, cy, ptr(g_ro), ptr(g_rd), ptr(g_c2w), st), 'rays bwd')
                check(L.adfp_camera_from_tensor_backward(ptr(S['cam']), ptr(g_c2w), ptr(g_cam), st), 'cam bwd')
                if n_groups == 2:
                    check(L.adfp_track_keep_best(ptr(loss), ptr(S['cam']), ptr(S['best_l']), ptr(S['best_c']), st), 'keep')
                check(L.adfp_adam_prep(ptr(S['steps']), ptr(S['derived']), n_groups, (C.c_float * n_groups)(*lrs), 0.9, 0.999, None, st), 'prep')
                parts = [(4, 3), (0, 4)] if n_groups == 2 else [(0, 7)]
                arr = (_lib.AdfpAdamGroup * len(parts))()
                for k, (off, cnt) in enumerate(parts):
                    a = arr[k]
                    a.param, a.grad = S['cam'].data_ptr() + 4 * off, g_cam.data_ptr() + 4 * off
                    a.exp_avg, a.exp_avg_sq = S['m'].data_ptr() + 4 * off, S['v'].data_ptr() + 4 * off
                    a.mask, a.nvox, a.channels, a.derived = None, cnt, 1, S['derived'][k].data_ptr()
                check(L.adfp_masked_adam_multi(len(parts), C.byref(arr), 0.9, 0.999, 1e-8, st), 'adam')
                if n_groups == 1:
                    check(L.adfp_track_keep_best(ptr(loss), ptr(S['cam']), ptr(S['best_l']), ptr(S['best_c']), st), 'keep')
            else:
                ha = _lib.AdfpTrackerHeadArgs()
                ha.cam, ha.c2w, ha.idx, ha.n = S['cam'].data_ptr(), c2w.data_ptr(), pick.data_ptr(), n
                ha.H0, ha.H1, ha.W0, ha.W1, ha.H, ha.W = H0, H1, W0, W1, H, W
                ha.depth_img, ha.color_img = depth.data_ptr(), color.data_ptr()
                ha.fx, ha.fy, ha.cx, ha.cy, ha.bound = fx, fy, cx, cy, bound.data_ptr()
                ha.pix_i, ha.pix_j, ha.gt_depth, ha.gt_color = pi.data_ptr(), pj.data_ptr(), gd.data_ptr(), gc.data_ptr()
                ha.rays_o, ha.rays_d, ha.keep, ha.depth_max = ro.data_ptr(), rd.data_ptr(), keep.data_ptr(), dmax.data_ptr()
                check(L.adfp_tracker_head(C.byref(ha), st), 'head')
                ta = _lib.AdfpTrackerTailArgs()
                ta.pix_i, ta.pix_j, ta.n, ta.fx, ta.fy, ta.cx, ta.cy = pi.data_ptr(), pj.data_ptr(), n, fx, fy, cx, cy
                ta.g_rays_o, ta.g_rays_d = g_ro.data_ptr(), g_rd.data_ptr()
                ta.cam, ta.g_c2w, ta.g_cam, ta.step = S['cam'].data_ptr(), g_c2w.data_ptr(), g_cam.data_ptr(), 1
                ta.exp_avg, ta.exp_avg_sq = S['m'].data_ptr(), S['v'].data_ptr()
                ta.steps, ta.derived, ta.n_groups = S['steps'].data_ptr(), S['derived'].data_ptr(), n_groups
                ta.lr[0], ta.lr[1] = lrs[0], lrs[1] if n_groups == 2 else 0.0
                ta.beta1, ta.beta2, ta.eps = 0.9, 0.999, 1e-8
                ta.loss, ta.best_loss, ta.best_cam = loss.data_ptr(), S['best_l'].data_ptr(), S['best_c'].data_ptr()
                check(L.adfp_tracker_tail(C.byref(ta), st), 'tail')
            torch.cuda.synchronize()
            outs.append([t.clone() for t in (c2w, pi, pj, gd, gc, ro, rd, keep, dmax, g_c2w[:12], g_cam, S['cam'], S['m'], S['v'], S['steps'], S['derived'],
                                             S['best_l'], S['best_c'])])
        names = 'c2w pix_i pix_j gt_depth gt_color rays_o rays_d keep depth_max g_c2w g_cam cam exp_avg exp_avg_sq steps derived best_loss best_cam'.split()
        for a, b, name in zip(outs[0], outs[1], names):
            assert torch.equal(a, b), f'iteration {it}: {name}'
        if n >= 257:
            assert 0 < int(outs[0][7].sum()) < n                         # the pre-filter drops some and keeps some
    assert B_['best_l'].item() == 3.0


class Bench:
    def __init__(self, n_samples=16, n_surface=8):
        self.sc = sc = synthetic.mini_scene(device=DEV)
        self.dec = A.DF()
        self.dec.load_state_dict(O.random_state_dict(3))
        self.dec.bound = sc.bound
        self.dec = self.dec.to(DEV)
        for p in self.dec.parameters():
            p.requires_grad_(False)
        self.rend = A.Renderer(make_cfg(n_samples, n_surface), None, sc)
        self.c2w = sc.default_c2w()
        self.depth = sc.depth_image(self.c2w, zero_band=0.05).to(DEV).float()
        self.color = torch.rand((sc.H, sc.W, 3), generator=torch.Generator().manual_seed(0)).to(DEV)
        self.tb = sc.tsdf_bnds.to(DEV)
        cam = common.get_tensor_from_camera(self.c2w.cpu())
        cam[4:] += torch.tensor([0.012, -0.008, 0.01])
        cam[:4] += torch.tensor([0.0, 0.004, -0.003, 0.002])
        self.cam0 = cam.to(DEV)

    def iteration(self, **kw):
        sc = self.sc
        it = TrackerIteration(self.rend, self.dec, sc.c, sc.tsdf_volume, self.tb, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, EDGE, EDGE, **kw)
        it.new_frame(self.cam0, self.depth, self.color)
        return it

    def picks(self, n, count, seed=2):
        g = torch.Generator().manual_seed(seed)
        return [torch.randint((self.sc.H - 2 * EDGE) * (self.sc.W - 2 * EDGE), (n,), generator=g).to(DEV) for _ in range(count)]

    def reference_shaped(self, cam, pick, handle_dynamic=True, w_color=0.5):
        """optimize_cam_in_batch up to loss.backward(), through the package's reference-shaped API (src/Tracker.py:91-131)."""
        sc = self.sc
        H, W = sc.H, sc.W
        c2w = common.get_camera_from_tensor(cam)
        Ww = W - 2 * EDGE
        jj, ii = (pick // Ww + EDGE).float(), (pick % Ww + EDGE).float()
        gd, gc = self.depth[jj.long(), ii.long()], self.color[jj.long(), ii.long()]
        ro, rd = common.get_rays_from_uv(ii, jj, c2w, H, W, sc.fx, sc.fy, sc.cx, sc.cy, DEV)
        ro, rd, gd, gc = common.filter_rays_in_bound(ro, rd, gd, gc, sc.bound.to(DEV))
        d, u, col, _ = self.rend.render_batch_ray(sc.c, self.dec, rd, ro, DEV, sc.tsdf_volume, self.tb, 'color', gt_depth=gd)
        return O.tracker_loss(d, u.detach(), col, gd, gc, handle_dynamic=handle_dynamic, w_color_loss=w_color), ro.shape[0]


@pytest.fixture(scope='module')
def tb():
    return Bench()


def test_fused_gradient_equals_the_reference_shaped_iteration(tb):
    it = tb.iteration(use_graph=False)
    for n, pick in zip((200, 1000), tb.picks(1000, 2)):
        pick = pick[:n]
        loss, g = it.gradient(n, pick)
        cam = tb.cam0.clone().requires_grad_(True)
        ref, kept = tb.reference_shaped(cam, pick)
        ref.backward()
        assert 0 < kept <= n
        assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item()), (loss.item(), ref.item())
        scale = cam.grad.abs().max().item()
        assert (g - cam.grad).abs().max().item() <= 2e-4 * scale, (g, cam.grad)        # float atomics order differs (keep flag vs compaction)


def test_fused_gradient_against_the_oracle(tb):
    """The whole chain on the CPU oracle with torch autograd: camera tensor -> c2w -> rays -> render -> Tracker loss."""
    sc = tb.sc
    it = tb.iteration(use_graph=False)
    pick = tb.picks(300, 1, seed=9)[0]
    loss, g = it.gradient(300, pick)
    cam = tb.cam0.cpu().clone().requires_grad_(True)
    c2w = common.get_camera_from_tensor(cam)
    Ww = sc.W - 2 * EDGE
    pk = pick.cpu()
    jj, ii = (pk // Ww + EDGE).float(), (pk % Ww + EDGE).float()
    gd, gc = tb.depth.cpu()[jj.long(), ii.long()], tb.color.cpu()[jj.long(), ii.long()]
    ro, rd = O.get_rays_from_uv(ii, jj, c2w, sc.fx, sc.fy, sc.cx, sc.cy)
    keep = O.prefilter_mask(ro.detach(), rd.detach(), gd, sc.bound)
    d, u, col, _ = O.render_batch_ray(O.random_state_dict(3), {k: v.cpu() for k, v in sc.c.items()}, rd[keep], ro[keep], sc.tsdf_volume.cpu(),
                                      sc.tsdf_bnds, sc.bound, 'color', gd[keep], 16, 8)
    ref = O.tracker_loss(d, u.detach(), col, gd[keep], gc[keep])
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 2e-4 * abs(ref.item()), (loss.item(), ref.item())
    scale = cam.grad.abs().max().item()
    assert (g.cpu() - cam.grad).abs().max().item() <= 2e-3 * scale, (g.cpu(), cam.grad)


def test_f16_split_pose_gradient_equals_the_exact_backward(tb):
    """With everything but the pose frozen the ray gradient comes from the f16-split backward kernels (k_decode_bwd_h / k_attention_bwd_h,
    PGRAD); latching the backward onto the exact f32-input MFMA kernels must give the same pose gradient to f32 rounding."""
    it = tb.iteration(use_graph=False)
    pick = tb.picks(1000, 1, seed=21)[0]
    assert not tb.dec._exact_latch
    loss, g = it.gradient(1000, pick)
    tb.dec._exact_latch.add('bwd')
    try:
        loss_x, g_x = it.gradient(1000, pick)
    finally:
        tb.dec._exact_latch.discard('bwd')
    assert loss.item() == loss_x.item()                       # same forward
    scale = g_x.abs().max().item()
    diff = (g - g_x).abs().max().item()
    assert 0 < diff <= 2e-5 * scale, (diff, scale, g, g_x)    # two different kernel families, one answer


def test_tracker_loss_with_many_equal_values():
    """Ties: the radix select must land on the tied value when the median falls inside a run of equal tmp."""
    n = 600
    g = torch.Generator().manual_seed(3)
    depth = torch.full((n,), 1.0, dtype=torch.float64).requires_grad_(True)
    unc = torch.full((n,), 0.04, dtype=torch.float64)
    gd = 1.0 + torch.randint(0, 4, (n,), generator=g).float() * 0.25           # four distinct values, ~150 rays each
    gd[::50] = 90.0
    color, gc = torch.rand(n, 3, generator=g).requires_grad_(True), torch.rand(n, 3, generator=g)
    ref = O.tracker_loss(depth, unc, color, gd, gc)
    ref.backward()
    loss, g_d, g_c = run_loss(depth.detach(), unc, color.detach(), gd, gc, None, True, 0.5)
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())           # the reference sums the colour term in float32
    assert torch.equal(g_d == 0, depth.grad == 0) and torch.equal(g_c, color.grad)


@pytest.mark.parametrize('separate', [False, True])
def test_ten_iterations_follow_torch_adam(tb, separate):
    """num_cam_iters = 10 (configs/df_prior.yaml:27) of the fused iteration vs the same loop with torch.optim.Adam: the pose
    trajectories and the best candidate agree."""
    n, iters = 200, 10
    picks = tb.picks(n, iters, seed=4)
    it = tb.iteration(use_graph=False, seperate_LR=separate)
    if separate:
        quad, T = tb.cam0[:4].clone().requires_grad_(True), tb.cam0[4:].clone().requires_grad_(True)
        opt = torch.optim.Adam([{'params': [T], 'lr': 1e-3}, {'params': [quad], 'lr': 1e-3 * 0.2}])
    else:
        cam = tb.cam0.clone().requires_grad_(True)
        opt = torch.optim.Adam([cam], lr=1e-3)
    best, cand = 1e10, None
    for k in range(iters):
        if separate:
            cam = torch.cat([quad, T], 0)
        opt.zero_grad()
        loss, _ = tb.reference_shaped(cam, picks[k])
        loss.backward()
        opt.step()
        l_f = it.step(n, picks[k]).item()
        assert abs(l_f - loss.item()) <= 1e-4 * abs(loss.item()), (k, l_f, loss.item())
        if loss.item() < best:
            best, cand = loss.item(), cam.clone().detach()
        now = torch.cat([quad, T], 0).detach() if separate else cam.detach()
        assert (it.camera_tensor - now).abs().max().item() <= 2e-5, (k, it.camera_tensor, now)
    assert (it.best_camera_tensor - cand).abs().max().item() <= 2e-5
    assert abs(it.best_loss.item() - best) <= 1e-4 * best
    assert (it.camera_tensor - tb.cam0).abs().max().item() > 1e-3              # it did move


@pytest.mark.parametrize('handle_dynamic,use_color', [(False, True), (True, False), (False, False)])
def test_loss_options_follow_the_reference(tb, handle_dynamic, use_color):
    """tracking.handle_dynamic / tracking.use_color_in_tracking (src/Tracker.py:116-129)."""
    it = tb.iteration(use_graph=False, handle_dynamic=handle_dynamic, use_color=use_color)
    pick = tb.picks(400, 1, seed=31)[0]
    loss, g = it.gradient(400, pick)
    cam = tb.cam0.clone().requires_grad_(True)
    ref, kept = tb.reference_shaped(cam, pick, handle_dynamic=handle_dynamic, w_color=0.5 if use_color else 0.0)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item())
    assert (g - cam.grad).abs().max().item() <= 2e-4 * cam.grad.abs().max().item()


def test_graph_replay_equals_the_eager_sequence(tb):
    n, iters = 200, 6
    picks = tb.picks(n, iters, seed=6)
    a, b = tb.iteration(use_graph=False), tb.iteration(use_graph=True)
    for k in range(iters):
        la, lb = a.step(n, picks[k]), b.step(n, picks[k])
        assert abs(la.item() - lb.item()) <= 1e-9 * abs(la.item())
        assert (a.camera_tensor - b.camera_tensor).abs().max().item() <= 1e-7
    assert len(b._graphs) == 1
    # a new frame reuses the graph; replaced grids (update_para_from_mapping) do not
    b.new_frame(tb.cam0, tb.depth, tb.color)
    a.new_frame(tb.cam0, tb.depth, tb.color)
    assert (a.step(n, picks[0]) - b.step(n, picks[0])).abs().item() <= 1e-9 * a.loss.abs().item() and len(b._graphs) == 1
    c2 = {k: (v * 1.01).contiguous() for k, v in tb.sc.c.items()}
    a.update_para(c=c2)
    b.update_para(c=c2)
    la, lb = a.step(n, picks[1]), b.step(n, picks[1])
    assert abs(la.item() - lb.item()) <= 1e-9 * abs(la.item()) and len(b._graphs) == 1
    # ... and an in-place change of a grid is seen too (the Mapper writes the shared grids in place)
    c2['grid_low'].mul_(1.02)
    la, lb = a.step(n, picks[2]), b.step(n, picks[2])
    assert abs(la.item() - lb.item()) <= 1e-9 * abs(la.item())
    # Another user of the SAME Renderer with other grids in between (the reference shares slam.renderer between Tracker and
    # Mapper): it takes the engine's one-slot-per-name layout cache, recycles the buffers, or clears it.  The graph reads the
    # iteration's own channels-last copies, re-registered before every replay, so it still tracks against ITS map.
    n_graphs = len(b._graphs)
    other = {k: (v * 0.5).contiguous() for k, v in tb.sc.c.items()}
    ro, rd, gd, _ = synthetic.make_ray_batch(tb.sc, 64, seed=2)
    for clear in (False, True):
        with torch.no_grad():
            tb.rend.render_batch_ray(other, tb.dec, rd.to(DEV), ro.to(DEV), DEV, tb.sc.tsdf_volume, tb.tb, 'color', gt_depth=gd.to(DEV))
        if clear:
            tb.rend._engine._grid_cache.clear()
        lb = b.step(n, picks[3 + clear])
        la = a.step(n, picks[3 + clear])
        assert abs(la.item() - lb.item()) <= 1e-9 * abs(la.item()) and len(b._graphs) == n_graphs
        assert (a.camera_tensor - b.camera_tensor).abs().max().item() <= 1e-6


def test_tracking_converges_towards_the_true_pose():
    """A rendering-consistent target: the sensor images are what the scene renders from the true pose, so the true pose minimises the
    loss; 30 fused iterations from a perturbed start reduce the pose error."""
    tb = Bench()
    sc = tb.sc
    with torch.no_grad():
        d, u, col = tb.rend.render_img(sc.c, tb.dec, tb.c2w.to(DEV), DEV, sc.tsdf_volume, tb.tb, 'color', gt_depth=tb.depth)
    true = common.get_tensor_from_camera(tb.c2w.cpu()).to(DEV)
    it = TrackerIteration(tb.rend, tb.dec, sc.c, sc.tsdf_volume, tb.tb, sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, EDGE, EDGE, cam_lr=2e-3)
    start = true.clone()
    start[4:] += torch.tensor([0.03, -0.02, 0.025], device=DEV)
    it.new_frame(start, d.float(), col.float())
    torch.manual_seed(0)
    first = None
    for k in range(40):
        l = it.step(1000)
        first = l.item() if first is None else first
    err0, err1 = (start[4:] - true[4:]).norm().item(), (it.best_camera_tensor[4:] - true[4:]).norm().item()
    assert it.best_loss.item() < first
    # The pose kept is the one of the LOWEST LOSS SEEN (src/Tracker.py:128-131), and the loss of an iteration is that of ITS 1 000 random
    # pixels: which iteration wins is a draw, not the end of the trajectory.  Measured over 3 seeds x {f16x3 on either MFMA shape, f32}
    # (tools/experiments/track_convergence.txt): 0.0439 m -> 0.013 - 0.016 m at iteration 20, and a kept pose between 0.019 and 0.031 m
    # after 40 - 120 iterations in every mode, the exact f32 one included.  The bound is what all of them meet.
    assert err1 < 0.85 * err0, (err0, err1)
