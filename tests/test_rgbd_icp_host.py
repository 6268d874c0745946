"""CPU: the RGB-D ICP's rule as tests/rgbd_icp_ref.py restates it, on the mini scene (48 x 64).

The colour is tests/test_gpu_slam_run.py's rule, 0.5 + 0.4 sin(hit (1.3, 1.7, 2.1) + (0, 1, 2)), at every pixel's world point; the
keyframe is the same scene seen from Exp(KEY_TWIST) P, 36 mm / 27 mrad from the frame's true pose P.  The scene's default pose is the
depth ICP's DEGENERATE case (tests/test_icp_host.py): with the photometric term the same view must go through."""
import numpy as np
import pytest

import icp_ref as R
import rgbd_icp_ref as G
from attentive_dfprior_amd import synthetic


def intr(sc):
    return sc.fx, sc.fy, sc.cx, sc.cy


def frame(sc, c2w):
    """-> (depth [H,W], map [H,W,4]) of the scene seen from c2w with the CPU raycast"""
    d = R.cpu_raycast(sc, c2w)
    return d, G.frame_map(G.color_of(d, c2w, *intr(sc)), d)


@pytest.fixture(scope='module')
def world():
    sc = synthetic.mini_scene()
    P = sc.default_c2w().numpy()
    K = G.key_pose(P)
    ds, cur = frame(sc, P)
    dk, key = frame(sc, K)
    guesses = [(R.exp_se3(np.asarray(R.TWIST) * s) @ P.astype(np.float64)).astype(np.float32) for s in R.SCALES]
    models = [R.cpu_raycast(sc, g) for g in guesses]
    return sc, P, K, cur, key, guesses, models


def fd_residuals(cur, key, K, T, sc, xi, **kw):
    idx, r, _ = G.photo_pairs(cur, key, K, R.exp_se3(xi) @ T, *intr(sc), **kw)
    return dict(zip(idx.tolist(), r.tolist()))


def test_jacobian_against_finite_differences(world):
    """r(xi) at Exp(xi) T, central differences over each of the six twist components: dr / dxi = -J (the point-to-plane convention:
    the step solves sum J J^T xi = sum J r).

    Twice.  (a) A keyframe whose intensity is a linear ramp over the image, I = (256 + 4 u + 3 v) / 1024 (the three channels equal,
    every value a float32): bilinear interpolation and central differences are both exact on it, so r is smooth in xi and the analytic J is its derivative;
    what is left is the finite difference's own truncation, eps^2 times a third derivative, and its rounding, 1e-16 / eps: with
    eps = 1e-5 both are below 1e-9 against entries of J around 0.1 - 1, and the bar is 1e-6 of the largest entry.  That pins every
    sign and factor of the chain.  (b) The scene's texture: there J interpolates central differences while r interpolates
    intensities, whose slope inside a cell is the forward difference; the two differ by at most half a pixel's change of the
    gradient, |I''| / 2 per pixel.  The texture's phase advances by at most 2.1 rad/m x 35 mm = 0.07 rad per pixel at 2 m, so the
    mismatch is below 0.07 / 2 of the gradient's amplitude; the bar is 5 % of the largest |J| entry, per entry."""
    sc, P, K, cur, key, guesses, _ = world
    T = guesses[1].astype(np.float64)
    H, W = cur.shape[:2]
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ramp = ((256 + 4 * u + 3 * v) / 1024).astype(np.float32)               # multiples of 2^-10: the float32 map holds the ramp exactly
    key_ramp = key.copy()
    key_ramp[..., :3] = G.frame_map(np.repeat(ramp[..., None], 3, -1), key[..., 3])[..., :3]
    assert (key_ramp[..., 0] == ramp).all() and (key_ramp[1:-1, 1:-1, 1] == 4 / 1024).all() and (key_ramp[1:-1, 1:-1, 2] == 3 / 1024).all()
    eps = 1e-5
    for name, kmap, bar, tol in (('ramp', key_ramp, 1e-6, 10.0), ('texture', key, 5e-2, 0.25)):
        idx, r0, J = G.photo_pairs(cur, kmap, K, T, *intr(sc), rgb_tol=tol)
        assert len(idx) > 2000
        base = dict(zip(idx.tolist(), range(len(idx))))
        worst, used = 0.0, len(idx)
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = eps
            rp, rm = fd_residuals(cur, kmap, K, T, sc, xi, rgb_tol=tol), fd_residuals(cur, kmap, K, T, sc, -xi, rgb_tol=tol)
            both = [i for i in base if i in rp and i in rm]                # a pair whose gates flip within eps is left out
            used = min(used, len(both))
            fd = np.array([(rp[i] - rm[i]) / (2 * eps) for i in both])
            worst = max(worst, float(np.abs(fd + J[[base[i] for i in both], k]).max()))
        scale = float(np.abs(J).max())
        print(f'{name}: max |fd + J| {worst:.3e} against max |J| {scale:.3e} ({worst / scale:.2e}, bar {bar:.0e}), {used} of {len(idx)} pairs')
        assert used > 0.99 * len(idx) and worst <= bar * scale, name


def test_the_degenerate_view_goes_through_with_the_photometric_term(world):
    sc, P, K, cur, key, guesses, models = world
    for k, (g, dm) in enumerate(zip(guesses, models)):
        _, _, status, rows, _ = G.refine(cur, dm, None, None, g, *intr(sc))
        assert status == R.DEGENERATE and rows[0, 2] < 1e-9, k
        c2w, cam, status, rows, rgb = G.refine(cur, dm, key, K, g, *intr(sc), rgb_weight=1.0)
        e0, e1 = R.pose_error(g, P), R.pose_error(c2w, P)
        print(f'guess {k}: {e0[0] * 1e3:.2f} mm {e0[1] * 1e3:.2f} mrad -> {e1[0] * 1e3:.4f} mm {e1[1] * 1e3:.4f} mrad, pivot ratio '
              f'{rows[:-1, 2].min():.2e}, pairs {rows[:-1, 0].min():.0f}..{rows[:-1, 0].max():.0f} geometric, {rgb[:-1, 0].min():.0f}..'
              f'{rgb[:-1, 0].max():.0f} photometric')
        assert status == R.OK and (rows[:, 5] == R.OK).all()
        assert e1[0] <= e0[0] / 10 and e1[1] <= e0[1] / 10, k
        assert (rows[:-1, 2] > 100 * 1e-6).all(), k                       # every pivot ratio > 100 x min_pivot
        assert np.array_equal(cam, R.camera_tensor(c2w))


def test_weight_zero_and_no_keyframe_are_the_depth_rule(world):
    sc, P, K, cur, key, guesses, models = world
    g, dm = guesses[0], models[0]
    ns, nm = R.normals(cur[..., 3], *intr(sc)), R.normals(dm, *intr(sc))
    ref, _ = R.step_sums(cur[..., 3], ns, dm, nm, g, g, *intr(sc))
    for kw in (dict(key_map=None, p_key=None), dict(key_map=key, p_key=K, rgb_weight=0.0)):
        s, _ = G.step_sums(cur, ns, dm, nm, g, kw['key_map'], kw['p_key'], g, *intr(sc), rgb_weight=kw.get('rgb_weight', 1.0))
        assert s[:29].tobytes() == ref.tobytes() and s[29] == 0 and s[30] == 0


def test_an_empty_model_image_still_yields_photometric_pairs(world):
    sc, P, K, cur, key, guesses, models = world
    g = guesses[1]
    zero = np.zeros_like(models[1])
    _, _, status, _, _ = G.refine(cur, zero, None, None, g, *intr(sc))
    assert status == R.FEW_PAIRS
    c2w, _, status, rows, rgb = G.refine(cur, zero, key, K, g, *intr(sc))
    assert status == R.OK and (rows[:-1, 0] == 0).all() and (rgb[:-1, 0] > 0.5 * 12).all()
    e0, e1 = R.pose_error(g, P), R.pose_error(c2w, P)
    print(f'photometric pairs alone: {e0[0] * 1e3:.2f} mm -> {e1[0] * 1e3:.3f} mm, pivot ratio {rows[:-1, 2].min():.2e}')
    assert e1[0] < e0[0]


def test_frame_map_borders_and_nan():
    rng = np.random.default_rng(0)
    color = rng.random((5, 7, 3), dtype=np.float32)
    color[2, 3, 1] = np.nan
    depth = rng.random((5, 7), dtype=np.float32)
    m = G.frame_map(color, depth)
    assert m[..., 3].tobytes() == depth.tobytes()
    assert not m[:, 0, 1].any() and not m[:, -1, 1].any() and not m[0, :, 2].any() and not m[-1, :, 2].any()
    assert np.isnan(m[2, 3, 0]) and np.isnan(m[2, 2, 1]) and np.isnan(m[2, 4, 1]) and np.isnan(m[1, 3, 2]) and np.isnan(m[3, 3, 2])
    assert np.isfinite(m[2, 3, 1:3]).all() and int(np.isnan(m).sum()) == 5
    I = 0.299 * color[..., 0].astype(np.float64) + 0.587 * color[..., 1] + 0.114 * color[..., 2]
    assert abs(m[1, 1, 1] - (I[1, 2] - I[1, 0]) / 2) < 1e-7 and abs(m[1, 1, 2] - (I[2, 1] - I[0, 1]) / 2) < 1e-7
    assert G.frame_map(color[:1, :1], depth[:1, :1])[0, 0, 1:3].tolist() == [0.0, 0.0]


def test_float32_against_float64(world):
    """The yardstick of the kernels' bars: how far single precision moves the frame map, one step's 31 sums, a refinement's pose."""
    sc, P0, K0, cur0, key0, guesses, models = world
    e_map = e_s = e_m = e_r = 0.0
    count_diff = 0
    for P, Gs in R.scene_cases(sc)[::3] + [(P0, None)]:
        d = R.cpu_raycast(sc, P)
        col = G.color_of(d, P, *intr(sc))
        m64, m32 = G.frame_map(col, d), G.frame_map(col, d, np.float32)
        e_map = max(e_map, float(np.abs(m64[..., :3].astype(np.float64) - m32[..., :3]).max()))
    for P, Gs in R.scene_cases(sc):
        ds, cur = frame(sc, P)
        K = G.key_pose(P, G.CASE_KEY_SCALE)
        _, key = frame(sc, K)
        dm = R.cpu_raycast(sc, Gs)
        ns, nm = R.normals(ds, *intr(sc)), R.normals(dm, *intr(sc))
        for stride in (1, 2):
            s64, scale = G.step_sums(cur, ns, dm, nm, Gs, key, K, Gs, *intr(sc), stride=stride)
            s32, _ = G.step_sums(cur, ns, dm, nm, Gs, key, K, Gs, *intr(sc), stride=stride, dtype=np.float32)
            assert s64[30] > 0.8 * (48 // stride) * (64 // stride)
            for q in (28, 30):
                assert abs(s64[q] - s32[q]) <= 1e-3 * s64[q]
                count_diff = max(count_diff, int(abs(s64[q] - s32[q])))
            e_s = max(e_s, float((np.abs(s64 - s32.astype(np.float64)) / scale).max()))
    for g, dm in zip(guesses, models):
        a, _, sa, _, _ = G.refine(cur0, dm, key0, K0, g, *intr(sc))
        b, _, sb, _, _ = G.refine(cur0, dm, key0, K0, g, *intr(sc), dtype=np.float32)
        assert sa == sb == R.OK
        m, r = R.pose_error(a, b)
        e_m, e_r = max(e_m, m), max(e_r, r)
    print(f'float32 vs float64: map {e_map:.3e}, sums {e_s:.3e} (pair counts differ by at most {count_diff}), pose {e_m:.3e} m {e_r:.3e} rad')
    assert e_map <= G.F32_VS_F64_MAP and e_s <= G.F32_VS_F64_SUMS and e_m <= G.F32_VS_F64_POSE_M and e_r <= G.F32_VS_F64_POSE_RAD
