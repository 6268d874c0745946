"""CPU: the host statement of the rendering metrics (tests/render_ref.py) against a second, independent restatement in torch f64 --
F.conv2d with the 11 x 11 outer-product window (121 terms in one sum instead of 11 + 11) and F.avg_pool2d with
padding = (H % 2, W % 2) -- and its fixed points.

Bounds: level sizes and window counts are integers, exact.  The sums are held to 1e-12 relative: both sides compute every moment
in f64 from the same taps, and differ in the order of a 121-term sum of products of magnitude <= 1 (<= 121 x 2^-53 = 1.3e-14 per
moment) ahead of quotients whose denominators are at least C2 = 9e-4 beside values of O(1); the difference measured 3e-15 on these
shapes.  Neither side is pytorch_msssim or skimage (not installed): the convention is restated from the formula."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import render_ref

SUM_TOL = 1e-12


def torch_rows(gt_color, color, levels):
    """([(H, W)] per level, [windows] per level, the 30 sums) with torch's own convolution and pooling."""
    x = torch.from_numpy(np.asarray(gt_color).astype(np.float64))
    y = torch.from_numpy(np.array(color))                                 # a copy: the shared cases are read-only
    y = torch.nan_to_num(y.clamp(0, 1), nan=0.0).to(torch.float64)       # clamp passes NaN on; the infinities are clipped first
    x, y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]             # [1, 3, H, W]
    g = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(g ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    k2 = torch.outer(g, g)[None, None].repeat(3, 1, 1, 1)                 # [3, 1, 11, 11], one per channel

    def blur(t):
        return F.conv2d(t, k2, groups=3)

    sizes, counts, sums = [], [], np.zeros(30)
    for k in range(levels):
        sizes.append(tuple(x.shape[-2:]))
        mx, my = blur(x), blur(y)
        sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        cs = (2 * sxy + 0.03 ** 2) / (sxx + syy + 0.03 ** 2)
        ssim = (2 * mx * my + 0.01 ** 2) / (mx ** 2 + my ** 2 + 0.01 ** 2) * cs
        counts.append(ssim.shape[-2] * ssim.shape[-1])
        for c in range(3):
            sums[6 * k + 2 * c] = float(ssim[0, c].sum())
            sums[6 * k + 2 * c + 1] = float(cs[0, c].sum())
        if k + 1 < levels:
            pad = (x.shape[-2] % 2, x.shape[-1] % 2)
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    return sizes, counts, sums


@pytest.mark.parametrize('dt', list(render_ref.DTYPES))
@pytest.mark.parametrize('name', list(render_ref.CASES))
def test_statement_against_torch(name, dt):
    gt_depth, gt_color, depth, color = render_ref.cases(name, render_ref.DTYPES[dt])
    H, W = gt_depth.shape
    top = render_ref.max_levels(H, W)
    assert top >= 1
    sizes, counts, sums = torch_rows(gt_color, color, top)
    assert sizes == render_ref.level_sizes(H, W, top)
    for levels in range(top + 1):
        row = render_ref.case_rows(name, render_ref.DTYPES[dt], levels)
        assert row.shape == (35,) and render_ref.windows(H, W, levels) == counts[:levels] + [0] * (5 - levels)
        want = np.where(np.arange(30) < 6 * levels, sums, 0.0)
        err = np.abs(row[5:] - want)
        rel = (err / np.where(want != 0, np.abs(want), 1.0)).max()
        print(f'{name} {dt} levels {levels}: worst relative difference of a sum {rel:.2e} (bound {SUM_TOL:g})')
        assert (err <= SUM_TOL * np.abs(want)).all(), (name, dt, levels, row[5:], want)
        assert (row[5 + 6 * levels:] == 0).all()
        assert np.isfinite(row).all()


def test_level_sizes_are_avg_pool2d_s():
    assert render_ref.level_sizes(47, 53, 3) == [(47, 53), (24, 27), (12, 14)]
    assert render_ref.max_levels(47, 53) == 3 and render_ref.max_levels(24, 32) == 2 and render_ref.max_levels(11, 11) == 1
    assert render_ref.max_levels(10, 500) == 0
    assert render_ref.max_levels(176, 176) == 5 and render_ref.max_levels(175, 176) == 5 and render_ref.max_levels(161, 177) == 5
    assert render_ref.max_levels(160, 1000) == 4 and render_ref.max_levels(680, 1200) == 5
    for n in range(1, 200):
        t = F.avg_pool2d(torch.zeros(1, 1, n, 2), 2, padding=(n % 2, 0))
        assert t.shape[-2] == render_ref.pooled_size(n), n


@pytest.mark.parametrize('dt', list(render_ref.DTYPES))
@pytest.mark.parametrize('name', ['exact_47x53', 'exact_11x11'])
def test_rendered_equal_to_sensor_is_a_fixed_point(name, dt):
    gt_depth, gt_color, depth, color = render_ref.cases(name, render_ref.DTYPES[dt])
    H, W = gt_depth.shape
    top = render_ref.max_levels(H, W)
    for ssim, cs in render_ref.level_maps(gt_color, color, top):
        assert np.abs(ssim - 1.0).max() <= 1e-15 and np.abs(cs - 1.0).max() <= 1e-15
    row = render_ref.case_rows(name, render_ref.DTYPES[dt], top)
    got = render_ref.per_frame(row, H, W, top)
    assert got['psnr'] == np.inf and got['depth_l1'] == 0.0 and abs(got['ssim'] - 1.0) <= 1e-15
    assert np.isnan(got['ms_ssim'])                       # fewer than five levels


def test_ms_ssim_with_a_negative_cs_mean_is_finite():
    """A rendered image that is the sensor's negative: the contrast-structure mean is negative at every level, a fractional power
    of which would be NaN -- the relu makes the product 0."""
    rng = np.random.RandomState(5)
    H = W = 176                                           # five levels, even at each: 176 -> 88 -> 44 -> 22 -> 11
    gt_color = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    color = (1.0 - gt_color).astype(np.float32)
    gt_depth = np.ones((H, W), np.float32)
    row = render_ref.rows(gt_depth, gt_color, gt_depth.astype(np.float64), color, 5)
    n = render_ref.windows(H, W, 5)
    assert n[4] == 1 and n[0] == 166 * 166
    cs_means = [row[5 + 6 * k + 2 * c + 1] / n[k] for k in range(5) for c in range(3)]
    assert min(cs_means) < 0
    got = render_ref.per_frame(row, H, W, 5)
    assert np.isfinite(got['ms_ssim']) and got['ms_ssim'] == 0.0
    # and of a frame against itself, five levels: 1
    same = render_ref.per_frame(render_ref.rows(gt_depth, gt_color, gt_depth.astype(np.float64), gt_color, 5), H, W, 5)
    assert abs(same['ms_ssim'] - 1.0) <= 1e-14 and abs(same['ssim'] - 1.0) <= 1e-15
    # a noisy rendering lies strictly between
    noisy = (gt_color + 0.1 * rng.standard_normal(gt_color.shape)).astype(np.float32)
    mid = render_ref.per_frame(render_ref.rows(gt_depth, gt_color, gt_depth.astype(np.float64), noisy, 5), H, W, 5)
    assert 0.0 < mid['ssim'] < mid['ms_ssim'] < 1.0
