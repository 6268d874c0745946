"""Host statement of the rendering metrics (include/adfp.h "rendering metrics"; attentive_dfprior_amd/render_eval.py) in numpy f64:
the 35 values adfp_frame_metrics writes for a frame, and what render_eval makes of them.  A helper, not a test.

The SSIM / MS-SSIM convention is the pytorch_msssim package's -- an 11-tap Gaussian window of sigma 1.5 applied separably without
padding, C1 = (0.01)^2, C2 = (0.03)^2 at data range 1, the mean over all window positions, 2 x 2 average pooling with
padding = size % 2 between levels, the five published weights -- restated here from its formula.  That package is not installed
where this was written, nor is skimage: the device numbers are pinned to THIS file (and this file to an independent torch f64
restatement, tests/test_render_ref_host.py), not to either package.

`cases()` are the shared inputs of the host and GPU tests: built once, never modified."""
import numpy as np

import vis_ref

N_ROW = 35
MAX_LEVELS = 5
TAPS = 11
SIGMA = 1.5
C1, C2 = 1e-4, 9e-4
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
DTYPES = {'f32': np.float32, 'f64': np.float64}


def window():
    """The 11 taps, normalised to sum 1 in f64."""
    d = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def images(gt_color, color):
    """(x, y) f64 [H, W, 3]: x = gt_color, y = clip(color, 0, 1) with NaN mapped to 0 (vis_ref.rgb_panel's rule)."""
    with np.errstate(all='ignore'):
        y = np.clip(color, 0, 1)
    return np.asarray(gt_color).astype(np.float64), np.where(np.isnan(y), 0, y).astype(np.float64)


def blur(img):
    """The window along the columns, then along the rows, no padding: [H, W, 3] -> [H - 10, W - 10, 3]."""
    g = window()
    H, W = img.shape[:2]
    rows = sum(g[k] * img[:, k:k + W - (TAPS - 1)] for k in range(TAPS))
    return sum(g[k] * rows[k:k + H - (TAPS - 1)] for k in range(TAPS))


def maps(x, y):
    """(ssim map, cs map), each [H - 10, W - 10, 3], of a level's two images."""
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    cs = (2.0 * sxy + C2) / (sxx + syy + C2)
    return (2.0 * mx * my + C1) / (mx * mx + my * my + C1) * cs, cs


def pooled_size(n):
    return (n + 2 * (n % 2) - 2) // 2 + 1


def pool(img):
    """F.avg_pool2d(img, 2, padding=(H % 2, W % 2)) of [H, W, 3]: 2 x 2 blocks, stride 2, after H % 2 rows and W % 2 columns of
    zeros on each side; the zeros count in the average."""
    H, W = img.shape[:2]
    p = np.pad(img, ((H % 2, H % 2), (W % 2, W % 2), (0, 0)))
    Ho, Wo = pooled_size(H), pooled_size(W)
    a = p[0:2 * Ho:2, 0:2 * Wo:2] + p[0:2 * Ho:2, 1:2 * Wo:2] + p[1:2 * Ho:2, 0:2 * Wo:2] + p[1:2 * Ho:2, 1:2 * Wo:2]
    assert a.shape[:2] == (Ho, Wo)
    return a * 0.25


def level_sizes(H, W, levels):
    out = []
    for _ in range(levels):
        out.append((H, W))
        H, W = pooled_size(H), pooled_size(W)
    return out


def max_levels(H, W):
    """The largest `levels` a frame takes: every level's image is at least 11 on a side."""
    n = 0
    while n < MAX_LEVELS and min(H, W) >= TAPS:
        n += 1
        H, W = pooled_size(H), pooled_size(W)
    return n


def windows(H, W, levels):
    """Window positions per level, 0 beyond `levels`: [5] ints."""
    assert 0 <= levels <= max_levels(H, W)
    return [(h - (TAPS - 1)) * (w - (TAPS - 1)) for h, w in level_sizes(H, W, levels)] + [0] * (MAX_LEVELS - levels)


def level_maps(gt_color, color, levels):
    """[(ssim map, cs map)] per level."""
    x, y = images(gt_color, color)
    out = []
    for k in range(levels):
        out.append(maps(x, y))
        if k + 1 < levels:
            x, y = pool(x), pool(y)
    return out


def rows(gt_depth, gt_color, depth, color, levels):
    """The 35 values of a frame, numpy's own f64 sums."""
    s = vis_ref.stats(gt_depth, gt_color, depth, color)
    row = np.zeros(N_ROW, np.float64)
    row[:5] = [s['n_valid'], s['depth_abs_sum'], s['color_sq_sum'], s['n_color'], s['n_nonfinite']]
    for k, (ssim, cs) in enumerate(level_maps(gt_color, color, levels)):
        for c in range(3):
            row[5 + 6 * k + 2 * c] = ssim[..., c].sum()
            row[5 + 6 * k + 2 * c + 1] = cs[..., c].sum()
    return row


def per_frame(row, H, W, levels):
    """What render_eval.FrameMetrics.per_frame makes of a row: psnr and depth_l1 by visualizer.stats_dict's formulas; ssim, level
    0's means averaged over the channels; ms_ssim, per channel prod_k relu(cs_k)^w_k (k < levels - 1) times
    relu(ssim_{levels-1})^w_{levels-1}, then the channel mean -- NaN unless levels == 5."""
    row = np.asarray(row, np.float64)
    n = windows(H, W, levels)
    out = {'n_valid': int(row[0]), 'n_nonfinite': int(row[4])}
    with np.errstate(all='ignore'):
        out['depth_l1'] = float(row[1] / row[0])
        out['psnr'] = float(-10.0 * np.log10(row[2] / (3.0 * row[3])))
    out['ssim'] = float(np.mean([row[5 + 2 * c] / n[0] for c in range(3)])) if levels >= 1 else float('nan')
    if levels == MAX_LEVELS:
        per_channel = []
        for c in range(3):
            v = 1.0
            for k in range(levels):
                m = row[5 + 6 * k + 2 * c + (0 if k == levels - 1 else 1)] / n[k]
                v *= max(m, 0.0) ** MS_SSIM_WEIGHTS[k]
            per_channel.append(v)
        out['ms_ssim'] = float(np.mean(per_channel))
    else:
        out['ms_ssim'] = float('nan')
    return out


# name -> (shape, content).  The shapes: one window; odd in both axes; a strip two window rows high; odd at two levels
# (47 -> 24 -> 12, 53 -> 27 -> 14); the end-to-end test's frame.
CASES = {
    'one_window_11x11': ((11, 11), 'noise'),
    'odd_13x17': ((13, 17), 'noise'),
    'strip_12x40': ((12, 40), 'noise'),
    'noise_47x53': ((47, 53), 'noise'),
    'noise_24x32': ((24, 32), 'noise'),
    'exact_47x53': ((47, 53), 'exact'),
    'exact_11x11': ((11, 11), 'exact'),
    'constant_47x53': ((47, 53), 'constant'),
    'out_of_range_47x53': ((47, 53), 'out_of_range'),
    'nonfinite_47x53': ((47, 53), 'nonfinite'),
    'nonfinite_13x17': ((13, 17), 'nonfinite'),
    'gt_depth_zero_24x32': ((24, 32), 'gt_depth_zero'),
    'nearly_black_47x53': ((47, 53), 'nearly_black'),
}


def case(name, color_dtype=np.float32):
    """(gt_depth f32 [H,W], gt_color [H,W,3], depth f64, color f32) of a named case."""
    hw, kind = CASES[name]
    seed = 300 + list(CASES).index(name)
    gt_depth, gt_color, depth, color = vis_ref.frame(seed, hw, color_dtype)
    rng = np.random.RandomState(seed + 50)
    n = hw[0] * hw[1]
    gd, d = gt_depth.reshape(-1), depth.reshape(-1)          # views
    gc, c = gt_color.reshape(-1, 3), color.reshape(-1, 3)
    if kind == 'exact':                                       # rendered = sensor exactly: colours that float32 holds
        gc[:] = gc.astype(np.float32).astype(color_dtype)
        c[:] = gc.astype(np.float32)
        d[:] = gd.astype(np.float64)
        assert np.array_equal(c.astype(np.float64), gc.astype(np.float64))
    elif kind == 'constant':
        c[:] = np.float32(0.3)
    elif kind == 'out_of_range':
        pos = rng.permutation(n)
        c[pos[:n // 8]] = rng.uniform(-1.0, 0.0, (n // 8, 3)).astype(np.float32)
        c[pos[n // 8:n // 4]] = rng.uniform(1.0, 2.5, (n // 4 - n // 8, 3)).astype(np.float32)
        gc[pos[n // 6:n // 3]] = rng.uniform(-0.5, 1.5, (n // 3 - n // 6, 3)).astype(color_dtype)
    elif kind == 'nonfinite':
        pos = rng.permutation(n)
        m = max(n // 20, 3)
        d[pos[:m]] = np.nan
        d[pos[m:m + 2]] = [np.inf, -np.inf]
        c[pos[m // 2:m // 2 + m], rng.randint(0, 3, m)] = np.nan
        c[pos[2 * m:2 * m + 3]] = np.array([[np.inf, 0.5, 0.25], [-np.inf, 0.5, 0.25], [np.nan, np.inf, -np.inf]], np.float32)
        gd[pos[m // 3:m]] = 0.0
    elif kind == 'gt_depth_zero':
        gd[:] = 0.0
    elif kind == 'nearly_black':                              # C1 and C2 decide
        gc[:] = (1e-3 * gc.astype(np.float64)).astype(color_dtype)
        c[:] = (1e-3 * rng.uniform(0.0, 1.0, (n, 3))).astype(np.float32)
    else:
        assert kind == 'noise'
    for a in (gt_depth, gt_color, depth, color):
        a.flags.writeable = False
    return gt_depth, gt_color, depth, color


_cases = {}
_rows = {}


def cases(name, color_dtype=np.float32):
    """case() built once per (name, dtype) and shared read-only."""
    key = (name, np.dtype(color_dtype).name)
    if key not in _cases:
        _cases[key] = case(name, color_dtype)
    return _cases[key]


def case_rows(name, color_dtype, levels):
    """rows() of a case, computed once."""
    key = (name, np.dtype(color_dtype).name, levels)
    if key not in _rows:
        r = rows(*cases(name, color_dtype), levels)
        r.flags.writeable = False
        _rows[key] = r
    return _rows[key]
