"""Host statement of the Visualizer's pixel contract (include/adfp.h "visualisation"): what the reference's
src/utils/Visualizer.py:71-114 hands to matplotlib, and what matplotlib maps those arrays to -- Normalize(0, vmax) followed by
Colormap.__call__ with N = 256 for the three depth panels, the float-RGB rule of imshow for the three colour panels -- restated in
numpy.  Not imshow's resampling into a figure, no titles or axes.  A helper, not a test; matplotlib is not imported here
(tests/golden/make_vis_golden.py asks matplotlib itself, tests/test_vis_host.py holds this file to its answers byte for byte).

Every operation is exactly rounded (IEEE division, a product by 256 or 255, a truncation), so this file decides every byte.
`cases()` are the shared inputs of the golden file, the host tests and the GPU tests: built once, never modified."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vis_panels.npz')
CASE_HW = (37, 53)                 # odd, no multiple of a wave or of a dword of canvas bytes
LAYOUTS = ((1, 8), (3, 0), (7, 5))     # (stride, gap)
CASES = ('bin_edges', 'zeros', 'depth_out_of_range', 'colour_out_of_range', 'nan', 'vmax_zero', 'random')
STATS = ('vmax', 'n_valid', 'depth_abs_sum', 'color_sq_sum', 'n_nonfinite', 'n_color')
_table = None


def table():
    """matplotlib's 'plasma' at its 256 indices as bytes [256, 3], as the golden file recorded it."""
    global _table
    if _table is None:
        _table = np.load(GOLDEN)['table']
    return _table


def canvas_shape(H, W, stride=1, gap=8):
    h, w = -(-H // stride), -(-W // stride)
    return 2 * h + 3 * gap, 3 * w + 4 * gap


def depth_index(v, vmax):
    """Table index of every element of v (float32 or float64), 256 where the value is NaN.  vmax: the np.float32 maximum."""
    v = np.asarray(v)
    assert v.dtype in (np.float32, np.float64) and isinstance(vmax, np.float32)
    if vmax == 0:                                    # Normalize with vmin == vmax: every value becomes 0
        return np.zeros(v.shape, np.int64)
    with np.errstate(all='ignore'):
        x = v / v.dtype.type(vmax)                   # f32 / f32, or f64 / (double)vmax
        x = x * v.dtype.type(256)
        idx = np.where(x == 256, 255, np.clip(np.where(np.isnan(x), 0, x), 0, 255).astype(np.int64))     # astype truncates
    return np.where(np.isnan(x), 256, idx)


def depth_panel(v, vmax, tab=None):
    tab = table() if tab is None else tab
    lut = np.concatenate([tab, np.full((1, 3), 255, np.uint8)])       # entry 256: white
    return lut[depth_index(v, vmax)]


def rgb_panel(v):
    """trunc(255 clip(v, 0, 1)) with the product in v's own dtype; NaN is 0."""
    v = np.asarray(v)
    assert v.dtype in (np.float32, np.float64)
    with np.errstate(all='ignore'):
        x = np.clip(v, 0, 1) * v.dtype.type(255)
    return np.where(np.isnan(x), 0, x).astype(np.uint8)


def residuals(gt_depth, gt_color, depth, color):
    """Visualizer.py:76-79: (depth residual f64, colour residual in the promoted dtype), both zero where gt_depth == 0."""
    assert gt_depth.dtype == np.float32 and depth.dtype == np.float64 and color.dtype == np.float32
    dres = np.abs(gt_depth.astype(np.float64) - depth)
    dres[gt_depth == 0.0] = 0.0
    cres = np.abs(gt_color - color)
    assert cres.dtype == gt_color.dtype
    cres[gt_depth == 0.0] = 0.0
    return dres, cres


def panels(gt_depth, gt_color, depth, color, tab=None):
    """The six full-resolution panels [6, H, W, 3] uint8: input depth, generated depth, depth residual, input RGB, generated RGB,
    RGB residual."""
    dres, cres = residuals(gt_depth, gt_color, depth, color)
    vmax = np.max(gt_depth)
    return np.stack([depth_panel(gt_depth, vmax, tab), depth_panel(depth, vmax, tab), depth_panel(dres, vmax, tab),
                     rgb_panel(gt_color), rgb_panel(color), rgb_panel(cres)])


def compose(six, stride=1, gap=8):
    """The white canvas with panel (r, k) at (gap + r (h + gap), gap + k (w + gap)), every stride-th source pixel."""
    _, H, W, _ = six.shape
    rows, cols = canvas_shape(H, W, stride, gap)
    h, w = -(-H // stride), -(-W // stride)
    out = np.full((rows, cols, 3), 255, np.uint8)
    for n in range(6):
        r, k = divmod(n, 3)
        y, x = gap + r * (h + gap), gap + k * (w + gap)
        out[y:y + h, x:x + w] = six[n, ::stride, ::stride]
    return out


def canvas(gt_depth, gt_color, depth, color, stride=1, gap=8, tab=None):
    return compose(panels(gt_depth, gt_color, depth, color, tab), stride, gap)


def stats(gt_depth, gt_color, depth, color):
    """The frame stats over the full-resolution frame, numpy's own f64 sums; the dict visualizer.Visualizer.panels returns."""
    cf = np.isfinite(color).all(-1)
    df = np.isfinite(depth)
    valid = (gt_depth > 0) & cf & df
    e = gt_color.astype(np.float64) - color.astype(np.float64)
    s = {'vmax': float(np.max(gt_depth)), 'n_valid': int(valid.sum()),
         'depth_abs_sum': float(np.abs(gt_depth.astype(np.float64) - depth)[valid].sum()),
         'color_sq_sum': float((e[cf] * e[cf]).sum()), 'n_nonfinite': int((~(cf & df)).sum()), 'n_color': int(cf.sum())}
    with np.errstate(all='ignore'):
        s['depth_l1'] = float(np.float64(s['depth_abs_sum']) / np.float64(s['n_valid']))
        s['psnr'] = float(-10.0 * np.log10(np.float64(s['color_sq_sum']) / np.float64(3 * s['n_color'])))
    return s


def frame(seed, hw, color_dtype=np.float32, top=3.9):
    """A seeded random frame: sensor depth in [0.5, top), a rendered depth near it, colours in [0, 1] and a rendered colour near
    them (a few values leave [0, 1] on their own)."""
    rng = np.random.RandomState(seed)
    H, W = hw
    gt_depth = rng.uniform(0.5, top, (H, W)).astype(np.float32)
    depth = gt_depth.astype(np.float64) + 0.1 * rng.standard_normal((H, W))
    gt_color = rng.uniform(0.0, 1.0, (H, W, 3)).astype(color_dtype)
    color = (gt_color.astype(np.float64) + 0.05 * rng.standard_normal((H, W, 3))).astype(np.float32)
    return gt_depth, gt_color, depth, color


def case(name, color_dtype=np.float32):
    """(gt_depth f32 [37,53], gt_color [37,53,3], depth f64, color f32) of a named case."""
    hw = CASE_HW
    seed = 100 + CASES.index(name)
    gt_depth, gt_color, depth, color = frame(seed, hw, color_dtype)
    rng = np.random.RandomState(seed + 50)
    n = hw[0] * hw[1]
    gd, d = gt_depth.reshape(-1), depth.reshape(-1)          # views
    gc, c = gt_color.reshape(-1, 3), color.reshape(-1, 3)
    if name == 'bin_edges':
        # vmax = 4.0: input depths exactly on the bin edges k / 256 * 4 (exact in f32), one pixel at vmax itself (index 255);
        # rendered depths on the same edges in f64, and just below them
        k = np.arange(256)
        pos = rng.permutation(n)
        gd[pos[:256]] = (k / 256.0 * 4.0).astype(np.float32)
        gd[pos[256]] = np.float32(4.0)
        d[pos[300:556]] = k / 256.0 * 4.0
        d[pos[556:812]] = np.nextafter(k / 256.0 * 4.0, -np.inf)
        d[pos[812]] = 4.0
        assert gd.max() == np.float32(4.0)
    elif name == 'zeros':
        gd[rng.permutation(n)[:n // 5]] = 0.0
    elif name == 'depth_out_of_range':
        pos = rng.permutation(n)
        d[pos[:200]] = rng.uniform(4.0, 9.0, 200)
        d[pos[200:400]] = rng.uniform(-3.0, 0.0, 200)
        d[pos[400:404]] = [np.inf, -np.inf, -0.0, 1e300]
        gd[pos[100:120]] = 0.0
    elif name == 'colour_out_of_range':
        pos = rng.permutation(n)
        c[pos[:300]] = rng.uniform(-1.0, 0.0, (300, 3)).astype(np.float32)
        c[pos[300:600]] = rng.uniform(1.0, 2.5, (300, 3)).astype(np.float32)
        gc[pos[200:400]] = rng.uniform(-0.5, 1.5, (200, 3)).astype(color_dtype)
        c[pos[600:604]] = np.array([[0.0, 1.0, -0.0], [1.0, 1.0, 1.0], [np.inf, -np.inf, 0.5], [np.nextafter(np.float32(1), np.float32(0)), 0.5, 2.0 ** -30]], np.float32)
        gc[pos[604:606]] = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]], color_dtype)
        gd[pos[250:350]] = 0.0
    elif name == 'nan':
        pos = rng.permutation(n)
        d[pos[:150]] = np.nan
        c[pos[100:250], rng.randint(0, 3, 150)] = np.nan
        c[pos[250:260]] = np.nan
        gd[pos[50:120]] = 0.0
        gd[pos[300:330]] = 0.0
    elif name == 'vmax_zero':
        gd[:] = 0.0
        d[rng.permutation(n)[:20]] = np.nan
    else:
        assert name == 'random'
    for a in (gt_depth, gt_color, depth, color):
        a.flags.writeable = False
    return gt_depth, gt_color, depth, color


_cases = {}


def cases(name, color_dtype=np.float32):
    """case() built once per (name, dtype) and shared read-only."""
    key = (name, np.dtype(color_dtype).name)
    if key not in _cases:
        _cases[key] = case(name, color_dtype)
    return _cases[key]
