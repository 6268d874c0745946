"""CPU: the Visualizer's pixel contract without a GPU.  tests/vis_ref.py (numpy) is held byte for byte to what matplotlib itself
maps the reference's six arrays to -- recorded in tests/golden/vis_panels.npz by tests/golden/make_vis_golden.py, and asked again
directly where matplotlib is installed -- the generated table of csrc/adfp_vis.h is that file's table, and the drop-in keeps the
reference's call signatures (tests/golden/visualizer_signatures.json, tests/golden/make_visualizer_golden.py)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

import vis_ref
from conftest import GOLDEN, ROOT
from attentive_dfprior_amd import visualizer

DTYPES = {'f32': np.float32, 'f64': np.float64}


def golden_panels(z, name, dt):
    """The golden's six full-resolution panels of a case."""
    six = z[name].copy()
    if dt == 'f64':
        six[[3, 5]] = z[name + '__f64']
    return six


def test_golden_file_holds_arrays_only():
    z = np.load(os.path.join(GOLDEN, 'vis_panels.npz'), allow_pickle=False)
    assert sorted(z.files) == sorted(['table'] + list(vis_ref.CASES) + [c + '__f64' for c in vis_ref.CASES])
    H, W = vis_ref.CASE_HW
    for name in vis_ref.CASES:
        assert z[name].shape == (6, H, W, 3) and z[name].dtype == np.uint8
        assert z[name + '__f64'].shape == (2, H, W, 3) and z[name + '__f64'].dtype == np.uint8
    assert z['table'].shape == (256, 3) and z['table'].dtype == np.uint8
    assert os.path.getsize(os.path.join(GOLDEN, 'vis_panels.npz')) < 512 * 1024


@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', vis_ref.CASES)
def test_restatement_equals_matplotlib_golden(name, dt):
    z = np.load(os.path.join(GOLDEN, 'vis_panels.npz'))
    inputs = vis_ref.cases(name, DTYPES[dt])
    six = golden_panels(z, name, dt)
    assert np.array_equal(vis_ref.panels(*inputs), six)
    H, W = vis_ref.CASE_HW
    for stride, gap in vis_ref.LAYOUTS:
        got = vis_ref.canvas(*inputs, stride=stride, gap=gap)
        h, w = (H + stride - 1) // stride, (W + stride - 1) // stride
        assert got.shape == (2 * h + 3 * gap, 3 * w + 4 * gap, 3) == vis_ref.canvas_shape(H, W, stride, gap) + (3,)
        # the layout, pixel by pixel and without vis_ref's own slicing
        want = np.full(got.shape, 255, np.uint8)
        for n in range(6):
            r, k = n // 3, n % 3
            for i in range(h):
                for j in range(w):
                    want[gap + r * (h + gap) + i, gap + k * (w + gap) + j] = six[n, i * stride, j * stride]
        assert np.array_equal(got, want), (name, dt, stride, gap)


def test_cases_cover_what_they_are_named_for():
    gd, gc, d, c = vis_ref.cases('bin_edges')
    vmax = np.max(gd)
    assert vmax == np.float32(4.0) and (gd == vmax).sum() == 1
    idx = vis_ref.depth_index(gd, vmax)
    assert idx[gd == vmax] == 255 and set(range(256)) <= set(idx.reshape(-1).tolist())        # every bin's lower edge is there
    k = np.round(gd.astype(np.float64) * 64).astype(int)
    on_edge = (k / 64.0 == gd) & (k < 256)
    assert on_edge.sum() >= 256 and (idx[on_edge] == k[on_edge]).all()                       # an edge belongs to the bin above it
    idx_d = vis_ref.depth_index(d, vmax)
    below = np.nextafter(np.arange(1, 256) / 64.0, -np.inf)
    assert all((idx_d[d == b] == kk).all() and (d == b).any() for kk, b in enumerate(below))       # just below edge k + 1: bin k
    assert (vis_ref.cases('zeros')[0] == 0).sum() > 100
    gd, gc, d, c = vis_ref.cases('depth_out_of_range')
    assert (d > gd.max()).sum() >= 200 and (d < 0).sum() >= 200 and np.isinf(d).sum() == 2
    gd, gc, d, c = vis_ref.cases('colour_out_of_range')
    assert (c < 0).sum() > 100 and (c > 1).sum() > 100 and (gc < 0).sum() > 10 and (gc > 1).sum() > 10
    gd, gc, d, c = vis_ref.cases('nan')
    assert np.isnan(d).sum() == 150 and np.isnan(c).any(-1).sum() == 160 and (np.isnan(d) & np.isnan(c).any(-1)).any()
    six = vis_ref.panels(gd, gc, d, c)
    assert (six[1][np.isnan(d)] == 255).all() and (six[4][np.isnan(c)] == 0).all()            # NaN: white depth, zero colour byte
    assert (six[2][np.isnan(d) & (gd == 0)] == vis_ref.table()[0]).all() and (np.isnan(d) & (gd == 0)).any()      # the mask wins
    gd, gc, d, c = vis_ref.cases('vmax_zero')
    assert gd.max() == 0 and np.isnan(d).any()
    assert (vis_ref.panels(gd, gc, d, c)[:3] == vis_ref.table()[0]).all()                    # every value, NaN included: index 0
    assert vis_ref.cases('random', np.float64)[1].dtype == np.float64
    s = vis_ref.stats(*vis_ref.cases('nan'))
    assert (s['n_nonfinite'], s['n_color']) == (150 + 160 - 50, gd.size - 160)               # 50 pixels have both a NaN depth and colour
    assert s['n_valid'] < gd.size - s['n_nonfinite']                                         # ... and some of the rest have no sensor depth


def test_restatement_equals_matplotlib_itself():
    pytest.importorskip('matplotlib')
    sys.path.insert(0, GOLDEN)
    try:
        import make_vis_golden
    finally:
        sys.path.pop(0)
    assert np.array_equal(make_vis_golden.mpl_table(), vis_ref.table())
    for name in vis_ref.CASES:
        for dt in DTYPES.values():
            inputs = vis_ref.cases(name, dt)
            assert np.array_equal(vis_ref.panels(*inputs), make_vis_golden.mpl_panels(*inputs)), (name, dt)
    inputs = vis_ref.frame(11, (97, 131), np.float64, top=6.0)                                # a frame the golden file does not hold
    assert np.array_equal(vis_ref.panels(*inputs), make_vis_golden.mpl_panels(*inputs))


def test_header_table_is_the_golden_table():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import gen_plasma_table
    finally:
        sys.path.pop(0)
    tab = gen_plasma_table.header_table()
    assert tab.shape == (256, 3) and np.array_equal(tab, vis_ref.table())
    # the generated block is what the generator renders from this table: nothing edited by hand
    src = open(gen_plasma_table.HEADER).read()
    a, b = src.index(gen_plasma_table.BEGIN), src.index(gen_plasma_table.END) + len(gen_plasma_table.END)
    assert src[a:b] == gen_plasma_table.render(vis_ref.table())


def _assert_compatible(mine, ref, what):
    """The reference's parameters (name, kind, default) come first and unchanged; anything after them has a default."""
    pm = [(p.name, p.kind, p.default) for p in inspect.signature(mine).parameters.values()]
    pr = [(n, getattr(inspect.Parameter, k), d if has else inspect.Parameter.empty) for n, k, has, d in ref]
    assert pm[:len(pr)] == pr, f'{what}: {pm} against the reference\'s {pr}'
    for n, k, d in pm[len(pr):]:
        assert d is not inspect.Parameter.empty, f'{what}: extra required parameter {n!r}'


def test_signatures_follow_the_reference(tmp_path):
    with open(os.path.join(GOLDEN, 'visualizer_signatures.json')) as f:
        ref = json.load(f)
    _assert_compatible(visualizer.Visualizer.__init__, ref['signatures']['Visualizer.__init__'], 'Visualizer.__init__')
    _assert_compatible(visualizer.Visualizer.vis, ref['signatures']['Visualizer.vis'], 'Visualizer.vis')
    names = [p.name for p in inspect.signature(visualizer.Visualizer.__init__).parameters.values()]
    assert names[len(ref['signatures']['Visualizer.__init__']):] == ['stride', 'gap', 'ext']
    v = visualizer.Visualizer(50, 25, str(tmp_path / 'vis' / 'mapping'), None, True)          # no GPU needed; the directory is made
    assert os.path.isdir(str(tmp_path / 'vis' / 'mapping'))
    for name in ref['attributes']:
        assert hasattr(v, name), name
    assert (v.freq, v.inside_freq, v.verbose, v.device, v.stride, v.gap, v.ext, v.last_stats) == (50, 25, True, 'cuda:0', 1, 8, 'jpg', None)
    with pytest.raises(ValueError):
        visualizer.Visualizer(50, 25, str(tmp_path), None, False, ext='bmp')
    with pytest.raises(ValueError):
        visualizer.Visualizer(50, 25, str(tmp_path), None, False, stride=0)


def test_stats_dict_derives_l1_and_psnr():
    s = visualizer.stats_dict([4.0, 10.0, 5.0, 0.03, 2.0, 100.0])
    assert list(s)[:6] == list(visualizer.STATS) == list(vis_ref.STATS)
    assert (s['vmax'], s['n_valid'], s['n_nonfinite'], s['n_color']) == (4.0, 10, 2, 100) and type(s['n_valid']) is int
    assert s['depth_l1'] == 0.5 and s['psnr'] == float(-10.0 * np.log10(np.float64(0.03) / 300.0))
    s = visualizer.stats_dict([0.0, 0.0, 0.0, 0.0, 5.0, 0.0])
    assert np.isnan(s['depth_l1']) and np.isnan(s['psnr'])
    ref = vis_ref.stats(*vis_ref.cases('nan'))
    got = visualizer.stats_dict([ref[k] for k in vis_ref.STATS])
    assert got == ref
