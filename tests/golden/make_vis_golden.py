"""Writes tests/golden/vis_panels.npz from matplotlib itself (3.10 when the committed file was made): for every case of
tests/vis_ref.py at 37 x 53, what matplotlib maps the six arrays of the reference's Visualizer (src/utils/Visualizer.py:71-114) to.

  depth panels   colormaps['plasma'](Normalize(0, vmax)(a), bytes=True), vmax = np.max(gt_depth) as the reference passes it;
                 entries of alpha 0 (the colormap's "bad" colour, for NaN) composited over white
  RGB panels     (np.clip(a, 0, 1) * 255).astype(np.uint8), what imshow does to float RGB.  The cast of a NaN is undefined in C;
                 numpy gives 0 on the machines this ran on, which is asserted here and is the contract's choice.

Arrays only: `table` [256, 3] (the colormap at its 256 indices), `<case>` [6, 37, 53, 3] for float32 gt_color and
`<case>__f64` [2, 37, 53, 3] (input RGB and RGB residual, the two panels that depend on gt_color's dtype).

    python tests/golden/make_vis_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vis_ref                                     # noqa: E402


def mpl_depth(a, vmax):
    from matplotlib import colormaps
    from matplotlib.colors import Normalize
    with np.errstate(all='ignore'):
        rgba = colormaps['plasma'](Normalize(0, vmax)(a), bytes=True)
    assert rgba.dtype == np.uint8 and set(np.unique(rgba[..., 3])) <= {0, 255}
    return np.where(rgba[..., 3:] == 0, np.uint8(255), rgba[..., :3])


def mpl_rgb(a):
    with np.errstate(all='ignore'):
        out = (np.clip(a, 0, 1) * 255).astype(np.uint8)
    assert (out[np.isnan(a)] == 0).all(), 'this numpy casts NaN to something else than 0'
    return out


def mpl_panels(gt_depth, gt_color, depth, color):
    """The reference's arrays (Visualizer.py:76-79, :84, :100-102) through matplotlib."""
    dres, cres = vis_ref.residuals(gt_depth, gt_color, depth, color)
    vmax = np.max(gt_depth)
    return np.stack([mpl_depth(gt_depth, vmax), mpl_depth(depth, vmax), mpl_depth(dres, vmax),
                     mpl_rgb(gt_color), mpl_rgb(color), mpl_rgb(cres)])


def mpl_table():
    from matplotlib import colormaps
    return np.ascontiguousarray(colormaps['plasma'](np.arange(256), bytes=True)[:, :3])


def main():
    out = {'table': mpl_table()}
    for name in vis_ref.CASES:
        six = mpl_panels(*vis_ref.case(name, np.float32))
        six64 = mpl_panels(*vis_ref.case(name, np.float64))
        assert np.array_equal(six[:3], six64[:3])          # the depth row does not see gt_color
        out[name] = six
        out[name + '__f64'] = six64[[3, 5]]
    path = os.path.join(HERE, 'vis_panels.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
