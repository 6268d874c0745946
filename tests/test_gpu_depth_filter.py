"""GPU: the depth bilateral filter (adfp_depth_bilateral, icp.depth_bilateral) against its restatement (tests/depth_filter_ref.py).

The bars: the validity pattern matches exactly; a value is within one float32 ulp (np.spacing) of the restatement's -- both add the
same float64 terms in the same order, the device's f64 exp differs from numpy's by about an ulp of float64, and that can move a
result across a float32 rounding boundary and no further; two calls give the same bytes.  The shapes: one pixel, one row, an image
smaller than the window, 17 x 33 (odd, crossing the 16 x 16 tile both ways), exactly one tile, two different images in one launch, and
a noisy 48 x 64 frame of the mini scene with holes and a step edge; radii 1, 2, 3, 8, sigma_depth_z2 0 and 0.02."""
import numpy as np
import pytest
import torch

import depth_filter_ref as F
import icp_ref as R
from attentive_dfprior_amd import icp, synthetic

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RADII = (1, 2, 3, 8)
Z2 = (0.0, 0.02)


def surface(H, W, seed):
    """A tilted plane 0.6 .. 1.4 m with 1 cm noise, a few outliers beyond 3 sigma_depth, holes of every invalid kind"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W]
    d = 0.6 + 0.8 * (u + 0.5 * v) / max(W + 0.5 * H, 1.0) + 0.01 * rng.standard_normal((H, W))
    d = d.astype(np.float32)
    n = H * W
    if n >= 7:
        flat = d.reshape(-1)
        pick = rng.permutation(n)
        flat[pick[0]] += np.float32(0.4)
        flat[pick[1]] = 0.0
        if n >= 40:
            flat[pick[2]], flat[pick[3]], flat[pick[4]], flat[pick[5]] = np.nan, np.inf, -1.0, -np.inf
            flat[pick[6:6 + n // 20]] = 0.0
    return d


def mini_frame():
    """The mini scene's first corner view through the sensor model (sigma = 0.02 z^2, holes at the depth edges) with a rectangle
    pushed 0.3 m back: a step edge inside the frame"""
    sc = synthetic.mini_scene()
    P, _ = R.scene_cases(sc)[0]
    clean = R.cpu_raycast(sc, P)
    clean[10:30, 20:45] += np.float32(0.3)
    d = synthetic.sensor_depth(clean, 5, a=0.0, b=0.02, z0=0.0, edge_jump=0.25)
    d[40:44, 5:9] = 0.0
    d[2, 60] = np.nan
    return d


IMAGES = {'1x1': lambda: np.array([[0.8]], dtype=np.float32), '1x7': lambda: surface(1, 7, 1), '5x3': lambda: surface(5, 3, 2),
          '17x33': lambda: surface(17, 33, 3), '16x16': lambda: surface(16, 16, 4),
          '2x17x33': lambda: np.stack([surface(17, 33, 5), surface(17, 33, 6)]), 'mini': mini_frame}


def hold(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.float32
    ok = R.depth_ok(ref)
    assert np.array_equal(R.depth_ok(got), ok), what
    assert (got[~ok].view(np.uint32) == 0).all(), what
    differ = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f'{what}: {differ} of {got.size} pixels not bit-equal')
    assert (np.abs(got[ok].astype(np.float64) - ref[ok]) <= np.spacing(ref[ok])).all(), what
    return differ


@pytest.mark.parametrize('name', list(IMAGES))
def test_against_the_restatement(name):
    d = IMAGES[name]()
    dd = torch.from_numpy(d).to(DEV)
    assert (~R.depth_ok(d)).any() or d.size == 1
    for radius in RADII:
        for z2 in Z2:
            kw = dict(radius=radius, sigma_space=1.0 + 0.5 * radius, sigma_depth=0.05, sigma_depth_z2=z2)
            got = icp.depth_bilateral(dd, **kw)
            assert got.shape == dd.shape and got.data_ptr() != dd.data_ptr()
            hold(got.cpu().numpy(), F.bilateral(d, **kw), f'{name}, radius {radius}, z2 {z2}')
    assert dd.cpu().numpy().tobytes() == d.tobytes()                   # the input is only read


def test_the_defaults_and_out():
    d = IMAGES['mini']()
    dd = torch.from_numpy(d).to(DEV)
    got = icp.depth_bilateral(dd)
    hold(got.cpu().numpy(), F.bilateral(d, **F.DEFAULTS), 'mini, defaults')
    out = torch.full_like(dd, -7.0)
    assert icp.depth_bilateral(dd, out=out) is out and out.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    one = icp.depth_bilateral(dd[None])                                # [1,H,W] is [H,W]
    assert one.shape == (1,) + d.shape and one[0].cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    with pytest.raises(RuntimeError):
        icp.depth_bilateral(dd, out=dd)                                # ADFP_E_ARG: not in place
    with pytest.raises(ValueError):
        icp.depth_bilateral(dd, radius=9)
    with pytest.raises(ValueError):
        icp.depth_bilateral(dd.double())


def test_two_calls_give_the_same_bytes():
    d = torch.from_numpy(IMAGES['2x17x33']()).to(DEV)
    m = torch.from_numpy(IMAGES['mini']()).to(DEV)
    for x, kw in ((d, dict(radius=8, sigma_depth_z2=0.02)), (m, dict(radius=3))):
        a = icp.depth_bilateral(x, **kw).cpu().numpy()
        out = torch.zeros_like(x)
        b = icp.depth_bilateral(x, out=out, **kw).cpu().numpy()
        assert a.tobytes() == b.tobytes()
    both = icp.depth_bilateral(d, radius=2).cpu().numpy()              # images of one launch do not see each other
    for v in range(2):
        assert both[v].tobytes() == icp.depth_bilateral(d[v].contiguous(), radius=2).cpu().numpy().tobytes()


def test_a_step_edge_separates_the_two_sides():
    """A 0.5 m step with sigma_depth 0.03: each side comes out as if the other were invalid, byte for byte (the 3 s_p gate)"""
    rng = np.random.default_rng(1)
    H, W = 20, 37
    d = (1.0 + 0.004 * rng.standard_normal((H, W))).astype(np.float32)
    near = np.arange(W)[None, :].repeat(H, 0) < 18
    d[~near] += np.float32(0.5)
    kw = dict(radius=3, sigma_space=2.0, sigma_depth=0.03)
    f = lambda x: icp.depth_bilateral(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), **kw).cpu().numpy()
    out, a, b = f(d), f(np.where(near, d, np.float32(0))), f(np.where(near, np.float32(0), d))
    assert out[near].tobytes() == a[near].tobytes() and out[~near].tobytes() == b[~near].tobytes()
    assert (a[~near] == 0).all() and (b[near] == 0).all() and (out > 0).all()
    assert out[near].tobytes() != d[near].tobytes()                    # it did filter


def test_a_constant_image_comes_back():
    d = np.full((19, 21), 2.718, dtype=np.float32)
    got = icp.depth_bilateral(torch.from_numpy(d).to(DEV), radius=8).cpu().numpy()
    assert (np.abs(got.astype(np.float64) - d) <= np.spacing(d)).all()
