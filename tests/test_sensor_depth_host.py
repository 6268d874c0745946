"""CPU: synthetic.sensor_depth, the sensor model of the synthetic sequences: seeded axial noise, quantisation, holes at depth edges."""
import numpy as np
import torch

from attentive_dfprior_amd import synthetic


def plane(H=20, W=30, z=1.0):
    return np.full((H, W), z, dtype=np.float32)


def test_the_same_seed_gives_the_same_bytes():
    d = plane() + np.linspace(0, 0.5, 30, dtype=np.float32)[None, :]
    a, b, c = synthetic.sensor_depth(d, 7), synthetic.sensor_depth(d, 7), synthetic.sensor_depth(d, 8)
    assert a.dtype == np.float32 and a.shape == d.shape
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes() and a.tobytes() != d.tobytes()
    t = synthetic.sensor_depth(torch.from_numpy(d), 7)                 # a tensor in, a tensor out, the same numbers
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.numpy().tobytes() == a.tobytes()
    v = synthetic.sensor_depth(np.stack([d, d]), 7)                    # [V,H,W]
    assert v.shape == (2,) + d.shape and v[0].tobytes() != v[1].tobytes()


def test_invalid_depths_stay_zero_and_move_no_other_pixel():
    d = plane()
    h = d.copy()
    h[3, 4], h[5, 6], h[7, 8], h[9, 10], h[0, 0] = 0.0, np.nan, np.inf, -1.0, -np.inf
    bad = ~(np.isfinite(h) & (h > 0))
    a, b = synthetic.sensor_depth(d, 3), synthetic.sensor_depth(h, 3)
    assert (b[bad].view(np.uint32) == 0).all() and (b[~bad] > 0).all()
    assert a[~bad].tobytes() == b[~bad].tobytes()
    tiny = synthetic.sensor_depth(np.full((50, 50), 1e-3, dtype=np.float32), 0, a=0.0, b=1.0, z0=1.0)      # sigma ~ 1 m at 1 mm
    assert (tiny >= 0).all() and (tiny == 0).any() and (tiny > 0).any()                                     # not > 0 becomes 0


def test_the_standard_deviation_is_the_models():
    n = 100000
    d = np.full((250, 400), 2.0, dtype=np.float32)
    assert d.size == n
    for kw, sigma in ((dict(), 0.0012 + 0.0019 * (2.0 - 0.4) ** 2), (dict(a=0.0, b=0.02, z0=0.0), 0.08), (dict(scale=3.0), 3 * (0.0012 + 0.0019 * 1.6 ** 2))):
        e = synthetic.sensor_depth(d, 11, **kw).astype(np.float64) - 2.0
        s = e.std(ddof=1)
        print(f'{kw}: sample sigma {s:.6f}, model {sigma:.6f}, mean {e.mean():.2e}')
        assert abs(s - sigma) <= 0.02 * sigma
        assert abs(e.mean()) <= 5 * sigma / np.sqrt(n)


def test_quantum():
    d = plane() + np.linspace(0, 1, 30, dtype=np.float32)[None, :]
    q = 0.005
    a = synthetic.sensor_depth(d, 5, quantum=q)
    k = a.astype(np.float64) / q
    assert np.abs(k - np.round(k)).max() <= 1e-4                       # multiples of q, to float32's rounding
    assert np.abs(a - synthetic.sensor_depth(d, 5)).max() <= q / 2 + 1e-6
    assert len(np.unique(a)) < len(np.unique(synthetic.sensor_depth(d, 5)))


def test_edge_jump_leaves_holes_at_depth_edges():
    d = plane()
    d[:, 15:] = 1.5
    d[10, 3] = 0.0                                                      # an invalid neighbour is no edge
    a = synthetic.sensor_depth(d, 2, edge_jump=0.1)
    hole = a == 0
    want = np.zeros_like(hole)
    want[:, 14:16] = True
    want[10, 3] = True
    assert np.array_equal(hole, want)
    assert np.array_equal(synthetic.sensor_depth(d, 2, edge_jump=0.6) == 0, d == 0)      # the step is 0.5 m: below the jump
    assert a[~want].tobytes() == synthetic.sensor_depth(d, 2)[~want].tobytes()
