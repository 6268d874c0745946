"""CPU: the depth bilateral filter's rule as tests/depth_filter_ref.py restates it, and what it buys the depth ICP's restatement
(tests/icp_ref.py) on a noisy sensor.

The tally: six of the mini scene's nine cases (two guesses of each pose), six noise seeds each, the sensor depth the TSDF raycast at
the true pose plus N(0, (0.02 z^2)^2), the default levels and gates, the filter's defaults on the sensor image only.  Its four
conditions compare two runs of the restatement; the device tests lean on them only because they hold here."""
import numpy as np
import pytest

import depth_filter_ref as F
import icp_ref as R
from attentive_dfprior_amd import synthetic


def holes_image(H=12, W=15, seed=0):
    rng = np.random.default_rng(seed)
    d = (0.5 + rng.random((H, W))).astype(np.float32)
    d[2, 3], d[5, 5], d[0, 0], d[H - 1, W - 1] = 0.0, np.nan, np.inf, -1.0
    d[7, 8:11] = 0.0
    d[3, 9], d[9, 2] = -np.inf, -0.0
    return d


def test_validity_pattern_is_preserved():
    d = holes_image()
    ok = R.depth_ok(d)
    assert 0 < (~ok).sum() < ok.size
    for kw in (dict(), dict(radius=1, sigma_depth=0.01), dict(radius=8, sigma_depth_z2=0.02)):
        out = F.bilateral(d, **kw)
        assert out.dtype == np.float32 and out.shape == d.shape
        assert np.array_equal(R.depth_ok(out), ok)
        assert (out[~ok].view(np.uint32) == 0).all()                  # +0.0, not -0.0, not NaN
        assert (out[ok] >= d[ok].min()).all() and (out[ok] <= d[ok].max()).all()      # a weighted mean of valid depths


def step_image(H=9, W=14):
    rng = np.random.default_rng(1)
    d = (1.0 + 0.004 * rng.standard_normal((H, W))).astype(np.float32)
    d[:, W // 2:] += np.float32(0.5)
    return d, np.arange(W)[None, :].repeat(H, 0) < W // 2


def test_a_step_edge_separates_the_two_sides():
    """|d_q - d_p| > 3 s_p keeps the far side out entirely: the bytes are those of filtering one side alone"""
    d, near = step_image()
    kw = dict(radius=3, sigma_space=2.0, sigma_depth=0.03)
    out = F.bilateral(d, **kw)
    a = F.bilateral(np.where(near, d, np.float32(0)), **kw)
    b = F.bilateral(np.where(near, np.float32(0), d), **kw)
    assert out[near].tobytes() == a[near].tobytes() and out[~near].tobytes() == b[~near].tobytes()
    assert (a[~near] == 0).all() and (b[near] == 0).all()
    wide = F.bilateral(d, radius=3, sigma_space=2.0, sigma_depth=0.3)         # 3 s_p = 0.9 m: the sides mix
    assert wide[near].tobytes() != a[near].tobytes()


def test_a_window_larger_than_the_image_is_clipped():
    rng = np.random.default_rng(2)
    d = (0.8 + 0.01 * rng.random((5, 3))).astype(np.float32)
    out = F.bilateral(d, radius=8, sigma_space=3.0, sigma_depth=0.05)
    # the same sums written out pixel by pixel, scalar by scalar
    a, b = 1.0 / ((2.0 * 3.0) * 3.0), 1.0 / ((2.0 * 0.05) * 0.05)
    for v in range(5):
        for u in range(3):
            num = den = 0.0
            for y in range(5):
                for x in range(3):
                    e = float(d[y, x]) - float(d[v, u])
                    w = float(np.exp(-(float((x - u) ** 2 + (y - v) ** 2) * a + (e * e) * b)))
                    num, den = num + w * float(d[y, x]), den + w
            assert np.float32(num / den) == out[v, u], (v, u)


def test_a_constant_image_comes_back():
    for c in (0.3, 1.0, 2.718, 7.5):
        d = np.full((7, 9), c, dtype=np.float32)
        out = F.bilateral(d, radius=2)
        assert (np.abs(out.astype(np.float64) - d) <= np.spacing(d)).all(), c


@pytest.fixture(scope='module')
def world():
    sc = synthetic.mini_scene()
    cases = R.scene_cases(sc)
    sensor, trials = {}, []
    for ci in F.TALLY_CASES:
        P, G = cases[ci]
        key = P.tobytes()
        if key not in sensor:
            sensor[key] = R.cpu_raycast(sc, P)
        dm = R.cpu_raycast(sc, G)
        for k in range(F.TALLY_SEEDS):
            trials.append((P, G, F.noisy(sensor[key], F.tally_seed(ci, k)), dm))
    clean = [(cases[ci][0], cases[ci][1], sensor[cases[ci][0].tobytes()], trials[F.TALLY_SEEDS * n][3]) for n, ci in enumerate(F.TALLY_CASES)]
    return sc, trials, clean


def intr(sc):
    return sc.fx, sc.fy, sc.cx, sc.cy


def test_the_noise_tally(world):
    sc, trials, _ = world
    assert len(trials) == 36
    t = F.tally(trials, intr(sc))
    print(F.tally_line('raw     ', t['raw']))
    print(F.tally_line('filtered', t['filtered']))
    print(f"filtered last step has more pairs in {t['more_pairs']} of {t['trials']} trials, smallest ratio {t['smallest_pair_ratio']:.2f}")
    assert t['filtered']['ok'] == 36
    assert t['more_pairs'] == 36
    assert t['filtered']['rot_le_half'] > t['raw']['rot_le_half']
    assert t['filtered']['worst_trans_ratio'] <= 0.5


def test_the_cost_on_clean_depth_is_printed(world):
    """An observation, not a bar: on clean depth at 48 x 64 the filter rounds the room's corners."""
    sc, _, clean = world
    for name, points in (('points True', True), ('points False', False)):
        t = F.tally(clean, intr(sc), points=points)
        raw = [r['raw'][0] * 1e3 for r in t['records']]
        fil = [r['filtered'][0] * 1e3 for r in t['records']]
        print(f'clean depth, {name}: raw ends {min(raw):.2f}-{max(raw):.2f} mm from the true pose, filtered {min(fil):.2f}-{max(fil):.2f} mm')
