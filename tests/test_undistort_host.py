"""CPU: the host side of lens undistortion (include/adfp.h "lens undistortion").  adfp_undistort_map is host code: its map is held
entry for entry to the numpy statement of the rule (tests/undistort_ref.py) -- both are the same f64 operations in the same
order, nothing is contracted, so nothing but equality is right.  The statement's remap is held to what it must do on maps whose
result is known without it."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref
from attentive_dfprior_amd import _lib, datasets

ARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize('k', range(len(undistort_ref.GEOMETRIES)))
def test_map_equals_the_restatement_entry_for_entry(k):
    hw, fx, fy, cx, cy, dist = undistort_ref.GEOMETRIES[k]
    got = datasets.undistort_map(hw, fx, fy, cx, cy, dist)
    want = undistort_ref.undistort_map(hw, fx, fy, cx, cy, dist)
    assert got.shape == hw + (2,) and got.dtype == np.int32 and want.dtype == np.int32
    differ = int((got != want).any(axis=-1).sum())
    sentinels = int((want[..., 0] == undistort_ref.SENTINEL).sum())
    print(f'{hw} {dist}: {differ} of {hw[0] * hw[1]} entries differ; {sentinels} sentinels; iu in [{want[..., 0].min()}, {want[..., 0].max()}]')
    assert np.array_equal(got, want)
    assert ((want[..., 0] == undistort_ref.SENTINEL) == (want[..., 1] == undistort_ref.SENTINEL)).all()
    if k == 3:
        # the denominator 1 - 4 r2 crosses zero inside this image: entries far outside the image on both sides
        assert (want[..., 0] < -32).any() and (want[..., 0] > 32 * 53).any()


def test_a_zero_denominator_gives_the_sentinel():
    # pixel (0, 0) at r2 = 0.25 exactly with k4 = -4: kr = 1 / 0 = inf, U = -inf
    m = datasets.undistort_map((2, 3), 2.0, 2.0, 1.0, 0.0, [0.0, 0, 0, 0, 0, -4.0, 0, 0])
    assert np.array_equal(m, undistort_ref.undistort_map((2, 3), 2.0, 2.0, 1.0, 0.0, [0.0, 0, 0, 0, 0, -4.0, 0, 0]))
    assert tuple(m[0, 0]) == (undistort_ref.SENTINEL, undistort_ref.SENTINEL) and tuple(m[0, 1]) == (32, 0)


@pytest.mark.parametrize('n', [4, 5, 8])
def test_zero_coefficients_give_the_identity_map(n):
    for hw, fx, fy, cx, cy in (((6, 8), 30.0, 31.0, 3.5, 2.5), ((37, 53), 40.0, 41.0, 25.5, 17.5), ((480, 640), 517.3, 516.5, 318.6, 255.3)):
        m = datasets.undistort_map(hw, fx, fy, cx, cy, [0.0] * n)
        assert np.array_equal(m, undistort_ref.identity_map(hw)), hw


def test_missing_coefficients_are_zero():
    hw, fx, fy, cx, cy, dist = undistort_ref.GEOMETRIES[1]
    dist = dist[:4]
    four = datasets.undistort_map(hw, fx, fy, cx, cy, dist)
    assert np.array_equal(four, datasets.undistort_map(hw, fx, fy, cx, cy, dist + [0.0]))
    assert np.array_equal(four, datasets.undistort_map(hw, fx, fy, cx, cy, dist + [0.0] * 4))
    assert not np.array_equal(four, datasets.undistort_map(hw, fx, fy, cx, cy, dist + [0.5]))


def test_argument_errors():
    L = _lib.lib()
    dist = (C.c_double * 8)(0.1, 0, 0, 0, 0, 0, 0, 0)
    out = (C.c_int * (6 * 8 * 2))()
    out[0] = -7
    call = lambda h=6, w=8, fx=30.0, fy=31.0, cx=3.5, cy=2.5, d=dist, n=5, m=out: L.adfp_undistort_map(h, w, fx, fy, cx, cy, d, n, m)
    assert call() == 0 and out[0] != -7
    out[0] = -7
    for n in (0, 1, 3, 6, 7, 9, 12, 14, -1):
        assert call(n=n) == UNSUPPORTED, n
    assert call(d=None) == ARG and call(m=None) == ARG
    assert call(h=0) == ARG and call(w=-1) == ARG
    assert call(h=32769) == UNSUPPORTED and call(w=32769) == UNSUPPORTED
    nan, inf = float('nan'), float('inf')
    for bad in (dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=-inf)):
        assert call(**bad) == ARG, bad
    assert out[0] == -7                                   # nothing was written by a refused call
    # the device entries refuse on the host, before any launch: no GPU is needed to see it
    g = _lib.AdfpIngestGeom(6, 8, 6, 8, 0, 0, 0, 1, 0, 0, 6553.5, 1.0)
    jobs = (_lib.AdfpIngestJob * 1)(_lib.AdfpIngestJob(16, 16, 16, 16))
    assert L.adfp_ingest_frames_undistort(None, 16, 1, jobs, None) == ARG
    assert L.adfp_ingest_frames_undistort(C.byref(g), 16, -1, jobs, None) == ARG
    assert L.adfp_ingest_frames_undistort(C.byref(g), 16, 1, None, None) == ARG
    assert L.adfp_ingest_frames_undistort(C.byref(g), 20, 1, jobs, None) == ARG            # a map that is not 8-byte aligned
    assert L.adfp_ingest_frames_undistort(C.byref(g), 16, _lib.INGEST_MAX_JOBS + 1, jobs, None) == UNSUPPORTED
    assert L.adfp_ingest_frames_undistort(C.byref(g), 16, 0, None, None) == 0
    assert L.adfp_ingest_frames_undistort(C.byref(g), None, 0, None, None) == 0
    for src, m, h, w, dst, code in ((None, 16, 6, 8, 16, ARG), (16, None, 6, 8, 16, ARG), (16, 16, 6, 8, None, ARG), (16, 20, 6, 8, 16, ARG),
                                    (16, 16, 0, 8, 16, ARG), (16, 16, 6, -1, 16, ARG), (16, 16, 32769, 8, 16, UNSUPPORTED),
                                    (16, 16, 6, 32769, 16, UNSUPPORTED)):
        assert L.adfp_undistort_image(src, m, h, w, dst, None) == code, (src, m, h, w, dst)
    # Python: a bad length is a ValueError, from the map builder and from both constructors' checks
    for n in (3, 6, 12, 14):
        with pytest.raises(ValueError, match='coefficients'):
            datasets.undistort_map((6, 8), 30.0, 31.0, 3.5, 2.5, [0.1] * n)


def test_restatement_remap_on_known_maps():
    rng = np.random.RandomState(11)
    img = rng.randint(0, 256, (6, 8, 3), dtype=np.uint8)
    ident = undistort_ref.identity_map((6, 8))
    assert np.array_equal(undistort_ref.remap(img, ident), img)
    # a whole-pixel shift: the border comes back 0
    shifted = undistort_ref.remap(img, ident + np.array([32, -64], np.int32))
    assert np.array_equal(shifted[2:, :-1], img[:-2, 1:]) and not shifted[:2].any() and not shifted[:, -1].any()
    # half a pixel in x: the rounded mean of two neighbours, and half of the last column against the border
    half = undistort_ref.remap(img, ident + np.array([16, 0], np.int32)).astype(np.int64)
    wide = img.astype(np.int64)
    assert np.array_equal(half[:, :-1], (wide[:, :-1] + wide[:, 1:] + 1) >> 1) and np.array_equal(half[:, -1], (wide[:, -1] + 1) >> 1)
    # the sentinel and the clamp's ends give 0; an all-255 image stays 255 wherever four taps are inside
    far = np.full((6, 8, 2), undistort_ref.SENTINEL, np.int32)
    assert not undistort_ref.remap(img, far).any()
    far[...] = 2 ** 30
    assert not undistort_ref.remap(img, far).any()
    white = np.full((6, 8, 3), 255, np.uint8)
    inner = ident[:-1, :-1] + np.array([31, 31], np.int32)
    assert (undistort_ref.remap(white, np.pad(inner, ((0, 1), (0, 1), (0, 0))))[:-1, :-1] == 255).all()
