"""Plain numpy restatements of the ray-order kernels (adfp_ray_sort_keys, adfp_ray_order_probe; include/adfp.h) and of the
sharded render's gather (adfp_gather_pack / adfp_gather_unpack), plus the fixed-seed inputs the GPU tests feed the kernels.
No import of the library: tests/test_ray_order_host.py pins these statements and the conditions on the inputs on the CPU,
tests/test_gpu_ray_order.py and tests/test_gpu_gather_rows.py hold the kernels to them.

The sort key of a ray
    t   = gt_depth, or 1 where gt_depth is not (> 0 and < 3e38) (0, negatives, +-inf, NaN) or where there is no gt_depth
    p   = o + d t                                                  (float64 here; the inputs are the kernel's float32 values)
    u   = (x - lo) / (hi - lo) per axis of tsdf_bnds
    origin cell  = clamp(floor(4 u(o)), 0, 3), surface cell = clamp(floor(256 u(p)), 0, 255), NaN -> 0
    key = morton(origin cell, 2 bits) << 24 | morton(surface cell, 8 bits),   x -> bit 3b, y -> bit 3b+1, z -> bit 3b+2

Which rays the float32 kernel may legitimately put into the neighbouring cell (`ambiguous`).  The kernel evaluates
    p = fmaf(d, t, o);  s = ((p - (float)lo) * (float)(1 / (hi - lo))) * cells
With eps = 2^-24 (half an ulp, relative) the absolute error of s against the float64 statement is bounded by
    fmaf's one rounding                 eps |p|
    lo rounded to float32               eps |lo|
    the subtraction's rounding          eps |p - lo|
  all three scaled by cells / (hi - lo), and
    the reciprocal's rounding to float32 and the product's rounding      2 eps |s|
  (the last multiplication, by 4 or 256, is exact), i.e.
    |ds| <= eps * cells * ((|p| + |lo| + |p - lo|) / (hi - lo) + 2 |u|).
rounding_half_width() evaluates that.  For the key cases below (|p|, |lo| <= 6 m, extents >= 3.1 m, |u| <= 1 inside the
clamp range) it is 256 * 6e-8 * (14 / 3.1 + 2) = 1.0e-4 surface cells and 1.6e-6 origin cells.  The statement uses the
wider HW_SURFACE = 1e-3 and HW_ORIGIN = 1e-4 cells (the host test asserts they cover the derived bound): a ray is
ambiguous when a scaled coordinate lies within that half-width of one of the integers 1 .. cells-1.  (0 and `cells`
separate nothing: both sides of them clamp to the same cell.)  On such a ray the kernel's key must be one of
candidate_keys(): the statement with every coordinate nudged by - and + the half-width.
"""
import itertools
import math

import numpy as np

ORIGIN_BITS, SURFACE_BITS = 2, 8
KEY_BITS = 3 * ORIGIN_BITS + 24                 # what Renderer._coherent_order hands the radix sort
HW_ORIGIN, HW_SURFACE = 1e-4, 1e-3              # half-widths of the ambiguity band, in cells
PROBE_PAIRS = 2048
EPS32 = 2.0 ** -24


# ================================================================================================== the statements
def morton(cx, cy, cz, bits):
    cx, cy, cz = (np.asarray(v, dtype=np.int64) for v in (cx, cy, cz))
    k = np.zeros(np.broadcast(cx, cy, cz).shape, dtype=np.int64)
    for b in range(bits):
        k = k + (((cx >> b) % 2) << (3 * b))
        k = k + (((cy >> b) % 2) << (3 * b + 1))
        k = k + (((cz >> b) % 2) << (3 * b + 2))
    return k


def ray_t(gd, n):
    """The ray parameter of the surface point, float64 [n]."""
    if gd is None:
        return np.ones(n)
    g = np.asarray(gd, dtype=np.float32).reshape(-1).astype(np.float64)
    with np.errstate(invalid='ignore'):
        ok = (g > 0) & (g < 3e38)
    return np.where(ok, g, 1.0)


def surface_points(ro, rd, gd):
    ro, rd = np.asarray(ro, np.float32).astype(np.float64), np.asarray(rd, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return ro + rd * ray_t(gd, ro.shape[0])[:, None]


def _scaled(x, bnds, cells):
    b = np.asarray(bnds, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return (x - b[:, 0]) / (b[:, 1] - b[:, 0]) * cells


def _cells(s, cells):
    """clamp(floor(s), 0, cells - 1), NaN -> 0."""
    with np.errstate(invalid='ignore'):
        c = np.clip(np.floor(np.where(np.isnan(s), 0.0, s)), 0, cells - 1)
    return c.astype(np.int64)


def _near_a_cell_face(s, cells, hw):
    with np.errstate(invalid='ignore'):
        r = np.rint(s)
        return np.isfinite(s) & (r >= 1) & (r <= cells - 1) & (np.abs(s - r) < hw)


def _key(co, cs):
    return (morton(co[:, 0], co[:, 1], co[:, 2], ORIGIN_BITS) << 24) | morton(cs[:, 0], cs[:, 1], cs[:, 2], SURFACE_BITS)


def ray_cells(ro, rd, gd, tsdf_bnds):
    """(origin cell [n,3], surface cell [n,3]) of the statement."""
    o = np.asarray(ro, np.float32).astype(np.float64)
    so, ss = _scaled(o, tsdf_bnds, 4), _scaled(surface_points(ro, rd, gd), tsdf_bnds, 256)
    return _cells(so, 4), _cells(ss, 256)


def sort_keys(ro, rd, gd, tsdf_bnds):
    """(key int64 [n], ambiguous bool [n])."""
    o = np.asarray(ro, np.float32).astype(np.float64)
    so, ss = _scaled(o, tsdf_bnds, 4), _scaled(surface_points(ro, rd, gd), tsdf_bnds, 256)
    amb = _near_a_cell_face(so, 4, HW_ORIGIN).any(axis=1) | _near_a_cell_face(ss, 256, HW_SURFACE).any(axis=1)
    return _key(_cells(so, 4), _cells(ss, 256)), amb


def candidate_keys(ro, rd, gd, tsdf_bnds):
    """[64, n]: the keys with each of the six scaled coordinates nudged by - or + its half-width.  All 64 rows agree on a ray
    that is not ambiguous."""
    o = np.asarray(ro, np.float32).astype(np.float64)
    so, ss = _scaled(o, tsdf_bnds, 4), _scaled(surface_points(ro, rd, gd), tsdf_bnds, 256)
    out = []
    for signs in itertools.product((-1.0, 1.0), repeat=6):
        sg = np.asarray(signs)
        out.append(_key(_cells(so + sg[:3] * HW_ORIGIN, 4), _cells(ss + sg[3:] * HW_SURFACE, 256)))
    return np.stack(out)


def rounding_half_width(ro, rd, gd, tsdf_bnds):
    """(origin, surface): the largest float32 rounding error, in cells, of the kernel's scaled coordinates over the coordinates
    of this batch that lie inside the clamp range (the bound derived in the module's docstring)."""
    b = np.asarray(tsdf_bnds, dtype=np.float64)
    lo, ext = b[:, 0], b[:, 1] - b[:, 0]
    res = []
    for x, cells, fma in ((np.asarray(ro, np.float32).astype(np.float64), 4, 0.0), (surface_points(ro, rd, gd), 256, 1.0)):
        with np.errstate(invalid='ignore', over='ignore'):
            u = (x - lo) / ext
            inside = np.isfinite(u) & (u > -0.01) & (u < 1.01)
            err = EPS32 * cells * ((fma * np.abs(x) + np.abs(lo) + np.abs(x - lo)) / ext + 2 * np.abs(u))
        res.append(float(err[inside].max()) if inside.any() else 0.0)
    return tuple(res)


def order_verdict(ro, rd, gd, far_distance):
    """(far, pairs, min_rel_margin) of adfp_ray_order_probe's sample of consecutive-ray pairs."""
    n = np.asarray(ro).shape[0]
    pairs = min(n - 1, PROBE_PAIRS)
    if pairs <= 0:
        return 0, max(pairs, 0), math.inf
    stride = (n - 1) // pairs
    p = surface_points(ro, rd, gd)
    i = np.arange(pairs) * stride
    dist = np.sqrt(((p[i + 1] - p[i]) ** 2).sum(axis=1))
    return int((dist > far_distance).sum()), pairs, float(np.abs(dist / far_distance - 1.0).min())


def gather_ref(per_rank_arrays):
    """per_rank_arrays[r][a]: rank r's rows of array a -> the gathered arrays (rank after rank)."""
    n_arrays = len(per_rank_arrays[0])
    return [np.concatenate([rank[a] for rank in per_rank_arrays], axis=0) for a in range(n_arrays)]


# ================================================================================================== shared inputs: cameras
def camera(center, yaw, pitch, roll=0.0):
    """camera-to-world [4,4] float32: looks along -z, y up; a general rotation for non-zero yaw, pitch and roll."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    m = np.eye(4)
    m[:3, :3] = Ry @ Rx @ Rz
    m[:3, 3] = center
    return m.astype(np.float32)


def get_rays(H, W, fx, fy, cx, cy, c2w):
    """(rays_o, rays_d) [H W, 3] float32 in pixel order (row-major)."""
    f = np.float32
    j, i = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing='ij')
    dirs = np.stack([(i - f(cx)) / f(fx), -(j - f(cy)) / f(fy), -np.ones_like(i)], -1).reshape(-1, 3)
    rot = np.asarray(c2w, dtype=f)[:3, :3]
    rd = (dirs[:, None, :] * rot[None]).sum(-1).astype(f)
    ro = np.broadcast_to(np.asarray(c2w, dtype=f)[:3, 3], rd.shape).copy()
    return ro, rd


def box_depth(ro, rd, lo_in, hi_in):
    """Sensor depth (= ray parameter: the camera-frame direction has z = -1) of the first wall hit from inside a box room."""
    o, d = ro.astype(np.float64), rd.astype(np.float64)
    with np.errstate(divide='ignore'):
        t = np.maximum((np.asarray(lo_in, np.float64) - o) / d, (np.asarray(hi_in, np.float64) - o) / d)
    return t.min(axis=-1).astype(np.float32)


# ================================================================================================== adfp_ray_sort_keys
KEY_BNDS = np.array([[-1.3, 2.9], [0.4, 3.7], [-2.2, 0.9]])          # unequal extents (4.2, 3.3, 3.1 m), lo != 0
KEY_SIZES = (1, 255, 256, 257, 5000)


def key_case(n):
    """n random rays: origins inside and up to 10 % of the extent outside KEY_BNDS, unit directions, depths 0.3 .. 3 m."""
    g = np.random.default_rng(1000 + n)
    lo, ext = KEY_BNDS[:, 0], KEY_BNDS[:, 1] - KEY_BNDS[:, 0]
    ro = (lo + ext * (g.random((n, 3)) * 1.2 - 0.1)).astype(np.float32)
    d = g.normal(size=(n, 3))
    rd = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    gd = (0.3 + 2.7 * g.random(n)).astype(np.float32)
    return ro, rd, gd


def shuffled_key_case(n=4099):
    """Rays of few distinct cells in a shuffled order: many equal keys, so the sort's stability is visible."""
    ro, rd, gd = key_case(n)
    ro, rd, gd = np.repeat(ro[::16], 16, axis=0)[:n], np.repeat(rd[::16], 16, axis=0)[:n], np.repeat(gd[::16], 16)[:n]
    perm = np.random.default_rng(7).permutation(n)
    return np.ascontiguousarray(ro[perm]), np.ascontiguousarray(rd[perm]), np.ascontiguousarray(gd[perm])


_BASE_O, _BASE_D = (0.75, 2.0, -0.5), (0.5, -0.25, 0.125)            # binary fractions: o + d and o + 2 d are exact
_BASE_CO, _BASE_CS1, _BASE_CS2 = (1, 1, 2), (155, 104, 150), (185, 85, 161)


def planted_rows():
    """Rows with hand-stated cells, none of them ambiguous.
    -> ro, rd, gd [m] float32, origin cells [m,3], surface cells [m,3], surface cells with gt_depth = NULL [m,3], names."""
    rows = []

    def add(name, o, d, gd, co, cs, cs_null=None):
        rows.append((name, o, d, gd, co, cs, cs if cs_null is None else cs_null))
    add('depth 1', _BASE_O, _BASE_D, 1.0, _BASE_CO, _BASE_CS1)
    add('depth 2', _BASE_O, _BASE_D, 2.0, _BASE_CO, _BASE_CS2, _BASE_CS1)
    for name, v in (('0', 0.0), ('-1', -1.0), ('+inf', np.inf), ('-inf', -np.inf), ('NaN', np.nan), ('3.5e38', 3.5e38), ('3.2e38', 3.2e38)):
        add(f'depth {name} acts as 1', _BASE_O, _BASE_D, v, _BASE_CO, _BASE_CS1)
    lo, hi = KEY_BNDS[:, 0], KEY_BNDS[:, 1]
    for a in range(3):
        for side, far_o, far_d, c4, c256 in (('below', lo[a] - 50.0, -1e6, 0, 0), ('above', hi[a] + 50.0, 1e6, 3, 255)):
            o, co, cs = list(_BASE_O), list(_BASE_CO), list(_BASE_CS2)
            o[a], co[a], cs[a] = far_o, c4, c256
            cs1 = list(_BASE_CS1)
            cs1[a] = c256
            add(f'origin far {side} on axis {a}', o, _BASE_D, 2.0, co, cs, cs1)
            d, cs = list(_BASE_D), list(_BASE_CS2)
            d[a], cs[a] = far_d, c256
            add(f'surface far {side} on axis {a}', _BASE_O, d, 2.0, _BASE_CO, cs, cs1)
    add('NaN origin x', (np.nan, 2.0, -0.5), _BASE_D, 1.0, (0, 1, 2), (0, 104, 150))
    add('NaN direction y', _BASE_O, (0.5, np.nan, 0.125), 1.0, _BASE_CO, (155, 0, 150))
    on_lo = tuple(float(np.float32(v)) for v in lo)
    add('origin on lo, direction 0', on_lo, (0.0, 0.0, 0.0), 1.0, (0, 0, 0), (0, 0, 0))
    add('origin on lo', on_lo, _BASE_D, 1.0, (0, 0, 0), (30, 0, 10))
    with np.errstate(over='ignore'):
        ro = np.array([r[1] for r in rows], dtype=np.float32)
        rd = np.array([r[2] for r in rows], dtype=np.float32)
        gd = np.array([r[3] for r in rows], dtype=np.float64).astype(np.float32)
    cells = [np.array([r[k] for r in rows], dtype=np.int64) for k in (4, 5, 6)]
    return ro, rd, gd, cells[0], cells[1], cells[2], [r[0] for r in rows]


def planted_keys(co, cs):
    return _key(np.asarray(co), np.asarray(cs))


# ================================================================================================== adfp_ray_order_probe
PROBE_FAR = 0.125                                                      # 8 voxels of 1/64 m
PROBE_ROOM = (np.array([-2.0, -1.5, -1.2]), np.array([2.0, 1.5, 1.2]))
PROBE_CAM = dict(H=320, W=320, fx=300.0, fy=280.0, cx=158.3, cy=161.7)
PROBE_SIZES = (2, 3, 257, 2049, 2050, 4097, 6151, 100003)
# name -> (n, which rays come from the other pose, depth variant)
PROBE_CASES = {}
for _n in PROBE_SIZES:
    PROBE_CASES[f'{_n}-mixed'] = (_n, 0.5, 'depth')
    PROBE_CASES[f'{_n}-mixed-null'] = (_n, 0.5, 'null')
    PROBE_CASES[f'{_n}-mixed-invalid'] = (_n, 0.5, 'invalid')
PROBE_CASES.update({
    '2-coherent': (2, 0.0, 'depth'), '2-jump': (2, 'odd', 'depth'), '3-jump': (3, 'odd', 'depth'),
    '257-coherent': (257, 0.0, 'depth'), '257-alternating': (257, 'odd', 'depth'),
    '2049-coherent': (2049, 0.0, 'depth'), '4097-alternating': (4097, 'odd', 'depth'), '100003-alternating': (100003, 'odd', 'null'),
})
_frames = {}


def _probe_frames():
    if not _frames:
        for name, c2w in (('a', camera((0.2, -0.1, 0.1), 0.4, -0.2, 0.1)), ('b', camera((-0.5, 0.4, -0.2), 0.4 + math.pi, 0.15, -0.2))):
            ro, rd = get_rays(c2w=c2w, **PROBE_CAM)
            _frames[name] = (ro, rd, box_depth(ro, rd, *PROBE_ROOM))
    return _frames


def probe_case(name):
    """-> ro, rd [n,3] float32, gd [n] float32 or None.  Consecutive pixels of frame a (a smooth depth: the walls of a box room);
    the rays named by the case's rule are those of the same pixels of frame b, a camera that looks the other way."""
    n, swap, variant = PROBE_CASES[name]
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    g = np.random.default_rng(seed)
    fa, fb = _probe_frames()['a'], _probe_frames()['b']
    mask = (np.arange(n) % 2 == 1) if swap == 'odd' else g.random(n) < swap
    ro, rd, gd = (np.where(mask.reshape((n,) + (1,) * (x.ndim - 1)), y[:n], x[:n]) for x, y in zip(fa, fb))
    if variant == 'null':
        return np.ascontiguousarray(ro), np.ascontiguousarray(rd), None
    if variant == 'invalid':
        pairs = min(n - 1, PROBE_PAIRS)
        stride = (n - 1) // pairs
        k = g.choice(pairs, size=max(1, pairs // 8), replace=False)
        idx = k * stride + g.integers(0, 2, size=k.shape[0])
        gd = gd.copy()
        gd[idx] = np.array([0.0, -1.0, np.inf, np.nan], dtype=np.float32)[g.integers(0, 4, size=k.shape[0])]
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), np.ascontiguousarray(gd)


# ================================================================================================== the Renderer-level batch
RENDER_N = 4099
RENDER_CAM = dict(H=60, W=72, fx=40.0, fy=42.0, cx=35.3, cy=29.6)


def render_batch(center, lo_in, hi_in):
    """RENDER_N rays in pixel order -- the first 2050 pixels of one frame of a camera at `center` of a box room, then the first 2049
    of a second camera that looks the other way (one jump in 4098 pairs) -- and a fixed permutation of them:
    -> (ro, rd, gd) float32, perm int64."""
    parts = []
    for (yaw, pitch, roll), cnt in (((0.5, -0.15, 0.05), 2050), ((0.5 + math.pi, 0.1, -0.05), RENDER_N - 2050)):
        ro, rd = get_rays(c2w=camera(center, yaw, pitch, roll), **RENDER_CAM)
        parts.append((ro[:cnt], rd[:cnt], box_depth(ro, rd, lo_in, hi_in)[:cnt]))
    batch = tuple(np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(3))
    return batch, np.random.default_rng(11).permutation(RENDER_N)


# ================================================================================================== gather cases
GATHER_WORLDS = {
    'w1': (33,), 'w3': (5, 0, 2), 'w4': (0, 0, 1, 0), 'w5': (257, 256, 255, 1, 300),
    'w64': tuple(int(v) for v in np.where(np.arange(64) % 7 == 3, 0, np.random.default_rng(64).integers(0, 41, size=64))),
    'big': (7600, 7421, 7600, 7379),
}
# name -> [(dtype, elements per row)]: widths in 4-byte words in the comment
GATHER_LAYOUTS = {
    'render': [('float64', 1), ('float64', 1), ('float32', 3)],                                             # 2 + 2 + 3 = 7
    'one-word': [('int32', 1)],
    'eight': [('int32', 1), ('float64', 1), ('float32', 3), ('int64', 2), ('int32', 5), ('float64', 3), ('float32', 7), ('int32', 9)],   # 1 2 3 4 5 6 7 9
}


def gather_inputs(sizes, layout):
    """per_rank[r][a]: [sizes[r], elements] arrays whose every 4-byte word is distinct over arrays, ranks, rows and words
    (a counter with the array in the top bits), so a misrouted word shows."""
    per_rank = []
    row0 = 0
    for rows in sizes:
        arrs = []
        for a, (dt, el) in enumerate(layout):
            words = el * np.dtype(dt).itemsize // 4
            w = ((a + 1) << 26) + (row0 + np.arange(rows, dtype=np.int64))[:, None] * 16 + np.arange(words, dtype=np.int64)[None, :]
            arrs.append(np.ascontiguousarray(w.astype(np.int32)).view(dt).reshape(rows, el))
        per_rank.append(arrs)
        row0 += rows
    return per_rank
