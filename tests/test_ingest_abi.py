"""CPU: the frame-ingestion entries of the C ABI without a GPU: argument errors come back as negative codes before any launch, the
output shape follows the host statement of the chain, and the ABI version is unchanged (the entries are additions)."""
import ctypes as C
import itertools

import ingest_ref
from attentive_dfprior_amd import _lib

ARG, UNSUPPORTED = -1, -2
DUMMY = 16                                         # never dereferenced: every launching call below fails its host-side checks first


def geom(color=(11, 13), depth=(5, 7), crop=(0, 0), edge=0, order=1, kind=0, out=0, png=6553.5, scale=1.0):
    return _lib.AdfpIngestGeom(color[0], color[1], depth[0], depth[1], crop[0], crop[1], edge, order, kind, out, png, scale)


def jobs(n, color=DUMMY, depth=DUMMY, color_out=DUMMY, depth_out=DUMMY):
    return (_lib.AdfpIngestJob * max(n, 1))(*[_lib.AdfpIngestJob(color, depth, color_out, depth_out) for _ in range(max(n, 1))])


def bad_geometries():
    nan, inf = float('nan'), float('inf')
    return [(geom(color=(0, 13)), ARG), (geom(color=(11, -1)), ARG), (geom(depth=(0, 7)), ARG), (geom(depth=(5, 0)), ARG),
            (geom(crop=(-1, 9)), ARG), (geom(crop=(6, -9)), ARG), (geom(crop=(6, 0)), ARG), (geom(crop=(0, 9)), ARG),
            (geom(edge=-1), ARG),
            (geom(edge=3), ARG), (geom(depth=(5, 6), edge=3), ARG), (geom(depth=(6, 5), edge=3), ARG),       # 2 edge >= the depth frame
            (geom(depth=(50, 70), crop=(6, 9), edge=3), ARG), (geom(depth=(50, 70), crop=(9, 6), edge=3), ARG),   # ... >= crop_size
            (geom(png=0.0), ARG), (geom(png=nan), ARG), (geom(png=inf), ARG), (geom(png=-inf), ARG),
            (geom(order=2), ARG), (geom(order=-1), ARG), (geom(kind=2), ARG), (geom(kind=-1), ARG), (geom(out=2), ARG), (geom(out=-1), ARG),
            (geom(color=(32769, 13)), UNSUPPORTED), (geom(depth=(5, 32769)), UNSUPPORTED), (geom(crop=(32769, 9)), UNSUPPORTED)]


def test_version_is_unchanged():
    assert _lib.lib().adfp_version() == 134 == _lib.ABI_VERSION


def test_ingest_argument_errors_need_no_gpu():
    L = _lib.lib()
    H, W = C.c_int(-7), C.c_int(-7)
    for g, code in bad_geometries():
        assert L.adfp_ingest_frames(C.byref(g), 1, jobs(1), None) == code
        assert L.adfp_ingest_out_shape(C.byref(g), C.byref(H), C.byref(W)) == code
        assert (H.value, W.value) == (-7, -7)
    g = geom()
    assert L.adfp_ingest_frames(None, 1, jobs(1), None) == ARG
    assert L.adfp_ingest_frames(C.byref(g), 1, None, None) == ARG
    assert L.adfp_ingest_frames(C.byref(g), -1, jobs(1), None) == ARG
    for field in ('color', 'depth', 'color_out', 'depth_out'):
        assert L.adfp_ingest_frames(C.byref(g), 1, jobs(1, **{field: None}), None) == ARG
        js = jobs(3)
        setattr(js[2], field, None)                  # a later job's pointer is checked too
        assert L.adfp_ingest_frames(C.byref(g), 3, js, None) == ARG
    assert _lib.INGEST_MAX_JOBS == 16
    assert L.adfp_ingest_frames(C.byref(g), _lib.INGEST_MAX_JOBS + 1, jobs(_lib.INGEST_MAX_JOBS + 1), None) == UNSUPPORTED
    assert L.adfp_ingest_out_shape(None, C.byref(H), C.byref(W)) == ARG
    assert L.adfp_ingest_out_shape(C.byref(g), None, C.byref(W)) == ARG
    assert L.adfp_ingest_out_shape(C.byref(g), C.byref(H), None) == ARG


def test_no_jobs_launch_nothing():
    L = _lib.lib()
    assert L.adfp_ingest_frames(C.byref(geom()), 0, None, None) == 0
    assert L.adfp_ingest_frames(C.byref(geom()), 0, jobs(1), None) == 0
    assert L.adfp_ingest_frames(C.byref(geom(png=0.0)), 0, None, None) == ARG       # the geometry is checked first


def test_out_shape_follows_the_host_chain():
    L = _lib.lib()
    H, W = C.c_int(), C.c_int()
    n = 0
    for color, depth, crop, edge in itertools.product([(11, 13), (5, 7), (968, 1296)], [(5, 7), (480, 640), (1, 70)],
                                                      [(0, 0), (6, 9), (384, 512), (3, 4)], [0, 1, 10]):
        h, w = crop if crop[0] else depth
        if 2 * edge >= h or 2 * edge >= w:
            continue
        assert L.adfp_ingest_out_shape(C.byref(geom(color=color, depth=depth, crop=crop, edge=edge)), C.byref(H), C.byref(W)) == 0
        assert (H.value, W.value) == ingest_ref.out_shape(depth, crop if crop[0] else None, edge), (color, depth, crop, edge)
        n += 1
    assert n >= 60
    assert L.adfp_ingest_out_shape(C.byref(geom(color=(968, 1296), depth=(480, 640), edge=10)), C.byref(H), C.byref(W)) == 0
    assert (H.value, W.value) == (460, 620)          # ScanNet's frame
