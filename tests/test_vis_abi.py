"""CPU: the visualisation entries of the C ABI without a GPU: argument errors come back as their codes before any launch (null
stream, dummy pointers), the canvas shape follows the host statement of the layout, and the ABI version is unchanged (the entries
are additions)."""
import ctypes as C
import itertools

import vis_ref
from attentive_dfprior_amd import _lib

ARG, UNSUPPORTED = -1, -2
DUMMY = 4096                                       # never dereferenced: every call below fails its host-side checks first


def geom(H=37, W=53, stride=1, gap=8, f64=0):
    return _lib.AdfpVisGeom(H, W, stride, gap, f64)


def panels(g, gt_depth=DUMMY, gt_color=DUMMY, depth=DUMMY, color=DUMMY, canvas=DUMMY, stats=DUMMY, workspace=DUMMY, nbytes=None):
    L = _lib.lib()
    if nbytes is None:
        nbytes = L.adfp_vis_workspace_bytes(C.byref(g)) if g is not None else 1 << 20
    return L.adfp_vis_panels(C.byref(g) if g is not None else None, gt_depth, gt_color, depth, color, canvas, stats, workspace, nbytes, None)


BAD = [(geom(H=0), ARG), (geom(H=-3), ARG), (geom(W=0), ARG), (geom(stride=0), ARG), (geom(stride=-1), ARG), (geom(gap=-1), ARG),
       (geom(f64=2), ARG), (geom(f64=-1), ARG),
       (geom(H=32769), UNSUPPORTED), (geom(W=32769), UNSUPPORTED), (geom(gap=32769), UNSUPPORTED)]


def test_version_is_unchanged():
    assert _lib.lib().adfp_version() == 134 == _lib.ABI_VERSION


def test_vis_argument_errors_need_no_gpu():
    L = _lib.lib()
    rows, cols = C.c_int(-7), C.c_int(-7)
    for g, code in BAD:
        assert panels(g, nbytes=1 << 20) == code
        assert L.adfp_vis_canvas_shape(C.byref(g), C.byref(rows), C.byref(cols)) == code
        assert (rows.value, cols.value) == (-7, -7)
        assert L.adfp_vis_workspace_bytes(C.byref(g)) == 0
    assert panels(None) == ARG
    assert L.adfp_vis_canvas_shape(None, C.byref(rows), C.byref(cols)) == ARG
    assert L.adfp_vis_workspace_bytes(None) == 0
    g = geom()
    assert L.adfp_vis_canvas_shape(C.byref(g), None, C.byref(cols)) == ARG
    assert L.adfp_vis_canvas_shape(C.byref(g), C.byref(rows), None) == ARG
    for field in ('gt_depth', 'gt_color', 'depth', 'color', 'canvas', 'stats', 'workspace'):
        assert panels(g, **{field: None}) == ARG, field
    need = L.adfp_vis_workspace_bytes(C.byref(g))
    assert need >= 6 * 8 and need % 256 == 0
    assert panels(g, nbytes=need - 1) == ARG and panels(g, nbytes=0) == ARG            # a workspace that is too small
    assert panels(g, workspace=DUMMY + 4) == ARG                                        # ... or not aligned for doubles
    big = geom(H=32768, W=32768)
    assert L.adfp_vis_workspace_bytes(C.byref(big)) == 1024 * 6 * 8                     # the partials stop growing at 1024 workgroups
    assert panels(big, gt_depth=None) == ARG                                            # the largest frame is a geometry like any other
    assert _lib.VIS_STATS == 6


def test_canvas_shape_follows_the_host_layout():
    L = _lib.lib()
    rows, cols = C.c_int(), C.c_int()
    n = 0
    for H, W, stride, gap in itertools.product((1, 37, 680), (1, 37, 680), (1, 3, 7), (0, 5)):
        assert L.adfp_vis_canvas_shape(C.byref(geom(H, W, stride, gap)), C.byref(rows), C.byref(cols)) == 0
        assert (rows.value, cols.value) == vis_ref.canvas_shape(H, W, stride, gap), (H, W, stride, gap)
        n += 1
    assert n == 54
    assert L.adfp_vis_canvas_shape(C.byref(geom(680, 1200, 1, 8)), C.byref(rows), C.byref(cols)) == 0
    assert (rows.value, cols.value) == (2 * 680 + 24, 3 * 1200 + 32)                    # Replica's frame
    assert L.adfp_vis_canvas_shape(C.byref(geom(37, 53, 40000, 0)), C.byref(rows), C.byref(cols)) == 0
    assert (rows.value, cols.value) == (2, 3)                                           # a stride beyond the frame: one pixel per panel
