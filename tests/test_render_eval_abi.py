"""CPU: the rendering-metrics entries of the C ABI without a GPU: argument errors come back as their codes before any launch (null
stream, dummy pointers), the window counts follow the host statement (tests/render_ref.py), and the ABI version is unchanged (the
entries are additions)."""
import ctypes as C
import itertools

import render_ref
from attentive_dfprior_amd import _lib, render_eval

ARG, UNSUPPORTED = -1, -2
DUMMY = 4096                                       # never dereferenced: every call below fails its host-side checks first


def geom(H=47, W=53, levels=3, f64=0):
    return _lib.AdfpMetricsGeom(H, W, levels, f64)


def metrics(g, gt_depth=DUMMY, gt_color=DUMMY, depth=DUMMY, color=DUMMY, row=DUMMY, workspace=DUMMY, nbytes=None):
    L = _lib.lib()
    if nbytes is None:
        nbytes = L.adfp_frame_metrics_workspace_bytes(C.byref(g)) if g is not None else 1 << 20
    return L.adfp_frame_metrics(C.byref(g) if g is not None else None, gt_depth, gt_color, depth, color, row, workspace, nbytes, None)


BAD = [(geom(H=0), ARG), (geom(H=-3), ARG), (geom(W=0), ARG), (geom(levels=-1), ARG), (geom(levels=6), ARG), (geom(f64=2), ARG),
       (geom(f64=-1), ARG),
       (geom(H=10, levels=1), ARG), (geom(W=10, levels=1), ARG),              # level 0 smaller than the window
       (geom(levels=4), ARG), (geom(H=21, W=400, levels=3), ARG),             # 47 -> 24 -> 12 -> 6; 21 -> 11 -> 6
       (geom(H=160, W=176, levels=5), ARG), (geom(H=176, W=159, levels=5), ARG),         # 160 -> 80 -> 40 -> 20 -> 10
       (geom(H=32769), UNSUPPORTED), (geom(W=32769), UNSUPPORTED), (geom(H=32769, levels=0), UNSUPPORTED)]


def test_version_is_unchanged():
    assert _lib.lib().adfp_version() == 134 == _lib.ABI_VERSION
    assert _lib.FRAME_METRICS == 35 == render_ref.N_ROW


def test_metrics_argument_errors_need_no_gpu():
    L = _lib.lib()
    win = (C.c_longlong * 5)(*([-7] * 5))
    for g, code in BAD:
        assert metrics(g, nbytes=1 << 30) == code, (g.H, g.W, g.levels, g.gt_color_f64)
        assert L.adfp_frame_metrics_windows(C.byref(g), win) == code
        assert list(win) == [-7] * 5
        assert L.adfp_frame_metrics_workspace_bytes(C.byref(g)) == 0
    assert metrics(None) == ARG
    assert L.adfp_frame_metrics_windows(None, win) == ARG
    assert L.adfp_frame_metrics_workspace_bytes(None) == 0
    for g in (geom(), geom(levels=0), geom(H=5, W=3, levels=0), geom(H=680, W=1200, levels=5, f64=1), geom(H=32768, W=32768, levels=5)):
        need = L.adfp_frame_metrics_workspace_bytes(C.byref(g))
        assert need > 0 and need % 8 == 0
        assert L.adfp_frame_metrics_windows(C.byref(g), None) == ARG
        for field in ('gt_depth', 'gt_color', 'depth', 'color', 'row', 'workspace'):
            assert metrics(g, **{field: None}) == ARG, field
        assert metrics(g, nbytes=need - 1) == ARG and metrics(g, nbytes=0) == ARG      # a workspace that is too small
        assert metrics(g, workspace=DUMMY + 4) == ARG                                  # ... or not aligned for doubles
        assert metrics(g, row=DUMMY + 4) == ARG and metrics(g, row=DUMMY + 1) == ARG
    # the workspace holds the pooled levels: more levels, more bytes
    sizes = [L.adfp_frame_metrics_workspace_bytes(C.byref(geom(680, 1200, k))) for k in range(6)]
    assert sizes == sorted(sizes) and sizes[5] > sizes[1] + 2 * 3 * 8 * 340 * 600


def test_windows_follow_the_host_statement():
    L = _lib.lib()
    win = (C.c_longlong * 5)()
    sides = (11, 12, 21, 22, 23, 161, 176, 177)
    n = 0
    for H, W, levels in itertools.product(sides, sides, range(6)):
        g = geom(H, W, levels)
        if levels > render_ref.max_levels(H, W):
            assert L.adfp_frame_metrics_windows(C.byref(g), win) == ARG, (H, W, levels)
            continue
        assert L.adfp_frame_metrics_windows(C.byref(g), win) == 0
        assert list(win) == render_ref.windows(H, W, levels), (H, W, levels)
        n += 1
    assert n == sum(render_ref.max_levels(H, W) + 1 for H in sides for W in sides)
    assert render_ref.max_levels(176, 176) == 5 and render_ref.max_levels(177, 161) == 5 and render_ref.max_levels(23, 176) == 2
    assert L.adfp_frame_metrics_windows(C.byref(geom(176, 177, 5)), win) == 0 and win[4] == 1 * 2      # 176 -> 11, 177 -> 12
    assert L.adfp_frame_metrics_windows(C.byref(geom(680, 1200, 5)), win) == 0
    assert list(win) == [670 * 1190, 330 * 590, 160 * 290, 75 * 140, 33 * 65]        # Replica's frame


def test_max_levels_is_the_geometry_s():
    for H, W in itertools.product((1, 10, 11, 21, 22, 23, 43, 44, 87, 88, 160, 161, 175, 176, 177, 680), repeat=2):
        assert render_eval.max_levels(H, W) == render_ref.max_levels(H, W), (H, W)
    assert render_eval.max_levels(161, 161) == 5 and render_eval.max_levels(160, 4000) == 4
    assert render_eval.MS_SSIM_WEIGHTS == render_ref.MS_SSIM_WEIGHTS
