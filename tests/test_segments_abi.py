"""CPU: adfp_draw_segments of the C ABI without a GPU -- both exports are bound in _lib's table, the version is unchanged, and every
argument error of include/adfp.h comes back as a negative code before any launch."""
import ctypes as C
import inspect

from attentive_dfprior_amd import _lib, render_mesh

NEW = ['adfp_draw_segments_workspace_bytes', 'adfp_draw_segments']
ARG, UNSUPPORTED = -1, -2
TOO_MANY = 2 ** 31 - 1024                  # one above 2^31 - 1025
d = C.c_void_p(16)                         # never dereferenced: every call below fails its host-side checks first
NAN, INF = float('nan'), float('inf')


def test_exports_are_bound_and_version_is_unchanged():
    names = [n for n, _, _ in _lib.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1, n
    L = _lib.lib()
    for n in NEW:
        assert getattr(L, n) is not None
    assert L.adfp_version() == _lib.ABI_VERSION == 134
    assert _lib.SEG_MAX_RANGES == 8
    sig = inspect.signature(render_mesh.draw_segments)
    assert list(sig.parameters)[:15] == ['rgb', 'depth', 'c2w', 'fx', 'fy', 'cx', 'cy', 'segments', 'colors', 'ranges', 'width',
                                         'near_clip', 'bias', 'hidden_alpha', 'want_seg']
    assert sig.parameters['width'].default == 2.0 and sig.parameters['near_clip'].default == 1e-3
    assert sig.parameters['hidden_alpha'].default == 0.0 and sig.parameters['ranges'].default is None


def test_workspace_bytes():
    L = _lib.lib()
    ws = L.adfp_draw_segments_workspace_bytes
    assert ws(3, 600) == 64 * 3 * 600 and ws(1, 1) == 256 and ws(2, 3) == 512
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(-1, 5) == 0 and ws(5, -1) == 0
    assert ws(TOO_MANY, 1) == 0 and ws(1, TOO_MANY) == 0 and ws(2 ** 20, 2 ** 20) == 0


def test_argument_errors_come_back_before_any_launch():
    L = _lib.lib()
    big = L.adfp_draw_segments_workspace_bytes(2, 10)

    def draw(rgb=d, depth=None, seg=None, nv=2, H=48, W=64, c2w=d, fx=50.0, fy=50.0, cx=31.5, cy=23.5, segments=d, colors=d, ns=10,
             ranges=None, nr=0, nl=0, hw=1.0, near=1e-3, br=0.0, ba=0.0, alpha=0.0, wsp=d, wsb=big):
        return L.adfp_draw_segments(rgb, depth, seg, nv, H, W, c2w, fx, fy, cx, cy, segments, colors, ns, ranges, nr, nl, hw, near, br, ba,
                                    alpha, wsp, wsb, None)
    assert draw(rgb=None) == ARG
    assert draw(c2w=None) == ARG
    assert draw(segments=None) == ARG
    assert draw(colors=None) == ARG
    assert draw(nv=-1) == ARG
    assert draw(ns=-1) == ARG
    assert draw(ranges=d, nr=1, nl=-1) == ARG
    assert draw(H=0) == ARG
    assert draw(W=0) == ARG
    assert draw(fx=0.0) == ARG
    assert draw(fy=0.0) == ARG
    for k in ('fx', 'fy', 'cx', 'cy'):
        assert draw(**{k: NAN}) == ARG and draw(**{k: INF}) == ARG
    for hw in (0.0, -1.0, 64.5, NAN, INF):
        assert draw(hw=hw) == ARG
    for near in (0.0, -1.0, NAN, INF):
        assert draw(near=near) == ARG
    for b in (-1e-9, NAN, INF):
        assert draw(br=b) == ARG and draw(ba=b) == ARG
    for alpha in (-0.1, 1.1, NAN):
        assert draw(alpha=alpha) == ARG
    assert draw(ranges=d, nr=0, nl=10) == ARG
    assert draw(ranges=d, nr=9, nl=10) == ARG
    assert draw(ranges=d, nr=-1, nl=10) == ARG
    assert draw(wsb=big - 1) == ARG                             # a workspace that is too small
    assert draw(wsp=None) == ARG
    assert draw(ranges=d, nr=3, nl=11) == ARG                   # ... for the ranges' list, which is longer than n_seg here
    assert draw(H=32769) == UNSUPPORTED
    assert draw(W=32769) == UNSUPPORTED
    assert draw(nv=TOO_MANY) == UNSUPPORTED
    assert draw(ns=TOO_MANY) == UNSUPPORTED
    assert draw(ranges=d, nr=1, nl=TOO_MANY) == UNSUPPORTED
    assert draw(nv=2 ** 20, ns=2 ** 20) == UNSUPPORTED
    assert draw(nv=0) == 0                                      # nothing to do
    assert draw(nv=0, segments=None, colors=None, ns=0, wsp=None, wsb=0) == 0
