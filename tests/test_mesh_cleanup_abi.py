"""CPU: the mesh clean-up entries of the C ABI without a GPU -- every export is bound in _lib's table, and null pointers, negative
counts, meshes beyond what the int32 sort carries and short workspaces come back as negative codes before any launch."""
import ctypes as C

from attentive_dfprior_amd import _lib

NEW = ['adfp_mesh_seen_mask', 'adfp_mesh_face_labels_workspace_bytes', 'adfp_mesh_face_labels_begin', 'adfp_mesh_face_labels_rounds',
       'adfp_mesh_component_keep_workspace_bytes', 'adfp_mesh_component_keep', 'adfp_mesh_compact_workspace_bytes',
       'adfp_mesh_compact_plan', 'adfp_mesh_compact_emit', 'adfp_mesh_merge_workspace_bytes', 'adfp_mesh_merge_plan',
       'adfp_mesh_merge_emit', 'adfp_mesh_color_bytes']
ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
TOO_MANY_VERTS = 2 ** 31 - 1024            # one above 2^31 - 1025
TOO_MANY_FACES = (2 ** 31 - 1025) // 3 + 1   # 3 F above 2^31 - 1025
d = C.c_void_p(16)                         # never dereferenced: every call below fails its host-side checks first


def test_exports_are_bound_and_version_is_unchanged():
    names = [n for n, _, _ in _lib.SYMBOLS]
    for n in NEW:
        assert names.count(n) == 1, n
    L = _lib.lib()
    for n in NEW:
        assert getattr(L, n) is not None
    assert L.adfp_version() == _lib.ABI_VERSION == 134
    assert _lib.SEEN_RULE == {'frustum': 0, 'max_depth': 1, 'depth_test': 2}


def test_seen_mask_argument_errors():
    L = _lib.lib()

    def seen(verts=d, nv=10, w2c=d, npose=2, rule=0, depth=None, dmax=None, W=64, H=48, out=d):
        return L.adfp_mesh_seen_mask(verts, nv, w2c, npose, rule, depth, dmax, 50.0, 50.0, 31.5, 23.5, W, H, out, None)
    assert seen(verts=None) == ARG
    assert seen(out=None) == ARG
    assert seen(w2c=None) == ARG
    assert seen(nv=-1) == ARG
    assert seen(npose=-1) == ARG
    assert seen(rule=3) == ARG
    assert seen(rule=-1) == ARG
    assert seen(rule=1) == ARG                              # the max-depth rule without its bounds
    assert seen(rule=2, dmax=d) == ARG                      # the depth test without its images
    assert seen(W=0) == ARG
    assert seen(H=0) == ARG
    assert seen(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert seen(npose=(2 ** 31 - 1025) // 12 + 1) == UNSUPPORTED
    assert seen(W=32769) == UNSUPPORTED
    assert seen(rule=2, depth=d, W=1) == UNSUPPORTED
    assert seen(nv=0, verts=None, out=None) == 0            # nothing to launch


def test_face_labels_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_face_labels_workspace_bytes(100)
    assert ws > 0 and L.adfp_mesh_face_labels_workspace_bytes(0) == 0 and L.adfp_mesh_face_labels_workspace_bytes(-1) == 0
    assert L.adfp_mesh_face_labels_workspace_bytes(TOO_MANY_FACES) == 0

    def begin(faces=d, nf=100, nv=50, keep=None, mate=d, labels=d, wsp=d, wsb=ws):
        return L.adfp_mesh_face_labels_begin(faces, nf, nv, keep, mate, labels, wsp, wsb, None)
    assert begin(faces=None) == ARG
    assert begin(mate=None) == ARG
    assert begin(labels=None) == ARG
    assert begin(wsp=None) == ARG
    assert begin(nf=-1) == ARG
    assert begin(nv=-1) == ARG
    assert begin(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert begin(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert begin(wsb=ws - 1) == WORKSPACE
    assert begin(nf=0, faces=None, mate=None, labels=None, wsp=None, wsb=0) == 0

    def rounds(mate=d, labels=d, nf=100, n=4, changed=d):
        return L.adfp_mesh_face_labels_rounds(mate, labels, nf, n, changed, None)
    assert rounds(mate=None) == ARG
    assert rounds(labels=None) == ARG
    assert rounds(changed=None) == ARG
    assert rounds(nf=-1) == ARG
    assert rounds(n=0) == ARG
    assert rounds(nf=TOO_MANY_FACES) == UNSUPPORTED


def test_component_keep_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_component_keep_workspace_bytes(100)
    assert ws > 0 and L.adfp_mesh_component_keep_workspace_bytes(0) == 0
    assert L.adfp_mesh_component_keep_workspace_bytes(TOO_MANY_FACES) == 0

    def keep(verts=d, nv=50, faces=d, nf=100, labels=d, largest=0, thr=0.1, out=d, wsp=d, wsb=ws):
        return L.adfp_mesh_component_keep(verts, nv, faces, nf, labels, largest, thr, out, wsp, wsb, None)
    assert keep(verts=None) == ARG
    assert keep(faces=None) == ARG
    assert keep(labels=None) == ARG
    assert keep(out=None) == ARG
    assert keep(wsp=None) == ARG
    assert keep(nf=-1) == ARG
    assert keep(nv=-1) == ARG
    assert keep(largest=2) == ARG
    assert keep(thr=float('nan')) == ARG
    assert keep(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert keep(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert keep(wsb=ws - 1) == WORKSPACE
    assert keep(nf=0, faces=None, labels=None, out=None, wsp=None, wsb=0) == 0


def test_compact_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_compact_workspace_bytes(50, 100)
    assert ws > 0 and L.adfp_mesh_compact_workspace_bytes(-1, 100) == 0 and L.adfp_mesh_compact_workspace_bytes(50, TOO_MANY_FACES) == 0

    def plan(faces=d, nf=100, nv=50, keep=d, wsp=d, wsb=ws, totals=d):
        return L.adfp_mesh_compact_plan(faces, nf, nv, keep, wsp, wsb, totals, None)
    assert plan(faces=None) == ARG
    assert plan(keep=None) == ARG
    assert plan(wsp=None) == ARG
    assert plan(totals=None) == ARG
    assert plan(nf=-1) == ARG
    assert plan(nv=-1) == ARG
    assert plan(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert plan(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert plan(wsb=ws - 1) == WORKSPACE

    def emit(verts=d, nv=50, faces=d, nf=100, wsp=d, wsb=ws, vo=d, nvo=10, fo=d, nfo=10):
        return L.adfp_mesh_compact_emit(verts, nv, faces, nf, wsp, wsb, vo, nvo, fo, nfo, None)
    assert emit(verts=None) == ARG
    assert emit(faces=None) == ARG
    assert emit(wsp=None) == ARG
    assert emit(vo=None) == ARG
    assert emit(fo=None) == ARG
    assert emit(nvo=-1) == ARG
    assert emit(nfo=-1) == ARG
    assert emit(nvo=51) == ARG                              # more survivors than vertices
    assert emit(nfo=101) == ARG
    assert emit(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert emit(wsb=ws - 1) == WORKSPACE
    assert emit(nvo=0, nfo=0, vo=None, fo=None) == 0


def test_merge_and_colour_argument_errors():
    L = _lib.lib()
    ws = L.adfp_mesh_merge_workspace_bytes(50)
    assert ws > 0 and L.adfp_mesh_merge_workspace_bytes(0) == 0 and L.adfp_mesh_merge_workspace_bytes(TOO_MANY_VERTS) == 0

    def plan(verts=d, nv=50, wsp=d, wsb=ws, total=d):
        return L.adfp_mesh_merge_plan(verts, nv, wsp, wsb, total, None)
    assert plan(verts=None) == ARG
    assert plan(wsp=None) == ARG
    assert plan(total=None) == ARG
    assert plan(nv=-1) == ARG
    assert plan(nv=TOO_MANY_VERTS) == UNSUPPORTED
    assert plan(wsb=ws - 1) == WORKSPACE

    def emit(verts=d, colors=None, nv=50, faces=d, nf=100, wsp=d, wsb=ws, vo=d, co=None, nvo=40, fo=d):
        return L.adfp_mesh_merge_emit(verts, colors, nv, faces, nf, wsp, wsb, vo, co, nvo, fo, None)
    assert emit(verts=None) == ARG
    assert emit(faces=None) == ARG
    assert emit(wsp=None) == ARG
    assert emit(vo=None) == ARG
    assert emit(fo=None) == ARG
    assert emit(colors=d) == ARG                            # colours in without colours out
    assert emit(co=d) == ARG
    assert emit(nv=-1) == ARG
    assert emit(nf=-1) == ARG
    assert emit(nvo=51) == ARG
    assert emit(nf=TOO_MANY_FACES) == UNSUPPORTED
    assert emit(wsb=ws - 1) == WORKSPACE
    assert emit(nv=0, nf=0, nvo=0) == 0

    assert L.adfp_mesh_color_bytes(None, 5, 4, d, None) == ARG
    assert L.adfp_mesh_color_bytes(d, 5, 4, None, None) == ARG
    assert L.adfp_mesh_color_bytes(d, -1, 4, d, None) == ARG
    assert L.adfp_mesh_color_bytes(d, 5, 2, d, None) == ARG
    assert L.adfp_mesh_color_bytes(d, TOO_MANY_VERTS, 4, d, None) == UNSUPPORTED
    assert L.adfp_mesh_color_bytes(None, 0, 4, None, None) == 0
