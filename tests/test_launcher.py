"""_lib.on / _lib.host / _lib.workspace: the one call path of the tool wrappers, against a stub in place of libadfp.so (no GPU)."""
import ctypes as C

import pytest
import torch

from attentive_dfprior_amd import _lib

STREAM = C.c_void_p(0x5eed)


class _Stub(object):
    """Stands where lib()'s handle stands: every entry point records its arguments and returns `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc
        return fn


@pytest.fixture
def world(monkeypatch):
    """A stub library, a counted current_stream and a fake current device (starts at 0)."""
    class World(object):
        stub, streams, device, switches = _Stub(), [], 0, []
    w = World()
    monkeypatch.setattr(_lib, '_lib', w.stub)

    def current_stream(dev):
        w.streams.append(dev)
        return STREAM

    def set_device(i):
        w.switches.append(i)
        w.device = i
    monkeypatch.setattr(_lib, 'current_stream', current_stream)
    monkeypatch.setattr(torch._C, '_cuda_getDevice', lambda: w.device)
    monkeypatch.setattr(torch._C, '_cuda_setDevice', set_device)
    return w


DEV = torch.device('cuda', 0)


def test_stream_is_last_and_read_once(world):
    with _lib.on(DEV) as L:
        L.adfp_cull_faces(1, 2)
        L.adfp_mesh_color_bytes(3)
        L.adfp_cull_faces()
    assert world.streams == [DEV]
    assert [(n, a[:-1]) for n, a in world.stub.calls] == [('adfp_cull_faces', (1, 2)), ('adfp_mesh_color_bytes', (3,)), ('adfp_cull_faces', ())]
    assert all(a[-1] is STREAM for _, a in world.stub.calls)


def test_arguments(world):
    t = torch.arange(6, dtype=torch.float32)
    view = t[2:]
    o = (C.c_double * 3)(1., 2., 3.)
    ref, vp, s = C.byref(o), C.c_void_p(64), 'text'
    with _lib.on(DEV) as L:
        L.adfp_cull_faces(t, view, torch.empty(0), t[:0], None, 7, 2.5, ref, o, vp, s)
    (_, a), = world.stub.calls
    assert isinstance(a[0], C.c_void_p) and a[0].value == t.data_ptr()
    assert isinstance(a[1], C.c_void_p) and a[1].value == t.data_ptr() + 8
    assert a[2] is None and a[3] is None and a[4] is None          # NULL: no elements (also a view into live storage), None
    assert a[5] == 7 and type(a[5]) is int and a[6] == 2.5
    assert a[7] is ref and a[8] is o and a[9] is vp and a[10] is s
    assert len(a) == 12


@pytest.mark.parametrize('rc,text', [(_lib.E_ARG, 'adfp_cull_faces: ADFP_E_ARG (null pointer / bad size)'),
                                     (_lib.E_UNSUPPORTED, 'adfp_cull_faces: ADFP_E_UNSUPPORTED'),
                                     (_lib.E_WORKSPACE, 'adfp_cull_faces: ADFP_E_WORKSPACE (workspace too small)'),
                                     (-77, 'adfp_cull_faces: -77'), (719, 'adfp_cull_faces: hipError_t 719')])
def test_return_code(world, rc, text):
    with _lib.on(DEV) as L:
        assert L.adfp_cull_faces() is None
        world.stub.rc = rc
        with pytest.raises(RuntimeError) as e:
            L.adfp_cull_faces()
    assert str(e.value) == text


def test_device_switch_and_restore(world):
    with _lib.on(DEV):
        assert world.device == 0
    assert world.switches == []                                  # already current: untouched
    other = torch.device('cuda', 3)
    with _lib.on(other) as L:
        assert world.device == 3 and world.streams[-1] == other
        L.adfp_cull_faces()
    assert world.device == 0 and world.switches == [3, 0]
    world.stub.rc = _lib.E_ARG
    with pytest.raises(RuntimeError):
        with _lib.on(other) as L:
            L.adfp_cull_faces()
    assert world.device == 0 and world.switches == [3, 0, 3, 0]
    with _lib.on(torch.device('cuda')):                          # no index: the current device, whatever it is
        assert world.device == 0
    assert world.switches == [3, 0, 3, 0]


def test_only_launches(world):
    not_launches = sorted(_lib.HOST_ONLY) + ['adfp_version', 'adfp_no_such_entry_point'] + \
        [name for name, res, _ in _lib.SYMBOLS if res is not C.c_int]
    assert 'adfp_mc_workspace_bytes' in not_launches and 'adfp_decoder_flat_floats' in not_launches
    with _lib.on(DEV) as L:
        for name in not_launches:
            with pytest.raises(AttributeError, match=name):
                getattr(L, name)
    assert world.stub.calls == []
    assert len(_lib.LAUNCHES) + len(not_launches) - 1 == len(_lib.SYMBOLS)


def test_host_only(world):
    h, w = C.c_int(), C.c_int()
    _lib.host.adfp_ingest_out_shape(None, h, w)
    assert world.stub.calls == [('adfp_ingest_out_shape', (None, h, w))] and world.streams == []       # no stream appended
    world.stub.rc = _lib.E_UNSUPPORTED
    with pytest.raises(RuntimeError) as e:
        _lib.host.adfp_mc_table(300, None)
    assert str(e.value) == 'adfp_mc_table: ADFP_E_UNSUPPORTED'
    for name in ('adfp_cull_faces', 'adfp_version', 'adfp_mc_workspace_bytes'):
        with pytest.raises(AttributeError, match=name):
            getattr(_lib.host, name)


def test_every_launch_ends_in_a_stream():
    """LAUNCHES is built from return types and HOST_ONLY; the header's own text must agree: `void* stream` closes exactly these."""
    import re
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', open(_lib.HEADER_PATH).read(), flags=re.S)
    with_stream = set(re.findall(r'\b(adfp_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;', text))
    assert with_stream == _lib.LAUNCHES


def test_workspace():
    ws = _lib.workspace(0, 'cpu')
    assert ws.dtype == torch.uint8 and ws.numel() == 1               # never a NULL pointer
    assert _lib.workspace(C.c_size_t(4096).value, 'cpu').numel() == 4096


@pytest.mark.gpu
def test_empty_device_tensor_has_a_null_pointer():
    """What the conversion leans on wherever a wrapper used to pass ptr(empty) unguarded."""
    assert torch.empty(0, device='cuda').data_ptr() == 0
    assert torch.empty((0, 3), dtype=torch.float64, device='cuda').data_ptr() == 0
