"""ctypes binding of libadfp.so, derived from include/adfp.h when the module is imported.

The header is the only statement of the C ABI.  Its structs become the ``ctypes.Structure`` classes below (``adfp_scene`` ->
``AdfpScene``), its prototypes the ``SYMBOLS`` table and its integer ``#define ADFP_X`` the constants ``X``: a new entry point is
a declaration in the header plus its definition in csrc/, nothing here.  A tool wrapper calls it as ``with on(dev) as L:
L.adfp_x(tensor, n, ..., out)``: its argument checks, its output allocation and that one line, which names the entry point once
(device, stream, NULL for an empty tensor and the return code are ``on``'s).
The product path has no CPU fallback: if the HIP library is missing, ``lib()`` raises and
every compute entry point of this package fails loudly.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ADFP_LIB_PATH') or os.path.join(_HERE, 'libadfp.so')   # override: kernel A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'adfp.h')

# ---- the header's declarations -> ctypes ---------------------------------------------------------------------
# Strict on purpose: whatever is not one of the forms below raises with the declaration's text (a binding that guesses a type
# passes silently wrong numbers).  When the header needs a new form, prefer spelling the declaration in one of these.
_SCALARS = {'int': C.c_int, 'long long': C.c_longlong, 'float': C.c_float, 'double': C.c_double, 'size_t': C.c_size_t,
            'unsigned': C.c_uint, 'unsigned char': C.c_ubyte, 'unsigned long long': C.c_ulonglong}
_POINTEES = set(_SCALARS) | {'void', 'signed char'}
_RESTYPES = ('int', 'size_t', 'long long')
# [const] [struct] type  [* [const] ...]  name[, name ...]  [dim][dim]
_DECL = re.compile(r'(?:const )?(?:struct )?(\w+(?: \w+)*?) ?((?:\* ?(?:const ?)?)*)(\w+(?: ?, ?\w+)*) ?((?:\[ ?\w+ ?\] ?)*)')


def _refuse(why, decl, where=''):
    raise ValueError(f'include/adfp.h: {why}: "{where and where + ": "}{" ".join(decl.split())}"')


def _declaration(decl, where, structs, defines, param):
    """One struct field (param=False) or parameter (param=True) of the struct or function `where` -> ([names], ctypes type).
    R1 a scalar -> its ctypes type; R2 a pointer to one of the header's structs -> POINTER(its class), which takes an instance,
    byref(instance) or an array of them and refuses another struct; R3 brackets -> the array type in a struct, POINTER(array type)
    for a parameter; R4 every other pointer (device memory, void* const*, host int* ...) -> c_void_p."""
    m = _DECL.fullmatch(' '.join(decl.split()))
    if m is None:                 # a function pointer, a bitfield, `T *a, *b`, `...`, an unnamed parameter
        _refuse('a declaration of no known form', decl, where)
    base, stars, names, dims = m.groups()
    names = re.split(' ?, ?', names)
    if base not in _POINTEES and base not in structs:
        _refuse(f'unknown type {base!r}', decl, where)
    shape = []
    for d in re.findall(r'\w+', dims):
        if not d.isdigit() and not isinstance(defines.get(d), int):
            _refuse(f'dimension {d} is not an integer or an integer #define', decl, where)
        shape.append(int(d) if d.isdigit() else defines[d])
    if stars:
        if len(names) > 1 or (param and shape):
            _refuse('pointers in a multi-declarator or in an array parameter', decl, where)
        t = C.POINTER(structs[base]) if base in structs and stars.count('*') == 1 else C.c_void_p     # R2, R4
    elif base in structs and not (param and not shape):
        t = structs[base]
    elif base in _SCALARS:
        t = _SCALARS[base]                                                                            # R1
    else:
        _refuse(f'{base!r} by value', decl, where)
    for n in reversed(shape):
        t = t * n
    return names, C.POINTER(t) if param and shape else t                                              # R3


def parse_header(text):
    """The text of a C header in adfp.h's style -> (structs {C name: Structure class}, prototypes [(name, restype, argtypes)],
    defines {name: int, or None for a value that is not an integer}), each in the header's order."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    defines = {}
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$', text, flags=re.M):
        try:
            defines[name] = int(value[1:-1] if value[0] + value[-1] == '()' else value, 0)
        except ValueError:
            defines[name] = None
    text = re.sub(r'#[ \t]*ifdef __cplusplus.*?#[ \t]*endif', '', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    structs = {}
    typedef = re.compile(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', re.S)
    for name, body, alias in typedef.findall(text):
        if alias != name or '{' in body:              # a nested struct or union
            _refuse('a struct that is not `typedef struct x { plain fields } x;`', f'struct {name} {{{body}}} {alias}')
        fields = []
        for decl in filter(str.strip, body.split(';')):
            names, t = _declaration(decl, name, structs, defines, False)
            fields += [(n, t) for n in names]
        structs[name] = type(''.join(p.capitalize() for p in name.split('_')), (C.Structure,), {'_fields_': fields})
    prototypes = []
    for decl in filter(str.strip, typedef.sub('', text).split(';')):
        decl = ' '.join(decl.split())
        if re.fullmatch(r'struct \w+', decl):         # a forward declaration
            continue
        m = re.fullmatch(r'(\w+(?: \w+)*?) ?(\w+) ?\((.*)\)', decl)
        if m is None or '(' in m.group(3):            # a union, a variable, a function pointer among the parameters
            _refuse('not a prototype of a known form', decl)
        restype, name, params = m.groups()
        if restype not in _RESTYPES:
            _refuse(f'return type {restype!r} is none of {_RESTYPES}', decl)
        params = [] if params.strip() in ('void', '') else params.split(',')
        prototypes.append((name, _SCALARS[restype], [_declaration(p, name, structs, defines, True)[1] for p in params]))
    return structs, prototypes, defines


def _load_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise RuntimeError(f'{HEADER_PATH} is missing ({e.strerror}): attentive_dfprior_amd derives its binding of libadfp.so from '
                           'this header, which ships in the repository beside the package.') from None


# {C struct name: its class}, [(name, restype, argtypes) as the rules give them], {#define name: int, or None}
STRUCTS, _prototypes, DEFINES = _load_header()
globals().update({cls.__name__: cls for cls in STRUCTS.values()})                       # AdfpScene, AdfpPoints, ...
globals().update({k[5:]: v for k, v in DEFINES.items() if k.startswith('ADFP_') and v is not None})      # ADFP_X -> X

# The arguments whose type is not the one the rules give.  Here they give POINTER(AdfpAdamGroup) / POINTER(AdfpAdamClGroup), and
# the callers pass byref(<array of groups>), which a typed pointer refuses and c_void_p takes.
OVERRIDES = {('adfp_masked_adam_multi', 1): C.c_void_p, ('adfp_adam_grids_cl', 1): C.c_void_p,
             ('adfp_adam_step', 1): C.c_void_p, ('adfp_adam_step', 3): C.c_void_p}
# every symbol include/adfp.h declares: (name, restype, argtypes)
SYMBOLS = [(name, res, [OVERRIDES.get((name, i), t) for i, t in enumerate(args)]) for name, res, args in _prototypes]

Bound = (C.c_double * 2) * 3


def _named(prefix, names):
    return {n: DEFINES[f'ADFP_{prefix}_{n.upper()}'] for n in names.split()}


ABI_VERSION = DEFINES['ADFP_VERSION']         # lib() refuses a libadfp.so built from another version of the header
STATUS_RANGE_BITS = _named('STATUS_F16_RANGE', 'low high color att bwd')
STAGE = _named('STAGE', 'low high color')
DEC_KIND = _named('DEC', 'low high color')
NET_ID = dict(DEC_KIND, att=DEFINES['ADFP_NET_ATT'])      # adfp_pack_split_image's `net`
ERRORS = {DEFINES['ADFP_E_ARG']: 'ADFP_E_ARG (null pointer / bad size)',
          DEFINES['ADFP_E_UNSUPPORTED']: 'ADFP_E_UNSUPPORTED',
          DEFINES['ADFP_E_WORKSPACE']: 'ADFP_E_WORKSPACE (workspace too small)'}
ICP_STATUS = _named('ICP', 'ok few_pairs degenerate rejected')
MC_OUT = _named('MC_OUT', 'lower higher')
CULL = _named('CULL', 'none back front')
SHADE_MODE = _named('SHADE', 'color shaded normal')
SEEN_RULE = _named('SEEN', 'frustum max_depth depth_test')
SIMPLIFY = _named('SIMPLIFY', 'average quadric')
BLEND = _named('BLEND', 'weighted best')
# what the header states in words only
COLOR_ORDER = {'bgr': 0, 'rgb': 1}      # adfp_ingest_geom.color_order
ICP_MOMENTS = 17                       # adfp_icp_moments' out[]
TRI_LEAVES = (4, 8, 16)                # the leaf sizes adfp_tri_bvh_build takes
SEG_MAX_RANGES = 8                      # adfp_draw_segments' n_ranges
LABEL_ROUNDS_MAX = 128                # above the worst case of adfp_mesh_face_labels_rounds (2 log2(F) + 2 < 66)

_lib = None


def lib():
    """Load libadfp.so once.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: build the HIP extension first '
                '(python -c "import __graft_entry__ as g; g.build()" or attentive_dfprior_amd/csrc/build.sh). '
                'attentive_dfprior_amd has no CPU fallback.')
        handle = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.adfp_version() != ABI_VERSION:
            raise RuntimeError(f'{LIB_PATH} is ABI version {handle.adfp_version()}, this package binds {ABI_VERSION}: rebuild it')
        if HOST_TIMING is not None:
            class _Timed(object):
                pass
            t = _Timed()
            for name, _, _ in SYMBOLS:
                setattr(t, name, timed(getattr(handle, name), name))
            handle = t
        _lib = handle
    return _lib


# ADFP_HOST_TIMING=1: host seconds spent inside each C entry point (name -> [calls, seconds]); tools/host_breakdown.py prints it
HOST_TIMING = {} if os.environ.get('ADFP_HOST_TIMING') else None


def timed(fn, name):
    import time

    def call(*a):
        t0 = time.perf_counter()
        rc = fn(*a)
        e = HOST_TIMING.setdefault(name, [0, 0.0])
        e[0] += 1
        e[1] += time.perf_counter() - t0
        return rc
    return call


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise RuntimeError(f'{what}: {ERRORS.get(rc, rc)}')
    raise RuntimeError(f'{what}: hipError_t {rc}')


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def current_stream(device):
    """The raw hipStream_t of torch's current stream on `device` (torch.cuda.current_stream(device).cuda_stream costs ~7 us of
    Python object construction per call; a training iteration asks a dozen times)."""
    import torch
    idx = device.index if isinstance(device, torch.device) else torch.device(device).index
    if idx is None:
        idx = torch._C._cuda_getDevice()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


class device_guard(object):
    """`with device_guard(dev):` = `with torch.cuda.device(dev):` -- the kernels launch on the CURRENT HIP device -- without the
    per-call argument parsing: switches only when `dev` is not the current device already."""
    __slots__ = ('idx', 'prev')

    def __init__(self, dev):
        self.idx = dev.index if dev.index is not None else -1
        self.prev = -1

    def __enter__(self):
        import torch
        if self.idx >= 0:
            cur = torch._C._cuda_getDevice()
            if cur != self.idx:
                torch._C._cuda_setDevice(self.idx)
                self.prev = cur
        return self

    def __exit__(self, *exc):
        if self.prev >= 0:
            import torch
            torch._C._cuda_setDevice(self.prev)
            self.prev = -1
        return False


# ---- the tool wrappers' call path ------------------------------------------------------------------------------
HOST_ONLY = {'adfp_mc_table', 'adfp_ingest_out_shape', 'adfp_undistort_map', 'adfp_vis_canvas_shape', 'adfp_frame_metrics_windows'}
assert HOST_ONLY < {name for name, _, _ in SYMBOLS}
# the entry points that end in `void* stream`: every int-returning one but adfp_version and the host-only five
LAUNCHES = {name for name, res, _ in SYMBOLS if res is C.c_int} - HOST_ONLY - {'adfp_version'}


_Tensor = None


def _checked(name, *tail):
    """lib().name as the wrappers call it: a tensor argument goes as its data pointer, None or a tensor of no elements as NULL,
    anything else as it is; `tail` is appended; the return code goes through check() under the entry point's own name."""
    global _Tensor
    if _Tensor is None:
        from torch import Tensor as _Tensor
    fn, Tensor, void = getattr(lib(), name), _Tensor, C.c_void_p

    def call(*args):
        rc = fn(*[a if not isinstance(a, Tensor) else void(a.data_ptr()) if a.numel() else None for a in args], *tail)
        if rc:
            check(rc, name)
    return call


class on(device_guard):
    """`with on(dev) as L: L.adfp_x(a, n, out)` = adfp_x(ptr(a), n, ptr(out), stream) on `dev`, checked: device_guard(dev), with
    current_stream(dev) read once on entry and appended to every launch.  Only LAUNCHES; sizes and host-only calls raise."""

    def __init__(self, dev):
        device_guard.__init__(self, dev)
        self.dev = dev

    def __enter__(self):
        device_guard.__enter__(self)
        self.stream = current_stream(self.dev)
        return self

    def __getattr__(self, name):           # once per name and `with`: the call is kept on the instance
        if name not in LAUNCHES:
            raise AttributeError(f'{name} is not an entry point of include/adfp.h that ends in a stream: call it through lib()')
        call = self.__dict__[name] = _checked(name, self.stream)
        return call


class _Host(object):
    """`host.adfp_x(...)`: the HOST_ONLY entry points (no device, no stream), arguments and return code as under on()."""

    def __getattr__(self, name):
        if name not in HOST_ONLY:
            raise AttributeError(f'{name} is not a host-only entry point of include/adfp.h')
        return _checked(name)


host = _Host()


def workspace(nbytes, dev):
    """A scratch buffer of `nbytes` (at least one, so that its pointer is never NULL) on `dev`."""
    import torch
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def fill_bound(dst, values):
    """values: nested [[lo,hi]]*3 python floats."""
    for k in range(3):
        dst[k][0] = float(values[k][0])
        dst[k][1] = float(values[k][1])


def require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(
            f'{name} is on {t.device}: attentive_dfprior_amd runs only on an MI355X through libadfp.so; '
            'there is no CPU fallback.')


# ---- sticky status words (adfp_scene.status) ---------------------------------------------------------------
# A word of pinned host memory: the kernels OR into it with a system-scope atomic (pinned host memory is device-visible under
# HIP's unified addressing), and the host reads it without synchronising.  Every DF module owns one (decoder.DF.status_word), so
# that an f16-range event is attributed to the network object it happened in; sub-networks called on their own share the
# process-wide word below.  An f16-range bit is NOT an error any more: the call that raised it repaired itself on the device
# (adfp_scene.flat_*, csrc/adfp_fallback.h), and the host answers by switching that network to its exact image (read_status ->
# DF._exact_latch).
_status = None


def new_status_word():
    import torch
    return torch.zeros(4, dtype=torch.int32).pin_memory()


def status_word():
    global _status
    if _status is None:
        _status = new_status_word()
    return _status


def status_ptr():
    return C.c_void_p(status_word().data_ptr())


_status_views = {}


def read_status(word, sync=False, device=None):
    """The bits an earlier call left in `word` (cleared on read).  sync=True waits for the device first.  Range bits are returned
    to the caller; any other bit is an error.  The word is read through a ctypes view of the pinned memory: indexing the tensor
    costs two dispatcher calls per render call."""
    if word is None:
        return 0
    if sync:
        import torch
        torch.cuda.synchronize(device)
    addr = word.data_ptr()
    view = _status_views.get(addr)
    if view is None or view[1]() is not word:
        import weakref
        view = _status_views[addr] = (C.c_int.from_address(addr), weakref.ref(word))
    v = view[0].value
    if v:
        view[0].value = 0
        if v & ~STATUS_F16_RANGE:
            raise RuntimeError(f'libadfp: status word {v:#x}')
    return v


def check_status(sync=False, device=None):
    """Process-wide word (sub-networks called on their own): returns its range bits, raises on anything else."""
    return read_status(_status, sync, device)
