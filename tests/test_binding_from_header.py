"""CPU: attentive_dfprior_amd/_lib.py derives its structs, its prototype table and its constants from include/adfp.h.  The parser's
rules on a short header written here, its refusals, and what it makes of the real header.  (tests/test_abi.py has gcc judge the
struct layouts.)"""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from attentive_dfprior_amd import _lib

MINI = '''
/* a comment that names int bogus(float x); and #define ADFP_BOGUS 1 */
#ifndef ADFP_MINI_H
#define ADFP_MINI_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define ADFP_VERSION 7
#define ADFP_E_ARG   (-1)   /* bad argument */
#define ADFP_ROWS 3
#define ADFP_RATIO 0.5
typedef struct adfp_cell { const float* data; int a, b; long long n; } adfp_cell;
typedef struct adfp_box {
    double bound[ADFP_ROWS][2];     /* two dimensions, one of them a define */
    adfp_cell cell;                 /* by value */
    adfp_cell cells[2];
    const adfp_cell* next;
    void* events[2];
    unsigned char* flags; unsigned mask; unsigned char tag; size_t bytes; unsigned long long big;
    float lr[2]; float beta1, beta2;
} adfp_box;
struct adfp_later;
int adfp_version(void);
long long adfp_count(int kind);
size_t adfp_bytes(long long n, unsigned flags, unsigned char tag, unsigned long long big, size_t have);
int adfp_run(const adfp_box* box /*host*/, const struct adfp_later* later, const double bound[3][2], const float c2w[16],
             const int lo[ADFP_ROWS],
             float lr /*[1]*/, double far, const float* rays, void* const* dst /*host [F]*/, int* H_out,
             signed char* table, void* stream);
typedef struct adfp_later { int x; } adfp_later;
#ifdef __cplusplus
}
#endif
#endif
'''


def test_rules_on_a_short_header():
    structs, protos, defines = _lib.parse_header(MINI)
    assert defines == {'ADFP_VERSION': 7, 'ADFP_E_ARG': -1, 'ADFP_ROWS': 3, 'ADFP_RATIO': None}       # ADFP_MINI_H has no value
    assert list(structs) == ['adfp_cell', 'adfp_box', 'adfp_later']
    Cell, Box, Later = structs.values()
    assert (Cell.__name__, Box.__name__, Later.__name__) == ('AdfpCell', 'AdfpBox', 'AdfpLater')
    assert all(issubclass(s, C.Structure) for s in structs.values())
    assert Cell._fields_ == [('data', C.c_void_p), ('a', C.c_int), ('b', C.c_int), ('n', C.c_longlong)]
    assert Box._fields_ == [('bound', (C.c_double * 2) * 3), ('cell', Cell), ('cells', Cell * 2), ('next', C.POINTER(Cell)),
                            ('events', C.c_void_p * 2), ('flags', C.c_void_p), ('mask', C.c_uint), ('tag', C.c_ubyte),
                            ('bytes', C.c_size_t), ('big', C.c_ulonglong), ('lr', C.c_float * 2), ('beta1', C.c_float),
                            ('beta2', C.c_float)]
    assert [p[0] for p in protos] == ['adfp_version', 'adfp_count', 'adfp_bytes', 'adfp_run']
    assert protos[0][1:] == (C.c_int, []) and protos[1][1:] == (C.c_longlong, [C.c_int])
    assert protos[2][1:] == (C.c_size_t, [C.c_longlong, C.c_uint, C.c_ubyte, C.c_ulonglong, C.c_size_t])                # R1
    assert protos[3][2] == [C.POINTER(Box), C.POINTER(Later),                                                          # R2
                            C.POINTER((C.c_double * 2) * 3), C.POINTER(C.c_float * 16), C.POINTER(C.c_int * 3),        # R3
                            C.c_float, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]         # R1, R4
    # what the typed pointers take and refuse
    box_p = protos[3][2][0]
    box_p.from_param(Box()), box_p.from_param(C.byref(Box())), box_p.from_param(None)
    with pytest.raises(TypeError):
        box_p.from_param(Cell())
    with pytest.raises(TypeError):
        protos[3][2][3].from_param((C.c_float * 12)())


PROLOGUE = '#define ADFP_HALF 0.5\ntypedef struct adfp_ok { int x; } adfp_ok;\n'
REFUSED = {
    'unknown type': 'int adfp_f(uint8_t x);',
    'unknown type in a struct': 'typedef struct adfp_s { short x; } adfp_s;',
    'function pointer parameter': 'int adfp_f(int (*cb)(int), void* stream);',
    'function pointer field': 'typedef struct adfp_s { void (*cb)(int); } adfp_s;',
    'union': 'typedef union adfp_u { int a; float b; } adfp_u;',
    'union in a struct': 'typedef struct adfp_s { union { int a; float b; } u; int c; } adfp_s;',
    'bitfield': 'typedef struct adfp_s { int a : 3; } adfp_s;',
    'variadic': 'int adfp_f(int n, ...);',
    'dimension that is no integer': 'typedef struct adfp_s { float w[ADFP_HALF]; } adfp_s;',
    'dimension that is not defined': 'int adfp_f(const float w[ADFP_NOWHERE]);',
    'multi-declarator with stars': 'typedef struct adfp_s { float *a, *b; } adfp_s;',
    'multi-declarator after a star': 'typedef struct adfp_s { float* a, b; } adfp_s;',
    'return type': 'float adfp_f(int x);',
    'pointer return type': 'const char* adfp_f(int x);',
    'struct by value parameter': 'int adfp_f(adfp_ok s);',
    'unnamed parameter': 'int adfp_f(int);',
}


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_parser_refuses(what):
    _lib.parse_header(PROLOGUE + 'int adfp_fine(const adfp_ok* s, int n);')
    with pytest.raises(ValueError, match='include/adfp.h: .+: ".*adfp_.*"'):        # says why and quotes the declaration
        _lib.parse_header(PROLOGUE + REFUSED[what])


def test_missing_header_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'include' / 'adfp.h'))
    with pytest.raises(RuntimeError, match=str(tmp_path / 'include' / 'adfp.h')):
        _lib._load_header()


def test_the_real_header():
    assert _lib.HEADER_PATH == os.path.join(ROOT, 'include', 'adfp.h')
    text = re.sub(r'/\*.*?\*/', '', open(_lib.HEADER_PATH).read(), flags=re.S)
    assert len(_lib.SYMBOLS) == 152 and len(_lib.STRUCTS) == 25
    names = [s[0] for s in _lib.SYMBOLS]
    assert len(set(names)) == 152
    at = [re.search(rf'\b{n}\s*\(', text).start() for n in names]
    assert at == sorted(at), 'SYMBOLS is in header order'
    at = [text.index(f'typedef struct {n} ') for n in _lib.STRUCTS]
    assert at == sorted(at)
    for cname, cls in _lib.STRUCTS.items():
        assert cls.__name__ == ''.join(p.capitalize() for p in cname.split('_')) and getattr(_lib, cls.__name__) is cls
    assert _lib.AdfpTrackerHeadArgs and _lib.AdfpTsdf and _lib.AdfpTrackLossArgs and _lib.AdfpScene().low.Z == 0
    assert _lib.ABI_VERSION == _lib.DEFINES['ADFP_VERSION'] == 134


def test_constants_are_the_defines():
    D = _lib.DEFINES
    for name, value in D.items():
        if name.startswith('ADFP_') and value is not None:
            assert getattr(_lib, name[5:]) == value, name
    table = {'STAGE': 'STAGE_', 'DEC_KIND': 'DEC_', 'STATUS_RANGE_BITS': 'STATUS_F16_RANGE_', 'ICP_STATUS': 'ICP_', 'MC_OUT': 'MC_OUT_',
             'CULL': 'CULL_', 'SHADE_MODE': 'SHADE_', 'SEEN_RULE': 'SEEN_', 'SIMPLIFY': 'SIMPLIFY_', 'BLEND': 'BLEND_'}
    for attr, prefix in table.items():
        d = getattr(_lib, attr)
        assert len(d) >= 2
        for key, value in d.items():
            assert value == D[f'ADFP_{prefix}{key.upper()}'], (attr, key)
    assert _lib.NET_ID == {'low': D['ADFP_DEC_LOW'], 'high': D['ADFP_DEC_HIGH'], 'color': D['ADFP_DEC_COLOR'], 'att': D['ADFP_NET_ATT']}
    assert set(_lib.ERRORS) == {-1, -2, -3} == {D['ADFP_E_ARG'], D['ADFP_E_UNSUPPORTED'], D['ADFP_E_WORKSPACE']}
    for code, word in ((D['ADFP_E_ARG'], 'ADFP_E_ARG'), (D['ADFP_E_UNSUPPORTED'], 'ADFP_E_UNSUPPORTED'), (D['ADFP_E_WORKSPACE'], 'ADFP_E_WORKSPACE')):
        assert _lib.ERRORS[code].startswith(word)
    assert (_lib.IMAGE_H, _lib.IMAGE_G, _lib.IMAGE_HT) == (D['ADFP_IMAGE_H'], D['ADFP_IMAGE_G'], D['ADFP_IMAGE_HT'])
    assert (_lib.PTS_RAYS, _lib.PTS_F64, _lib.PTS_F32) == (D['ADFP_PTS_RAYS'], D['ADFP_PTS_F64'], D['ADFP_PTS_F32'])
    # the header states these in words only (no #define of the name): adfp_ingest_geom.color_order's comment
    assert _lib.COLOR_ORDER == {'bgr': 0, 'rgb': 1} and not any('COLOR_ORDER' in k for k in D)


def test_overrides_are_few_alive_and_needed():
    """Each override names an existing entry and argument, and differs from what the rules give there (a dead one must go)."""
    ruled = {name: args for name, _, args in _lib._prototypes}
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert len(_lib.OVERRIDES) == 4
    for (name, i), t in _lib.OVERRIDES.items():
        assert name in ruled and 0 <= i < len(ruled[name]), (name, i)
        assert ruled[name][i] is not t, (name, i)
        assert bound[name][i] is t
        assert ruled[name][i].__name__ in ('LP_AdfpAdamGroup', 'LP_AdfpAdamClGroup')
    changed = [(n, i) for n in ruled for i, t in enumerate(ruled[n]) if bound[n][i] is not t]
    assert sorted(changed) == sorted(_lib.OVERRIDES)


def test_respelled_parameters_keep_their_types():
    """The three host arrays whose length moved into the declaration, and the one argument that became stricter."""
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert bound['adfp_nn_query'][5] is C.POINTER(C.c_double * 12)
    assert bound['adfp_icp_moments'][2] is C.POINTER(C.c_double * 12) and bound['adfp_icp_moments'][3] is C.POINTER(C.c_double * 3)
    windows = bound['adfp_frame_metrics_windows'][1]
    assert windows is C.POINTER(C.c_longlong * 5)
    windows.from_param((C.c_longlong * 5)()), windows.from_param(None)
    assert bound['adfp_eval_points_train'][8] is C.POINTER(_lib.AdfpTrainState)
