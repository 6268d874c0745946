"""CPU: the C-ABI library loads, exports every symbol include/adfp.h declares, and the ctypes
structs of attentive_dfprior_amd/_lib.py have the C layout (checked with gcc).  No compute call is
made here (no GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from attentive_dfprior_amd import _lib

HEADER = os.path.join(ROOT, 'include', 'adfp.h')


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(adfp_[a-z_0-9]+)\s*\(', src)))


def test_library_is_built():
    assert os.path.exists(_lib.LIB_PATH), 'run __graft_entry__.build() first'


def test_exports_every_declared_symbol():
    names = declared_symbols()
    assert len(names) >= 15
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f'{n} declared in include/adfp.h but not exported'
    bound = {s[0] for s in _lib.SYMBOLS}
    assert bound == set(names), (sorted(bound ^ set(names)))


def test_version_and_sizes():
    L = _lib.lib()
    assert L.adfp_version() == _lib.ABI_VERSION
    # parameter counts of the reference's modules (decoder.py:110-166, :212-228)
    assert [L.adfp_decoder_flat_floats(k) for k in range(3)] == [15800, 20920, 15899]
    assert L.adfp_attention_flat_floats() == 33410
    assert L.adfp_decoder_flat_floats(7) < 0
    # every network's packed image must fit the 160 KiB LDS of one CU
    for k in range(3):
        assert L.adfp_decoder_packed_floats(k) * 4 <= 160 * 1024
    assert L.adfp_attention_packed_floats() * 4 <= 160 * 1024
    assert L.adfp_workspace_bytes(0) >= 256
    assert L.adfp_workspace_bytes(1000) >= 1000 * 37


def test_host_side_argument_errors_need_no_gpu():
    L = _lib.lib()
    assert L.adfp_relayout_grid(None, None, 32, 1, 1, 1, None) == -1
    assert L.adfp_pack_decoder(0, None, None, None) == -1
    assert L.adfp_composite(None, None, 1, 1, None, None, None, None, None) == -1
    assert L.adfp_render_forward(None, None, None) == -1


@pytest.mark.skipif(subprocess.call(['which', 'gcc'], stdout=subprocess.DEVNULL) != 0, reason='no gcc')
def test_ctypes_struct_layout_matches_c(tmp_path):
    """gcc is the judge of the binding's header parser: sizeof of every struct class _lib built and offsetof + size of every field
    of it, from a generated C program compiled against include/adfp.h."""
    structs = _lib.STRUCTS
    assert len(structs) == 25 and all(getattr(_lib, cls.__name__) is cls for cls in structs.values())
    lines = []
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
    prog = tmp_path / 'layout.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "adfp.h"\nint main(void) {\n' + '\n'.join(lines) + '\nreturn 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)])
    c_says = {k: list(map(int, v)) for k, *v in (line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())}
    ctypes_says = {}
    for name, cls in structs.items():
        ctypes_says[name] = [ctypes.sizeof(cls)]
        ctypes_says.update({f'{name}.{f}': [getattr(cls, f).offset, getattr(cls, f).size] for f, _ in cls._fields_})
    assert len(c_says) == len(lines) > 300
    assert ctypes_says == c_says, sorted(k for k in c_says if ctypes_says.get(k) != c_says[k])


def test_reference_fusion_kernel_builds_as_a_checker():
    """oracle/_ref: the reference's CUDA C kernel string (src/fusion.py:69-142) compiled by hipcc from where it lies, in the
    as-written and the contracted variant; both export the launcher tests/test_gpu_fusion.py calls on the GPU box."""
    import ctypes
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists('/root/reference/src/fusion.py'):
        pytest.skip('/root/reference is not present (GPU box): the prebuilt oracle/_ref files are used as they are')
    sys.path.insert(0, os.path.join(root, 'oracle'))
    try:
        import build_ref_fusion
        assert 'SourceModule' not in build_ref_fusion.kernel_string() and '__global__ void integrate' in build_ref_fusion.kernel_string()
        assert build_ref_fusion.build()
    finally:
        sys.path.pop(0)
    for name in ('libref_fusion_exact.so', 'libref_fusion_contract.so'):
        lib = ctypes.CDLL(os.path.join(root, 'oracle', '_ref', name))
        assert hasattr(lib, 'ref_fusion_integrate')
    # nothing of the reference's text is kept in the repository
    for dirpath, _, files in os.walk(os.path.join(root, 'oracle')):
        for f in files:
            if f.endswith(('.py', '.hip', '.cu', '.txt')):
                assert 'float voxel_x = floorf' not in open(os.path.join(dirpath, f), errors='ignore').read(), f
