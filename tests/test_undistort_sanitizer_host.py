"""CPU: the host side of the lens-undistortion entries under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program (tests/asan/undistort_driver.cpp) linked against csrc/adfp_ingest.h built with its host translation instrumented
(tests/asan/ingest_only.hip; the device code is built as in the product, -fno-gpu-sanitize).  adfp_undistort_map converts doubles
to int: the driver feeds it positions beyond int32, infinities and a zero denominator, which the contract clamps or replaces
before the conversion.  No GPU is used: the device entries are walked through their argument errors only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-I' + os.path.join(ROOT, 'include')]


def test_undistort_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    clang = '/opt/rocm/lib/llvm/bin/clang++'
    if not (os.path.exists(hipcc) and os.path.exists(clang)):
        pytest.skip('no hipcc / clang++ on this box')
    out = str(tmp_path)
    build = [[hipcc, '--offload-arch=gfx950', '-ffp-contract=off', '-fno-slp-vectorize', '-fno-gpu-sanitize', *FLAGS,
              '-I' + os.path.join(ROOT, 'attentive_dfprior_amd', 'csrc'), '-shared', '-fPIC', '-o', os.path.join(out, 'libadfp_ingest_asan.so'),
              os.path.join(ROOT, 'tests', 'asan', 'ingest_only.hip')],
             [clang, *FLAGS, os.path.join(ROOT, 'tests', 'asan', 'undistort_driver.cpp'), '-L' + out, '-ladfp_ingest_asan',
              '-Wl,-rpath,' + out, '-o', os.path.join(out, 'undistort_driver')]]
    for cmd in build:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    r = subprocess.run([os.path.join(out, 'undistort_driver')], capture_output=True, text=True, env=env, timeout=120)
    tail = (r.stdout + r.stderr)[-3000:]
    assert 'ERROR: AddressSanitizer' not in tail and 'runtime error' not in tail, tail
    assert r.returncode == 0 and 'undistort sanitizer driver: 0 failed expectations' in r.stdout, tail
