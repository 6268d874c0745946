"""GPU: a plain `python bench.py` (no `--full`) does only what the headline needs -- set-up, warm-up, the timed steps, the
outputs of `--dump-outputs`, the result line -- and its line carries the contract fields and none of the `--full` legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every key of a plain run's line: the contract fields and what qualifies them, nothing a --full leg adds
PLAIN_KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'math', 'config', 'source_hash'}
PLAIN_CONFIG_KEYS = {'workload', 'grid_std_scale', 'rays_per_step', 'rays_per_step_per_gpu', 'samples_per_ray', 'tsdf_voxels', 'grid_high'}


def run_bench(args, env=None, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone_and_dumps_its_outputs(tmp_path):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = run_bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(tmp_path)], env=env)
    assert set(r) == PLAIN_KEYS, sorted(set(r) ^ PLAIN_KEYS)
    assert set(r['config']) == PLAIN_CONFIG_KEYS, sorted(set(r['config']) ^ PLAIN_CONFIG_KEYS)
    assert r['metric'] == 'rendered rays/sec (64 samples/ray), Replica room0' and r['unit'] == 'rays/s'
    assert r['higher_is_better'] is True and r['scaling'] == 'strong' and r['n_gpus'] == 1
    assert r['steps'] == 3 and r['warmup'] == 1 and r['ms_per_step'] > 0
    assert abs(r['value'] - 640 * 480 / (r['ms_per_step'] * 1e-3)) <= 1e-6 * r['value']
    assert r['dtype'].startswith('f32')
    shapes = {'depth': (480, 640), 'uncertainty': (480, 640), 'color': (480, 640, 3)}
    for name, shape in shapes.items():
        a = np.load(os.path.join(str(tmp_path), name + '.npy'))
        assert a.shape == shape and a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name     # f64 stays f64
    assert (np.load(os.path.join(str(tmp_path), 'depth.npy')) > 0).any()

