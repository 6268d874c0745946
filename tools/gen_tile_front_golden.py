"""Records tests/golden/tile_front.npz: what the cases of tests/tile_front_cases.py compute, in both math modes, with the library given
by --lib (default: the tree's).  Run ONCE on the GPU with the build of the commit BEFORE the tile fronts were reworked; the test
(tests/test_gpu_tile_front.py) holds every later build to these bits.

  python tools/gen_tile_front_golden.py [--lib tools/ab_libs/libadfp_parent.so] [--out tests/golden/tile_front.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import bench                                                         # noqa: E402
import attentive_dfprior_amd as A                                    # noqa: E402
from attentive_dfprior_amd import _lib                               # noqa: E402
import tile_front_cases as T                                         # noqa: E402

KEYS = ('depth', 'uncertainty', 'color', 'weight', 'raw', 'att_occ')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'tile_front.npz'))
    args = ap.parse_args()
    if args.lib:
        _lib._lib = None
        _lib.LIB_PATH = os.path.abspath(args.lib)
    L = _lib.lib()
    dev = torch.device('cuda:0')
    sc = T.Scene()
    cases = T.cases(sc)
    out = {'source_hash': np.array(bench.source_hash()), 'lib': np.array(os.path.basename(_lib.LIB_PATH))}
    for math in ('f16x3', 'f32'):
        os.environ['ADFP_MATH'] = math
        sc_dev, dec = T.device_scene(A, sc, dev)
        for name, case in cases.items():
            r = T.run_rays(A, L, sc_dev, dec, case, dev)
            print(f'{math} {name}: {case["ro"].shape[0]} rays x {case["ns"] + case["nf"]}, in-band {r["count"]}')
            out[f'{math}.{name}.count'] = np.array(r['count'])
            if name == 'many':
                out[f'{math}.{name}.sha256'] = np.array(T.digest(*[r[k] for k in KEYS]))
            else:
                for k in KEYS:
                    out[f'{math}.{name}.{k}'] = r[k]
        for k, v in T.run_points(A, sc_dev, dec, dev).items():
            out[f'{math}.points.{k}'] = v
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
