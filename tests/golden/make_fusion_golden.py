"""
Golden vectors of the REFERENCE's own TSDF-fusion kernel (the CUDA C string of src/fusion.py:69-142) for
tests/test_gpu_fusion.py::test_integrate_matches_the_reference_kernel: needs a GPU and the two builds oracle/build_ref_fusion.py
makes in oracle/_ref/ (`python oracle/build_ref_fusion.py` where the reference checkout is present).

    python tests/golden/make_fusion_golden.py [OUT]      ->  tests/golden/mini_ref_fusion.npz (or OUT)

Three frames of the mini scene (their colour / depth / K / pose stored as the inputs) integrated into one volume at each voxel size
of the test, launched like PyCUDA launches the kernel (src/fusion.py:146-154 / :226-251), once per build:
    v<i>_exact_{tsdf,weight,color}      as-written build (-ffp-contract=off), the whole volume -- or, for a volume too large to
                                        store, v<i>_exact_sha256: sha256 over the tsdf, weight and colour volumes' float32 bytes
    v<i>_contract_{tsdf,weight,color}   contracted build, the whole volume -- or at v<i>_sample (a seeded voxel sample)
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from attentive_dfprior_amd import synthetic, _lib               # noqa: E402
from attentive_dfprior_amd.fusion import TSDFVolume             # noqa: E402
from test_gpu_fusion import frames, _reference_launch_geometry as reference_launch_geometry, VOXELS, FULL_VOXELS, SAMPLE   # noqa: E402

OUT = os.path.join(HERE, 'mini_ref_fusion.npz')
DEV = 'cuda:0'


def ref_lib(name):
    lib = C.CDLL(os.path.join(ROOT, 'oracle', '_ref', name))
    lib.ref_fusion_integrate.restype = C.c_int
    lib.ref_fusion_integrate.argtypes = [C.c_void_p] * 10 + [C.c_int] * 5 + [C.c_void_p]
    return lib


def volume_sha256(t, w, c):
    h = hashlib.sha256()
    for a in (t, w, c):
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def main():
    libs = {'exact': ref_lib('libref_fusion_exact.so'), 'contract': ref_lib('libref_fusion_contract.so')}
    sc = synthetic.mini_scene(device=DEV)
    fr = frames(sc, 3)
    out = {}
    for k, (color, depth, K, pose) in enumerate(fr):
        out[f'frame{k}_color'], out[f'frame{k}_depth'], out[f'frame{k}_K'], out[f'frame{k}_pose'] = color, depth, K, pose
    st = _lib.current_stream(torch.device(DEV))
    for i, voxel in enumerate(VOXELS):
        vol = TSDFVolume(sc.bound.numpy(), voxel, device=DEV)
        dims = tuple(int(v) for v in vol._vol_dim)
        n = int(np.prod(dims))
        gx, gy, gz, loops = reference_launch_geometry(n)
        out[f'v{i}_dims'] = np.array(dims, np.int64)
        # + 1 element: the reference's bound check is `voxel_idx > N`, so thread N writes one element past the volume
        state = {name: (torch.full((n + 1,), -1.0, device=DEV), torch.zeros(n + 1, device=DEV), torch.zeros(n + 1, device=DEV))
                 for name in libs}
        for color, depth, K, pose in fr:
            packed = np.floor(color[..., 2].astype(np.float32) * 65536 + color[..., 1].astype(np.float32) * 256 + color[..., 0].astype(np.float32))
            im_h, im_w = depth.shape
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(DEV)            # noqa: E731
            args = [dev(vol._vol_dim.astype(np.float32)), dev(vol._vol_origin), dev(K), dev(pose),
                    dev(np.array([[k, vol._voxel_size, im_h, im_w, vol._trunc_margin, 1.0] for k in range(loops)], np.float32)), dev(packed), dev(depth)]
            for name, lib in libs.items():
                t, w, c = state[name]
                rc = lib.ref_fusion_integrate(t.data_ptr(), w.data_ptr(), c.data_ptr(), *[a.data_ptr() for a in args], loops, gx, gy, gz, 1024, st)
                assert rc == 0, rc
            torch.cuda.synchronize()
        vols = {name: [x[:n].cpu().numpy().reshape(dims) for x in s] for name, s in state.items()}
        if voxel in FULL_VOXELS:
            for name, (t, w, c) in vols.items():
                out[f'v{i}_{name}_tsdf'], out[f'v{i}_{name}_weight'], out[f'v{i}_{name}_color'] = t, w, c
        else:
            out[f'v{i}_exact_sha256'] = np.array(volume_sha256(*vols['exact']))
            idx = np.sort(np.random.default_rng(1234).choice(n, SAMPLE, replace=False)).astype(np.int64)
            out[f'v{i}_sample'] = idx
            for a, what in zip(vols['contract'], ('tsdf', 'weight', 'color')):
                out[f'v{i}_contract_{what}'] = a.reshape(-1)[idx]
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
