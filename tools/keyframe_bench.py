"""The Mapper's two keyframe costs that grow with the sequence, device against host, at ScanNet's camera (640x480, the intrinsics of
configs/ScanNet/scannet.yaml) and seeded poses:

  1. overlap selection (Mapper.keyframe_selection_overlap, src/Mapper.py:160-222) at K = 10, 100, 1 000, 2 000 keyframes: the
     device drop-in (keyframes.keyframe_selection_overlap: draw, one launch, read-back of the K counts, host ranking) per call,
     synchronised, fed from a KeyframeStore prefix and (second column) from a keyframe_dict list, whose K poses it stacks; against
     a numpy restatement of the reference's per-keyframe loop on the same points and poses.  The counts of the two are checked
     against each other under the tests' rule (|difference| <= the keyframe's ambiguous points).
  2. the Mapper's ray batch per iteration, a window of 10 frames and 5 000 rays: get_samples_multi over KeyframeStore frames against
     the reference's pattern (host images .to(device) every iteration, get_samples per frame, torch.cat); the two batches are checked
     bit for bit under the same torch seed.

    python tools/keyframe_bench.py [--iters 50] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from attentive_dfprior_amd import common, keyframes as KF     # noqa: E402

H, W, FX, FY, CX, CY = 480, 640, 577.590698, 578.729797, 318.905426, 242.683609
DEV = 'cuda:0'


def scene(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    depth = (0.5 + 3.5 * torch.rand(H, W, generator=g)).float()
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([1.0, 0.5, 1.2])
    poses = []
    for _ in range(K):
        q = torch.randn(4, generator=g)
        q = q / q.norm()
        if q[0] < 0.8:                                   # mostly near the current view, some far off
            q = torch.tensor([0.9, 0.0, 0.0, 0.0]) + 0.25 * q
            q = q / q.norm()
        p = torch.eye(4)
        p[:3, :3] = common.quad2rotation(q[None])[0]
        p[:3, 3] = c2w[:3, 3] + (torch.rand(3, generator=g) - 0.5)
        poses.append(p)
    return depth, c2w, torch.stack(poses).float()


def numpy_loop(vertices, poses):
    """The reference's per-keyframe loop restated in numpy (f32 inverse, the 4x4 product, the f64 projection): counts [K]."""
    Kmat = np.array([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]])
    homo = np.concatenate([vertices, np.ones((len(vertices), 1), np.float32)], 1)[..., None]
    counts = []
    for p in poses:
        w2c = np.linalg.inv(p)
        cam = (w2c @ homo)[:, :3]
        cam[:, 0] *= -1
        uv = Kmat @ cam
        z = uv[:, -1:] + 1e-5
        uv = (uv[:, :2] / z).astype(np.float32)
        m = (uv[:, 0] < W - 20) & (uv[:, 0] > 20) & (uv[:, 1] < H - 20) & (uv[:, 1] > 20) & (z[:, :, 0] < 0)
        counts.append(int(m.sum()))
    return np.array(counts)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_selection(iters):
    rows = []
    for K in (10, 100, 1000, 2000):
        depth, c2w, poses = scene(K, seed=K)
        kd = [{'est_c2w': p.to(DEV)} for p in poses]
        depth_d, c2w_d = depth.to(DEV), c2w.to(DEV)
        torch.manual_seed(0)
        idx = torch.randint(H * W, (100,), device=DEV)
        dev_counts, pts = KF.keyframe_overlap_counts(idx, depth_d, c2w_d, poses.to(DEV), 16, H, W, FX, FY, CX, CY, return_points=True)
        vertices = pts.cpu().numpy()
        host_counts = numpy_loop(vertices, poses.numpy())
        amb = KF.overlap_ambiguity(vertices, poses.numpy(), FX, FY, CX, CY, H, W)
        diff = np.abs(dev_counts.cpu().numpy() - host_counts)
        ok = bool((diff <= amb).all())

        st = KF.KeyframeStore(H, W, DEV, capacity=K + 1)
        zd, zc = torch.zeros(H, W, device=DEV), torch.zeros(H, W, 3, device=DEV)      # the selection reads only the poses
        for n, p in enumerate(poses):
            st.append(n, zc, zd, p)

        def store_call():
            KF.keyframe_selection_overlap(None, depth_d, c2w_d, st[:K], 10, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, device=DEV)

        def dict_call():
            KF.keyframe_selection_overlap(None, depth_d, c2w_d, kd, 10, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, device=DEV)

        t_dev = timed(store_call, iters)
        t_dict = timed(dict_call, iters)
        reps = max(1, min(iters, 20000 // K))
        t0 = time.perf_counter()
        for _ in range(reps):
            numpy_loop(vertices, poses.numpy())
        t_np = (time.perf_counter() - t0) / reps
        rows.append({'K': K, 'device_ms': t_dev * 1e3, 'device_dict_ms': t_dict * 1e3, 'numpy_ms': t_np * 1e3, 'ratio': t_np / t_dev,
                     'counts_ok': ok, 'counts_differ': int((diff > 0).sum()), 'ambiguous_keyframes': int((amb > 0).sum())})
        print(f'selection K={K:5d}: device {t_dev * 1e3:7.3f} ms/call (from a keyframe_dict: {t_dict * 1e3:7.3f})  '
              f'numpy loop {t_np * 1e3:9.3f} ms/call  x{t_np / t_dev:7.1f}  '
              f'counts agree under the ambiguity rule: {ok} ({int((diff > 0).sum())} differ)', flush=True)
    return rows


def bench_batch(iters, window=10, rays=5000):
    n = rays // window
    g = torch.Generator().manual_seed(9)
    host = [(torch.rand(H, W, 3, generator=g), 0.5 + 3 * torch.rand(H, W, generator=g)) for _ in range(window)]
    poses = [torch.eye(4) for _ in range(window)]
    for p in poses:
        p[:3, 3] = torch.rand(3, generator=g)
    poses_d = [p.to(DEV) for p in poses]
    st = KF.KeyframeStore(H, W, DEV, capacity=window)
    for f, ((color, depth), p) in enumerate(zip(host, poses)):
        st.append(5 * f, color, depth, p)
    frames = [st.frame(i) for i in range(window)]

    def store_iter():
        return common.get_samples_multi(0, H, 0, W, n, H, W, FX, FY, CX, CY, frames, DEV)

    def reference_iter():
        parts = [common.get_samples(0, H, 0, W, n, H, W, FX, FY, CX, CY, p, d.to(DEV), c.to(DEV), DEV)
                 for (c, d), p in zip(host, poses_d)]
        return [torch.cat([q[k].float() for q in parts]) for k in range(4)]

    torch.manual_seed(3)
    a = store_iter()
    torch.manual_seed(3)
    b = reference_iter()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    t_store = timed(store_iter, iters)
    t_ref = timed(reference_iter, max(3, iters // 5))
    print(f'batch window={window} rays={rays}: store {t_store * 1e3:8.3f} ms/iter  host upload + per frame {t_ref * 1e3:8.3f} ms/iter  '
          f'x{t_ref / t_store:6.1f}  bit-identical: {same}', flush=True)
    return {'window': window, 'rays': rays, 'store_ms': t_store * 1e3, 'reference_ms': t_ref * 1e3, 'ratio': t_ref / t_store,
            'bit_identical': same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'keyframe_bench needs a GPU'
    res = {'selection': bench_selection(a.iters), 'batch': bench_batch(a.iters)}
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    ok = all(r['counts_ok'] for r in res['selection']) and res['batch']['bit_identical']
    print('parity:', 'ok' if ok else 'FAILED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
