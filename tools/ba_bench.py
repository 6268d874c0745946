"""What bundle adjustment costs per Mapper iteration (mapping.MapperIteration's BA mode against the same iteration without it).

The iteration is bench_train.py's: the room0-sized synthetic scene, 5 000 rays of 48 + 16 samples, the fused, graph-replayed
iteration -- here over a ten-frame window (500 pixels of each frame, drawn anew every iteration like Mapper.optimize_map does), once
per stage.  BA off samples with common.get_samples_multi and steps; BA on samples with MapperIteration.sample_ba (adfp_ba_head) and
steps (the backward also returns ray cotangents, adfp_ba_tail joins the sequence).  The two alternate in blocks inside one process,
each block timed with a host clock around a device synchronise; the head and tail launches alone are timed between two events.

  python tools/ba_bench.py [--iters 50] [--rounds 5] [--out profiles/ba_bench.json]

No threshold: the number to read is the ratio of the two iterations of the same session."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import attentive_dfprior_amd as A                                   # noqa: E402
from attentive_dfprior_amd import _lib, common, mapping, synthetic  # noqa: E402

STAGE_LR = {'low': dict(low=0.1, high=0.0, color=0.0, decoders=0.0, mlp=0.0),
            'high': dict(low=0.005, high=0.005, color=0.0, decoders=0.0, mlp=0.005),
            'color': dict(low=0.005, high=0.005, color=0.005, decoders=0.005, mlp=0.005)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rays', type=int, default=5000)
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--scene', default='room0')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ba_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/ba_bench.py measures on the GPU: none found')
    dev = torch.device('cuda:0')
    F, n = args.frames, args.rays // args.frames
    scene = synthetic.Scene(args.scene, device=dev, grid_std_scale=20.0)
    scene.c['grid_high'] = scene.c['grid_high'] * 100
    H, W, intr = scene.H, scene.W, (scene.fx, scene.fy, scene.cx, scene.cy)
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = scene.bound
    dec = dec.to(dev)
    for p in list(dec.low_decoder.parameters()) + list(dec.high_decoder.parameters()):
        p.requires_grad_(False)
    tsdf_bnds = scene.tsdf_bnds.to(dev)
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 48, 'N_surface': 16, 'N_importance': 0},
           'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}
    g = torch.Generator().manual_seed(0)
    frames = []
    for k in range(F):
        c2w = scene.default_c2w(offset=(0.05 * k, -0.03 * k, 0.0), yaw=0.3 + 0.2 * k, pitch=-0.1).float().contiguous()
        frames.append((c2w, scene.depth_image(c2w).float().contiguous(), torch.rand(H, W, 3, generator=g).to(dev)))
    cams = torch.stack([common.get_tensor_from_camera(c2w.cpu()) for c2w, _, _ in frames])
    free = [k != 0 for k in range(F)]
    c = {k: v.detach().clone() for k, v in scene.c.items()}
    it = mapping.MapperIteration(A.Renderer(cfg, None, scene), dec, c, None, scene.tsdf_volume, tsdf_bnds, STAGE_LR)

    def arm(ba):
        it.new_frame()
        if ba:
            it.set_ba(cams, free, 0.0002, frames, H, W, *intr)

    def block(ba, stage, iters):
        for _ in range(iters):
            batch = it.sample_ba(n) if ba else common.get_samples_multi(0, H, 0, W, n, H, W, *intr, frames, dev, out=it.input_buffers(F * n))
            it.step(*batch, stage)

    res = {'rays': F * n, 'frames': F, 'samples_per_ray': 64, 'iters_per_block': args.iters, 'rounds': args.rounds, 'scene': args.scene, 'stages': {}}
    for stage in ('low', 'high', 'color'):
        times = {False: [], True: []}
        for ba in (False, True):                                    # captures and warm-up of both modes
            arm(ba)
            block(ba, stage, 5)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for ba in (False, True):
                arm(ba)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                block(ba, stage, args.iters)
                torch.cuda.synchronize()
                times[ba].append((time.perf_counter() - t0) / args.iters * 1e3)
        off, on = statistics.median(times[False]), statistics.median(times[True])
        res['stages'][stage] = {'ms_per_iter_ba_off': off, 'ms_per_iter_ba_on': on, 'ratio_on_over_off': on / off,
                                'ba_off_blocks_ms': times[False], 'ba_on_blocks_ms': times[True]}
        print(json.dumps({'stage': stage, **{k: v for k, v in res['stages'][stage].items() if not k.endswith('blocks_ms')}}))

    # the head and the tail alone, between two events (the tail on the cotangents the last backward left is not kept: random ones)
    arm(True)
    N = F * n
    it.sample_ba(n)
    pix = it._ba_pix[N]
    g_o, g_d = torch.randn(N, 3, device=dev), torch.randn(N, 3, device=dev)
    ta = _lib.AdfpBaTailArgs()
    ta.n_frames, ta.n = F, n
    ta.fx, ta.fy, ta.cx, ta.cy = intr
    ta.pix_i, ta.pix_j, ta.g_rays_o, ta.g_rays_d = pix[0].data_ptr(), pix[1].data_ptr(), g_o.data_ptr(), g_d.data_ptr()
    ta.cam, ta.g_c2w, ta.g_cam, ta.free_flags, ta.step = it.ba_cam.data_ptr(), it.ba_g_c2w.data_ptr(), it.ba_g_cam.data_ptr(), it.ba_free.data_ptr(), 0
    st = _lib.current_stream(dev)

    def timed(fn, reps=200):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3
    with torch.cuda.device(dev):
        ha, _, keep = it._ba_head_args(n)
    res['head_us_per_call_back_to_back'] = timed(lambda: _lib.check(_lib.lib().adfp_ba_head(C.byref(ha), st), 'adfp_ba_head'))
    res['tail_us_per_call_back_to_back'] = timed(lambda: _lib.check(_lib.lib().adfp_ba_tail(C.byref(ta), st), 'adfp_ba_tail'))
    print(json.dumps({k: res[k] for k in ('head_us_per_call_back_to_back', 'tail_us_per_call_back_to_back')}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
