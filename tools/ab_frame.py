"""Interleaved A/B of two builds of libadfp.so in ONE process (same clocks, same allocator state, same lease):

  python tools/ab_frame.py --a tools/ab_libs/libadfp_parent.so --b attentive_dfprior_amd/libadfp.so [--rounds 7] [--steps 10]

Both libraries are loaded side by side (they are different files, so the loader keeps two copies with their own statics); every
round times, for A then for B, with device events:
  frame       bench.py's headline step (room0 640 x 480 render_img, 48 + 16 samples, caches cleared every step), ms per frame
  sample<N>   adfp_sample_rays alone on the first N rays of the frame (no relayout blocks in the launch), us per call:
              200 (a Tracker batch), 1 000, 5 000 (a Mapper batch), 16 384, 38 400 (1/8 frame), 100 000, 307 200 (the frame)
  low_color   adfp_decode_stage(LOW_COLOR) on a 100 000-ray batch (k_decode_lc16), ms per call
  mapper_bwd  adfp_render_backward (Engine.render_backward on a saved training forward) of 5 000 random rays of the frame x 64 samples,
              stage colour, every grid and parameter gradient wanted (the Mapper's iteration: the f16-split kernels), us per call
  ba_bwd      the same with the ray gradients wanted too (bundle adjustment: the exact kernels), us per call
  tracker_bwd the same entry at 200 rays x 64 samples with the ray gradients only (the Tracker: k_decode_bwd_h_pgrad3), us per call
Each library has its own Renderer and decoders (nothing one build packed is read by the other).  Give the same file twice (a copy
under another name) for the A/A spread of the process.  Prints one JSON line: per quantity and side the per-round values, median
and minimum, and the sha256 of the frame's three images per side."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                         # noqa: E402
import attentive_dfprior_amd as A                                    # noqa: E402
from attentive_dfprior_amd import synthetic, _lib                    # noqa: E402
from attentive_dfprior_amd.common import get_rays                    # noqa: E402


def load(path):
    _lib._lib = None
    _lib.LIB_PATH = os.path.abspath(path)
    return _lib.lib()


class Side(object):
    def __init__(self, path, scene, dev):
        self.path = path
        self.L = load(path)
        self.dec = A.DF()
        self.dec.load_state_dict(synthetic.seeded_state_dict(0))
        self.dec.bound = scene.bound
        self.dec = self.dec.to(dev)
        self.rend = A.Renderer(bench.CFG64, None, scene)

    def use(self):
        _lib._lib = self.L


def ev_time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--a', required=True)
    ap.add_argument('--b', required=True)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    scene, _, _ = bench.build_scene(A, synthetic, 'room0', dev, std_scale=bench.GRID_STD_SCALE, high_extra=bench.GRID_HIGH_EXTRA)
    tsdf_bnds = scene.tsdf_bnds.to(dev)
    c2w = scene.default_c2w(offset=(0.0, 0.0, 0.0), yaw=0.3, pitch=-0.1)
    gt_depth = scene.depth_image(c2w)
    ro, rd = get_rays(scene.H, scene.W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
    ro, rd, gd = ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), gt_depth.reshape(-1).contiguous().float()
    n_rays = ro.shape[0]
    z = torch.empty((n_rays, 64), dtype=torch.float64, device=dev)
    dmax = gd.max().reshape(1).contiguous()
    scratch = torch.zeros(64, dtype=torch.float32, device=dev)
    bound = _lib.Bound()
    for i in range(3):
        for j in range(2):
            bound[i][j] = float(scene.bound[i, j])
    st = _lib.current_stream(dev)
    sides = {'a': Side(args.a, scene, dev), 'b': Side(args.b, scene, dev)}
    NB = 100000

    def frame(s):
        s.rend._engine._grid_cache.clear()
        s.dec._packed.clear()
        return s.rend.render_img(scene.c, s.dec, c2w, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth=gt_depth)

    def sample(s, n):
        rc = s.L.adfp_sample_rays(_lib.ptr(ro), _lib.ptr(rd), _lib.ptr(gd), n, bound, 48, 16, 0, 0.0, None, _lib.ptr(dmax),
                                  _lib.ptr(z), _lib.ptr(scratch), st)
        assert rc == 0, rc

    # name -> rays, grids and parameters wanted, rays wanted
    BWD = {'mapper_bwd_us': (5000, True, False), 'ba_bwd_us': (5000, True, True), 'tracker_bwd_us': (200, False, True)}
    pick = torch.randperm(n_rays, generator=torch.Generator().manual_seed(4)).to(dev)

    def train_forward(s, n, params):
        """The saved state of a training forward on n rays and seeded cotangents for its backward."""
        eng, idx = s.rend._engine, pick[:n]
        flat = {k: params for k in ('low', 'high', 'color', 'att')}
        d, u, col, w, saved = eng.render_forward(s.dec, scene.c, ro[idx].contiguous(), rd[idx].contiguous(), gd[idx].contiguous(), scene.tsdf_volume,
                                                 tsdf_bnds, s.rend.bound, 'color', 48, 16, train=True, need_flat=flat)
        return saved, (torch.randn_like(d), torch.randn_like(col), torch.randn_like(w).reshape(n, -1))

    def backward(s, q, saved, cot):
        n, params, rays = BWD[q]
        want = {k: params for k in ('low', 'high', 'color', 'att')}
        return s.rend._engine.render_backward(s.dec, scene.c, scene.tsdf_volume, tsdf_bnds, s.rend.bound, 'color', saved, cot[0], None, cot[1], cot[2],
                                              want, want, rays)

    sizes = (200, 1000, 5000, 16384, 38400, 100000, n_rays)
    quantities = ('frame_ms', 'low_color_ms') + tuple(BWD) + tuple('sample%d_us' % n for n in sizes)
    res = {k: {q: [] for q in quantities} for k in sides}
    stage, trained = {}, {}
    with torch.no_grad():
        for k, s in sides.items():
            s.use()
            out = frame(s)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for t in out:
                h.update(t.float().contiguous().cpu().numpy().tobytes())
            sample(s, n_rays)
            torch.cuda.synchronize()
            h2 = hashlib.sha256(z.cpu().numpy().tobytes())
            res[k]['lib'] = os.path.basename(s.path)
            res[k]['frame_sha256'] = h.hexdigest()
            res[k]['z_vals_sha256'] = h2.hexdigest()
            # the fused low + colour launch on the first 100 000 rays of the frame
            sc, keep = s.rend._engine.scene(s.dec, scene.c, scene.tsdf_volume, tsdf_bnds, scene.bound, 'color', images='hg')
            apts = _lib.AdfpPoints()
            apts.mode, apts.n_points = _lib.PTS_RAYS, NB * 64
            apts.rays_o, apts.rays_d, apts.z_vals, apts.S = ro.data_ptr(), rd.data_ptr(), z.data_ptr(), 64
            stage[k] = (sc, keep, apts)
            trained[k] = {q: train_forward(s, BWD[q][0], BWD[q][1]) for q in BWD}
        raw = torch.empty((NB * 64, 4), dtype=torch.float32, device=dev)
        wb = torch.empty((NB * 64,), dtype=torch.float32, device=dev)
        cnt = torch.zeros((4,), dtype=torch.int32, device=dev)
        for rnd in range(args.rounds + 1):                      # round 0 is a warm-up and is dropped
            for k, s in sides.items():
                s.use()
                sc, keep, apts = stage[k]
                vals = {
                    'frame_ms': ev_time(lambda: frame(s), args.steps),
                    'low_color_ms': ev_time(lambda: s.L.adfp_decode_stage(C.byref(sc), C.byref(apts), 3, _lib.ptr(raw), _lib.ptr(wb),
                                                                          _lib.ptr(cnt[1:]), st), 5),
                }
                for q in BWD:
                    vals[q] = ev_time(lambda: backward(s, q, *trained[k][q]), 20) * 1e3
                for n in sizes:
                    vals['sample%d_us' % n] = ev_time(lambda: sample(s, n), 100 if n < 50000 else 20) * 1e3
                if rnd:
                    for q, v in vals.items():
                        res[k][q].append(round(v, 4))
    for k in sides:
        for q in quantities:
            v = sorted(res[k][q])
            res[k][q + '_median'] = v[len(v) // 2]
            res[k][q + '_min'] = v[0]
    res['source_hash'] = bench.source_hash()
    res['rounds'] = args.rounds
    print(json.dumps(res))


if __name__ == '__main__':
    main()
