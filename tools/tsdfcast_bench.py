"""The TSDF raycast (tsdf_raycast.TsdfRaycaster, csrc/adfp_tsdfcast.h) at the volumes and frames a run has: the room0 and office0
box rooms (4/256 m voxels: 0.73 and 1.5 GB) at 640 x 480 and at Replica's native 680 x 1200, one pose inside the room, half-voxel
steps.  Per scene and frame:

  skip      adfp_tsdf_raycast with the empty-space bitmap
  noskip    the same call with ADFP_CAST_NO_SKIP (the same image, byte for byte: checked before anything is timed)
  torch     the restatement of tests/tsdfcast_ref.py on the GPU: the marching loop over F.grid_sample, the baseline
  render    Renderer.render_img of the same frame with the raycast as gt_depth (stage colour, 32 + 16 samples): what the guide
            costs a novel view is skip / (skip + render)
  bricks    building the bitmap (once per volume)

Device events around each call, median (min, max) of `--reps` repetitions after a warm-up call; the legs alternate within a
repetition.  Also the lookups each leg made (the call's own counter, in a run of its own) and the kernel against the torch
restatement at full size (largest difference where both hit, pixels only one side hits).

    python tools/tsdfcast_bench.py [--reps 5] [--json profiles/tsdfcast_bench.json] [--scenes room0 office0] [--no-torch]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import tsdfcast_ref                                            # noqa: E402
import attentive_dfprior_amd as A                              # noqa: E402
from attentive_dfprior_amd import synthetic                    # noqa: E402
from attentive_dfprior_amd.tsdf_raycast import TsdfRaycaster   # noqa: E402

DEV = 'cuda:0'
# frame -> (H, W), (fx, fy, cx, cy): the synthetic scenes' 640 x 480 camera; configs/Replica/replica.yaml
FRAMES = {'640x480': ((480, 640), (577.6, 577.6, 319.5, 239.5)), 'replica': ((680, 1200), (600.0, 600.0, 599.5, 339.5))}


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2], 'min_ms': ms[0], 'max_ms': ms[-1], 'all_ms': ms}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def bench_frame(sc, rc, dec, name, hw, cam, reps, with_torch):
    H, W = hw
    geo = (H, W) + cam
    c2w = sc.default_c2w(yaw=0.7, pitch=-0.15)
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = geo
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
           'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}
    rend = A.Renderer(cfg, None, sc)
    tb = sc.tsdf_bnds.to(DEV)

    legs = {'skip': lambda: rc.render_depth(c2w, *geo), 'noskip': lambda: rc.render_depth(c2w, *geo, skip=False)}
    guide, n_skip = rc.render_depth(c2w, *geo, count=True)
    plain, n_plain = rc.render_depth(c2w, *geo, skip=False, count=True)
    same = bool((guide.view(torch.int32) == plain.view(torch.int32)).all())
    legs['render'] = lambda: rend.render_img(sc.c, dec, c2w, DEV, sc.tsdf_volume, tb, 'color', gt_depth=guide)
    res = {'frame': [H, W], 'step_voxels': 0.5, 'skip_equals_noskip_bytes': same, 'lookups_skip': n_skip, 'lookups_noskip': n_plain,
           'share_looked_up': n_skip / n_plain, 'lookups_per_ray_noskip': n_plain / (H * W), 'hits': int((guide > 0).sum()), 'pixels': H * W}
    if with_torch:
        legs['torch'] = lambda: tsdfcast_ref.raycast(sc.tsdf_volume, tb, c2w, *geo, device=DEV)
        ref = legs['torch']()
        both, one = (guide > 0) & (ref > 0), (guide > 0) != (ref > 0)
        res['against_torch'] = {'max_abs_diff_m': float((guide - ref).abs()[both].max()), 'one_sided_pixels': int(one.sum())}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    res.update({k: stats(v) for k, v in t.items()})
    res['noskip_over_skip'] = res['noskip']['median_ms'] / res['skip']['median_ms']
    res['guide_share_of_novel_view'] = res['skip']['median_ms'] / (res['skip']['median_ms'] + res['render']['median_ms'])
    if with_torch:
        res['torch_over_skip'] = res['torch']['median_ms'] / res['skip']['median_ms']
    line = ', '.join(f'{k} {res[k]["median_ms"]:.3f} ({res[k]["min_ms"]:.3f}, {res[k]["max_ms"]:.3f})' for k in legs)
    print(f'{sc.name} {name}: {line} ms; looked up {100 * res["share_looked_up"]:.1f} % of {res["lookups_per_ray_noskip"]:.0f} samples per ray; '
          f'bytes equal {same}; {res.get("against_torch")}', flush=True)
    return res


def bench_scene(name, reps, with_torch):
    sc = synthetic.Scene(name, device=DEV, grid_std_scale=20.0)
    sc.c['grid_high'] = sc.c['grid_high'] * 100
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    rc = TsdfRaycaster(sc.tsdf_volume, sc.tsdf_bnds.to(DEV))
    Z, Y, X = sc.tsdf_volume.shape[2:]
    rc._engine.tsdf_bricks(sc.tsdf_volume)
    build = []
    for _ in range(reps):
        rc.invalidate_tsdf()
        build.append(timed(lambda: rc._engine.tsdf_bricks(sc.tsdf_volume)))
    bricks = rc._engine.tsdf_bricks(sc.tsdf_volume)
    words = bricks.cpu().numpy().view('uint32')
    set_bits = int(sum(bin(int(w)).count('1') for w in words))
    n_bricks = ((X + 7) // 8) * ((Y + 7) // 8) * ((Z + 7) // 8)
    res = {'volume': [X, Y, Z], 'volume_bytes': 4 * X * Y * Z, 'bitmap_bytes': bricks.numel() * 4, 'bricks': n_bricks, 'bricks_set': set_bits,
           'bricks_build': stats(build), 'frames': {}}
    print(f'{name}: volume {X} x {Y} x {Z} ({res["volume_bytes"] / 1e6:.0f} MB), bitmap {res["bitmap_bytes"]} bytes, {set_bits} of {n_bricks} bricks set, '
          f'build {res["bricks_build"]["median_ms"]:.3f} ms', flush=True)
    for fname, (hw, cam) in FRAMES.items():
        res['frames'][fname] = bench_frame(sc, rc, dec, fname, hw, cam, reps, with_torch)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--scenes', nargs='+', default=['room0', 'office0'])
    ap.add_argument('--no-torch', action='store_true', help='leave the torch baseline out')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'tsdfcast_bench needs a GPU'
    assert a.reps >= 5, 'at least 5 repetitions'
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'scenes': {}}
    for name in a.scenes:
        res['scenes'][name] = bench_scene(name, a.reps, not a.no_torch)
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    ok = all(fr['skip_equals_noskip_bytes'] for s in res['scenes'].values() for fr in s['frames'].values())
    print('skip == noskip:', 'ok' if ok else 'FAILED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
