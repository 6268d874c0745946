"""Mesh views on the MI355X (attentive_dfprior_amd.render_mesh): what carrying the hit's identity costs, and the rest of a view.

On tools/recon_bench.py --2d's room (a 512^3 lattice, ~1 M faces) and one chunk of 100 views at 500 x 500:

  * render_depth against render_hits of the same build (depth + face + bary, and depth alone) -- the same walk, the same lanes;
  * the vertex-normal build, the shading pass over the hit images (each mode), and the whole MeshViews.render with the download of
    its rgb, as render_mesh() runs it;
  * --depth_only --root TREE: render_depth alone with the package of another checkout (its own libadfp.so), e.g. the parent commit;
    --parent FILE merges that run's JSON and records the ratios.

Device legs: one warm-up, then --reps repetitions between torch.cuda events, min / median / max; the legs of one invocation share
the process and the device.  Writes profiles/render_mesh_bench.json (or --out) and prints the same JSON line.

    python tools/render_mesh_bench.py [--reps 7] [--parent FILE] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
H = W = 500
CAM = (H, W, 300.0, 300.0, 249.5, 249.5)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'min_ms': round(min(ms), 4), 'median_ms': round(float(np.median(ms)), 4), 'max_ms': round(max(ms), 4)}


def wall(fn, reps):
    fn()
    s = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        s.append((time.perf_counter() - t0) * 1e3)
    return {'min_ms': round(min(s), 3), 'median_ms': round(float(np.median(s)), 3), 'max_ms': round(max(s), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--root', default=HERE, help='the checkout whose package (and libadfp.so) is measured')
    ap.add_argument('--depth_only', action='store_true', help='render_depth alone: all an older checkout has')
    ap.add_argument('--parent', help="JSON of a --depth_only run of the parent commit's checkout, merged into the result")
    ap.add_argument('--out', default=os.path.join(HERE, 'profiles', 'render_mesh_bench.json'))
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path[:0] = [root, os.path.join(root, 'tools')]
    import recon_bench                                                           # the room and the views of its --2d leg
    from attentive_dfprior_amd import _lib, mesh, raycast, recon_eval
    import tempfile

    out = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'root': os.path.relpath(root, HERE), 'views': a.views, 'H': H, 'W': W}
    v, f = recon_bench.room(a.res)
    vn = v.cpu().numpy()
    out['faces'], out['verts'] = int(f.shape[0]), int(v.shape[0])
    rng = np.random.default_rng(0)
    pc = np.stack([rng.uniform(-1.6, -1.0, 2000), rng.uniform(0.6, 1.1, 2000), np.full(2000, 0.9)], 1)
    with tempfile.TemporaryDirectory() as d:
        gt_p = os.path.join(d, 'gt.ply')
        mesh.write_ply(gt_p, vn, f.cpu().numpy())
        extents, transform = recon_eval.get_cam_position(gt_p)
    np.random.seed(0)
    import random
    random.seed(0)
    views, _ = recon_eval.sample_views(pc, extents, transform, a.views, device=DEV)
    c2w = np.stack(views)
    near = recon_eval.NEAR_FRACTION * float((vn.max(0) - vn.min(0)).max())
    bvh = raycast.MeshBVH(v, f, DEV)
    rays = a.views * H * W
    out['render_depth'] = timed(lambda: bvh.render_depth(c2w, *CAM, near, 20.0), a.reps)
    out['render_depth']['mrays_per_s'] = round(rays / (out['render_depth']['median_ms'] * 1e-3) / 1e6, 1)
    if not a.depth_only:
        from attentive_dfprior_amd import render_mesh
        out['render_hits'] = timed(lambda: bvh.render_hits(c2w, *CAM, near, 20.0), a.reps)
        out['render_hits_depth_alone'] = timed(lambda: bvh.render_hits(c2w, *CAM, near, 20.0, want=('depth',)), a.reps)
        out['render_depth_again'] = timed(lambda: bvh.render_depth(c2w, *CAM, near, 20.0), a.reps)       # drift within the run
        out['hits_over_depth'] = round(out['render_hits']['median_ms'] / out['render_depth']['median_ms'], 4)
        out['hits_depth_alone_over_depth'] = round(out['render_hits_depth_alone']['median_ms'] / out['render_depth']['median_ms'], 4)
        h = bvh.render_hits(c2w, *CAM, near, 20.0)
        assert torch.equal(h['depth'], bvh.render_depth(c2w, *CAM, near, 20.0))
        out['hit_share'] = round(float((h['face'] >= 0).float().mean()), 4)
        out['vertex_normals'] = timed(lambda: mesh.vertex_normals(v, f, DEV), a.reps)
        colors = torch.randint(0, 256, (int(v.shape[0]), 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
        mv = render_mesh.MeshViews(v, f, colors, DEV)
        for mode in _lib.SHADE_MODE:
            out[f'shade_{mode}'] = timed(lambda: mv.shade(h['face'], h['bary'], c2w, *CAM[2:], mode=mode), a.reps)
        out['shade_rgb_alone'] = timed(lambda: mv.shade(h['face'], h['bary'], c2w, *CAM[2:], want=('rgb',)), a.reps)
        del h
        out['meshviews_render_with_download'] = wall(lambda: mv.render(c2w, *CAM, mode='shaded')['rgb'].cpu(), a.reps)
        out['meshviews_build'] = wall(lambda: render_mesh.MeshViews(v, f, colors, DEV), max(1, a.reps // 2))
        if a.parent:
            with open(a.parent) as fh:
                p = json.load(fh)
            assert (p['faces'], p['views'], p['device']) == (out['faces'], out['views'], out['device'])
            out['parent_render_depth'] = p['render_depth']
            out['depth_over_parent_depth'] = round(out['render_depth']['median_ms'] / p['render_depth']['median_ms'], 4)
            out['hits_over_parent_depth'] = round(out['render_hits']['median_ms'] / p['render_depth']['median_ms'], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
