"""ScanNet mesh evaluation on the MI355X (attentive_dfprior_amd.evaluate_scannet / refusion).  One JSON line.

A ScanNet-sized synthetic case: a 7 x 5 x 3 m room with a crate (refuse_ref.scene at a 1.7 cm grid: ~1 M faces) as the
prediction, the same room at 3 cm as the ground truth, and 560 views at 460 x 620 (ScanNet's 480 x 640 less crop_edge 10) on a
ring inside the room.  Per stage, over `--reps` runs after a warm-up, median and range in ms (host clock around synchronised
calls): render (culled BVH depth), touch (marks + the compact unit list), integrate, extract (marching cubes + compaction), then
the two voxel downsamples, the NN queries (index builds included) and the metric sums of evaluate; and the whole evaluate_mesh
command on a temporary ScanNet tree.  The integration rate is reported as voxel-view updates per second (every voxel of a unit a
view touched counts once) and the bytes one chunk moves (the volume's touched units read and written once, the chunk's depth
images read from L2 / MALL).  The numpy oracle (tests/refuse_ref.py) runs on a reduced case (the GPU tests' room, 20 views at
30 x 40) next to the device pipeline on the same case.

    python tools/scannet_bench.py [--reps 3] [--views 560]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import refuse_ref as R                                                   # noqa: E402
from attentive_dfprior_amd import evaluate_scannet as E, mesh, recon, refusion   # noqa: E402

DEV = 'cuda:0'
H, W = 460, 620
CFG = {'cam': {'H': 480, 'W': 640, 'fx': 577.590698, 'fy': 578.729797, 'cx': 318.905426, 'cy': 242.683609, 'crop_edge': 10}}


def stats(ms):
    return {'median_ms': round(float(np.median(ms)), 3), 'min_ms': round(float(min(ms)), 3), 'max_ms': round(float(max(ms)), 3)}


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t) * 1e3


def case(n_views, step_pred=0.017, step_gt=0.03):
    pv, pf = R.scene(step=step_pred, shift=(0.02, -0.03, 0.0), size=(7.0, 5.0, 3.0), crate=((1.0, -1.5, -1.5), (2.2, -0.3, -0.6)))
    gv, gf = R.scene(step=step_gt, size=(7.0, 5.0, 3.0), crate=((1.0, -1.5, -1.5), (2.2, -0.3, -0.6)))
    poses = [p.astype(np.float32) for p in R.orbit_poses(n_views, radius=1.5, height=0.2, seed=4)]
    return (pv, pf), (gv, gf), poses


def bench_stages(pred, gt, poses, reps):
    m = E.LoadedMesh(*pred)
    m.faces = m.faces[:, ::-1].copy()
    _, _, fx, fy, cx, cy = E.update_cam(CFG)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    runs, info = [], {}
    refused = None
    for r in range(reps + 1):
        t = {}
        refused = E.refuse_chunked(m, poses, K, CFG, timings=t)
        if r:
            runs.append(t)
    out = {k: stats([t[k] for t in runs]) for k in ('render', 'touch', 'integrate', 'extract')}
    upd = runs[0]['voxel_view_updates']
    chunk = refusion.chunk_views(H, W)
    n_chunks = -(-len(poses) // chunk)
    out['integrate']['voxel_view_updates'] = upd
    out['integrate']['g_updates_per_s'] = round(upd / (out['integrate']['median_ms'] * 1e-3) / 1e9, 2)
    out['integrate']['units_listed_per_chunk'] = round(runs[0]['units_listed'] / n_chunks, 1)
    out['integrate']['bytes_per_chunk_volume'] = int(runs[0]['units_listed'] / n_chunks * 4096 * 16)   # tsdf + weight, read + write
    out['integrate']['bytes_per_chunk_depth'] = chunk * H * W * 4
    out['views_per_chunk'] = chunk
    info['refused_vertices'], info['refused_faces'] = int(refused.vertices.shape[0]), int(refused.faces.shape[0])
    box = refusion.UnitBox.around(m.vertices, E.VOXEL, E.SDF_TRUNC)
    info['box_voxels'] = int(np.prod(box.shape))
    pred_v = refused.vertices.to(torch.float64)
    gt_v = torch.from_numpy(E.LoadedMesh(*gt).vertices).to(DEV)
    ds, nn, met = [], [], []
    for r in range(reps + 1):
        (pd, _), a = wall(lambda: refusion.voxel_down_sample(pred_v, 0.02, DEV))
        (td, _), b = wall(lambda: refusion.voxel_down_sample(gt_v, 0.02, DEV))
        (d1, d2), c = wall(lambda: (recon.NNIndex(pd).query(td)[0], recon.NNIndex(td).query(pd)[0]))
        _, d = wall(lambda: (recon.metric_sums(d1, 0.05), recon.metric_sums(d2, 0.05)))
        if r:
            ds.append(a + b)
            nn.append(c)
            met.append(d)
    out['downsample'] = stats(ds)
    out['nn'] = stats(nn)
    out['metric'] = stats(met)
    info['downsampled'] = [int(pd.shape[0]), int(td.shape[0])]
    return out, info


def bench_cli(pred, gt, poses, reps):
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, 'configs', 'ScanNet'))
        with open(os.path.join(root, 'configs', 'df_prior.yaml'), 'w') as fh:
            fh.write('scale: 1\n')
        with open(os.path.join(root, 'configs', 'ScanNet', 's.yaml'), 'w') as fh:
            c = CFG['cam']
            fh.write(f"dataset: scannet\ncam:\n  H: {c['H']}\n  W: {c['W']}\n  fx: {c['fx']}\n  fy: {c['fy']}\n  cx: {c['cx']}\n"
                     f"  cy: {c['cy']}\n  crop_edge: 10\ndata:\n  input_folder: scene\n  id: 1\n")
        fr = os.path.join(root, 'scene', 'frames')
        os.makedirs(os.path.join(fr, 'color'))
        os.makedirs(os.path.join(fr, 'pose'))
        for i in range(10 * len(poses)):
            open(os.path.join(fr, 'color', f'{i}.jpg'), 'wb').close()
            mtx = poses[i // 10] if i % 10 == 0 else np.eye(4)
            with open(os.path.join(fr, 'pose', f'{i}.txt'), 'w') as fh:
                fh.write('\n'.join(' '.join(repr(float(x)) for x in row) for row in mtx) + '\n')
        md = os.path.join(root, 'output', 'scannet', 'scans', 'scene0001_00', 'mesh')
        os.makedirs(md)
        mesh.write_ply(os.path.join(md, 'final_mesh.ply'), *pred)
        gd = os.path.join(root, 'Datasets', 'scannet', 'GTmesh_lowres')
        os.makedirs(gd)
        with open(os.path.join(gd, '0001_00.obj'), 'w') as fh:
            fh.write(''.join(f'v {x!r} {y!r} {z!r}\n' for x, y, z in gt[0].tolist()))
            fh.write(''.join(f'f {a + 1} {b + 1} {c + 1}\n' for a, b, c in gt[1].tolist()))
        cwd, argv = os.getcwd(), sys.argv
        os.chdir(root)
        sys.argv = ['evaluate_scannet', 'configs/ScanNet/s.yaml']
        try:
            ms, metrics = [], None
            for r in range(reps + 1):
                metrics, t = wall(E.evaluate_mesh)
                if r:
                    ms.append(t)
        finally:
            os.chdir(cwd)
            sys.argv = argv
    return stats(ms), metrics


def bench_oracle():
    v, f = R.scene()
    f = f[:, ::-1].copy()
    poses = [p.astype(np.float32) for p in R.orbit_poses(20)]
    h, w, fx, fy, cx, cy = 30, 40, 32.0, 32.0, 19.6, 14.7
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    t = time.perf_counter()
    ts, wt, lo, dim, _ = R.refuse_tsdf(v, f, poses, K, h, w, fx, fy, cx, cy)
    R.extract_vertices(ts, wt, lo, 0.01)
    oracle_ms = (time.perf_counter() - t) * 1e3
    cfg = {'cam': {'H': h, 'W': w, 'fx': fx, 'fy': fy, 'cx': cx, 'cy': cy, 'crop_edge': 0}}
    m = E.LoadedMesh(v, f)
    E.refuse_chunked(m, poses, K, cfg)
    _, dev_ms = wall(lambda: E.refuse_chunked(m, poses, K, cfg))
    return {'case': '1.6 x 1.2 x 1 m room, 20 views at 30 x 40', 'oracle_refuse_ms': round(oracle_ms, 1),
            'device_refuse_ms': round(dev_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--views', type=int, default=560)
    ap.add_argument('--no_cli', action='store_true')
    a = ap.parse_args()
    pred, gt, poses = case(a.views)
    res = {'bench': 'scannet_eval', 'faces_pred': int(len(pred[1])), 'faces_gt': int(len(gt[1])), 'views': len(poses),
           'image': [H, W]}
    res['stages'], res['info'] = bench_stages(pred, gt, poses, a.reps)
    if not a.no_cli:
        res['evaluate_mesh'], metrics = bench_cli(pred, gt, poses, max(1, a.reps - 1))
        res['metrics'] = {k: round(v, 6) for k, v in metrics.items()}
    res['oracle_reduced'] = bench_oracle()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
