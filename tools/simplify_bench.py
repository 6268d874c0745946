"""Mesh simplification (mesh.simplify_vertex_clustering) on the mesh of tools/mesh_bench.py: the synthetic room0 at 512^3 after the
Mesher's clean-up.  Voxels of 1x, 2x and 4x the lattice spacing and one voxel as large as the model (one cell holds every vertex:
the degenerate request), both contractions.  Per case: the device call (plan + read-back of the totals + emit) beside the tests'
numpy statement of the same rules on the host (tests/simplify_ref.py), both in this one run, alternating, wall clock with a device
synchronisation on both ends (median, min, spread); the output sizes, whether the two sides agree, and the accuracy / completion /
completion ratio of the simplified mesh against the unsimplified one with the package's own 3D metric (recon.py: 200 000 seeded
surface samples each, no alignment -- the two meshes share a frame).  No thresholds.  One JSON line.

    python tools/simplify_bench.py [--res 512] [--reps 5] > profiles/simplify_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')]

import attentive_dfprior_amd as A                     # noqa: E402
from attentive_dfprior_amd import mesh, synthetic      # noqa: E402
from attentive_dfprior_amd.mesher import Mesher        # noqa: E402
from attentive_dfprior_amd.recon import NNIndex, draw_uniforms, metric_sums, sample_surface      # noqa: E402
from mesh_bench import DEV, Slam, against              # noqa: E402
import simplify_ref                                    # noqa: E402

SAMPLES = 200000


def cleaned_room(res):
    """(verts, faces) on the device: mesh_bench's scene through lattice, hull fill, marching cubes, seen mask, component clean-up."""
    sc = synthetic.Scene('room0', device=DEV, grid_std_scale=30.0)
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(seed=0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 32, 'N_surface': 16, 'N_importance': 0},
           'scale': 1, 'occupancy': True,
           'meshing': {'resolution': res, 'level_set': 0.0, 'clean_mesh_bound_scale': 1.02,
                       'remove_small_geometry_threshold': 0.2, 'color_mesh_extraction_method': 'direct_point_query',
                       'get_largest_components': False, 'depth_test': False},
           'mapping': {'marching_cubes_bound': sc.bound.tolist()}}
    slam = Slam()
    slam.bound = sc.bound
    slam.vol_bnds = slam.tsdf_bnds = sc.tsdf_bnds.to(DEV)
    slam.verbose = False
    slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy
    slam.renderer = A.Renderer(cfg, None, slam)
    kfs = []
    for k in range(4):
        c2w = sc.default_c2w(offset=(0.1 * k, -0.05 * k, 0.0), yaw=1.2 * k, pitch=-0.1)
        kfs.append({'est_c2w': c2w.cpu(), 'depth': sc.depth_image(c2w).cpu(), 'color': torch.zeros(sc.H, sc.W, 3)})
    est = torch.stack([kf['est_c2w'] for kf in kfs])
    m = Mesher(cfg, None, slam)
    with torch.no_grad():
        xyz = m.get_grid_uniform(res)['xyz']
        z, ax = m.lattice(sc.c, dec, sc.tsdf_volume, xyz, DEV)
        mesh.hull_fill(z, ax, m.get_bound_planes(kfs, 1), 100.)
        sp = tuple(x[2] - x[1] for x in xyz)
        v, f, _ = mesh.marching_cubes(z, 0.0, sp, tuple(x[0] for x in xyz))
        seen = m.seen_mask(v, kfs, est, 0, DEV)
        v, f = mesh._clean_components(v, f, seen.to(torch.uint8), m.remove_small_geometry_threshold, False)
    return v, f, float(max(sp))


def metric(base, simple, seed=0):
    """accuracy (cm), completion (cm), completion ratio (% within 5 cm) of `simple` against `base`, recon_eval.metric_3d's sums"""
    g = torch.Generator().manual_seed(seed)
    us, ub = draw_uniforms(SAMPLES, DEV, g), draw_uniforms(SAMPLES, DEV, g)
    rec, _ = sample_surface(simple[0], simple[1], u_face=us[0], u_bary=us[1], device=DEV)
    gt, _ = sample_surface(base[0], base[1], u_face=ub[0], u_bary=ub[1], device=DEV)
    d_acc = NNIndex(gt, DEV).query(rec)[0]
    d_comp = NNIndex(rec, DEV).query(gt)[0]
    s_acc, _ = metric_sums(d_acc, 0.0)
    s_comp, c_comp = metric_sums(d_comp, 0.05)
    return {'accuracy_cm': round(s_acc / SAMPLES * 100, 5), 'completion_cm': round(s_comp / SAMPLES * 100, 5),
            'completion_ratio_pct': round(c_comp / SAMPLES * 100, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    v, f, spacing = cleaned_room(a.res)
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    extent = float(np.ptp(vn, 0).max())
    out = {'workload': f'synthetic room0, Mesher clean-up output at {a.res}^3', 'device': torch.cuda.get_device_name(0), 'reps': a.reps,
           'verts': int(v.shape[0]), 'faces': int(f.shape[0]), 'lattice_spacing': spacing, 'extent': extent, 'samples': SAMPLES,
           'workspace_bytes': int(mesh.lib().adfp_mesh_simplify_workspace_bytes(int(v.shape[0]), int(f.shape[0]))), 'cases': {}}
    # the metric's floor: the unsimplified mesh against itself, through the same two independent draws of surface samples
    out['mesh_against_itself'] = metric((v, f), (v, f))
    voxels = [('1x', spacing), ('2x', 2 * spacing), ('4x', 4 * spacing), ('model', 4 * extent)]
    for name, vs in voxels:
        for contraction in ('average', 'quadric'):
            h, d = {}, {}
            r = against(lambda: h.__setitem__('o', simplify_ref.simplify(vn, fn, vs, contraction)),
                        lambda: d.__setitem__('o', mesh._simplify_vertex_clustering(v, f, vs, contraction, None)),
                        a.reps if name != 'model' else max(1, a.reps // 2))
            (hv, hf, _), (dv, df, _) = h['o'], d['o']
            r['voxel'] = vs
            r['verts_out'], r['faces_out'] = int(dv.shape[0]), int(df.shape[0])
            r['faces_equal'] = bool(np.array_equal(hf, df.cpu().numpy()))
            r['max_position_difference'] = float(np.abs(hv.astype(np.float64) - dv.cpu().numpy()).max()) if len(hv) == dv.shape[0] and len(hv) else 0.0
            if df.shape[0]:
                r.update(metric((v, f), (dv, df)))
            out['cases'][f'{name}_{contraction}'] = r
            print(f'{name} {contraction}: host {r["host"]["median_ms"]} ms, device {r["device"]["median_ms"]} ms', file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
