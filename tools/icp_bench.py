"""The depth ICP (icp.DepthICP, csrc/adfp_icp.h) at Replica's frame, 680 x 1200, in the room0 box-room volume (4/256 m voxels), from
a corner-facing pose inside the room with the guess 35 mm / 1.5 degrees off.  The sensor depth is the raycast at the true pose.

  raycast    the model's depth image from the guess (adfp_tsdf_raycast), what refine starts with
  normals    adfp_depth_normals for both images in one launch
  step_sN    one adfp_icp_step (the sums' launch and the solve's) over every N-th pixel of every N-th row, N = 4, 2, 1
  steps      begin, the ten steps of the default levels (4, 3, 3 at strides 4, 2, 1), end
  refine     DepthICP.refine as a whole: upload of the guess, copy of the sensor depth, raycast, normals, steps
  track10    ten TrackerIteration.step replays of 200 pixels after a new_frame: the tracking the refinement precedes

The RGB-D ICP (icp.RgbdICP, csrc/adfp_rgbd.h) on the same frame, the colour test_gpu_slam_run's rule at every pixel's world point, the
keyframe the scene seen from 36 mm / 27 mrad away (tests/rgbd_icp_ref.py's KEY_TWIST):

  frame_map      adfp_rgbd_frame_map of one frame
  joint_sN       one adfp_rgbd_step over every N-th pixel, beside step_sN
  promote        RgbdICP.promote: the map's copy and the pose's upload
  rgbd_refine    RgbdICP.refine as a whole, beside refine

The depth bilateral filter (icp.depth_bilateral, csrc/adfp_depthfilter.h) and DepthICP(bilateral={...}); the sensor depth of these
legs is the same frame through synthetic.sensor_depth's default noise model:

  filter_rN / filter_tum_rN      the filter's launch alone at radius N = 2, 3, on this frame and on TUM RGB-D's (480 x 640)
  refine_bilateral               DepthICP(bilateral={}).refine on the CLEAN frame, beside `refine`, the path before the filter: both go
                                 through all ten steps, so their difference is the filter's launch and what it changes in the steps
  refine_noisy                   DepthICP.refine without the filter on the noisy frame (a refinement that fails does nothing in its
                                 remaining steps, so a failed leg is short: read its status beside its time)
  refine_noisy_bilateral         DepthICP(bilateral={}).refine on the same frame (points and normals of the filtered image)
  refine_noisy_bilateral_raw_points    the same with points: False

Device events around each leg, median (min, max) of `--reps` repetitions after a warm-up; the legs alternate within a repetition.  No
thresholds: the numbers go into DESIGN.md sections 5.13, 5.13.1 and 5.13.2.

    python tools/icp_bench.py [--reps 7] [--json profiles/icp_bench.json] [--rgbd-json profiles/rgbd_icp_bench.json]
                              [--filter-json profiles/icp_filter_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import icp_ref                                                 # noqa: E402
import rgbd_icp_ref                                            # noqa: E402
import attentive_dfprior_amd as A                              # noqa: E402
from attentive_dfprior_amd import _lib, common, synthetic      # noqa: E402
from attentive_dfprior_amd.icp import DepthICP, RgbdICP, depth_bilateral        # noqa: E402
from attentive_dfprior_amd.tracking import TrackerIteration    # noqa: E402

DEV = 'cuda:0'
GEO = (680, 1200, 600.0, 600.0, 599.5, 339.5)                  # configs/Replica/replica.yaml
GEO_TUM = (480, 640, 517.3, 516.5, 318.6, 255.3)               # TUM RGB-D, freiburg1
CFG = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 48, 'N_surface': 16, 'N_importance': 0},
       'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=None)
    ap.add_argument('--rgbd-json', default=None)
    ap.add_argument('--filter-json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'icp_bench needs a GPU'
    assert a.reps >= 5, 'at least 5 repetitions'
    sc = synthetic.Scene('room0', device=DEV, grid_std_scale=20.0)
    sc.c['grid_high'] = sc.c['grid_high'] * 100
    sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy = GEO
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    for p in dec.parameters():
        p.requires_grad_(False)
    rend = A.Renderer(CFG, None, sc)
    tb = sc.tsdf_bnds.to(DEV)
    icp = DepthICP(sc.tsdf_volume, tb, *GEO, engine=rend._engine)
    P = sc.default_c2w(offset=(0.3, 0.2, 0.1), yaw=0.75, pitch=-0.6)
    G = torch.from_numpy((icp_ref.exp_se3(np.asarray(icp_ref.TWIST)) @ P.cpu().numpy().astype(np.float64)).astype(np.float32))
    sensor = icp.raycaster.render_depth(P, *GEO)
    color = torch.rand((GEO[0], GEO[1], 3), generator=torch.Generator().manual_seed(0)).to(DEV)
    cam = icp.refine(G, sensor).clone()
    rows = icp.last_stats().numpy()
    got = icp.c2w_out.cpu().numpy()
    e0, e1 = icp_ref.pose_error(G.numpy(), P.cpu().numpy()), icp_ref.pose_error(got, P.cpu().numpy())
    fused = TrackerIteration(rend, dec, sc.c, sc.tsdf_volume, tb, GEO[0], GEO[1], *GEO[2:], 20, 20)
    dev = torch.device(DEV)

    def one_step(stride):
        def fn():
            with _lib.on(dev) as L:
                icp._begin(icp.p_ref, L)
                icp._step((icp.depth, icp.normals), icp.p_ref, stride, 0, L)
        return fn

    def track10():
        fused.new_frame(cam, sensor, color)
        for _ in range(10):
            fused.step(200)

    # the RGB-D ICP on the same frame
    rgbd = RgbdICP(sc.tsdf_volume, tb, *GEO, engine=rend._engine)
    Pn = P.cpu().numpy()
    Kn = rgbd_icp_ref.key_pose(Pn)
    key_depth = icp.raycaster.render_depth(torch.from_numpy(Kn), *GEO)
    paint = lambda d, c2w: torch.from_numpy(rgbd_icp_ref.color_of(d.cpu().numpy(), c2w, *GEO[2:])).to(DEV)
    sensor_color, key_color = paint(sensor, Pn), paint(key_depth, Kn)
    rgbd.set_keyframe(torch.from_numpy(Kn), key_color, key_depth)
    rgbd.refine(G, sensor, sensor_color)
    rgbd_rows, rgbd_rgb, rgbd_got = rgbd.last_stats().numpy(), rgbd.last_rgb_stats().numpy(), rgbd.c2w_out.cpu().numpy()
    rgbd_e1 = icp_ref.pose_error(rgbd_got, Pn)
    rgbd_final = rgbd.c2w_out.clone()

    def joint_step(stride):
        def fn():
            with _lib.on(dev) as L:
                rgbd._begin(rgbd.p_ref, L)
                rgbd._rgbd_step(rgbd.maps[0], rgbd.normals, rgbd.depth[1], rgbd.p_ref, stride, 0, L)
        return fn

    def rgbd_refine():
        rgbd.set_keyframe(torch.from_numpy(Kn), key_color, key_depth)      # not timed apart: one frame_map launch and a pose upload
        rgbd.refine(G, sensor, sensor_color)

    rgbd_legs = {'frame_map': lambda: rgbd.frame_map(sensor_color, sensor, out=rgbd.maps[0]),
                 'joint_s4': joint_step(4), 'joint_s2': joint_step(2), 'joint_s1': joint_step(1),
                 'promote': lambda: rgbd.promote(rgbd_final), 'rgbd_refine': rgbd_refine}

    legs = {'raycast': lambda: icp.raycaster.render_depth(icp.p_ref, *GEO, out=icp.depth[1:2]),
            'normals': lambda: icp.compute_normals(icp.depth, out=icp.normals),
            'step_s4': one_step(4), 'step_s2': one_step(2), 'step_s1': one_step(1),
            'steps': icp.run_steps, 'refine': lambda: icp.refine(G, sensor), 'track10': track10}
    legs.update(rgbd_legs)

    # the bilateral filter alone and in front of the refinement, on the frame through the sensor model
    noisy = synthetic.sensor_depth(sensor, 0)
    tum_noisy = synthetic.sensor_depth(icp.raycaster.render_depth(P, *GEO_TUM), 1)
    filt_out, tum_out = torch.empty_like(noisy), torch.empty_like(tum_noisy)
    filt = DepthICP(sc.tsdf_volume, tb, *GEO, engine=rend._engine, bilateral={})
    filt_raw = DepthICP(sc.tsdf_volume, tb, *GEO, engine=rend._engine, bilateral={'points': False})
    plain = DepthICP(sc.tsdf_volume, tb, *GEO, engine=rend._engine)
    filter_legs = {'filter_r2': lambda: depth_bilateral(noisy, radius=2, out=filt_out), 'filter_r3': lambda: depth_bilateral(noisy, radius=3, out=filt_out),
                   'filter_tum_r2': lambda: depth_bilateral(tum_noisy, radius=2, out=tum_out),
                   'filter_tum_r3': lambda: depth_bilateral(tum_noisy, radius=3, out=tum_out),
                   'refine_bilateral': lambda: filt.refine(G, sensor), 'refine_noisy': lambda: plain.refine(G, noisy), 'refine_noisy_bilateral': lambda: filt.refine(G, noisy),
                   'refine_noisy_bilateral_raw_points': lambda: filt_raw.refine(G, noisy)}
    if a.filter_json:
        legs.update(filter_legs)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    res = {'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'frame': list(GEO[:2]), 'volume': list(sc.tsdf_volume.shape[2:][::-1]),
           'levels': {'strides': list(icp.strides), 'iters': list(icp.iters)},
           'begin_is_timed_with_each_step': True,
           'status': int(rows[-1, 5]), 'pairs_per_step': rows[:-1, 0].tolist(), 'pivot_ratio_min': float(rows[:-1, 2].min()),
           'error_before_m_rad': list(e0), 'error_after_m_rad': list(e1),
           'valid_sensor_normals': int((icp.normals[0] != 0).any(-1).sum()), 'valid_model_normals': int((icp.normals[1] != 0).any(-1).sum())}
    res.update({k: stats(v) for k, v in t.items()})
    res['refine_over_track10'] = res['refine']['median_ms'] / res['track10']['median_ms']
    for k in legs:
        print(f'{k:11s} {res[k]["median_ms"]:.3f} ({res[k]["min_ms"]:.3f}, {res[k]["max_ms"]:.3f}) ms', flush=True)
    print(f'status {res["status"]}, pairs {rows[0, 0]:.0f} .. {rows[-2, 0]:.0f}, error {e0[0] * 1e3:.1f} mm {np.degrees(e0[1]):.2f} deg -> '
          f'{e1[0] * 1e3:.2f} mm {np.degrees(e1[1]):.3f} deg; refine / ten tracking iterations = {res["refine_over_track10"]:.2f}')
    assert common.get_camera_from_tensor(cam).shape == (3, 4)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({k: v for k, v in res.items() if k not in rgbd_legs and k not in filter_legs}, f, indent=1)
            f.write('\n')
    if a.filter_json:
        fo = {k: res[k] for k in ('device', 'reps', 'frame', 'volume', 'levels', 'refine')}
        filt.refine(G, sensor)
        st = filt.last_stats().numpy()
        res['refine_bilateral'].update({'status': int(st[-1, 5]), 'pairs_per_step': st[:-1, 0].tolist(),
                                        'error_after_m_rad': list(icp_ref.pose_error(filt.c2w_out.cpu().numpy(), P.cpu().numpy()))})
        fo['refine'] = dict(fo['refine'], status=res['status'], pairs_per_step=res['pairs_per_step'], error_after_m_rad=res['error_after_m_rad'])
        fo.update({k: res[k] for k in filter_legs})
        Pn_ = P.cpu().numpy()
        for name, obj in (('refine_noisy', plain), ('refine_noisy_bilateral', filt), ('refine_noisy_bilateral_raw_points', filt_raw)):
            obj.refine(G, noisy)
            st = obj.last_stats().numpy()
            fo[name].update({'status': int(st[-1, 5]), 'pairs_per_step': st[:-1, 0].tolist(),
                             'error_after_m_rad': list(icp_ref.pose_error(obj.c2w_out.cpu().numpy(), Pn_)),
                             'valid_sensor_normals': int((obj.normals[0] != 0).any(-1).sum())})
        fo.update({'tum_frame': list(GEO_TUM[:2]), 'bilateral': dict(filt.bilateral), 'error_before_m_rad': list(e0),
                   'sensor_model': 'synthetic.sensor_depth defaults: sigma = 0.0012 + 0.0019 (z - 0.4)^2 m',
                   'sensor_depth_range_m': [float(noisy[noisy > 0].min()), float(noisy.max())],
                   'filter_share_of_refine': res['filter_r2']['median_ms'] / res['refine_bilateral']['median_ms'],
                   'refine_bilateral_over_refine': res['refine_bilateral']['median_ms'] / res['refine']['median_ms'],
                   'refine_bilateral_minus_refine_ms': res['refine_bilateral']['median_ms'] - res['refine']['median_ms']})
        with open(a.filter_json, 'w') as f:
            json.dump(fo, f, indent=1)
            f.write('\n')
    if a.rgbd_json:
        out = {k: res[k] for k in ('device', 'reps', 'frame', 'volume', 'levels', 'begin_is_timed_with_each_step', 'step_s4', 'step_s2', 'step_s1',
                                   'refine')}
        out.update({k: res[k] for k in rgbd_legs})
        out.update({'rgb_weight': rgbd.rgb_weight, 'rgb_tol': rgbd.rgb_tol, 'rgbd_refine_sets_the_keyframe_too': True,
                    'keyframe_distance_m_rad': list(icp_ref.pose_error(Kn, Pn)), 'status': int(rgbd_rows[-1, 5]),
                    'pairs_per_step': rgbd_rows[:-1, 0].tolist(), 'rgb_pairs_per_step': rgbd_rgb[:-1, 0].tolist(),
                    'pivot_ratio_min': float(rgbd_rows[:-1, 2].min()), 'error_before_m_rad': list(e0), 'error_after_m_rad': list(rgbd_e1),
                    'rgbd_refine_over_refine': res['rgbd_refine']['median_ms'] / res['refine']['median_ms']})
        with open(a.rgbd_json, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
