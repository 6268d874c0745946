"""
Golden vectors of the Mapper's overlap keyframe selection (src/Mapper.py:160-222, Mapper.keyframe_selection_overlap).  src/Mapper.py
cannot be IMPORTED in the build container (it needs cv2 / colorama), so, like make_mapper_golden.py, this script reads the method's
own source lines from the reference and EXECUTES them as a method of a stub `self` (H .. cy of synthetic.mini_scene(), device
'cpu'), with the reference's own get_samples (src/common.py).  One namespace binding: `sorted` records `list_keyframe` (each
keyframe's percent_inside) and the method's `vertices` (the sample points, read from the calling frame) before sorting as the
built-in does.  Build container only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_keyframe_golden.py

  mapper_keyframes.npz, per case <c>:
    <c>.idx [pixels] int64        the pixel draw (torch.manual_seed(<c>.torch_seed), then the reference's one torch.randint)
    <c>.depth [H,W], <c>.c2w [4,4] the current frame;  <c>.poses [K,4,4] the keyframes' est_c2w
    <c>.points [pixels*16,3] f32  the sample points (`vertices`)
    <c>.percent [K] f64           each keyframe's percent_inside;  <c>.ambiguous [K] int  points within 1e-3 px of an image-edge
                                  bound or within 1e-9 of z = 0 (f64, keyframes.overlap_ambiguity)
    <c>.sel.<s>.<k>               the selected list for np.random.seed(s) and k
"""
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from attentive_dfprior_amd import synthetic                    # noqa: E402
from attentive_dfprior_amd.keyframes import overlap_ambiguity  # noqa: E402

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
NP_SEEDS = (0, 1, 7)
PIXELS, N_SAMPLES = 100, 16


def ref_method():
    src = open(os.path.join(REF, 'src', 'Mapper.py')).read().split('\n')
    block = src[159:222]
    assert 'def keyframe_selection_overlap(self, gt_color, gt_depth, c2w, keyframe_dict, k, N_samples=16, pixels=100):' in block[0]
    assert 'return selected_keyframe_list' in block[-1]
    spec = importlib.util.spec_from_file_location('ref_common', os.path.join(REF, 'src', 'common.py'))
    ref_common = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_common)
    record = {}

    def recording_sorted(items, **kw):
        record['percent'] = np.array([d['percent_inside'] for d in items], dtype=np.float64)
        record['points'] = np.array(sys._getframe(1).f_locals['vertices'], dtype=np.float32)
        return sorted(items, **kw)

    ns = {'torch': torch, 'np': np, 'get_samples': ref_common.get_samples, 'sorted': recording_sorted}
    exec(textwrap.dedent('\n'.join(block)), ns)
    return ns['keyframe_selection_overlap'], record


def case_poses(sc, c2w, rng):
    """K = 48: the current pose, three poses facing away, a triple and a pair of duplicates, random poses around the box."""
    poses = [c2w.clone()]
    for yaw in (0.3 + np.pi, 0.3 + 0.9 * np.pi, 0.3 - 0.95 * np.pi):
        poses.append(sc.default_c2w(offset=(0.0, 0.0, 0.0), yaw=float(yaw), pitch=-0.1))
    dup = sc.default_c2w(offset=(0.04, -0.02, 0.03), yaw=0.4, pitch=-0.05)
    poses += [dup, dup.clone(), dup.clone()]
    dup2 = sc.default_c2w(offset=(-0.05, 0.01, 0.02), yaw=0.2, pitch=-0.15)
    while len(poses) < 48:
        off = tuple(float(v) for v in rng.uniform(-0.25, 0.25, 3))
        poses.append(sc.default_c2w(offset=off, yaw=float(0.3 + rng.uniform(-0.6, 0.6)), pitch=float(rng.uniform(-0.4, 0.3))))
        if len(poses) in (20, 33):
            poses.append(dup2.clone())
    return poses[:48]


def main():
    fn, record = ref_method()
    sc = synthetic.mini_scene()
    stub = types.SimpleNamespace(H=sc.H, W=sc.W, fx=sc.fx, fy=sc.fy, cx=sc.cx, cy=sc.cy, device='cpu')
    rng = np.random.default_rng(5)
    out = {'source_lines': np.array('src/Mapper.py:160-222'),
           'intrinsics': np.array([sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy], dtype=np.float64),
           'pixels': np.array(PIXELS), 'n_samples': np.array(N_SAMPLES), 'np_seeds': np.array(NP_SEEDS)}
    cases = []
    c2w = sc.default_c2w()
    cases.append(('main', c2w, sc.depth_image(c2w, zero_band=0.0), case_poses(sc, c2w, rng), 11))
    c2w = sc.default_c2w(offset=(0.1, -0.05, 0.0), yaw=0.5, pitch=-0.2)
    cases.append(('zeros', c2w, sc.depth_image(c2w, zero_band=0.4), case_poses(sc, c2w, rng), 12))
    c2w = sc.default_c2w(offset=(-0.1, 0.05, 0.05), yaw=0.1, pitch=0.0)
    rand = []
    for _ in range(40):
        off = tuple(float(v) for v in rng.uniform(-0.3, 0.3, 3))
        rand.append(sc.default_c2w(offset=off, yaw=float(0.1 + rng.uniform(-0.5, 0.5)), pitch=float(rng.uniform(-0.3, 0.3))))
    cases.append(('random', c2w, sc.depth_image(c2w, zero_band=0.1), rand, 13))
    cases.append(('empty', c2w, sc.depth_image(c2w, zero_band=0.1), [], 14))
    out['cases'] = np.array([c[0] for c in cases])
    for name, c2w, depth, poses, tseed in cases:
        color = torch.rand(sc.H, sc.W, 3, generator=torch.Generator().manual_seed(tseed))
        keyframe_dict = [{'est_c2w': p.clone(), 'idx': i} for i, p in enumerate(poses)]
        P = torch.stack(poses).numpy() if poses else np.zeros((0, 4, 4), np.float32)
        torch.manual_seed(tseed)
        idx = torch.randint(sc.H * sc.W, (PIXELS,)).numpy()
        out[f'{name}.torch_seed'] = np.array(tseed)
        out[f'{name}.idx'], out[f'{name}.depth'], out[f'{name}.c2w'], out[f'{name}.poses'] = idx, depth.numpy(), c2w.numpy(), P
        n_sel = None
        for s in NP_SEEDS:
            for k in (0, 3, 8, 1000):
                torch.manual_seed(tseed)
                np.random.seed(s)
                sel = fn(stub, color, depth, c2w, keyframe_dict, k)
                out[f'{name}.sel.{s}.{k}'] = np.array(sel, dtype=np.int64)
                if k == 1000:
                    n_sel = len(sel)
        out[f'{name}.points'], out[f'{name}.percent'] = record['points'], record['percent']
        amb = overlap_ambiguity(record['points'], P, sc.fx, sc.fy, sc.cx, sc.cy, sc.H, sc.W)
        out[f'{name}.ambiguous'] = amb
        cnt = np.rint(record['percent'] * PIXELS * N_SAMPLES).astype(np.int64)
        print(name, 'K', len(poses), 'selected', n_sel, 'counts', cnt.tolist(), 'ambiguous', int(amb.sum()), 'in', int((amb > 0).sum()))
    np.savez_compressed(os.path.join(OUT, 'mapper_keyframes.npz'), **out)


if __name__ == '__main__':
    main()
