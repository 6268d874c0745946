"""
Golden vectors for the reference's src/tools/evaluate_scannet.py.  The script imports open3d, pyrender and trimesh at module level
(none is installed in the build container) and its dataset imports cv2.  This script puts STUB modules for those four into
sys.modules (as make_depth_golden.py does) and EXECUTES the reference's own code:
  * update_cam on configs/ScanNet/scene0050.yaml, loaded by the reference's own src/config.py;
  * get_pose over a tiny synthetic ScanNet folder in a temporary directory (23 frames; frame 10's pose is all -inf, frame 20's is
    partly non-finite) through the reference's own ScanNet dataset (its __getitem__'s image reads are stubbed: cv2.imread returns a
    blank image; only the poses are recorded);
  * refuse's control flow, with a stub renderer and a stub ScalableTSDFVolume that record the viewport, the camera intrinsics, the
    fix_pose output, the extrinsic handed to integrate (np.linalg.inv of the f32 pose), depth_scale, depth_trunc, the voxel length
    and sdf_trunc;
  * evaluate with the real sklearn KDTree and down_sample=None on two small point sets, and with down_sample=0.02, where the stub
    PointCloud.voxel_down_sample calls tests/refuse_ref.py's numpy oracle -- that part pins only the formulas around it.
Nothing is written under the reference (sys.dont_write_bytecode).  Build container only.

    python tests/golden/make_scannet_golden.py

mini_scannet.npz: cam (update_cam's six values), poses [n,4,4] (get_pose's), K, HW, refuse.* (the recorded calls), eval.* (the
point sets and the metrics).  scannet_signatures.json: inspect.signature of the six reference functions.
"""
import contextlib
import inspect
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get('ADFP_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
for p in (TESTS,):
    if p not in sys.path:
        sys.path.insert(0, p)

import refuse_ref  # noqa: E402

N_FRAMES = 23


def pose_of(i):
    """Frame i's pose file content (OpenCV camera-to-world)."""
    rng = np.random.default_rng(100 + i)
    a = rng.uniform(0, 2 * np.pi)
    m = refuse_ref.look_at((0.3 * np.cos(a), 0.3 * np.sin(a), 1.2), (2 * np.cos(a + 0.5), 2 * np.sin(a + 0.5), 0.8 + 0.1 * i))
    m[:3, 3] += rng.uniform(-0.01, 0.01, 3) + np.array([1.0 / 3.0, 2.0 / 7.0, 0.0])
    if i == 10:
        m = np.full((4, 4), -np.inf)
    if i == 20:
        m[1, 3] = np.nan
    return m


def write_tree(root):
    fr = os.path.join(root, 'frames')
    for d in ('color', 'depth', 'pose'):
        os.makedirs(os.path.join(fr, d), exist_ok=True)
    for i in range(N_FRAMES):
        open(os.path.join(fr, 'color', f'{i}.jpg'), 'wb').close()
        open(os.path.join(fr, 'depth', f'{i}.png'), 'wb').close()
        with open(os.path.join(fr, 'pose', f'{i}.txt'), 'w') as fh:
            fh.write('\n'.join(' '.join(repr(float(x)) for x in row) for row in pose_of(i)) + '\n')


def _stubs(log):
    cv2 = types.ModuleType('cv2')
    cv2.IMREAD_UNCHANGED = -1
    cv2.COLOR_BGR2RGB = 4
    cv2.imread = lambda path, *a: np.zeros((480, 640, 3), np.uint8) if path.endswith('.jpg') else np.zeros((480, 640), np.uint16)
    cv2.cvtColor = lambda img, code: img
    cv2.resize = lambda img, size, **k: np.zeros((size[1], size[0]) + img.shape[2:], img.dtype)
    cv2.undistort = lambda img, K, d: img

    trimesh = types.ModuleType('trimesh')
    pyrender = types.ModuleType('pyrender')

    class OffscreenRenderer(object):
        def __init__(self, width, height):
            log['renderer_init'] = (width, height)
            self.viewport_width, self.viewport_height = width, height

        def render(self, scene):
            log['viewport'].append((self.viewport_height, self.viewport_width))
            return None, np.zeros((self.viewport_height, self.viewport_width), np.float32)

    class Scene(object):
        def clear(self):
            pass

        def add(self, obj, pose=None):
            if pose is not None:
                log['gl_pose'].append(np.array(pose, np.float64))

    class IntrinsicsCamera(object):
        def __init__(self, fx, fy, cx, cy, **k):
            log['gl_cam'].append((float(fx), float(fy), float(cx), float(cy)))
    pyrender.OffscreenRenderer, pyrender.Scene, pyrender.IntrinsicsCamera = OffscreenRenderer, Scene, IntrinsicsCamera
    pyrender.Mesh = types.SimpleNamespace(from_trimesh=lambda m: m)

    open3d = types.ModuleType('open3d')

    class PinholeCameraIntrinsic(object):
        def __init__(self, width=None, height=None, fx=None, fy=None, cx=None, cy=None):
            self.args = (width, height, fx, fy, cx, cy)
            self.intrinsic_matrix = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)

    class PointCloud(object):
        def __init__(self):
            self.points = np.zeros((0, 3))

        def voxel_down_sample(self, vs):
            p = PointCloud()
            p.points = refuse_ref.voxel_down_sample(np.asarray(self.points), vs)[0]
            return p

    class ScalableTSDFVolume(object):
        def __init__(self, voxel_length, sdf_trunc, color_type):
            log['volume'] = (float(voxel_length), float(sdf_trunc))

        def integrate(self, rgbd, intrinsic, extrinsic):
            log['extrinsic'].append(np.array(extrinsic))
            log['o3d_intrinsic'].append(tuple(float(x) for x in intrinsic.args))

        def extract_triangle_mesh(self):
            return 'mesh'

    def create_from_color_and_depth(rgb, depth, depth_scale, depth_trunc, convert_rgb_to_intensity):
        log['rgbd'].append((float(depth_scale), float(depth_trunc), bool(convert_rgb_to_intensity)))
        return None
    open3d.camera = types.SimpleNamespace(PinholeCameraIntrinsic=PinholeCameraIntrinsic)
    open3d.geometry = types.SimpleNamespace(PointCloud=PointCloud, Image=lambda x: x,
                                            RGBDImage=types.SimpleNamespace(create_from_color_and_depth=create_from_color_and_depth))
    open3d.utility = types.SimpleNamespace(Vector3dVector=lambda x: np.asarray(x, np.float64))
    open3d.pipelines = types.SimpleNamespace(integration=types.SimpleNamespace(
        ScalableTSDFVolume=ScalableTSDFVolume, TSDFVolumeColorType=types.SimpleNamespace(RGB8=1)))
    return {'cv2': cv2, 'trimesh': trimesh, 'pyrender': pyrender, 'open3d': open3d}


@contextlib.contextmanager
def reference(log):
    saved = {k: sys.modules.get(k) for k in ('cv2', 'trimesh', 'pyrender', 'open3d')}
    sys.modules.update(_stubs(log))
    sys.dont_write_bytecode = True
    cwd = os.getcwd()
    sys.path.insert(0, REF)
    os.chdir(REF)
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location('ref_evaluate_scannet', os.path.join(REF, 'src', 'tools', 'evaluate_scannet.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        yield mod
    finally:
        os.chdir(cwd)
        sys.path.remove(REF)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def point_sets():
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, (400, 3))
    b = a[:300] + rng.normal(0, 0.03, (300, 3))
    return a, b


def main():
    log = {k: [] for k in ('viewport', 'gl_pose', 'gl_cam', 'extrinsic', 'o3d_intrinsic', 'rgbd')}
    out = {}
    with reference(log) as ref:
        from src import config
        cfg = config.load_config('configs/ScanNet/scene0050.yaml', 'configs/df_prior.yaml')
        cfg['device'] = 'cpu'
        out['cam'] = np.array(ref.update_cam(cfg), np.float64)
        with tempfile.TemporaryDirectory() as d:
            write_tree(d)
            args = types.SimpleNamespace(input_folder=d, output=None)
            import torch
            cuda = torch.Tensor.to
            torch.Tensor.to = lambda self, *a, **k: self                     # the dataset moves its tensors to cuda:0
            try:
                poses, K, H, W = ref.get_pose(cfg, args)
            finally:
                torch.Tensor.to = cuda
            out['poses'] = np.stack(poses)
            out['pose_dtype_f32'] = np.array(all(p.dtype == np.float32 for p in poses))
            out['K'], out['HW'] = np.asarray(K, np.float64), np.array([H, W])
            out['tree_poses'] = np.stack([pose_of(i) for i in range(N_FRAMES)])
            ref.refuse(None, poses, K, H, W, cfg)
        out['refuse.viewport'] = np.array(log['viewport'])
        out['refuse.gl_cam'] = np.array(log['gl_cam'])
        out['refuse.gl_pose'] = np.stack(log['gl_pose'])
        out['refuse.extrinsic'] = np.stack(log['extrinsic'])
        out['refuse.extrinsic_f32'] = np.array(all(e.dtype == np.float32 for e in log['extrinsic']))
        out['refuse.o3d_intrinsic'] = np.array(log['o3d_intrinsic'])
        out['refuse.rgbd'] = np.array(log['rgbd'])
        out['refuse.volume'] = np.array(log['volume'])
        a, b = point_sets()
        out['eval.a'], out['eval.b'] = a, b
        keys = ['Acc', 'Comp', 'Chamfer', 'Prec', 'Recal', 'F-score']
        Mesh = types.SimpleNamespace
        for name, ds in (('none', None), ('ds02', 0.02)):
            m = ref.evaluate(Mesh(vertices=a), Mesh(vertices=b), down_sample=ds)
            out[f'eval.{name}'] = np.array([float(m[k]) for k in keys])
        sigs = {n: str(inspect.signature(getattr(ref, n)))
                for n in ('nn_correspondance', 'evaluate', 'update_cam', 'get_pose', 'refuse', 'evaluate_mesh')}
    np.savez_compressed(os.path.join(OUT, 'mini_scannet.npz'), **out)
    with open(os.path.join(OUT, 'scannet_signatures.json'), 'w') as fh:
        json.dump(sigs, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
