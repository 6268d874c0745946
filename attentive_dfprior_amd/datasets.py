"""
Drop-in for the reference's ``src/utils/datasets.py``: ``get_dataset``, ``dataset_dict``, ``BaseDataset``, ``Replica`` and ``ScanNet``
with the reference's constructor arguments, attributes and file layouts, and ``__getitem__`` returning ``(index, color, depth,
pose)`` on the device.  What the reference does to every frame on the host (``/ 255.`` into float64, ``cv2.resize`` on doubles, two
``F.interpolate`` passes for ``crop_size``, the edge crop, a float64 upload) is one launch of libadfp.so here
(``adfp_ingest_frames``, include/adfp.h "frame ingestion"): the decoded bytes go up as they are, 3 + 2 bytes per pixel.

``FrameIngest`` is the layer without files: decoded images in, device tensors out, one frame or a batch per launch.

Deviations from the reference, all deliberate:
  * the colour comes back as float32 unless ``color_dtype=torch.float64`` is asked for: every consumer of this package converts;
  * ``__getitem__`` returns a copy of the pose whose translation is scaled ONCE; the reference scales the stored pose in place on
    every access (src/utils/datasets.py:112).  The two agree at ``scale: 1``;
  * undistortion (``cam.distortion``) stays on the host and needs a caller-supplied ``undistort(img, K, dist)``;
  * a dataset built with ``device='cpu'`` (the reference's Mesher builds one for its length) has its paths, poses and length,
    but indexing it raises: the frames exist only on the GPU.
EXR depth, TUM's timestamp association and Azure's trajectory log are not built.  A dataset pickles (the reference hands it to
its Tracker and Mapper processes and to a DataLoader worker); each process builds its own FrameIngest on first use.
"""
import ctypes as C
import glob
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib
from ._lib import lib, check


def imread_cv2(path, unchanged=False):
    """cv2's decoder: colour as BGR."""
    import cv2
    return cv2.imread(path, cv2.IMREAD_UNCHANGED) if unchanged else cv2.imread(path)


def imread_pil(path, unchanged=False):
    """PIL's decoder: colour as RGB; a 16-bit PNG as the uint16 values it holds."""
    from PIL import Image
    with Image.open(path) as im:
        if not unchanged:
            return np.asarray(im.convert('RGB'))
        a = np.asarray(im)
    if a.dtype.kind in 'iu' and a.dtype != np.uint16 and a.ndim == 2:      # a 16-bit PNG opened as mode 'I'
        a = a.astype(np.uint16)
    return a


def _default_imread():
    """(imread(path, unchanged=False) -> numpy array, channel order of its colour images): cv2 when it imports, else PIL.  Both
    are module-level functions: a dataset is pickled into every process the reference starts."""
    try:
        import cv2  # noqa: F401
        return imread_cv2, 'bgr'
    except ImportError:
        return imread_pil, 'rgb'


class FrameIngest(object):
    """``ingest = FrameIngest(cfg['cam'], scale, device)``; ``color, depth = ingest(color_u8, depth_raw)`` for one frame,
    ``ingest.batch(colors, depths)`` for n frames in one launch ([n,H,W,3] and [n,H,W]).

    color_u8 [h,w,3] uint8 in `color_order`; depth_raw [H0,W0] uint16 (int16 storage is read as uint16) or float32.  Inputs may be
    numpy arrays, CPU tensors or device tensors.  Host inputs go through two pinned staging buffers used in turn, each guarded by
    an event, and a non_blocking copy on the current stream: a call waits at most for the copy that last read the buffer it is
    about to fill, never for the device.  ``out=(color, depth)`` takes contiguous destinations (for a batch: tensors with a leading
    n, or sequences of n per-frame tensors, e.g. frames of a KeyframeStore block)."""

    def __init__(self, cfg_cam, scale, device, color_order='rgb', color_dtype=torch.float32):
        if color_order not in _lib.COLOR_ORDER:
            raise ValueError(f'color_order {color_order!r}: one of {sorted(_lib.COLOR_ORDER)}')
        if color_dtype not in (torch.float32, torch.float64):
            raise ValueError(f'color_dtype {color_dtype}: torch.float32 or torch.float64')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'FrameIngest on {self.device}: attentive_dfprior_amd runs only on an MI355X through libadfp.so; '
                               'there is no CPU fallback.')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.scale = float(scale)
        self.png_depth_scale = float(cfg_cam['png_depth_scale'])
        crop = cfg_cam.get('crop_size')
        self.crop_size = (int(crop[0]), int(crop[1])) if crop else None
        self.crop_edge = int(cfg_cam['crop_edge'])
        self.color_order = color_order
        self.color_dtype = color_dtype
        self._frame_hw = (int(cfg_cam['H']), int(cfg_cam['W'])) if 'H' in cfg_cam and 'W' in cfg_cam else None
        self._staging = [None, None]                 # pinned uint8 buffers
        self._events = [None, None]                  # recorded after the copy that read the buffer
        self._turn = 0

    # ---- geometry
    def _geom(self, color_hw, depth_hw, depth_f32):
        ch, cw = self.crop_size or (0, 0)
        return _lib.AdfpIngestGeom(color_hw[0], color_hw[1], depth_hw[0], depth_hw[1], ch, cw, self.crop_edge,
                                   _lib.COLOR_ORDER[self.color_order], int(depth_f32), int(self.color_dtype == torch.float64),
                                   self.png_depth_scale, self.scale)

    def out_shape_for(self, depth_hw):
        """(H, W) of the tensors a depth image of depth_hw comes back as (adfp_ingest_out_shape)."""
        H, W = C.c_int(), C.c_int()
        check(lib().adfp_ingest_out_shape(C.byref(self._geom(depth_hw, depth_hw, False)), C.byref(H), C.byref(W)), 'adfp_ingest_out_shape')
        return H.value, W.value

    @property
    def out_shape(self):
        """(H, W) for the frame of cfg cam.H, cam.W (the size of the dataset's depth images)."""
        if self._frame_hw is None:
            raise ValueError('cfg cam has no H, W: ask out_shape_for(depth_hw)')
        return self.out_shape_for(self._frame_hw)

    # ---- inputs
    @staticmethod
    def _as_list(x):
        if isinstance(x, (list, tuple)):
            return list(x)
        return [x[i] for i in range(x.shape[0])]

    @staticmethod
    def _kind(x, what):
        """('color' | 'u16' | 'f32') after a dtype check."""
        dt = str(x.dtype).replace('torch.', '')
        if what == 'color':
            if dt != 'uint8' or x.ndim != 3 or x.shape[-1] != 3:
                raise ValueError(f'colour image: uint8 [h,w,3] expected, got {dt} {tuple(x.shape)}')
            return 'color'
        if x.ndim != 2 or dt not in ('uint16', 'int16', 'float32'):
            raise ValueError(f'depth image: uint16 or float32 [h,w] expected, got {dt} {tuple(x.shape)}')
        return 'f32' if dt == 'float32' else 'u16'

    @staticmethod
    def _host_bytes(x):
        """A flat uint8 numpy view of a host image."""
        if torch.is_tensor(x):
            return x.contiguous().view(torch.uint8).reshape(-1).numpy()
        return np.ascontiguousarray(x).reshape(-1).view(np.uint8)

    def _upload(self, host):
        """host: flat uint8 arrays.  One pinned buffer, one copy; returns the device buffer and each array's offset in it."""
        offs, total = [], 0
        for h in host:
            offs.append(total)
            total += (h.size + 255) // 256 * 256
        k = self._turn
        self._turn ^= 1
        if self._events[k] is not None:
            self._events[k].synchronize()            # the copy that last read this buffer
        if self._staging[k] is None or self._staging[k].numel() < total:
            self._staging[k] = torch.empty(total, dtype=torch.uint8).pin_memory()
        stage = self._staging[k].numpy()
        for h, o in zip(host, offs):
            stage[o:o + h.size] = h
        dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev.copy_(self._staging[k][:total], non_blocking=True)
        if self._events[k] is None:
            self._events[k] = torch.cuda.Event()
        self._events[k].record(torch.cuda.current_stream(self.device))
        return dev, offs

    def _dest(self, out, n, H, W, single):
        """Per-frame destination tensors (colour list, depth list) and what the call returns."""
        if out is None:
            co = torch.empty((n, H, W, 3), dtype=self.color_dtype, device=self.device)
            do = torch.empty((n, H, W), dtype=torch.float32, device=self.device)
            return list(co), list(do), ((co[0], do[0]) if single else (co, do))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError('out: a pair (color, depth)')
        dests = []
        for o, shape, dtype, name in ((out[0], (H, W, 3), self.color_dtype, 'color'), (out[1], (H, W), torch.float32, 'depth')):
            if single:
                frames = [o]
            elif torch.is_tensor(o):
                if o.dim() != len(shape) + 1 or o.shape[0] != n:
                    raise ValueError(f'out {name}: shape {(n,) + shape} expected, got {tuple(o.shape)}')
                frames = list(o)
            else:
                frames = list(o)
                if len(frames) != n:
                    raise ValueError(f'out {name}: {n} frames expected, got {len(frames)}')
            for f in frames:
                if not torch.is_tensor(f) or tuple(f.shape) != shape or f.dtype != dtype or f.device != self.device or not f.is_contiguous():
                    got = (tuple(f.shape), f.dtype, f.device) if torch.is_tensor(f) else type(f)
                    raise ValueError(f'out {name}: a contiguous {dtype} tensor of shape {shape} on {self.device} expected, got {got}')
            dests.append(frames)
        return dests[0], dests[1], (out[0], out[1])

    # ---- calls
    def __call__(self, color_u8, depth_raw, out=None):
        return self._run([color_u8], [depth_raw], out, True)

    def batch(self, colors, depths, out=None):
        return self._run(self._as_list(colors), self._as_list(depths), out, False)

    def _run(self, colors, depths, out, single):
        n = len(colors)
        if n != len(depths):
            raise ValueError(f'{n} colour images, {len(depths)} depth images')
        if n == 0:
            raise ValueError('no frames')
        kinds = {self._kind(d, 'depth') for d in depths}
        for c in colors:
            self._kind(c, 'color')
        color_hw, depth_hw = tuple(colors[0].shape[:2]), tuple(depths[0].shape)
        if len(kinds) != 1 or any(tuple(c.shape[:2]) != color_hw for c in colors) or any(tuple(d.shape) != depth_hw for d in depths):
            raise ValueError('the frames of a batch share their shapes and depth dtype')
        geom = self._geom(color_hw, depth_hw, kinds == {'f32'})
        H, W = self.out_shape_for(depth_hw)
        cdst, ddst, result = self._dest(out, n, H, W, single)
        # sources: device tensors as they are, host images through one staging buffer
        srcs, host, keep = [], [], []
        for x in colors + depths:
            if torch.is_tensor(x) and x.is_cuda:
                if x.device != self.device:
                    raise ValueError(f'input on {x.device}, this FrameIngest is on {self.device}')
                x = x.contiguous()
                keep.append(x)
                srcs.append(x.data_ptr())
            else:
                srcs.append(None)
                host.append(self._host_bytes(x))
        with _lib.device_guard(self.device):
            if host:
                dev, offs = self._upload(host)
                it = iter(offs)
                srcs = [s if s is not None else dev.data_ptr() + next(it) for s in srcs]
            stream = _lib.current_stream(self.device)
            for j0 in range(0, n, _lib.INGEST_MAX_JOBS):
                m = min(_lib.INGEST_MAX_JOBS, n - j0)
                jobs = (_lib.AdfpIngestJob * m)(*[_lib.AdfpIngestJob(srcs[j], srcs[n + j], cdst[j].data_ptr(), ddst[j].data_ptr())
                                                  for j in range(j0, j0 + m)])
                check(lib().adfp_ingest_frames(C.byref(geom), m, jobs, stream), 'adfp_ingest_frames')
        return result


class BaseDataset(Dataset):
    """The reference's BaseDataset (src/utils/datasets.py:51-113).  Trailing keyword extensions: `imread(path, unchanged=False)`
    replaces the decoder (then `color_order` must say which channel order it returns; a picklable callable if the dataset
    goes to another process), `undistort(img, K, dist)` is applied to the decoded colour
    image when cfg cam.distortion is set, `color_dtype=torch.float64` gives the reference's colour dtype."""

    def __init__(self, cfg, args, scale, device='cuda:0', imread=None, color_order=None, undistort=None, color_dtype=torch.float32):
        super(BaseDataset, self).__init__()
        self.name = cfg['dataset']
        self.device = device
        self.scale = scale
        cam = cfg['cam']
        self.png_depth_scale = cam['png_depth_scale']
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cam['H'], cam['W'], cam['fx'], cam['fy'], cam['cx'], cam['cy']
        self.distortion = np.array(cam['distortion']) if 'distortion' in cam else None
        self.crop_size = cam['crop_size'] if 'crop_size' in cam else None
        self.input_folder = cfg['data']['input_folder'] if args.input_folder is None else args.input_folder
        self.crop_edge = cam['crop_edge']
        if self.distortion is not None and undistort is None:
            raise NotImplementedError("cfg['cam']['distortion'] is set: undistortion is not built on the device (OpenCV's uint8 remap is "
                                      '1/32-pixel fixed point); pass undistort=callable(img, K, dist), e.g. cv2.undistort')
        self.undistort = undistort
        if imread is None:
            imread, order = _default_imread()
            color_order = color_order or order
        elif color_order is None:
            raise ValueError("imread= needs color_order='bgr' or 'rgb': the channel order of the colour images it returns")
        if color_order not in _lib.COLOR_ORDER:
            raise ValueError(f'color_order {color_order!r}: one of {sorted(_lib.COLOR_ORDER)}')
        self.imread = imread
        self.color_order = color_order
        self.color_dtype = color_dtype
        self._ingest = None

    @property
    def ingest(self):
        if self._ingest is None:                     # on first use: constructing a dataset needs no GPU
            self._ingest = FrameIngest({'png_depth_scale': self.png_depth_scale, 'crop_edge': self.crop_edge, 'H': self.H, 'W': self.W,
                                        **({'crop_size': self.crop_size} if self.crop_size is not None else {})},
                                       self.scale, self.device, self.color_order, self.color_dtype)
        return self._ingest

    def __getstate__(self):
        """A dataset travels to the processes of a run and to DataLoader workers by pickle: without its FrameIngest (pinned
        buffers, events), which every process builds on first use."""
        state = self.__dict__.copy()
        state['_ingest'] = None
        return state

    def __len__(self):
        return self.n_img

    def _decode(self, index):
        color_path, depth_path = self.color_paths[index], self.depth_paths[index]
        color = self.imread(color_path)
        if '.png' in depth_path:
            depth = self.imread(depth_path, unchanged=True)
        else:
            raise NotImplementedError(f'{depth_path}: only PNG depth is read (EXR needs OpenEXR, which this package does not use)')
        if self.distortion is not None:
            K = np.array([[self.fx, 0., self.cx], [0., self.fy, self.cy], [0., 0., 1.]])
            color = self.undistort(color, K, self.distortion)
        return np.asarray(color), np.asarray(depth)

    def pose(self, index):
        """A copy of the stored pose with its translation scaled once."""
        pose = self.poses[index].clone()
        pose[:3, 3] *= self.scale
        return pose

    def __getitem__(self, index):
        color, depth = self.ingest(*self._decode(index))
        return index, color, depth, self.pose(index).to(self.device)

    def frames(self, indices):
        """(colors [n,H,W,3], depths [n,H,W], poses [n,4,4]) on the device: decoded on the host, one upload, one launch per
        _lib.INGEST_MAX_JOBS frames."""
        indices = list(indices)
        decoded = [self._decode(i) for i in indices]
        colors, depths = self.ingest.batch([c for c, _ in decoded], [d for _, d in decoded])
        poses = torch.stack([self.pose(i) for i in indices]).to(self.device)
        return colors, depths, poses


def _flipped(c2w):
    """float32 pose with the y and z columns negated (src/utils/datasets.py:134-136)."""
    c2w = np.array(c2w, dtype=np.float64).reshape(4, 4)
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1
    return torch.from_numpy(c2w).float()


class Replica(BaseDataset):
    def __init__(self, cfg, args, scale, device='cuda:0', **kw):
        super(Replica, self).__init__(cfg, args, scale, device, **kw)
        self.color_paths = sorted(glob.glob(f'{self.input_folder}/results/frame*.jpg'))
        self.depth_paths = sorted(glob.glob(f'{self.input_folder}/results/depth*.png'))
        self.n_img = len(self.color_paths)
        self.load_poses(f'{self.input_folder}/traj.txt')

    def load_poses(self, path):
        with open(path, 'r') as f:
            lines = f.readlines()
        self.poses = [_flipped([float(v) for v in lines[i].split()]) for i in range(self.n_img)]


class ScanNet(BaseDataset):
    def __init__(self, cfg, args, scale, device='cuda:0', **kw):
        super(ScanNet, self).__init__(cfg, args, scale, device, **kw)
        self.input_folder = os.path.join(self.input_folder, 'frames')
        self.color_paths = self._by_stem(os.path.join(self.input_folder, 'color', '*.jpg'))
        self.depth_paths = self._by_stem(os.path.join(self.input_folder, 'depth', '*.png'))
        self.load_poses(os.path.join(self.input_folder, 'pose'))
        self.n_img = len(self.color_paths)

    @staticmethod
    def _by_stem(pattern):
        return sorted(glob.glob(pattern), key=lambda p: int(os.path.basename(p)[:-4]))

    def load_poses(self, path):
        self.poses = []
        for pose_path in self._by_stem(os.path.join(path, '*.txt')):
            with open(pose_path, 'r') as f:
                self.poses.append(_flipped([float(v) for line in f.readlines() for v in line.split()]))


def _refusal(name, why):
    class _NotBuilt(BaseDataset):
        def __init__(self, cfg, args, scale, device='cuda:0', **kw):
            raise NotImplementedError(f'dataset {name!r} is not built: {why}')
    _NotBuilt.__name__ = _NotBuilt.__qualname__ = name
    return _NotBuilt


CoFusion = _refusal('CoFusion', 'its depth is EXR, which needs the OpenEXR library')
Azure = _refusal('Azure', 'its configs set cam.distortion, which needs OpenCV\'s undistortion, and its poses come from a trajectory log')
TUM_RGBD = _refusal('TUM_RGBD', 'its configs set cam.distortion, which needs OpenCV\'s undistortion, and its frames are associated by '
                    'timestamp with scipy')

dataset_dict = {
    'replica': Replica,
    'scannet': ScanNet,
    'cofusion': CoFusion,
    'azure': Azure,
    'tumrgbd': TUM_RGBD,
}


def get_dataset(cfg, args, scale, device='cuda:0', **kw):
    return dataset_dict[cfg['dataset']](cfg, args, scale, device=device, **kw)
