"""
Drop-in for the reference's ``src/utils/datasets.py``: ``get_dataset``, ``dataset_dict``, ``BaseDataset``, ``Replica``, ``ScanNet``,
``Azure`` and ``TUM_RGBD`` with the reference's constructor arguments, attributes and file layouts, and ``__getitem__`` returning
``(index, color, depth, pose)`` on the device.  What the reference does to every frame on the host (``/ 255.`` into float64, ``cv2.resize`` on doubles, two
``F.interpolate`` passes for ``crop_size``, the edge crop, a float64 upload) is one launch of libadfp.so here
(``adfp_ingest_frames``, include/adfp.h "frame ingestion"): the decoded bytes go up as they are, 3 + 2 bytes per pixel.

``FrameIngest`` is the layer without files: decoded images in, device tensors out, one frame or a batch per launch.

Deviations from the reference, all deliberate:
  * the colour comes back as float32 unless ``color_dtype=torch.float64`` is asked for: every consumer of this package converts;
  * ``__getitem__`` returns a copy of the pose whose translation is scaled ONCE; the reference scales the stored pose in place on
    every access (src/utils/datasets.py:112).  The two agree at ``scale: 1``;
  * undistortion (``cam.distortion``) needs its route stated: ``cam.undistort: device`` in the config, or the keyword
    ``undistort='device'``, runs it as a stage of the ingestion launch (``adfp_ingest_frames_undistort``) by this package's own
    rule -- the scheme of ``cv2.undistort(img, K, dist)``: a 1/32-pixel fixed-point map, bilinear, border 0 (include/adfp.h "lens
    undistortion") -- which has NOT been compared with cv2 and claims no byte parity with it; ``undistort=callable(img, K, dist)``
    keeps the host route for whoever needs cv2's own bytes.  The keyword wins over the config; without either, a config with
    ``cam.distortion``, and the ``azure`` and ``tumrgbd`` datasets, raise NotImplementedError;
  * ``TUM_RGBD.parse_list`` reads the list files itself (comment and blank lines dropped after ``skiprows``, fields separated by
    single spaces) instead of ``np.loadtxt(dtype=np.unicode_)``, and ``pose_matrix_from_quaternion`` is numpy (x y z w, normalised,
    scipy's formula): scipy is not a dependency;
  * a dataset built with ``device='cpu'`` (the reference's Mesher builds one for its length) has its paths, poses and length,
    but indexing it raises: the frames exist only on the GPU.
CoFusion (EXR depth) is not built.  A dataset pickles (the reference hands it to its Tracker and Mapper processes and to a
DataLoader worker); each process builds its own FrameIngest, and its undistortion map, on first use.
"""
import ctypes as C
import glob
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from . import _lib


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


def _distortion(dist):
    """cfg cam.distortion as a float64 vector k1 k2 p1 p2 [k3 [k4 k5 k6]]."""
    d = np.asarray(dist, dtype=np.float64).reshape(-1)
    if d.size not in (4, 5, 8):
        raise ValueError(f'cam.distortion has {d.size} coefficients: 4, 5 or 8 (k1 k2 p1 p2 [k3 [k4 k5 k6]]) are built')
    return d


def undistort_map(color_hw, fx, fy, cx, cy, dist):
    """The 1/32-pixel fixed-point map [h,w,2] (int32, numpy) of include/adfp.h "lens undistortion" (adfp_undistort_map; host only)."""
    h, w = int(color_hw[0]), int(color_hw[1])
    d = np.ascontiguousarray(_distortion(dist))
    out = np.empty((h, w, 2), dtype=np.int32)
    _lib.host.adfp_undistort_map(h, w, float(fx), float(fy), float(cx), float(cy), d.ctypes.data, d.size, out.ctypes.data)
    return out


class FrameIngest(object):
    """``ingest = FrameIngest(cfg['cam'], scale, device)``; ``color, depth = ingest(color_u8, depth_raw)`` for one frame,
    ``ingest.batch(colors, depths)`` for n frames in one launch ([n,H,W,3] and [n,H,W]).

    color_u8 [h,w,3] uint8 in `color_order`; depth_raw [H0,W0] uint16 (int16 storage is read as uint16) or float32.  Inputs may be
    numpy arrays, CPU tensors or device tensors.  Host inputs go through two pinned staging buffers used in turn, each guarded by
    an event, and a non_blocking copy on the current stream: a call waits at most for the copy that last read the buffer it is
    about to fill, never for the device.  ``out=(color, depth)`` takes contiguous destinations (for a batch: tensors with a leading
    n, or sequences of n per-frame tensors, e.g. frames of a KeyframeStore block).

    ``undistort='device'`` (or ``cfg_cam['undistort'] == 'device'``; the keyword wins) with a ``distortion`` in cfg_cam undistorts
    the colour image inside the same launch (include/adfp.h "lens undistortion"): the 1/32-pixel map of cfg_cam's fx, fy, cx, cy
    and distortion is built on the first frame of each colour size and uploaded once.  ``ingest.undistort(color_u8)`` returns
    the undistorted uint8 image on its own.  Without a distortion nothing is undistorted."""

    def __init__(self, cfg_cam, scale, device, color_order='rgb', color_dtype=torch.float32, undistort=None):
        if color_order not in _lib.COLOR_ORDER:
            raise ValueError(f'color_order {color_order!r}: one of {sorted(_lib.COLOR_ORDER)}')
        if color_dtype not in (torch.float32, torch.float64):
            raise ValueError(f'color_dtype {color_dtype}: torch.float32 or torch.float64')
        route = undistort if undistort is not None else cfg_cam.get('undistort')
        if route not in (None, 'device'):
            raise ValueError(f"undistort {route!r}: 'device' or None (a host callable belongs to the dataset)")
        self._lens = None                            # (fx, fy, cx, cy, coefficients) when the launch undistorts
        if route == 'device' and cfg_cam.get('distortion') is not None:
            self._lens = (float(cfg_cam['fx']), float(cfg_cam['fy']), float(cfg_cam['cx']), float(cfg_cam['cy']),
                          _distortion(cfg_cam['distortion']))
        self._maps = {}                              # colour (h, w) -> device int32 [h,w,2]
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

    def __getstate__(self):
        """Without what belongs to a process: the pinned buffers, their events and the device maps are built again on use."""
        state = self.__dict__.copy()
        state.update(_staging=[None, None], _events=[None, None], _turn=0, _maps={})
        return state

    # ---- undistortion
    def _map(self, color_hw):
        """The device map [h,w,2] (int32) of a colour size, or None when the launch does not undistort; built on first use."""
        if self._lens is None:
            return None
        m = self._maps.get(color_hw)
        if m is None:
            m = self._maps[color_hw] = torch.from_numpy(undistort_map(color_hw, *self._lens)).to(self.device)
        return m

    def undistort(self, color_u8, map=None):
        """The undistorted uint8 image [h,w,3] on the device (adfp_undistort_image): what the launch reads where stage A reads a
        source byte.  `map`: a device int32 [h,w,2] map in place of the configured lens's."""
        self._kind(color_u8, 'color')
        h, w = int(color_u8.shape[0]), int(color_u8.shape[1])
        if map is None:
            map = self._map((h, w))
            if map is None:
                raise ValueError('this FrameIngest has no distortion to undo: cfg cam.distortion with undistort=\'device\', or map=')
        if not torch.is_tensor(map) or map.dtype != torch.int32 or tuple(map.shape) != (h, w, 2) or map.device != self.device \
                or not map.is_contiguous():
            raise ValueError(f'map: a contiguous int32 tensor of shape {(h, w, 2)} on {self.device} expected')
        src = color_u8 if torch.is_tensor(color_u8) else torch.from_numpy(np.ascontiguousarray(color_u8))
        src = src.to(self.device).contiguous()
        dst = torch.empty_like(src)
        with _lib.on(self.device) as L:
            L.adfp_undistort_image(src, map, h, w, dst)
        return dst

    # ---- geometry
    def _geom(self, color_hw, depth_hw, depth_f32):
        ch, cw = self.crop_size or (0, 0)
        return _lib.AdfpIngestGeom(color_hw[0], color_hw[1], depth_hw[0], depth_hw[1], ch, cw, self.crop_edge,
                                   _lib.COLOR_ORDER[self.color_order], int(depth_f32), int(self.color_dtype == torch.float64),
                                   self.png_depth_scale, self.scale)

    def out_shape_for(self, depth_hw):
        """(H, W) of the tensors a depth image of depth_hw comes back as (adfp_ingest_out_shape)."""
        H, W = C.c_int(), C.c_int()
        _lib.host.adfp_ingest_out_shape(C.byref(self._geom(depth_hw, depth_hw, False)), C.byref(H), C.byref(W))
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
        with _lib.on(self.device) as L:
            lens_map = self._map(color_hw)
            if host:
                dev, offs = self._upload(host)
                it = iter(offs)
                srcs = [s if s is not None else dev.data_ptr() + next(it) for s in srcs]
            for j0 in range(0, n, _lib.INGEST_MAX_JOBS):
                m = min(_lib.INGEST_MAX_JOBS, n - j0)
                jobs = (_lib.AdfpIngestJob * m)(*[_lib.AdfpIngestJob(srcs[j], srcs[n + j], cdst[j].data_ptr(), ddst[j].data_ptr())
                                                  for j in range(j0, j0 + m)])
                if lens_map is None:
                    L.adfp_ingest_frames(C.byref(geom), m, jobs)
                else:
                    L.adfp_ingest_frames_undistort(C.byref(geom), lens_map, m, jobs)
        return result


class BaseDataset(Dataset):
    """The reference's BaseDataset (src/utils/datasets.py:51-113).  Trailing keyword extensions: `imread(path, unchanged=False)`
    replaces the decoder (then `color_order` must say which channel order it returns; a picklable callable if the dataset
    goes to another process), `undistort` states the route cfg cam.distortion takes -- 'device' for the ingestion launch's own
    stage (as cfg cam.undistort: device does; the keyword wins), or a callable `undistort(img, K, dist)` applied to the decoded
    colour image on the host -- and `color_dtype=torch.float64` gives the reference's colour dtype."""

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
        if undistort is None:
            undistort = cam.get('undistort')
        if undistort is not None and undistort != 'device' and not callable(undistort):
            raise ValueError(f"undistort {undistort!r}: 'device' (also cfg cam.undistort: device) or a callable(img, K, dist)")
        if self.distortion is not None and undistort is None:
            raise NotImplementedError("cfg['cam']['distortion'] is set and no route for the undistortion is stated: set "
                                      "cfg['cam']['undistort'] = 'device' (or pass undistort='device') for this package's own "
                                      'fixed-point remap inside the ingestion launch, which is not cv2\'s byte for byte, or pass '
                                      'undistort=callable(img, K, dist), e.g. cv2.undistort')
        if self.distortion is not None and undistort == 'device':
            _distortion(self.distortion)
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
            on_device = self.distortion is not None and self.undistort == 'device'
            self._ingest = FrameIngest({'png_depth_scale': self.png_depth_scale, 'crop_edge': self.crop_edge, 'H': self.H, 'W': self.W,
                                        **({'crop_size': self.crop_size} if self.crop_size is not None else {}),
                                        **({'fx': self.fx, 'fy': self.fy, 'cx': self.cx, 'cy': self.cy,
                                            'distortion': self.distortion} if on_device else {})},
                                       self.scale, self.device, self.color_order, self.color_dtype,
                                       undistort='device' if on_device else None)
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
        if self.distortion is not None and callable(self.undistort):      # 'device': a stage of the ingestion launch
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


def _need_route(ds, name):
    """The datasets whose shipped configs set cam.distortion are built only from a config (or call) that states the route."""
    if ds.undistort is None:
        raise NotImplementedError(f"dataset {name!r}: its configs set cam.distortion, and no route for the undistortion is stated: set "
                                  "cfg['cam']['undistort'] = 'device' (or pass undistort='device') for this package's own fixed-point "
                                  'remap, or pass undistort=callable(img, K, dist), e.g. cv2.undistort')


class Azure(BaseDataset):
    """src/utils/datasets.py:140-178: color/*.jpg and depth/*.png sorted by name, poses from scene/trajectory.log (records of five
    lines: a header and four rows), identity poses without the log."""

    def __init__(self, cfg, args, scale, device='cuda:0', **kw):
        super(Azure, self).__init__(cfg, args, scale, device, **kw)
        _need_route(self, 'azure')
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, 'color', '*.jpg')))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, 'depth', '*.png')))
        self.n_img = len(self.color_paths)
        self.load_poses(os.path.join(self.input_folder, 'scene', 'trajectory.log'))

    def load_poses(self, path):
        self.poses = []
        if os.path.exists(path):
            with open(path) as f:
                content = f.readlines()
            for i in range(0, len(content) - 4, 5):
                self.poses.append(_flipped([float(v) for v in ''.join(content[i + 1:i + 5]).split()]))
        else:
            self.poses = [torch.eye(4) for _ in range(self.n_img)]


class TUM_RGBD(BaseDataset):
    """src/utils/datasets.py:234-321: rgb.txt, depth.txt and groundtruth.txt (or else pose.txt) associated by timestamp (each image
    with its nearest depth and pose, both strictly nearer than max_dt), thinned to frame_rate, poses relative to the first kept
    frame."""

    def __init__(self, cfg, args, scale, device='cuda:0', **kw):
        super(TUM_RGBD, self).__init__(cfg, args, scale, device, **kw)
        _need_route(self, 'tumrgbd')
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self.n_img = len(self.color_paths)

    def parse_list(self, filepath, skiprows=0):
        """The rows of a list file as a 2-D array of strings: `skiprows` lines skipped, then what follows a '#' and blank lines
        dropped, fields separated by single spaces (np.loadtxt(delimiter=' ', dtype=str))."""
        with open(filepath) as f:
            lines = f.readlines()[skiprows:]
        rows = [line.split('#', 1)[0].strip() for line in lines]
        rows = [r.split(' ') for r in rows if r]
        if len({len(r) for r in rows}) > 1:
            raise ValueError(f'{filepath}: rows of {sorted({len(r) for r in rows})} fields')
        return np.array(rows, dtype=str).reshape(len(rows), -1)

    def associate_frames(self, tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
        """(i, j[, k]) for every image i whose nearest depth j (and pose k) lies strictly within max_dt."""
        associations = []
        for i, t in enumerate(tstamp_image):
            j = np.argmin(np.abs(tstamp_depth - t))
            if tstamp_pose is None:
                if np.abs(tstamp_depth[j] - t) < max_dt:
                    associations.append((i, j))
            else:
                k = np.argmin(np.abs(tstamp_pose - t))
                if (np.abs(tstamp_depth[j] - t) < max_dt) and (np.abs(tstamp_pose[k] - t) < max_dt):
                    associations.append((i, j, k))
        return associations

    def loadtum(self, datapath, frame_rate=-1):
        pose_list = os.path.join(datapath, 'groundtruth.txt')
        if not os.path.isfile(pose_list):
            pose_list = os.path.join(datapath, 'pose.txt')
        if not os.path.isfile(pose_list):
            raise FileNotFoundError(f'{datapath}: neither groundtruth.txt nor pose.txt')
        image_data = self.parse_list(os.path.join(datapath, 'rgb.txt'))
        depth_data = self.parse_list(os.path.join(datapath, 'depth.txt'))
        pose_data = self.parse_list(pose_list, skiprows=1)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        tstamp_image = image_data[:, 0].astype(np.float64)
        tstamp_depth = depth_data[:, 0].astype(np.float64)
        tstamp_pose = pose_data[:, 0].astype(np.float64)
        associations = self.associate_frames(tstamp_image, tstamp_depth, tstamp_pose)
        if not associations:
            return [], [], []
        indicies = [0]
        for i in range(1, len(associations)):
            t0 = tstamp_image[associations[indicies[-1]][0]]
            t1 = tstamp_image[associations[i][0]]
            if t1 - t0 > 1.0 / frame_rate:
                indicies += [i]
        images, poses, depths = [], [], []
        inv_pose = None
        for ix in indicies:
            i, j, k = associations[ix]
            images += [os.path.join(datapath, image_data[i, 1])]
            depths += [os.path.join(datapath, depth_data[j, 1])]
            c2w = self.pose_matrix_from_quaternion(pose_vecs[k])
            if inv_pose is None:
                inv_pose = np.linalg.inv(c2w)
                c2w = np.eye(4)
            else:
                c2w = inv_pose @ c2w
            poses += [_flipped(c2w)]
        return images, depths, poses

    def pose_matrix_from_quaternion(self, pvec):
        """4 x 4 pose of (tx ty tz qx qy qz qw): the quaternion normalised, then scipy's Rotation.as_matrix formula."""
        x, y, z, w = np.asarray(pvec[3:7], dtype=np.float64) / np.sqrt(np.sum(np.square(np.asarray(pvec[3:7], dtype=np.float64))))
        x2, y2, z2, w2 = x * x, y * y, z * z, w * w
        xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
        pose = np.eye(4)
        pose[:3, :3] = [[x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw)],
                        [2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw)],
                        [2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2]]
        pose[:3, 3] = pvec[:3]
        return pose


dataset_dict = {
    'replica': Replica,
    'scannet': ScanNet,
    'cofusion': CoFusion,
    'azure': Azure,
    'tumrgbd': TUM_RGBD,
}


def get_dataset(cfg, args, scale, device='cuda:0', **kw):
    return dataset_dict[cfg['dataset']](cfg, args, scale, device=device, **kw)
