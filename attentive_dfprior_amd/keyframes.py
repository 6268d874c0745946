"""The Mapper's keyframes on the device: the overlap selection of ``Mapper.keyframe_selection_overlap`` (reference
src/Mapper.py:160-222) in one launch of libadfp.so (``adfp_keyframe_overlap``, csrc/adfp_keyframes.h), and ``KeyframeStore``, the
keyframes' images and poses resident in device memory so that the Mapper's per-iteration ray batch (``common.get_samples_multi``)
reads them where they are instead of uploading every window frame on every iteration (src/Mapper.py:414-418).

The selection makes the reference's random draws: one ``torch.randint`` over the image's pixels (``common.draw_pixels``, the call
``get_samples`` makes) and one ``np.random.permutation`` of the selected ids, also when there is no keyframe.  What runs on the
device is the part whose cost grows with the sequence: the 1 600 sample points, every keyframe's inverse pose and the projection of
every point into every keyframe.  The host reads back the K counts and ranks them as the reference does.
"""
import numpy as np
import torch

from . import _lib, common

EDGE = 20                      # the reference's image margin (src/Mapper.py:207)


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def _as_tensor(x):
    return torch.from_numpy(np.asarray(x)) if not isinstance(x, torch.Tensor) else x


def keyframe_overlap_counts(idx, depth, c2w, poses, N_samples, H, W, fx, fy, cx, cy, edge=EDGE, return_points=False):
    """``counts`` (int32 [K], on idx's device): how many of the current frame's ``len(idx) * N_samples`` sample points each keyframe
    sees, by the reference's test.  ``idx`` [n] int64 on the device: the draw over ``H * W`` (row-major pixels); ``depth`` [H,W] and
    ``c2w`` [4,4] (or [3,4]) of the current frame and ``poses`` [K,4,4] (keyframe camera-to-world) may be host or device tensors.
    With ``return_points`` also the sample points [n N_samples, 3] f32 (None when K = 0: nothing is launched then)."""
    _lib.require_cuda(idx, 'idx')
    dev = idx.device
    n = idx.numel()
    if n == 0:
        raise ValueError('keyframe_overlap_counts: no pixels drawn')
    with _lib.on(dev) as L:
        i = idx.reshape(-1).to(torch.int64).contiguous()
        d = _as_tensor(depth).to(dev, torch.float32).contiguous()
        if tuple(d.shape) != (H, W):
            raise ValueError(f'keyframe_overlap_counts: depth must be [{H},{W}], got {tuple(d.shape)}')
        m = _as_tensor(c2w).detach().to(dev, torch.float32).contiguous()
        if tuple(m.shape) not in ((4, 4), (3, 4)):
            raise ValueError(f'keyframe_overlap_counts: c2w must be [4,4] or [3,4], got {tuple(m.shape)}')
        P = _as_tensor(poses).detach().to(dev, torch.float32).reshape(-1, 4, 4).contiguous()
        K = P.shape[0]
        counts = torch.empty((max(K, 1),), dtype=torch.int32, device=dev)        # never a null pointer, also for K = 0
        pts = torch.empty((n * N_samples, 3), dtype=torch.float32, device=dev) if return_points and K > 0 else None
        L.adfp_keyframe_overlap(i, n, d, H, W, m, int(N_samples), P, K, float(fx), float(fy), float(cx), float(cy), int(edge), counts, pts)
    counts = counts[:K]
    return (counts, pts) if return_points else counts


def select_from_counts(counts, total, k):
    """The reference's ranking (src/Mapper.py:216-222) of per-keyframe counts: ``percent = count / total`` (float64, as
    ``mask.sum() / uv.shape[0]``), a stable descending sort, the ids with ``percent > 0``, then ``np.random.permutation(...)[:k]``
    on numpy's global stream.  Returns a list of numpy ints."""
    percent = np.asarray(counts, dtype=np.int64) / int(total)
    order = sorted(range(len(percent)), key=lambda i: percent[i], reverse=True)       # sorted() is stable under reverse=True
    ids = [i for i in order if percent[i] > 0.0]
    return list(np.random.permutation(np.array(ids))[:k])


def _overlap_points_host(idx, depth, c2w, N_samples, H, W, fx, fy, cx, cy):
    """The sample points on the host with torch's f32 ops, in the reference's order (src/Mapper.py:179-190)."""
    idx = idx.reshape(-1).cpu()
    i, j = (idx % W).float(), torch.div(idx, W, rounding_mode='floor').float()
    c2w = _as_tensor(c2w).detach().cpu().float()
    rays_o, rays_d = common.get_rays_from_uv(i, j, c2w, H, W, fx, fy, cx, cy, 'cpu')
    d = _as_tensor(depth).cpu().float().reshape(-1)[idx].reshape(-1, 1).repeat(1, N_samples)
    t_vals = torch.linspace(0., 1., steps=N_samples)
    z_vals = (d * 0.8) * (1. - t_vals) + (d + 0.5) * t_vals
    return (rays_o.reshape(-1, 1, 3) + rays_d.reshape(-1, 1, 3) * z_vals[..., None]).reshape(-1, 3)


def _project_counts(pts, poses, fx, fy, cx, cy, H, W, edge, block=64):
    """Per keyframe: how many points land inside, by the contract of adfp_keyframe_overlap (numpy; keyframes in blocks)."""
    x = np.asarray(pts, np.float32).reshape(1, -1, 3)
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    out = np.zeros(len(poses), np.int64)
    lo, hi_u, hi_v = np.float32(edge), np.float32(W - edge), np.float32(H - edge)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for b in range(0, len(poses), block):
            w = np.linalg.inv(poses[b:b + block].astype(np.float64)).astype(np.float32)[:, None, :3, :]      # [B,1,3,4]
            cam = ((w[..., 0] * x[..., 0:1] + w[..., 1] * x[..., 1:2]) + w[..., 2] * x[..., 2:3]) + w[..., 3]      # [B,N,3] f32
            X, Y, Z = -cam[..., 0].astype(np.float64), cam[..., 1].astype(np.float64), cam[..., 2].astype(np.float64)
            zz = Z + 1e-5
            u = ((fx * X + cx * Z) / zz).astype(np.float32)
            v = ((fy * Y + cy * Z) / zz).astype(np.float32)
            out[b:b + block] = ((u < hi_u) & (u > lo) & (v < hi_v) & (v > lo) & (zz < 0)).sum(1)
    return out


def keyframe_overlap_counts_host(idx, depth, c2w, poses, N_samples, H, W, fx, fy, cx, cy, edge=EDGE, return_points=False):
    """``keyframe_overlap_counts`` on the host (numpy int64 counts; points as a CPU tensor)."""
    pts = _overlap_points_host(_as_tensor(idx), depth, c2w, N_samples, H, W, fx, fy, cx, cy)
    counts = _project_counts(pts.numpy(), _as_tensor(poses).detach().cpu().numpy(), fx, fy, cx, cy, H, W, edge)
    return (counts, pts) if return_points else counts


def overlap_ambiguity(pts, poses, fx, fy, cx, cy, H, W, edge=EDGE, px=1e-3, dz=1e-9, block=64):
    """Per keyframe: how many points sit where the inside test can go either way between two correct evaluations (an f32 LAPACK
    inverse against an f64 one, BLAS orders): within ``px`` pixels of an image-edge bound or within ``dz`` of z = 0, evaluated
    in f64.  Counts of two implementations may differ by at most this number per keyframe."""
    x = np.asarray(pts, np.float64).reshape(1, -1, 3)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    out = np.zeros(len(poses), np.int64)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for b in range(0, len(poses), block):
            w = np.linalg.inv(poses[b:b + block])[:, None, :3, :]
            cam = ((w[..., 0] * x[..., 0:1] + w[..., 1] * x[..., 1:2]) + w[..., 2] * x[..., 2:3]) + w[..., 3]
            X, Y, Z = -cam[..., 0], cam[..., 1], cam[..., 2]
            zz = Z + 1e-5
            u, v = (fx * X + cx * Z) / zz, (fy * Y + cy * Z) / zz
            amb = np.abs(zz) < dz
            for val, bound in ((u, edge), (u, W - edge), (v, edge), (v, H - edge)):
                amb |= np.abs(val - bound) < px
            out[b:b + block] = amb.sum(1)
    return out


def _keyframe_poses(keyframes):
    """[K,4,4] poses of a keyframe_dict slice (list of dicts with 'est_c2w'), a KeyframeStore or prefix, or a [K,4,4] tensor."""
    if isinstance(keyframes, (KeyframeStore, KeyframePrefix)):
        return keyframes.poses()
    if isinstance(keyframes, torch.Tensor):
        return keyframes.reshape(-1, 4, 4)
    mats = [kf['est_c2w'] for kf in keyframes]
    if not mats:
        return torch.empty((0, 4, 4), dtype=torch.float32)
    try:
        return torch.stack(mats).detach().float().reshape(-1, 4, 4)         # one op when they are tensors on one device
    except (TypeError, RuntimeError):
        mats = [_as_tensor(m).detach().float().reshape(4, 4).cpu() for m in mats]
        return torch.stack(mats)


def keyframe_selection_overlap(gt_color, gt_depth, c2w, keyframes, k, N_samples=16, pixels=100, *, H, W, fx, fy, cx, cy, device):
    """Drop-in for ``Mapper.keyframe_selection_overlap`` (src/Mapper.py:160-222): ``keyframes`` is the reference's
    ``keyframe_dict[:-1]`` (dicts with 'est_c2w') or a ``KeyframeStore`` prefix (``store[:-1]``); ``H .. cy`` and ``device`` are the
    Mapper's.  Same random draws as the reference (one ``torch.randint`` of shape [pixels] over H W on ``device``, one
    ``np.random.permutation``), same result type (a list of numpy ints).  On a GPU device: one launch and one read-back of the K
    counts; ``gt_color`` is not read (the reference gathers it only to discard it)."""
    dev = _cuda_device(device)
    pick = common.draw_pixels(0, H, 0, W, pixels, dev)
    poses = _keyframe_poses(keyframes)
    if poses.shape[0] == 0:
        counts = np.zeros(0, np.int64)
    elif dev.type == 'cuda':
        counts = keyframe_overlap_counts(pick, gt_depth, c2w, poses, N_samples, H, W, fx, fy, cx, cy).cpu().numpy()
    else:
        counts = keyframe_overlap_counts_host(pick, gt_depth, c2w, poses, N_samples, H, W, fx, fy, cx, cy)
    return select_from_counts(counts, pixels * N_samples, k)


class KeyframePrefix(object):
    """The first ``n`` keyframes of a KeyframeStore (what ``store[:n]`` / ``store[:-1]`` returns)."""

    def __init__(self, store, n):
        self.store, self.n = store, n

    def __len__(self):
        return self.n

    def poses(self):
        return self.store.poses(self.n)


class KeyframeStore(object):
    """The keyframes' depth [cap,H,W] f32, colour [cap,H,W,3] f32 and est_c2w [cap,4,4] f32 resident in device memory, beside the
    reference's ``keyframe_dict`` (which the Logger's checkpoints and the Mesher keep reading).  16 bytes per pixel per keyframe:
    4.9 MB per 640x480 frame, about 5 GB at 1 000 keyframes (a ScanNet scene of 5 000 frames with ``keyframe_every: 5``).  The
    buffers grow geometrically from ``capacity``; growing copies the existing keyframes.

    ``frame(i)`` gives ``(c2w, depth, color)`` device views in the shapes ``common.get_samples_multi`` takes in its single-launch
    path; ``poses(n)`` the contiguous [n,4,4] block ``keyframe_selection_overlap`` reads, ``depths(n)`` the [n,H,W] depth block; ``ids`` the frame indices (the reference's
    ``keyframe_list``)."""

    def __init__(self, H, W, device, capacity=16):
        dev = _cuda_device(device)
        if dev.type != 'cuda':
            raise ValueError(f'KeyframeStore: a GPU device is required, got {device}')
        self.H, self.W, self.device = int(H), int(W), dev
        self.ids = []
        self._n = 0
        self._depth = self._color = self._c2w = None
        self._grow(max(1, int(capacity)))

    def _grow(self, cap):
        H, W, dev = self.H, self.W, self.device
        depth = torch.empty((cap, H, W), dtype=torch.float32, device=dev)
        color = torch.empty((cap, H, W, 3), dtype=torch.float32, device=dev)
        c2w = torch.empty((cap, 4, 4), dtype=torch.float32, device=dev)
        if self._n:
            depth[:self._n].copy_(self._depth[:self._n])
            color[:self._n].copy_(self._color[:self._n])
            c2w[:self._n].copy_(self._c2w[:self._n])
        self._depth, self._color, self._c2w = depth, color, c2w

    @property
    def capacity(self):
        return self._depth.shape[0]

    def __len__(self):
        return self._n

    def __getitem__(self, s):
        if not isinstance(s, slice) or s.start not in (None, 0) or s.step not in (None, 1):
            raise TypeError('KeyframeStore: only prefixes store[:n] can be taken; frame(i) gives one keyframe')
        return KeyframePrefix(self, len(range(*s.indices(self._n))))

    def append(self, idx, color, depth, est_c2w):
        """Add one keyframe (host or device tensors / arrays): one copy of each of depth [H,W], colour [H,W,3] and est_c2w [4,4]."""
        if self._n == self.capacity:
            self._grow(2 * self.capacity)
        n = self._n
        with _lib.on(self.device):
            self._depth[n].copy_(_as_tensor(depth).detach().reshape(self.H, self.W))
            self._color[n].copy_(_as_tensor(color).detach().reshape(self.H, self.W, 3))
            m = _as_tensor(est_c2w).detach()
            if tuple(m.shape) == (3, 4):
                m = torch.cat([m.float(), torch.tensor([[0., 0., 0., 1.]], device=m.device)])
            self._c2w[n].copy_(m.reshape(4, 4))
        self.ids.append(int(idx))
        self._n += 1

    def poses(self, n=None):
        """The first n (default: all) keyframe poses, a contiguous [n,4,4] f32 view."""
        return self._c2w[:self._n if n is None else int(n)]

    def depths(self, n=None):
        """The first n (default: all) keyframe depth images, a contiguous [n,H,W] f32 view (what Mesher.seen_mask reads)."""
        return self._depth[:self._n if n is None else int(n)]

    def colors(self, n=None):
        """The first n (default: all) keyframe colour images, a contiguous [n,H,W,3] f32 view (what mesh.project_colors reads)."""
        return self._color[:self._n if n is None else int(n)]

    def frame(self, i):
        """(c2w [4,4], depth [H,W], color [H,W,3]) of keyframe i: device views."""
        if not 0 <= i < self._n:
            raise IndexError(f'KeyframeStore: keyframe {i} of {self._n}')
        return self._c2w[i], self._depth[i], self._color[i]

    @classmethod
    def from_keyframe_dict(cls, keyframe_dict, H, W, device, capacity=None):
        """A store of a loaded checkpoint's ``keyframe_dict`` (dicts with 'idx', 'color', 'depth', 'est_c2w'), in order."""
        store = cls(H, W, device, capacity=max(16, len(keyframe_dict)) if capacity is None else capacity)
        for kf in keyframe_dict:
            store.append(kf['idx'], kf['color'], kf['depth'], kf['est_c2w'])
        return store
