"""Depth images of the TSDF prior from any pose: KinectFusion's raycast on the MI355X (adfp_tsdf_raycast, csrc/adfp_tsdfcast.h).

The reference renders a frame only where a sensor depth image exists (src/utils/Renderer.py:292: render_img needs gt_depth, and
16 of a ray's samples sit within 5 % of it).  The prior volume is resident for the whole run and answers for any pose: the first
+ -> - crossing of the TSDF along a pixel's ray is the depth the sampler wants.  Renderer.render_novel renders through it.

    rc = TsdfRaycaster(tsdf_volume, tsdf_bnds)
    depth = rc.render_depth(c2w, H, W, fx, fy, cx, cy)            # [H, W] float32, 0 where the ray meets no surface

The rule (ray, interval, march, hit) is stated in include/adfp.h and restated in torch in tests/tsdfcast_ref.py.  Two things to
know about it: a ray that starts behind a surface (first sample <= 0) gets 0, and a ray that reaches a surface from behind
through unobserved space reports a crossing at the truncation boundary -- the rule is on interpolated values with no band test,
as KinectFusion's is."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import Engine


class TsdfRaycaster(object):
    """Raycasts one TSDF volume ([1,1,Z,Y,X] float32 on the device, any strides) inside `tsdf_bnds` ([3,2]).

    Owns the empty-space bitmap (one bit per brick of 8^3 voxels), built on first use and cached on the volume's version counter;
    `invalidate_tsdf()` drops it after a write PyTorch did not see, like Renderer.invalidate_tsdf.  `engine`: share a Renderer's
    Engine, so that one invalidate_tsdf serves both and a corner-block copy the engine already holds is read."""

    def __init__(self, tsdf_volume, tsdf_bnds, engine=None):
        _lib.require_cuda(tsdf_volume, 'tsdf_volume')
        if tsdf_volume.dtype != torch.float32 or tsdf_volume.dim() != 5 or tsdf_volume.shape[0] != 1 or tsdf_volume.shape[1] != 1:
            raise RuntimeError(f'tsdf_volume: expected float32 [1,1,Z,Y,X], got {tsdf_volume.dtype} {tuple(tsdf_volume.shape)}')
        self.tsdf_volume = tsdf_volume
        self.tsdf_bnds = tsdf_bnds
        self._engine = engine if engine is not None else Engine()

    def invalidate_tsdf(self):
        self._engine.invalidate_tsdf_blocks()

    def voxel(self):
        """The TSDF voxel in metres: the smallest of extent / size over the axes (fusion's voxel_size for a volume it built)."""
        ext = self._engine.host_bound(self.tsdf_bnds, 'tsdf_bnds')
        Z, Y, X = self.tsdf_volume.shape[2:]
        return min((ext[0][1] - ext[0][0]) / X, (ext[1][1] - ext[1][0]) / Y, (ext[2][1] - ext[2][0]) / Z)

    def render_depth(self, c2w, H, W, fx, fy, cx, cy, near=0., far=0., step=None, skip=True, tsdf_blocks=None, count=False, out=None):
        """c2w [V,4,4] or [4,4] -> depth [V,H,W] or [H,W] float32 on the volume's device.

        near, far: the ray interval in sensor depth (far = 0: to the volume's exit); step: metres between samples, default half a
        voxel; skip=False looks every sample up (the same image, byte for byte).  tsdf_blocks: None reads the corner-block copy if
        the engine holds a current one, False never, a tensor is the caller's own copy.  count=True also returns the number of
        trilinear lookups the call made (one read-back).  out: a contiguous float32 [V,H,W] on the volume's device to write into
        instead of a new tensor (icp.DepthICP's model slot)."""
        t = self.tsdf_volume
        dev = t.device
        if isinstance(c2w, np.ndarray):
            c2w = torch.from_numpy(c2w)
        m = c2w.detach().to(dev, torch.float32)
        single = m.dim() == 2
        if single:
            m = m[None]
        if m.dim() != 3 or tuple(m.shape[1:]) != (4, 4) or m.shape[0] < 1:
            raise ValueError(f'c2w: expected [V,4,4] or [4,4], got {tuple(c2w.shape)}')
        m = m.contiguous()
        V = m.shape[0]
        if step is None:
            step = 0.5 * self.voxel()
        with _lib.on(dev) as L:
            td = _lib.AdfpTsdf()
            keep = []
            self._engine.fill_tsdf(td, t, keep)
            cb = tsdf_blocks
            if cb is None:
                cb = self._engine.tsdf_blocks_cached(t)
            if isinstance(cb, torch.Tensor):
                td.corner_blocks = cb.data_ptr()
            b = _lib.Bound()
            _lib.fill_bound(b, self._engine.host_bound(self.tsdf_bnds, 'tsdf_bnds'))
            bricks, nbytes = None, 0
            if skip:
                bricks = self._engine.tsdf_bricks(t)
                nbytes = bricks.numel() * 4
            if out is None:
                depth = torch.empty((V, int(H), int(W)), dtype=torch.float32, device=dev)
            else:
                if out.dtype != torch.float32 or tuple(out.shape) != (V, int(H), int(W)) or out.device != dev or not out.is_contiguous():
                    raise ValueError(f'out: expected contiguous float32 [{V},{int(H)},{int(W)}] on {dev}, got {out.dtype} {tuple(out.shape)}')
                depth = out
            n =torch.zeros((1,), dtype=torch.int64, device=dev) if count else None
            L.adfp_tsdf_raycast(C.byref(td), C.byref(b), bricks, nbytes, m, V, int(H), int(W), fx, fy, cx, cy, float(near), float(far),
                                float(step), 0 if skip else _lib.CAST_NO_SKIP, depth, n)
        out = depth[0] if single else depth
        return (out, int(n.item())) if count else out
