"""Drop-in for the reference's src/utils/Visualizer.py without matplotlib or open3d: after render_img the work is two launches
(adfp_vis_panels: csrc/adfp_vis.h) and one download of a uint8 canvas, written with PIL.

The reference pulls the two input images and the two rendered images to the host, forms the residuals in numpy and pushes six
imshows through a 640 x 480 matplotlib figure.  Here the six panels are built on the device at the frame's own resolution (every
`stride`-th pixel), side by side on a white canvas: what matplotlib maps each array to (Normalize(0, max depth) and the 'plasma'
table for the depth row, the float-RGB rule for the colour row; include/adfp.h "visualisation", tests/vis_ref.py), without imshow's
resampling, titles or axes.  The frame's stats (depth L1, PSNR, non-finite pixels) come out of the same pass: additions, the
reference has none."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib
from .common import get_camera_from_tensor

STATS = ('vmax', 'n_valid', 'depth_abs_sum', 'color_sq_sum', 'n_nonfinite', 'n_color')      # adfp_vis_panels' stats[], in order
_COUNTS = ('n_valid', 'n_nonfinite', 'n_color')


class Visualizer(object):
    """The six-panel picture of a frame -- sensor, rendered and residual depth above sensor, rendered and residual colour --
    written as one image file, for the iterations the two frequencies select.  The Mapper and the Tracker call `vis` from every
    iteration (src/Mapper.py:403-405), so the call costs nothing when it does not fire.

    Parameter and attribute names are the reference's (src/utils/Visualizer.py:15-22).  stride, gap and ext are not in the
    reference: every stride-th pixel of the frame, the white gutter in canvas pixels, and the file type ('jpg' like the
    reference's, or 'png').

    One object serves one stream at a time: workspace, canvas and stats are kept per frame shape and every call with that shape
    writes them again, so calls queued on different streams would race on them."""

    def __init__(self, freq, inside_freq, vis_dir, renderer, verbose, device='cuda:0', stride=1, gap=8, ext='jpg'):
        if ext not in ('jpg', 'png'):
            raise ValueError(f"ext {ext!r}: 'jpg' or 'png'")
        if int(stride) < 1 or int(gap) < 0:
            raise ValueError(f'stride {stride} must be >= 1 and gap {gap} >= 0')
        self.renderer, self.device = renderer, device
        self.freq, self.inside_freq = freq, inside_freq              # frame index and iteration number a picture is made at
        self.vis_dir, self.verbose = vis_dir, verbose
        self.stride, self.gap, self.ext = int(stride), int(gap), ext
        self.last_stats = None
        self._buffers = {}                           # (H, W, gt_color is f64, device) -> geometry, workspace, canvas, stats
        os.makedirs(vis_dir, exist_ok=True)

    def canvas_shape(self, H, W):
        """(rows, cols) of the canvas of an H x W frame (adfp_vis_canvas_shape)."""
        rows, cols = C.c_int(), C.c_int()
        geom = _lib.AdfpVisGeom(H, W, self.stride, self.gap, 0)
        _lib.host.adfp_vis_canvas_shape(C.byref(geom), C.byref(rows), C.byref(cols))
        return rows.value, cols.value

    def _buffers_for(self, H, W, f64, device):
        key = (H, W, f64, device)
        b = self._buffers.get(key)
        if b is None:
            geom = _lib.AdfpVisGeom(H, W, self.stride, self.gap, int(f64))
            rows, cols = self.canvas_shape(H, W)
            nbytes = lib().adfp_vis_workspace_bytes(C.byref(geom))
            b = self._buffers[key] = (geom, torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes,
                                      torch.empty((rows, cols, 3), dtype=torch.uint8, device=device),
                                      torch.empty(_lib.VIS_STATS, dtype=torch.float64, device=device))
        return b

    def panels_async(self, gt_depth, gt_color, depth, color):
        """panels() without its read-back: (canvas, stats float64 [6] in STATS' order), both on the device and both this object's
        buffers for the frame's shape; the two launches are queued on the current stream and nothing waits for them.  The next
        call with that shape overwrites both, and it must be queued on the same stream (or after a wait for this one): the
        buffers carry no event."""
        _lib.require_cuda(gt_depth, 'gt_depth')
        dev = gt_depth.device
        H, W = gt_depth.shape
        f64 = gt_color.dtype == torch.float64
        gt_depth = gt_depth.to(torch.float32).contiguous()
        gt_color = gt_color.to(device=dev, dtype=torch.float64 if f64 else torch.float32).contiguous()
        depth = depth.to(device=dev, dtype=torch.float64).contiguous()
        color = color.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(gt_color.shape) != (H, W, 3) or tuple(depth.shape) != (H, W) or tuple(color.shape) != (H, W, 3):
            raise ValueError(f'panels: gt_depth {tuple(gt_depth.shape)}, gt_color {tuple(gt_color.shape)}, depth {tuple(depth.shape)}, '
                             f'color {tuple(color.shape)} are not one frame')
        geom, ws, ws_bytes, canvas, stats = self._buffers_for(H, W, f64, dev)
        with _lib.on(dev) as L:
            L.adfp_vis_panels(C.byref(geom), gt_depth, gt_color, depth, color, canvas, stats, ws, ws_bytes)
        return canvas, stats

    def panels(self, gt_depth, gt_color, depth, color):
        """(canvas uint8 [rows, cols, 3] on the device, stats dict) of a frame: gt_depth [H,W], gt_color [H,W,3] float32 or float64,
        and the rendered depth [H,W] and color [H,W,3] as render_img returns them.  No rendering, nothing written.  The canvas is
        this object's buffer for the frame's shape -- the next call with that shape writes it again; clone() what must stay.
        Reading the stats is the call's one synchronisation."""
        canvas, stats = self.panels_async(gt_depth, gt_color, depth, color)
        return canvas, stats_dict(stats.cpu().numpy())

    def fires(self, idx, iter):
        """Whether `vis` does anything for frame idx at iteration iter (the rule of Visualizer.py:42)."""
        return idx % self.freq == 0 and iter % self.inside_freq == 0

    def pose(self, c2w_or_camera_tensor):
        """The 4 x 4 camera-to-world matrix of what the callers pass: a matrix as it is (the Mapper), or the Tracker's [7]
        quaternion-and-translation tensor through common.get_camera_from_tensor with the row (0, 0, 0, 1) below its [3, 4]
        (Visualizer.py:45-53).  The tensor is not part of any graph afterwards."""
        if c2w_or_camera_tensor.dim() != 1:
            return c2w_or_camera_tensor
        top = get_camera_from_tensor(c2w_or_camera_tensor.detach().clone())
        last_row = top.new_tensor([[0.0, 0.0, 0.0, 1.0]]).to(self.device)
        return torch.cat((top.to(self.device), last_row))

    def vis(self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders, tsdf_volume, tsdf_bnds):
        """Renders frame idx from the given pose and writes its picture to {vis_dir}/{idx:05d}_{iter:04d}.{ext} -- when
        `fires(idx, iter)`; otherwise nothing is rendered or written.  gt_depth [H,W] and gt_color [H,W,3] are the frame's sensor
        images on the device, c the feature grids, decoders / tsdf_volume / tsdf_bnds what render_img takes.  Returns None like the
        reference's; the frame's stats stay in self.last_stats.  The argument names are the reference's (Visualizer.py:24-25)."""
        if not self.fires(idx, iter):
            return
        with torch.no_grad():
            depth, _, color = self.renderer.render_img(c, decoders, self.pose(c2w_or_camera_tensor), self.device, tsdf_volume,
                                                       tsdf_bnds, stage='color', gt_depth=gt_depth)
            canvas, self.last_stats = self.panels(gt_depth, gt_color, depth, color)
        from PIL import Image
        path = '%s/%05d_%04d.%s' % (self.vis_dir, idx, iter, self.ext)
        Image.fromarray(canvas.cpu().numpy()).save(path)
        if self.verbose:
            print('Saved rendering visualization of color/depth image at', path)      # the reference's line


def stats_dict(values):
    """adfp_vis_panels' stats[] as a dict, plus depth_l1 = depth_abs_sum / n_valid and psnr = -10 log10(color_sq_sum / (3 n_color))
    (NaN or inf where a count or the sum is zero)."""
    v = np.asarray(values, dtype=np.float64)
    s = {k: (int(v[i]) if k in _COUNTS else float(v[i])) for i, k in enumerate(STATS)}
    with np.errstate(all='ignore'):
        s['depth_l1'] = float(v[2] / v[1])
        s['psnr'] = float(-10.0 * np.log10(v[3] / (3.0 * v[5])))
    return s
