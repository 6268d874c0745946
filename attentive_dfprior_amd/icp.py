"""Frame-to-model point-to-plane ICP over the whole depth image on the MI355X (adfp_depth_normals, adfp_icp_*, csrc/adfp_icp.h):
KinectFusion's tracker against the TSDF prior that is resident for the whole run.

The Tracker starts a frame from the constant-speed guess and looks at 200 pixels per iteration; the prior volume, its raycast
(tsdf_raycast.TsdfRaycaster) and the frame's full sensor depth image are on the device all along.  DepthICP aligns the whole sensor
depth image with the raycast of the prior from the guess and hands the Tracker a better start -- or, with ``tracking.iters: 0``, is
the tracker (``tracking.init: icp``, slam.Tracker).

    icp = DepthICP(tsdf_volume, tsdf_bnds, H, W, fx, fy, cx, cy, engine=renderer._engine)
    cam = icp.refine(guess_c2w, gt_depth)          # [7] float32 on the device: quaternion r, i, j, k, then the translation
    icp.last_stats()                               # [steps + 1, 6] float64 on the host, on demand

The rule (normal map, association, normal equations, solve, gate) is stated in include/adfp.h ("Depth ICP") and restated in numpy in
tests/icp_ref.py.  Everything is decided on the device: a refinement is a fixed sequence of launches with no read-back, and a
refinement that fails (too few pairs, a direction the pairs do not constrain, a result too far from the guess) returns the guess.

RgbdICP (``tracking.icp_rgb``) is DepthICP with a photometric term against the last tracked frame in every step's normal equations
(adfp_rgbd_frame_map, adfp_rgbd_step, csrc/adfp_rgbd.h; include/adfp.h "RGB-D ICP", tests/rgbd_icp_ref.py): texture constrains what a
view of one or two walls leaves free, and an empty model image still yields pairs.

depth_bilateral (adfp_depth_bilateral, csrc/adfp_depthfilter.h; include/adfp.h "Depth bilateral filter", tests/depth_filter_ref.py) is
the filter KinectFusion applies to the raw depth before anything else, and ``DepthICP(bilateral={...})`` (``tracking.icp.bilateral``)
puts it in front of the sensor's normal map: the normals are one-pixel differences of the depth, and a noisy normal fails cos_tol."""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import lib
from .tsdf_raycast import TsdfRaycaster

OK, FEW_PAIRS, DEGENERATE, REJECTED = 0, 1, 2, 3
STATUS_NAMES = {v: k for k, v in _lib.ICP_STATUS.items()}
STATS_COLUMNS = ('pairs', 'rmse', 'pivot_ratio', 'omega', 'shift', 'status')
BILATERAL_DEFAULTS = {'radius': 2, 'sigma_space': 1.5, 'sigma_depth': 0.05, 'sigma_depth_z2': 0.0, 'points': True}
BILATERAL_MAX_RADIUS = 8               # ADFP_BILATERAL_MAX_RADIUS


def _bilateral_numbers(radius, sigma_space, sigma_depth, sigma_depth_z2):
    if isinstance(radius, bool) or int(radius) != radius or not 1 <= int(radius) <= BILATERAL_MAX_RADIUS:
        raise ValueError(f'bilateral radius {radius!r}: an integer in 1 .. {BILATERAL_MAX_RADIUS}')
    ss, sd, sz = float(sigma_space), float(sigma_depth), float(sigma_depth_z2)
    if not ss > 0 or not sd > 0 or not sz >= 0:
        raise ValueError(f'bilateral sigma_space {sigma_space!r} and sigma_depth {sigma_depth!r} must be > 0, sigma_depth_z2 '
                         f'{sigma_depth_z2!r} >= 0')
    return int(radius), ss, sd, sz


def bilateral_config(bilateral, points=True):
    """The ``bilateral`` keyword -> None (off) or the full dict; `points` is the default of the key of that name."""
    if bilateral is None or bilateral is False:
        return None
    if not isinstance(bilateral, dict):
        raise ValueError(f'bilateral: None, False or a dict with keys from {sorted(BILATERAL_DEFAULTS)}, got {bilateral!r}')
    unknown = sorted(set(bilateral) - set(BILATERAL_DEFAULTS))
    if unknown:
        raise ValueError(f'bilateral: unknown keys {unknown}; the keys are {sorted(BILATERAL_DEFAULTS)}')
    cfg = dict(BILATERAL_DEFAULTS, points=points)
    cfg.update(bilateral)
    cfg['radius'], cfg['sigma_space'], cfg['sigma_depth'], cfg['sigma_depth_z2'] = _bilateral_numbers(
        cfg['radius'], cfg['sigma_space'], cfg['sigma_depth'], cfg['sigma_depth_z2'])
    if not isinstance(cfg['points'], bool):
        raise ValueError(f"bilateral points {cfg['points']!r}: True or False")
    return cfg


def depth_bilateral(depth, radius=2, sigma_space=1.5, sigma_depth=0.05, sigma_depth_z2=0.0, out=None):
    """Bilateral filter of depth images, [V,H,W] or [H,W] float32 on the device -> the same shape (adfp_depth_bilateral, one launch;
    `out`: where to, not `depth` itself).  A (2 radius + 1)^2 window, sigma_space in pixels, the range term sigma_depth +
    sigma_depth_z2 d^2 in metres at the centre's depth d, neighbours further than three of it in depth left out; an invalid pixel
    (<= 0 or not finite) stays 0 and takes no part.  The defaults are the mini scene's (48 x 64, depths 0.3-1.2 m) and, like the
    ICP's other defaults, have not been tuned on anything else."""
    _lib.require_cuda(depth, 'depth')
    if depth.dtype != torch.float32 or depth.dim() not in (2, 3) or not depth.is_contiguous():
        raise ValueError(f'depth: expected contiguous float32 [V,H,W] or [H,W], got {depth.dtype} {tuple(depth.shape)}')
    radius, ss, sd, sz = _bilateral_numbers(radius, sigma_space, sigma_depth, sigma_depth_z2)
    H, W = depth.shape[-2:]
    V = depth.shape[0] if depth.dim() == 3 else 1
    with _lib.on(depth.device) as L:
        if out is None:
            out = torch.empty_like(depth)
        elif out.dtype != torch.float32 or out.shape != depth.shape or not out.is_contiguous() or out.device != depth.device:
            raise ValueError(f'out: expected contiguous float32 {tuple(depth.shape)} on {depth.device}, got {out.dtype} {tuple(out.shape)}')
        L.adfp_depth_bilateral(depth, V, H, W, radius, ss, sd, sz, out)
    return out


def _takes_bilateral(init):
    """DepthICP(..., bilateral=None): the keyword is taken and validated here, ahead of the constructor proper, whose own keyword list
    (what inspect.signature reports through __wrapped__, and what tests/test_icp_api_signatures.py pins) is the one the ICP had
    before the filter.  The wrapper's __kwdefaults__ carry the new keyword and its default."""
    @functools.wraps(init)
    def __init__(self, *args, bilateral=None, **keywords):
        self.bilateral = bilateral_config(bilateral, points=self._BILATERAL_POINTS)
        init(self, *args, **keywords)
    return __init__


class DepthICP(object):
    """ICP of H x W sensor depth images against one TSDF volume ([1,1,Z,Y,X] float32 on the device) inside `tsdf_bnds`.

    strides / iters: the levels, coarse to fine: iters[k] steps over every strides[k]-th pixel of every strides[k]-th row.  dist_tol
    (metres) and cos_tol gate a pair; min_pivot is the smallest LDL^T pivot over the largest diagonal entry a step accepts; min_pairs
    is the SHARE of a level's strided pixels a step needs as pairs; max_jump (metres, 0: off) invalidates normals across depth
    edges; max_shift (metres) and max_angle (radians) bound how far the result may move from the guess; near (metres of sensor
    depth, 0: from the camera) is where the model's raycast starts marching -- a ray whose first sample lies in unobserved space
    (-1 in a fused volume, which the camera's own voxel is unless another frame saw it) reports no surface.  `engine`: share a
    Renderer's Engine, so that one invalidate_tsdf serves both.  All buffers are allocated here, once; refine() allocates only the
    raycaster's scratch and synchronises nothing.

    bilateral: None or False (off: nothing changes), or a dict with any of radius, sigma_space, sigma_depth, sigma_depth_z2 (the
    arguments of depth_bilateral, with its defaults and its caveat: the mini scene's, tuned on nothing else) and points.  set_frame
    then filters the sensor image (one more launch, between the raycast and the normals; the model image is not filtered) and the
    sensor's normals come from the filtered image.  points True (the default, as KinectFusion does): so do the sensor's points;
    points False: the points are the raw image's, since on clean depth at a small resolution the filter rounds the corners of a room
    and costs a millimetre or two of the final pose."""
    _BILATERAL_POINTS = True           # the default of bilateral's `points`

    @_takes_bilateral
    def __init__(self, tsdf_volume, tsdf_bnds, H, W, fx, fy, cx, cy, engine=None, strides=(4, 2, 1), iters=(4, 3, 3), dist_tol=0.1,
                 cos_tol=0.8, min_pivot=1e-6, min_pairs=0.05, max_jump=0.0, max_shift=0.5, max_angle=0.5, near=0.0):
        self.raycaster = TsdfRaycaster(tsdf_volume, tsdf_bnds, engine=engine)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = int(H), int(W), float(fx), float(fy), float(cx), float(cy)
        self.strides, self.iters = tuple(int(s) for s in strides), tuple(int(n) for n in iters)
        if len(self.strides) != len(self.iters) or not self.strides or min(self.strides) < 1 or min(self.iters) < 0:
            raise ValueError(f'strides {strides!r} and iters {iters!r}: one step count >= 0 per stride >= 1')
        self.dist_tol, self.cos_tol, self.min_pivot, self.min_pairs = float(dist_tol), float(cos_tol), float(min_pivot), float(min_pairs)
        self.max_jump, self.max_shift, self.max_angle = float(max_jump), float(max_shift), float(max_angle)
        self.near = float(near)
        self.n_steps = sum(self.iters)
        dev = self.dev = tsdf_volume.device
        nbytes = int(lib().adfp_icp_workspace_bytes(self.H, self.W))
        if nbytes == 0:
            raise RuntimeError(f'adfp_icp_workspace_bytes refuses a {self.H} x {self.W} image')
        if self.bilateral is None:
            self.depth = torch.zeros((2, self.H, self.W), dtype=torch.float32, device=dev)         # sensor, model
            self.raw_depth = self.points_depth = self.depth[0]
        else:                                              # raw sensor, filtered sensor, model: the last two are the normals' launch
            self._depth3 = torch.zeros((3, self.H, self.W), dtype=torch.float32, device=dev)
            self.depth = self._depth3[1:]
            self.raw_depth = self._depth3[0]
            self.points_depth = self.depth[0] if self.bilateral['points'] else self.raw_depth
        self.normals = torch.zeros((2, self.H, self.W, 3), dtype=torch.float32, device=dev)
        self.p_ref = torch.zeros((4, 4), dtype=torch.float32, device=dev)
        self.state = torch.zeros((_lib.ICP_STATE_BYTES // 8,), dtype=torch.float64, device=dev)
        self.stats = torch.zeros((self.n_steps + 1, _lib.ICP_STATS), dtype=torch.float64, device=dev)
        self.workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
        self.c2w_out = torch.zeros((4, 4), dtype=torch.float32, device=dev)
        self.cam_out = torch.zeros((7,), dtype=torch.float32, device=dev)

    def invalidate_tsdf(self):
        self.raycaster.invalidate_tsdf()

    def strided_pixels(self, stride):
        return ((self.H + stride - 1) // stride) * ((self.W + stride - 1) // stride)

    def pairs_needed(self, stride):
        """min_pairs as a count at this level"""
        return float(math.ceil(self.min_pairs * self.strided_pixels(stride)))

    # ---- the launches ----------------------------------------------------------------------------------------------------------
    def compute_normals(self, depth, out=None):
        """depth [V,H,W] float32 on the device -> normals [V,H,W,3] (adfp_depth_normals, one launch)."""
        _lib.require_cuda(depth, 'depth')
        if depth.dtype != torch.float32 or depth.dim() != 3 or tuple(depth.shape[1:]) != (self.H, self.W) or not depth.is_contiguous():
            raise ValueError(f'depth: expected contiguous float32 [V,{self.H},{self.W}], got {depth.dtype} {tuple(depth.shape)}')
        V = depth.shape[0]
        with _lib.on(depth.device) as L:
            if out is None:
                out = torch.empty((V, self.H, self.W, 3), dtype=torch.float32, device=depth.device)
            L.adfp_depth_normals(depth, V, self.H, self.W, self.fx, self.fy, self.cx, self.cy, self.max_jump, out)
        return out

    def _begin(self, guess, L):
        L.adfp_icp_begin(guess, self.state)

    def _step(self, maps, p_ref, stride, row, L, sums=None, points=None):
        """points: the image the sensor's points come from when it is not the one its normals were taken of (maps' first)"""
        depth, normals = maps
        depth_s = depth[0] if points is None else points
        L.adfp_icp_step(depth_s, normals[0], depth[1], normals[1], p_ref, self.H, self.W, self.fx, self.fy, self.cx, self.cy, int(stride),
                        self.dist_tol, self.cos_tol, self.min_pivot, self.pairs_needed(stride), self.state, self.stats,
                        self.stats.shape[0], int(row), sums, self.workspace, self.workspace.numel() * 8)

    def _end(self, row, L):
        L.adfp_icp_end(self.state, self.max_shift, self.max_angle, self.c2w_out, self.cam_out, self.stats, self.stats.shape[0], int(row))

    def run_steps(self):
        """begin, the steps level by level, end, on the maps and the reference pose this object holds (refine's tail: a fixed sequence
        of launches that a HIP graph can capture).  Returns cam_out [7]."""
        with _lib.on(self.dev) as L:
            self._begin(self.p_ref, L)
            row = 0
            for stride, n in zip(self.strides, self.iters):
                for _ in range(n):
                    self._step((self.depth, self.normals), self.p_ref, stride, row, L, points=self.points_depth)
                    row += 1
            self._end(row, L)
        return self.cam_out

    def set_frame(self, guess_c2w, gt_depth):
        """The refinement's inputs: the sensor depth, the raycast of the prior from the guess, with `bilateral` the filtered sensor
        depth (one launch), both normal maps (one launch)."""
        g = _c2w44(guess_c2w, self.dev, 'guess_c2w')
        if tuple(gt_depth.shape) != (self.H, self.W):
            raise ValueError(f'gt_depth: expected [{self.H},{self.W}], got {tuple(gt_depth.shape)}')
        _lib.require_cuda(gt_depth, 'gt_depth')
        self.p_ref.copy_(g)
        self.raw_depth.copy_(gt_depth)
        self.raycaster.render_depth(self.p_ref, self.H, self.W, self.fx, self.fy, self.cx, self.cy, near=self.near, out=self.depth[1:2])
        if self.bilateral is not None:
            b = self.bilateral
            depth_bilateral(self.raw_depth, b['radius'], b['sigma_space'], b['sigma_depth'], b['sigma_depth_z2'], out=self.depth[0])
        self.compute_normals(self.depth, out=self.normals)

    def refine(self, guess_c2w, gt_depth):
        """guess_c2w [4,4] (or [3,4]) camera-to-world, gt_depth [H,W] on the device -> the camera tensor [7] float32 on the device
        (this object's own buffer: the next refine overwrites it).  The guess itself comes back when the refinement fails."""
        self.set_frame(guess_c2w, gt_depth)
        return self.run_steps()

    def last_stats(self):
        """The stats rows of the last refinement on the host (one download): a row per step -- pairs, rmse before the update,
        smallest pivot ratio, |omega|, |t|, status -- and the gate's row: 0, 0, 0, angle and shift from the guess, final status."""
        return self.stats.cpu()

    def last_status(self):
        return int(self.last_stats()[-1, 5].item())

    def step_system(self, c2w, depth_s, normals_s, depth_m, normals_m, p_ref, stride=1):
        """One step from the estimate `c2w` (float32 [4,4]) on the caller's maps: -> (sums [29] float64, stats row [6], estimate
        after the step [4,4] float32, its camera tensor [7]), all on the device.  For tests: the sums are the step's normal
        equations as adfp_icp_step's order lists them."""
        dev = self.dev
        c2w = c2w.detach().to(dev, torch.float32).contiguous()
        p_ref = p_ref.detach().to(dev, torch.float32).contiguous()
        depth = torch.stack([depth_s.to(dev, torch.float32), depth_m.to(dev, torch.float32)]).contiguous()
        normals = torch.stack([normals_s.to(dev, torch.float32), normals_m.to(dev, torch.float32)]).contiguous()
        if tuple(depth.shape) != (2, self.H, self.W) or tuple(normals.shape) != (2, self.H, self.W, 3):
            raise ValueError(f'maps: expected [{self.H},{self.W}] depths and [{self.H},{self.W},3] normals')
        sums = torch.zeros((_lib.ICP_SUMS,), dtype=torch.float64, device=dev)
        with _lib.on(dev) as L:
            self._begin(c2w, L)
            self._step((depth, normals), p_ref, stride, 0, L, sums=sums)
            # no gate: the step's own result comes out
            L.adfp_icp_end(self.state, float('inf'), float('inf'), self.c2w_out, self.cam_out, None, 0, 0)
        return sums, self.stats[0].clone(), self.c2w_out.clone(), self.cam_out.clone()


RGB_STATS_COLUMNS = ('rgb_pairs', 'rgb_rmse')


def _c2w44(c2w, dev, what='c2w'):
    """[4,4] or [3,4], numpy or torch, anywhere -> [4,4] float32 on `dev`; `what` names the argument in the refusal"""
    if isinstance(c2w, np.ndarray):
        c2w = torch.from_numpy(c2w)
    g = c2w.detach().to(dev, torch.float32)
    if tuple(g.shape) == (3, 4):
        g = torch.cat([g, g.new_tensor([[0., 0., 0., 1.]])], 0)
    if tuple(g.shape) != (4, 4):
        raise ValueError(f'{what}: expected [4,4] or [3,4], got {tuple(c2w.shape)}')
    return g


class RgbdICP(DepthICP):
    """DepthICP whose every step adds a photometric term against the last tracked frame (the "keyframe": its sensor colour, its
    sensor depth and its final pose) to the geometric normal equations (adfp_rgbd_frame_map, adfp_rgbd_step, csrc/adfp_rgbd.h; the
    rule: include/adfp.h "RGB-D ICP", tests/rgbd_icp_ref.py).  Texture constrains the directions a view of one or two walls leaves
    free, and a frame-to-frame term needs no prior, so an empty model image still yields pairs.

        icp = RgbdICP(tsdf_volume, tsdf_bnds, H, W, fx, fy, cx, cy, engine=renderer._engine, rgb_weight=1.0)
        icp.set_keyframe(c2w0, color0, depth0)             # the first frame
        cam = icp.refine(guess_c2w, gt_depth, gt_color)    # [7] float32 on the device
        icp.promote(final_c2w)                             # the frame just refined becomes the keyframe

    rgb_weight multiplies the photometric normal equations (intensities are 0..1, geometric residuals metres), rgb_tol drops pairs
    whose intensities differ by more; both defaults are the mini scene's and have not been tuned on anything else.  Before the first
    set_keyframe, and with rgb_weight 0, a step is the depth rule.  Everything is allocated here, once.

    bilateral (DepthICP's keyword): the sensor's normals come from the filtered image.  The frame map is always built from the raw
    sensor depth, so maps[0], and after promote the keyframe's map, are the bytes they are without the filter; a step reads the
    sensor's depth from that map, so the points are the raw image's: `points` defaults to False here and True is refused."""
    _BILATERAL_POINTS = False

    def __init__(self, tsdf_volume, tsdf_bnds, H, W, fx, fy, cx, cy, engine=None, rgb_weight=1.0, rgb_tol=0.25, **depth_icp_keywords):
        super().__init__(tsdf_volume, tsdf_bnds, H, W, fx, fy, cx, cy, engine=engine, **depth_icp_keywords)
        if self.bilateral is not None and self.bilateral['points']:
            raise ValueError('RgbdICP: bilateral points True is not available, a joint step reads the sensor depth from the frame map, '
                             'which is built from the raw depth')
        self.rgb_weight, self.rgb_tol = float(rgb_weight), float(rgb_tol)
        if not self.rgb_weight >= 0 or self.rgb_tol != self.rgb_tol:
            raise ValueError(f'rgb_weight {rgb_weight!r} must be >= 0 and rgb_tol {rgb_tol!r} a number')
        dev = self.dev
        nbytes = int(lib().adfp_rgbd_workspace_bytes(self.H, self.W))
        self.maps = torch.zeros((2, self.H, self.W, 4), dtype=torch.float32, device=dev)          # current frame, keyframe
        self.p_key = torch.zeros((4, 4), dtype=torch.float32, device=dev)
        self.rgb_stats = torch.zeros((self.n_steps + 1, _lib.RGBD_STATS), dtype=torch.float64, device=dev)
        self.rgbd_workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
        self.has_keyframe = False

    def frame_map(self, color, depth, out=None):
        """color [H,W,3], depth [H,W] float32 on the device -> [H,W,4] = (I, gx, gy, d) (adfp_rgbd_frame_map, one launch)."""
        _lib.require_cuda(color, 'color')
        _lib.require_cuda(depth, 'depth')
        H, W = self.H, self.W
        if tuple(color.shape) != (H, W, 3) or tuple(depth.shape) != (H, W) or color.dtype != torch.float32 or depth.dtype != torch.float32:
            raise ValueError(f'expected float32 color [{H},{W},3] and depth [{H},{W}], got {color.dtype} {tuple(color.shape)} and '
                             f'{depth.dtype} {tuple(depth.shape)}')
        color, depth = color.detach().contiguous(), depth.detach().contiguous()
        with _lib.on(depth.device) as L:
            if out is None:
                out = torch.empty((H, W, 4), dtype=torch.float32, device=depth.device)
            L.adfp_rgbd_frame_map(color, depth, H, W, out)
        return out

    def set_keyframe(self, c2w, color, depth):
        """The frame the photometric term compares with: its pose and one frame-map launch into the keyframe map."""
        self.p_key.copy_(_c2w44(c2w, self.dev))
        self.frame_map(color, depth, out=self.maps[1])
        self.has_keyframe = True

    def promote(self, c2w):
        """The frame last given to refine becomes the keyframe, at the pose `c2w`.  A copy, not a swap of pointers: a captured graph
        of run_steps stays valid."""
        self.p_key.copy_(_c2w44(c2w, self.dev))
        self.maps[1].copy_(self.maps[0])
        self.has_keyframe = True

    def _rgbd_step(self, cur, normals, depth_m, p_ref, stride, row, L, sums=None, key=True):
        key = key and self.has_keyframe
        L.adfp_rgbd_step(cur, normals[0], depth_m, normals[1], p_ref, self.maps[1] if key else None, self.p_key if key else None,
                         self.H, self.W, self.fx, self.fy, self.cx, self.cy, int(stride), self.dist_tol, self.cos_tol, self.rgb_weight,
                         self.rgb_tol, self.min_pivot, self.pairs_needed(stride), self.state, self.stats, self.rgb_stats,
                         self.stats.shape[0], int(row), sums, self.rgbd_workspace, self.rgbd_workspace.numel() * 8)

    def run_steps(self):
        """DepthICP.run_steps with adfp_rgbd_step on the maps this object holds.  Returns cam_out [7]."""
        with _lib.on(self.dev) as L:
            self._begin(self.p_ref, L)
            row = 0
            for stride, n in zip(self.strides, self.iters):
                for _ in range(n):
                    self._rgbd_step(self.maps[0], self.normals, self.depth[1], self.p_ref, stride, row, L)
                    row += 1
            self._end(row, L)
        return self.cam_out

    def refine(self, guess_c2w, gt_depth, gt_color):
        """DepthICP.refine with the frame's colour [H,W,3]: the parent's set_frame, one frame-map launch, the joint steps."""
        self.set_frame(guess_c2w, gt_depth)
        self.frame_map(gt_color, self.raw_depth, out=self.maps[0])
        return self.run_steps()

    def last_rgb_stats(self):
        """The photometric (pairs, rmse) of the last refinement's steps on the host, row for row beside last_stats (the gate's row: 0)."""
        return self.rgb_stats.cpu()

    def step_system_rgbd(self, c2w, cur_map, normals_s, depth_m, normals_m, p_ref, key_map=None, p_key=None, stride=1):
        """One joint step from the estimate `c2w` on the caller's maps (key_map None: no photometric term): -> (sums [31] float64,
        stats row [6], rgb stats row [2], estimate after the step [4,4] float32, its camera tensor [7]), all on the device.  For
        tests, in the manner of step_system.  The keyframe this object holds is left as it was."""
        dev = self.dev
        c2w, p_ref = _c2w44(c2w, dev).contiguous(), _c2w44(p_ref, dev).contiguous()
        cur = cur_map.to(dev, torch.float32).contiguous()
        normals = torch.stack([normals_s.to(dev, torch.float32), normals_m.to(dev, torch.float32)]).contiguous()
        depth_m = depth_m.to(dev, torch.float32).contiguous()
        if tuple(cur.shape) != (self.H, self.W, 4) or tuple(normals.shape) != (2, self.H, self.W, 3) or tuple(depth_m.shape) != (self.H, self.W):
            raise ValueError(f'maps: expected a [{self.H},{self.W},4] map, a [{self.H},{self.W}] depth and [{self.H},{self.W},3] normals')
        if (key_map is None) != (p_key is None):
            raise ValueError('key_map and p_key: both or neither')
        saved = (self.maps[1].clone(), self.p_key.clone(), self.has_keyframe)
        if key_map is not None:
            self.maps[1].copy_(key_map.to(dev, torch.float32))
            self.p_key.copy_(_c2w44(p_key, dev))
        self.has_keyframe = key_map is not None
        sums = torch.zeros((_lib.RGBD_SUMS,), dtype=torch.float64, device=dev)
        with _lib.on(dev) as L:
            self._begin(c2w, L)
            self._rgbd_step(cur, normals, depth_m, p_ref, stride, 0, L, sums=sums)
            L.adfp_icp_end(self.state, float('inf'), float('inf'), self.c2w_out, self.cam_out, None, 0, 0)
        out = sums, self.stats[0].clone(), self.rgb_stats[0].clone(), self.c2w_out.clone(), self.cam_out.clone()
        self.maps[1].copy_(saved[0])
        self.p_key.copy_(saved[1])
        self.has_keyframe = saved[2]
        return out
