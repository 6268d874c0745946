"""
Drop-in for the reference's ``src/utils/Renderer.py``: same constructor, same methods, same
argument order (note ``render_batch_ray(c, decoders, rays_d, rays_o, ...)`` takes d BEFORE o),
same return dtypes -- implemented on the MI355X by libadfp.so.

  Renderer(cfg, args, slam, points_batch_size=500000, ray_batch_size=100000)   Renderer.py:7-25
  eval_points(p, decoders, tsdf_volume, tsdf_bnds, c, stage, device)            Renderer.py:27-71
  sample_grid_tsdf / eval_points_tsdf                                          Renderer.py:73-107
  render_batch_ray(c, decoders, rays_d, rays_o, device, tsdf_volume, tsdf_bnds,
                   stage, gt_depth) -> (depth f64, uncertainty f64, color, weight[N,S,1])
                                                                                Renderer.py:110-255
  render_img(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage, gt_depth)  Renderer.py:258-327
  render_novel(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage)          not in the reference: a frame without sensor depth
"""
import torch

from . import _lib
from .common import get_rays
from .engine import Engine


class Renderer(object):
    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.ray_batch_size = ray_batch_size
        self.points_batch_size = points_batch_size      # kept for API parity; the kernels do not chunk
        r = cfg['rendering']
        self.lindisp = r['lindisp']
        self.perturb = r['perturb']
        self.N_samples = r['N_samples']
        self.N_surface = r['N_surface']
        self.N_importance = r['N_importance']
        self.scale = cfg['scale']
        self.occupancy = cfg['occupancy']
        self.bound = slam.bound
        self.sample_mode = 'bilinear'
        self.tsdf_bnds = slam.vol_bnds
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.resolution = cfg['meshing']['resolution']
        if self.N_importance > 0:
            raise NotImplementedError('N_importance > 0 is dead (and broken) in the reference '
                                      '(configs/df_prior.yaml:96, Renderer.py:235-252); not supported')
        if not self.occupancy:
            raise NotImplementedError('occupancy=False (density compositing) is not used by the reference '
                                      'configs (configs/df_prior.yaml:4); not supported')
        self.need_param_grad = True          # see render_batch_ray
        # Not in the reference: a large inference batch whose rays arrive in INCOHERENT order (e.g. a random subset of several
        # images' pixels) is rendered in a spatially sorted order and handed back in the caller's (see _coherent_order).
        self.sort_rays_min = 65536           # batches below this are not looked at (0 / None: never sort)
        # TSDF layout for INCOHERENT batches (the order probe's verdict): 'auto' = the corner-block copy of the volume (Engine.tsdf_blocks:
        # one aligned 32-byte piece per lookup instead of four 8-byte column pieces in four sectors; 8 x the volume's memory, built once),
        # False = never.  Coherent batches (frames in pixel order) always read the volume as it stands.
        # ADFP_TSDF_BLOCKS=0 in the HOST process's environment is the deployment switch (e.g. a Tracker and a Mapper process sharing
        # one smaller-memory GPU: each process would hold its own copy): the library itself reads no environment.
        import os
        self.tsdf_blocks = False if os.environ.get('ADFP_TSDF_BLOCKS', 'auto').lower() in ('0', 'off', 'false', 'no') else 'auto'
        # Sorting an incoherent batch by (origin cell, surface cell) on top of that: round 4's answer to such batches (TSDF stage
        # 0.66 -> 1.22 TB/s on the plain volume).  With the corner blocks the stage runs at 1.8 TB/s as given and 2.05 TB/s sorted, and
        # keys + radix sort + four gathers + the outputs' way back cost more than the 0.04 ms that saves (whole 131 072-ray batch:
        # 4.58 ms as given, 4.63 ms sorted; profiles/r05_config5.json) -- so it is taken only when the corner blocks are not (switched
        # off, or no room for 8 x the volume).
        self.sort_incoherent = 'auto'
        self._order_verdict = {}             # batch size -> pinned verdict words of adfp_ray_order_probe
        self._engine = Engine()

    def check_overflow(self, device=None, decoders=None):
        """Not in the reference.  The default f16-split decoders (ADFP_MATH=f16x3) cannot represent operands with |x| >= 65504.
        A call that meets one repairs its outputs on the device (an f32 fallback kernel, csrc/adfp_fallback.h) and the next call
        runs that network on the exact f32 kernels -- nothing is raised and no invalid value is handed out.  This waits for the
        device and returns the set of networks of `decoders` that are latched to the exact kernels (empty = all f16-split)."""
        torch.cuda.synchronize(device)
        if decoders is None:
            return set()
        decoders.absorb_status()
        return set(decoders._exact_latch)

    def invalidate_tsdf(self):
        """Not in the reference (its TSDF is static for a run).  Call after the TSDF volume was written by something PyTorch's version
        counter does not see (another process through CUDA IPC, a raw-pointer kernel): the corner-block copy incoherent batches read
        (`tsdf_blocks`) is rebuilt from the volume on its next use.  `fusion.TSDFVolume.integrate` needs no call (it bumps the
        version), nor does any in-place torch op on the volume."""
        self._engine.invalidate_tsdf_blocks()

    # ---- point queries --------------------------------------------------------------------
    def eval_points(self, p, decoders, tsdf_volume, tsdf_bnds, c=None, stage='color', device='cuda:0'):
        """raw [P,4] (rgb, occ; occ = 100 outside ``self.bound``) and attention weight [P]."""
        return self._engine.eval_points(decoders, p, c, tsdf_volume, tsdf_bnds, self.bound, stage,
                                        apply_bound_rule=True)

    def sample_grid_tsdf(self, p, tsdf_volume, device='cuda:0'):
        """Trilinear TSDF lookup of p [1, P, 3] -> [1, 1, P] (grid_sample's [N, C, P], Renderer.py:73-81)."""
        return self._engine.sample_tsdf(p, tsdf_volume, self.tsdf_bnds).reshape(1, 1, -1)

    def eval_points_tsdf(self, p, tsdf_volume, device='cuda:0'):
        """TSDF value of every point of p [P,3] -> [1, P] (Renderer.py:84-107: sample_grid_tsdf(...).squeeze(0))."""
        return self.sample_grid_tsdf(p, tsdf_volume, device).squeeze(0)

    # ---- rays -----------------------------------------------------------------------------
    def render_batch_ray(self, c, decoders, rays_d, rays_o, device, tsdf_volume, tsdf_bnds, stage, gt_depth=None,
                         depth_max=None, need_param_grad=None):
        """Render depth / uncertainty / colour / attention weight of a batch of rays.

        ``depth_max`` (not in the reference) lets a ray shard use the max sensor depth of the full
        batch so that sharded renders reproduce the unsharded far clamp (Renderer.py:159, :195).
        ``need_param_grad`` (not in the reference; default = ``self.need_param_grad`` = True): False skips the
        decoder-parameter gradients in the backward.  The reference's Tracker deep-copies decoders whose
        parameters keep requires_grad=True although only the camera pose is optimised (src/Tracker.py:144, :112-133);
        autograd then computes weight gradients nobody reads.  A tracker sets ``renderer.need_param_grad = False``
        (or calls ``decoders.requires_grad_(False)``) and pays for the ray gradients only."""
        _lib.require_cuda(rays_o, 'rays_o')
        N = rays_o.shape[0]
        t_rand = None
        if self.perturb > 0.:
            t_rand = torch.rand(N, self.N_samples)                        # CPU generator, as Renderer.py:216
        if need_param_grad is None:
            need_param_grad = self.need_param_grad
        needs_grad = torch.is_grad_enabled() and (
            any(v.requires_grad for v in c.values()) or (need_param_grad and decoders.any_requires_grad())
            or rays_o.requires_grad or rays_d.requires_grad)
        if needs_grad:
            from .autograd import render_with_grad
            return render_with_grad(self._engine, decoders, c, rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds,
                                    self.bound, stage, self.N_samples, self.N_surface, self.lindisp, self.perturb,
                                    t_rand, depth_max, need_param_grad)
        perm, blocks = None, False
        if self.sort_rays_min and N >= self.sort_rays_min and stage != 'low' and gt_depth is not None and t_rand is None:
            incoherent = self._batch_is_incoherent(rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds)
            if incoherent:
                blocks = bool(self.tsdf_blocks) and self._engine.tsdf_blocks(tsdf_volume) is not None
                if self.sort_incoherent is True or (self.sort_incoherent == 'auto' and not blocks):
                    perm = self._coherent_order(rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds, probe=False)
        if perm is not None:
            # rays are independent units: the far clamp's batch maximum (Renderer.py:159, :195) is order-free, everything else is
            # per ray -- the sorted render returns the same values, restored to the caller's order
            if depth_max is None:
                depth_max = gt_depth.detach().reshape(-1).float().max().reshape(1)
            d, u, col, w, _ = self._engine.render_forward(
                decoders, c, rays_o.detach().index_select(0, perm), rays_d.detach().index_select(0, perm),
                gt_depth.detach().reshape(-1).index_select(0, perm), tsdf_volume, tsdf_bnds, self.bound, stage,
                self.N_samples, self.N_surface, self.lindisp, self.perturb, None, depth_max, tsdf_blocks=blocks)
            depth, unc, color, weight = torch.empty_like(d), torch.empty_like(u), torch.empty_like(col), torch.empty_like(w)
            depth.index_copy_(0, perm, d)
            unc.index_copy_(0, perm, u)
            color.index_copy_(0, perm, col)
            weight.index_copy_(0, perm, w)
            return depth, unc, color, weight
        depth, unc, color, weight, _ = self._engine.render_forward(
            decoders, c, rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds, self.bound, stage,
            self.N_samples, self.N_surface, self.lindisp, self.perturb, t_rand, depth_max, tsdf_blocks=blocks)
        return depth, unc, color, weight

    @staticmethod
    def _f32_rays(rays_o, rays_d, gt_depth):
        ro = rays_o.detach()
        if ro.dtype != torch.float32 or not ro.is_contiguous():
            ro = ro.float().contiguous()
        rd = rays_d.detach()
        if rd.dtype != torch.float32 or not rd.is_contiguous():
            rd = rd.float().contiguous()
        gd = gt_depth.detach().reshape(-1)
        if gd.dtype != torch.float32 or not gd.is_contiguous():
            gd = gd.float().contiguous()
        return ro, rd, gd

    def _batch_is_incoherent(self, rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds, wait=False):
        """Are the neighbours of this batch's rays unrelated (a random subset of an image) rather than neighbouring pixels?

        Why it matters: the TSDF lookup of the volume as it stands fetches four 8-byte column pieces per sample.  In pixel order a
        wave's 64 lanes (the same sample of 64 neighbouring rays) find them in a few cache lines; with unrelated neighbours every piece
        is its own 64-byte sector and its own page (1024^3 volume, 131 072 random rays x 128 samples: 175 B fetched per sample against
        9 B in pixel order, profiles/r04_pmc_hbm_config5_random.csv).  Such a batch reads the corner-block copy of the volume instead
        (one aligned 32-byte piece per lookup, Engine.tsdf_blocks) and / or is rendered in spatial order (_coherent_order).

        Measured by ONE tiny kernel (adfp_ray_order_probe: do consecutive rays land within a few voxels of each other?) that writes
        its verdict to pinned host memory; nothing waits for it -- the verdict of a call steers the NEXT call of the same batch size
        (callers send streams of like batches: frames in pixel order, or random draws).  `wait=True` (tests, bench) waits for this
        batch's own verdict."""
        import ctypes as C
        dev = rays_o.device
        N = rays_o.shape[0]
        L = _lib.lib()
        ro, rd, gd = self._f32_rays(rays_o, rays_d, gt_depth)
        slot = self._order_verdict.get(N)
        if slot is None:
            ext = self._engine.host_bound(tsdf_bnds, 'tsdf_bnds')
            Z, Y, X = tsdf_volume.shape[2:]
            voxel = max((ext[0][1] - ext[0][0]) / X, (ext[1][1] - ext[1][0]) / Y, (ext[2][1] - ext[2][0]) / Z)
            word = torch.zeros(2, dtype=torch.int32).pin_memory()
            slot = self._order_verdict[N] = (word, C.c_int.from_address(word.data_ptr()), C.c_int.from_address(word.data_ptr() + 4), 8.0 * voxel)
        word, far, pairs, far_distance = slot
        with _lib.device_guard(dev):
            st = _lib.current_stream(dev)
            incoherent = pairs.value > 0 and 2 * far.value > pairs.value              # the PREVIOUS like batch's verdict
            _lib.check(L.adfp_ray_order_probe(_lib.ptr(ro), _lib.ptr(rd), _lib.ptr(gd), N, far_distance, C.c_void_p(word.data_ptr()), st),
                       'adfp_ray_order_probe')
            if wait:
                torch.cuda.synchronize(dev)
                incoherent = 2 * far.value > pairs.value
        return incoherent

    def _coherent_order(self, rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds, wait=False, probe=True):
        """None if the batch is coherent (probe=True: _batch_is_incoherent is asked first), otherwise the permutation (int64 [N]) that
        sorts its rays by (cell of the origin, cell of the surface point) -- adfp_ray_sort_keys + the library's radix sort.  A 5 %
        random sample of an image stays sparser than the image after sorting, but the rays a workgroup walks together are
        millimetres to centimetres apart again."""
        import ctypes as C
        if probe and not self._batch_is_incoherent(rays_o, rays_d, gt_depth, tsdf_volume, tsdf_bnds, wait=wait):
            return None
        dev = rays_o.device
        N = rays_o.shape[0]
        L = _lib.lib()
        ro, rd, gd = self._f32_rays(rays_o, rays_d, gt_depth)
        with _lib.device_guard(dev):
            st = _lib.current_stream(dev)
            key, val = torch.empty((N,), dtype=torch.int32, device=dev), torch.empty((N,), dtype=torch.int32, device=dev)
            kt, vt = torch.empty_like(key), torch.empty_like(val)
            b = _lib.Bound()
            _lib.fill_bound(b, self._engine.host_bound(tsdf_bnds, 'tsdf_bnds'))
            _lib.check(L.adfp_ray_sort_keys(_lib.ptr(ro), _lib.ptr(rd), _lib.ptr(gd), N, C.byref(b), _lib.ptr(key), _lib.ptr(val), st), 'adfp_ray_sort_keys')
            nb = int(L.adfp_sort_workspace_bytes(N))
            ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
            _lib.check(L.adfp_sort_pairs(_lib.ptr(key), _lib.ptr(val), _lib.ptr(kt), _lib.ptr(vt), N, 30, _lib.ptr(ws), nb, st), 'adfp_sort_pairs')
        return val.long()

    def _fits_in_one_call(self, n, S, dev):
        """ray_batch_size exists in the reference to BOUND memory (Renderer.py:294-313).  The one-call frame needs the forward
        workspace for all n x S samples at once (~37 B per sample x 1.25) plus the [n, S] attention-weight output; it is taken
        only when that fits in half of what the device has free (or the engine's workspace is that large already) -- otherwise
        the frame is rendered batch by batch like the reference's."""
        need_ws = int(_lib.lib().adfp_workspace_bytes(n * S))
        ws = self._engine._ws
        have = ws.numel() if ws is not None and ws.device == dev else 0
        extra = (int(need_ws * 1.25) if have < need_ws else 0) + n * (4 * S + 28)
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        return extra <= free // 2

    def segment_depth_max(self, gt_depth):
        """max(gt_depth) of every ray_batch_size segment of a frame (float32 [nseg]): what each of render_img's batches clamps `far`
        with (src/utils/Renderer.py:294-313 with :159, :195)."""
        gd = gt_depth.detach().reshape(-1).float()
        n, B = gd.shape[0], self.ray_batch_size
        nseg = (n + B - 1) // B
        if nseg * B != n:
            gd = torch.nn.functional.pad(gd, (0, nseg * B - n), value=float('-inf'))
        return gd.view(nseg, B).amax(dim=1).contiguous()

    def render_img_shard(self, c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage, gt_depth, lo, hi):
        """Not in the reference: pixels [lo, hi) (row-major) of the frame render_img returns, as flat (depth [hi-lo] f64,
        uncertainty [hi-lo] f64, colour [hi-lo,3] f32) -- one GPU's contiguous share of a ray-sharded frame (SURVEY.md section 8e,
        dist.render_img_sharded).  Bit for bit the values of render_img: a ray sees its batch only through the max(gt_depth) of its
        ray_batch_size segment, and those maxima are taken over the WHOLE frame here (adfp_render_args.depth_max_first_ray)."""
        if gt_depth is None or self.perturb > 0:
            raise NotImplementedError('render_img_shard: a frame with sensor depth and perturb = 0 (what render_img is called with)')
        with torch.no_grad():
            H, W = self.H, self.W
            lo, hi = int(lo), int(hi)
            if not (0 <= lo <= hi <= H * W):
                raise ValueError(f'render_img_shard: [{lo}, {hi}) is not a pixel range of a {H}x{W} frame')
            if (H * W + self.ray_batch_size - 1) // self.ray_batch_size > 48:
                raise NotImplementedError('render_img_shard: more than 48 ray batches per frame')
            # ONE call, whose first launch also writes the rays of the rank's OWN pixels and reduces the whole frame's segment
            # maxima (adfp_frame_job): a rank spends nothing on the rays of the other ranks' pixels, and no launch on the maxima
            depth, unc, color, _, _ = self._engine.render_forward(
                decoders, c, None, None, None, tsdf_volume, tsdf_bnds, self.bound, stage, self.N_samples, self.N_surface, self.lindisp,
                self.perturb, None, None, depth_max_segment=self.ray_batch_size, depth_max_first_ray=lo, frame=self._frame_job(c2w, gt_depth, hi - lo))
            return depth, unc, color

    def _frame_job(self, c2w, gt_depth, n_rays):
        import numpy as np
        if isinstance(c2w, np.ndarray):
            c2w = torch.from_numpy(c2w)
        return dict(c2w=c2w, H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, depth=gt_depth, n_rays=n_rays)

    def render_img(self, c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage, gt_depth=None):
        """Full-frame render under no_grad in ``ray_batch_size`` batches -> depth [H,W] f64,
        uncertainty [H,W] f64, color [H,W,3] f32.  Each batch clamps ``far`` with ITS OWN max
        depth, exactly like the reference's loop (Renderer.py:294-313)."""
        with torch.no_grad():
            H, W = self.H, self.W
            if gt_depth is not None:
                gt_depth = gt_depth.reshape(-1)
            n, S = H * W, self.N_samples + (self.N_surface if gt_depth is not None else 0)
            nseg = (n + self.ray_batch_size - 1) // self.ray_batch_size
            on_gpu = torch.device(device).type == 'cuda' and gt_depth is not None and gt_depth.is_cuda
            if on_gpu and self.perturb == 0 and 1 < nseg <= 48 and n * S < 2 ** 31 and self._fits_in_one_call(n, S, gt_depth.device):
                # The reference walks the frame in ray batches (memory), and the only thing a batch shares is max(gt_depth) for
                # the far clamp -- carried per SEGMENT of ray_batch_size rays here (adfp_render_args.depth_max_segment), the whole
                # frame is one kernel sequence with the batched loop's values bit for bit (tests: the golden image was rendered
                # by the reference in 1 000-ray batches).  The rays come out of the call's first launch (adfp_frame_job).
                depth, unc, color, _, _ = self._engine.render_forward(
                    decoders, c, None, None, None, tsdf_volume, tsdf_bnds, self.bound, stage, self.N_samples, self.N_surface, self.lindisp,
                    self.perturb, None, None, depth_max_segment=self.ray_batch_size, frame=self._frame_job(c2w, gt_depth, n))
                return depth.reshape(H, W), unc.reshape(H, W), color.reshape(H, W, 3)
            rays_o, rays_d = get_rays(H, W, self.fx, self.fy, self.cx, self.cy, c2w, device)
            rays_o = rays_o.reshape(-1, 3)
            rays_d = rays_d.reshape(-1, 3)
            ds, us, cs = [], [], []
            for i in range(0, rays_d.shape[0], self.ray_batch_size):
                sl = slice(i, i + self.ray_batch_size)
                d, u, col, _ = self.render_batch_ray(c, decoders, rays_d[sl], rays_o[sl], device, tsdf_volume,
                                                     tsdf_bnds, stage,
                                                     gt_depth=None if gt_depth is None else gt_depth[sl])
                ds.append(d.double())
                us.append(u.double())
                cs.append(col)
            depth = torch.cat(ds, dim=0).reshape(H, W)
            uncertainty = torch.cat(us, dim=0).reshape(H, W)
            color = torch.cat(cs, dim=0).reshape(H, W, 3)
            return depth, uncertainty, color

    def render_novel(self, c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage):
        """Not in the reference, whose render_img needs a sensor depth image (Renderer.py:292): a full frame from a pose that has
        none -> (depth [H,W] f64, uncertainty [H,W] f64, color [H,W,3] f32, guide [H,W] f32).  The guide is the raycast of the
        TSDF prior (tsdf_raycast.TsdfRaycaster: the first + -> - crossing along every pixel's ray, 0 where there is none) and
        takes gt_depth's place in render_img: 16 of a ray's samples sit within 5 % of it, and a pixel whose ray meets no surface
        is sampled like a pixel without sensor depth.  The raycaster shares this Renderer's engine: invalidate_tsdf() drops its
        empty-space bitmap together with the corner-block copy."""
        from .tsdf_raycast import TsdfRaycaster
        rc = getattr(self, '_novel', None)
        if rc is None or rc.tsdf_volume is not tsdf_volume or rc.tsdf_bnds is not tsdf_bnds:
            rc = self._novel = TsdfRaycaster(tsdf_volume, tsdf_bnds, engine=self._engine)
        with torch.no_grad():
            guide = rc.render_depth(c2w, self.H, self.W, self.fx, self.fy, self.cx, self.cy)
        depth, uncertainty, color = self.render_img(c, decoders, c2w, device, tsdf_volume, tsdf_bnds, stage, gt_depth=guide)
        return depth, uncertainty, color, guide
