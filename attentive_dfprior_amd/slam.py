"""The run itself: ``DF_Prior``, ``Mapper``, ``Tracker`` and ``Logger`` with the reference's constructor signatures and attribute
names (src/DF_Prior.py, src/Mapper.py, src/Tracker.py, src/utils/Logger.py), from a dataset directory to checkpoints, meshes and the
trajectory error in ONE process on one MI355X.

The hot paths are the graph-replayed iterations of this package: ``mapping.MapperIteration`` (one ``step`` per mapping iteration)
and ``tracking.TrackerIteration`` (one ``step`` per tracking iteration).  Around them the loops keep the reference's rules: which
frames are mapped, the stage and warm-up term of every iteration, the keyframe window, the keyframe / checkpoint / mesh rules, the
colour refinement of the last frame, the constant-speed pose guess.  Per tracked frame the host adds one 16-float download (the
tracked pose), one 7-float upload (the next guess) and the decode of the next frame, which a background thread does ahead of the
GPU (``FrameFeed``).

Deliberate differences from the reference:
  * one process.  The reference starts a Tracker and a Mapper process and synchronises them through shared tensors; here ``run()``
    walks the frames in the order ``sync_method: strict`` produces.  ``loose`` and ``free`` run in that order too (one logged line).
  * the Tracker reads the Mapper's grids and decoders instead of deep copies of them: nothing maps while it tracks.
  * ``tracking.iters: 0`` keeps the constant-speed guess (the reference would fail on ``candidate_cam_tensor = None``).
  * ``pretrained_decoders.low_high: null`` leaves the decoders as the seed initialised them.
  * ``--prior online``: the TSDF prior is fused during the run from the ESTIMATED poses of the mapped frames.
  * ``--last_frame N`` ends the run at frame N (the reference hard-codes frame 4640 of ScanNet scene 50).
  * ``mapping.BA: True`` (default False): bundle adjustment as the reference's parent project runs it -- with more than four
    keyframes the window's poses, all but the oldest keyframe's, are optimised with the map (``mapping.BA_cam_lr``, stage color).
  * ``tracking.init: icp`` (default ``guess``): the constant-speed guess is refined by point-to-plane ICP of the frame's whole depth
    image against the raycast of the TSDF prior (``icp.DepthICP``) before the iterations start from it; with ``tracking.iters: 0``
    the refined pose is the frame's pose.  ``Tracker.icp_status`` holds one status per tracked frame.
  * ``tracking.icp.bilateral: {radius, sigma_space, sigma_depth, sigma_depth_z2, points}`` (absent, null or false: off; ``{}``: the
    defaults 2, 1.5 px, 0.05 m, 0, true): the ICP takes the sensor's normals, and with ``points`` its points, from the bilaterally
    filtered sensor depth (``icp.depth_bilateral``).  Only the ICP sees the filtered image: the iterations, the Mapper and the
    online prior's fusion read the raw depth.  ``--tracking_icp_bilateral`` switches it on with the defaults.
"""
import logging
import os
import random
import shutil
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import get_model
from .common import get_camera_from_tensor, get_tensor_from_camera, random_select
from .config import TRACKING_INITS, mapping_setting, tracking_setting

log = logging.getLogger('attentive_dfprior_amd')
STAGES = ('low', 'high', 'color')


def setup_seed(seed):
    """The reference's run.py:11-16."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


class FrameFeed(object):
    """Frames of a dataset reader in increasing order, decoded one frame ahead.

    ``get(idx)`` returns ``(color, depth, gt_c2w)``: the two images on the reader's device (``reader.ingest``: one upload and one
    launch, on the calling thread and its current stream) and the ground-truth pose as the CPU tensor ``reader.pose`` gives.  With
    ``prefetch`` a single background thread runs ``reader._decode(idx + 1)`` (file reads and JPEG / PNG decoding: host work that
    touches no device) while the caller works on frame idx.  Results do not depend on it: the decoded bytes are the same.

    ``decode_s`` sums the time spent decoding (on whichever thread), ``wait_s`` the time ``get`` waited for a decoded frame."""

    def __init__(self, reader, n_img=None, prefetch=True):
        self.reader = reader
        self.n_img = len(reader) if n_img is None else int(n_img)
        self.prefetch = bool(prefetch)
        self._pool = ThreadPoolExecutor(max_workers=1) if self.prefetch else None
        self._pending = {}
        self.decode_s = 0.0
        self.wait_s = 0.0
        self.frames = 0

    def _decode(self, idx):
        t0 = time.perf_counter()
        out = self.reader._decode(idx)
        return out, time.perf_counter() - t0

    def get(self, idx):
        t0 = time.perf_counter()
        fut = self._pending.pop(idx, None)
        decoded, dt = fut.result() if fut is not None else self._decode(idx)
        self.wait_s += time.perf_counter() - t0
        self.decode_s += dt
        self.frames += 1
        if self.prefetch and idx + 1 < self.n_img and idx + 1 not in self._pending:
            self._pending[idx + 1] = self._pool.submit(self._decode, idx + 1)
        color, depth = self.reader.ingest(*decoded)
        return color, depth, self.reader.pose(idx)

    def close(self):
        for fut in self._pending.values():
            fut.cancel()
        self._pending = {}
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None


class Logger(object):
    """Save checkpoints to file (src/utils/Logger.py)."""

    def __init__(self, cfg, args, slam):
        self.verbose = slam.verbose
        self.ckptsdir = slam.ckptsdir
        self.shared_c = slam.shared_c
        self.gt_c2w_list = slam.gt_c2w_list
        self.shared_decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list
        self.tsdf_volume = slam.tsdf_volume_shared

    def log(self, idx, keyframe_dict, keyframe_list, selected_keyframes=None):
        path = os.path.join(self.ckptsdir, '{:05d}.tar'.format(idx))
        torch.save({
            'c': self.shared_c,
            'decoder_state_dict': self.shared_decoders.state_dict(),
            'gt_c2w_list': self.gt_c2w_list,
            'estimate_c2w_list': self.estimate_c2w_list,
            'keyframe_list': keyframe_list,
            'keyframe_dict': keyframe_dict,
            'selected_keyframes': selected_keyframes,
            'idx': idx,
            'tsdf_volume': self.tsdf_volume,
        }, path, _use_new_zipfile_serialization=False)
        if self.verbose:
            print('Saved checkpoints at', path)


class Mapper(object):
    """The mapping loop (src/Mapper.py:262-606).  ``map_frame`` is one pass of the reference's ``run`` loop body; ``optimize_map``
    keeps the reference's signature and drives ``mapping.MapperIteration`` instead of autograd and ``torch.optim.Adam``."""

    def __init__(self, cfg, args, slam):
        self.cfg = cfg
        self.args = args

        self.idx = slam.idx
        self.c = slam.shared_c
        self.bound = slam.bound
        self.logger = slam.logger
        self.mesher = slam.mesher
        self.output = slam.output
        self.verbose = slam.verbose
        self.renderer = slam.renderer
        self.low_gpu_mem = slam.low_gpu_mem
        self.mapping_idx = slam.mapping_idx
        self.mapping_cnt = slam.mapping_cnt
        self.decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list
        self.mapping_first_frame = slam.mapping_first_frame
        self.scene_id = slam.scene_id
        self.tsdf_volume_shared = slam.tsdf_volume_shared
        self.tsdf_bnds = slam.tsdf_bnds
        self.prior = getattr(slam, 'prior', None)             # the fusion.TSDFVolume of --prior online, else None

        self.scale = cfg['scale']
        self.occupancy = cfg['occupancy']
        self.sync_method = cfg['sync_method']

        m = cfg['mapping']
        self.device = m['device']
        self.fix_high = m['fix_high']
        self.eval_rec = cfg['meshing']['eval_rec']
        self.mesh_freq = m['mesh_freq']
        self.ckpt_freq = m['ckpt_freq']
        self.fix_color = m['fix_color']
        self.mapping_pixels = m['pixels']
        self.num_joint_iters = m['iters']
        self.clean_mesh = cfg['meshing']['clean_mesh']
        self.every_frame = m['every_frame']
        self.color_refine = m['color_refine']
        self.w_color_loss = m['w_color_loss']
        self.keyframe_every = m['keyframe_every']
        self.high_iter_ratio = m['high_iter_ratio']
        self.low_iter_ratio = m['low_iter_ratio']
        self.mapping_window_size = m['mapping_window_size']
        self.no_vis_on_first_frame = m['no_vis_on_first_frame']
        self.no_log_on_first_frame = m['no_log_on_first_frame']
        self.no_mesh_on_first_frame = m['no_mesh_on_first_frame']
        self.frustum_feature_selection = m['frustum_feature_selection']
        self.keyframe_selection_method = m['keyframe_selection_method']
        self.save_selected_keyframes_info = m['save_selected_keyframes_info']
        if self.save_selected_keyframes_info:
            self.selected_keyframes = {}
        # bundle adjustment (the reference's parent project; the reference dropped it): off unless the config asks for it
        self.BA = bool(mapping_setting(cfg, 'BA'))
        self.BA_cam_lr = float(mapping_setting(cfg, 'BA_cam_lr'))       # a user setting: not scaled by lr_factor

        self.keyframe_dict = []
        self.keyframe_list = []
        self.frame_reader = slam.frame_reader                 # one reader for the whole process (the reference builds one per thread)
        self.n_img = slam.n_img
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        self.keyframe_store = self._new_keyframe_store()
        if 'Demo' not in self.output:  # disable this visualization in demo
            self.visualizer = self._new_visualizer()
        self.init = True
        self.stage = None
        self._iterations = {}          # (lr_factor, frustum selection, trained networks) -> MapperIteration
        self.prior_s = 0.0             # host time spent queueing the online prior's integrations

    # ---- the parts a test replaces with recording stand-ins ----------------------------------------------------------------
    def _new_keyframe_store(self):
        from .keyframes import KeyframeStore
        return KeyframeStore(self.H, self.W, self.device)

    def _new_visualizer(self):
        from .visualizer import Visualizer
        m = self.cfg['mapping']
        os.makedirs(os.path.join(self.output, 'mapping_vis'), exist_ok=True)
        return Visualizer(freq=m['vis_freq'], inside_freq=m['vis_inside_freq'], vis_dir=os.path.join(self.output, 'mapping_vis'),
                          renderer=self.renderer, verbose=self.verbose, device=self.device)

    def _new_iteration(self, masks, stage_lr, train):
        from .mapping import MapperIteration
        return MapperIteration(self.renderer, self.decoders, self.c, masks, self.tsdf_volume_shared, self.tsdf_bnds, stage_lr,
                               w_color_loss=self.w_color_loss, train=train)

    def _frustum_masks(self, c2w, gt_depth):
        """get_mask_from_c2w for every grid (src/Mapper.py:345-346), on the device."""
        from .mapping import frustum_mask
        return {k: frustum_mask(c2w, v.shape[2:], gt_depth, self.bound, self.H, self.W, self.fx, self.fy, self.cx, self.cy)
                for k, v in self.c.items()}

    def _sample_batch(self, it, frames, pixs_per_image):
        """The iteration's ray batch (src/Mapper.py:412-436): pixs_per_image random pixels of every window frame, written by one
        launch into the static buffers the iteration's graphs read."""
        from .common import get_samples_multi
        n = pixs_per_image * len(frames)
        return get_samples_multi(0, self.H, 0, self.W, pixs_per_image, self.H, self.W, self.fx, self.fy, self.cx, self.cy, frames,
                                 self.device, out=it.input_buffers(n))

    def _ba_begin(self, it, optimize_frame, frames):
        """Bundle adjustment for this mapped frame: the window's poses join the iteration's Adam.  The oldest keyframe of the window
        stays fixed (the gauge); every other frame, the current one (-1) included, gets the camera tensor of its pose.  Returns the
        free flags, one per window frame."""
        from . import _lib
        if len(optimize_frame) > _lib.KEYFRAMES_MAX:
            raise ValueError(f'mapping.BA: a window of {len(optimize_frame)} frames, at most {_lib.KEYFRAMES_MAX} are supported')
        oldest_frame = min(f for f in optimize_frame if f != -1)
        free = [f != oldest_frame for f in optimize_frame]
        poses = torch.stack([torch.as_tensor(c2w).detach().float().reshape(4, 4) for c2w, _, _ in frames]).cpu()      # one download
        cams = torch.stack([get_tensor_from_camera(m) for m in poses])
        it.set_ba(cams, free, self.BA_cam_lr, frames, self.H, self.W, self.fx, self.fy, self.cx, self.cy)
        return free

    def _ba_end(self, it, optimize_frame, free, keyframe_dict, cur_c2w):
        """After the iterations: every free keyframe's new pose into its row of the store and into keyframe_dict; returns the current
        frame's new pose.  One launch writes them all."""
        cur = torch.empty_like(cur_c2w, dtype=torch.float32).contiguous()
        dst = [None if not fr else (cur if f == -1 else self.keyframe_store.frame(f)[0]) for f, fr in zip(optimize_frame, free)]
        it.poses(dst=dst)
        for f, fr in zip(optimize_frame, free):
            if fr and f != -1:
                keyframe_dict[f]['est_c2w'] = self.keyframe_store.frame(f)[0].clone()
        return cur

    def _integrate_prior(self, idx, gt_color, gt_depth):
        """--prior online: frame idx into the prior volume with its ESTIMATED pose, as get_tsdf.init_tsdf_volume integrates a frame
        with its ground-truth one (columns 1 and 2 flipped back to the camera the volume integrates in, colours floor(255 c))."""
        t0 = time.perf_counter()
        c2w = self.estimate_c2w_list[idx].numpy().copy()
        c2w[:3, 1] *= -1.0
        c2w[:3, 2] *= -1.0
        intrinsic = np.array([[self.fx, 0., self.cx], [0., self.fy, self.cy], [0., 0., 1.]])
        self.prior.integrate(torch.floor(gt_color * 255), gt_depth, intrinsic, c2w, obs_weight=1.)
        self.prior_s += time.perf_counter() - t0

    # ---- the reference's methods -------------------------------------------------------------------------------------------
    def keyframe_selection_overlap(self, gt_color, gt_depth, c2w, keyframe_dict, k, N_samples=16, pixels=100):
        """Select overlapping keyframes to the current camera observation (src/Mapper.py:160-222): the same two random draws, the
        projection of the sample points into every keyframe in one launch (keyframes.keyframe_selection_overlap).  keyframe_dict is
        the reference's argument, ``self.keyframe_dict[:-1]``; its poses are read from the resident store's prefix of that length."""
        from .keyframes import keyframe_selection_overlap
        return keyframe_selection_overlap(gt_color, gt_depth, c2w, self.keyframe_store[:len(keyframe_dict)], k, N_samples, pixels,
                                          H=self.H, W=self.W, fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy, device=self.device)

    def _iteration(self, lr_factor, masks):
        train = tuple(n for n, fixed in (('high', self.fix_high), ('color', self.fix_color)) if not fixed) + ('att',)
        key = (float(lr_factor), masks is not None, train)
        it = self._iterations.get(key)
        if it is None:
            stage_lr = {st: {k[:-3]: v * lr_factor for k, v in self.cfg['mapping']['stage'][st].items()} for st in STAGES}
            it = self._iterations[key] = self._new_iteration(masks, stage_lr, train)
        return it

    def optimize_map(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth, gt_cur_c2w, keyframe_dict, keyframe_list,
                     tsdf_volume, cur_c2w):
        """Mapping iterations of one frame (src/Mapper.py:262-484): the keyframe window, then num_joint_iters iterations, each a ray
        batch over the window and one MapperIteration.step in the stage its index selects.  With ``mapping.BA`` and more than four
        keyframes the window's poses are optimised too (all but the oldest keyframe's) and the current frame's new pose is returned;
        else None."""
        if len(keyframe_dict) == 0:
            optimize_frame = []
        else:
            num = self.mapping_window_size - 2
            if self.keyframe_selection_method == 'global':
                optimize_frame = random_select(len(self.keyframe_dict) - 1, num)
            elif self.keyframe_selection_method == 'overlap':
                optimize_frame = self.keyframe_selection_overlap(cur_gt_color, cur_gt_depth, cur_c2w, keyframe_dict[:-1], num)
            else:
                raise ValueError(f'keyframe_selection_method {self.keyframe_selection_method!r}: global or overlap')

        # add the last keyframe and the current frame (-1 denotes it)
        if len(keyframe_list) > 0:
            optimize_frame = optimize_frame + [len(keyframe_list) - 1]
        optimize_frame += [-1]
        optimize_frame = [int(f) for f in optimize_frame]

        if self.save_selected_keyframes_info:
            keyframes_info = []
            for frame in optimize_frame:
                if frame != -1:
                    info = {'idx': keyframe_list[frame], 'gt_c2w': keyframe_dict[frame]['gt_c2w'], 'est_c2w': keyframe_dict[frame]['est_c2w']}
                else:
                    info = {'idx': idx, 'gt_c2w': gt_cur_c2w, 'est_c2w': cur_c2w}
                keyframes_info.append(info)
            self.selected_keyframes[idx] = keyframes_info

        pixs_per_image = self.mapping_pixels // len(optimize_frame)

        masks = self._frustum_masks(cur_c2w, cur_gt_depth) if self.frustum_feature_selection else None
        it = self._iteration(lr_factor, masks)
        it.new_frame(masks)                                   # a fresh Adam (:374) and this frame's frustum masks
        frames = [self.keyframe_store.frame(f) if f != -1 else (cur_c2w, cur_gt_depth, cur_gt_color) for f in optimize_frame]
        ba = self.BA and len(self.keyframe_list) > 4
        if ba:
            free = self._ba_begin(it, optimize_frame, frames)
        self.last_window = (list(optimize_frame), pixs_per_image)
        low_end = int(num_joint_iters * self.low_iter_ratio)
        high_end = int(num_joint_iters * self.high_iter_ratio)

        for joint_iter in range(num_joint_iters):
            if joint_iter <= low_end:
                self.stage = 'low'
            elif joint_iter <= high_end:
                self.stage = 'high'
            else:
                self.stage = 'color'

            if (not (idx == 0 and self.no_vis_on_first_frame)) and ('Demo' not in self.output):
                self.visualizer.vis(idx, joint_iter, cur_gt_depth, cur_gt_color, cur_c2w, self.c, self.decoders, tsdf_volume, self.tsdf_bnds)

            # with bundle adjustment the rays come from the poses the camera tensors give in THIS iteration
            batch = it.sample_ba(pixs_per_image) if ba else self._sample_batch(it, frames, pixs_per_image)
            warmup = low_end < joint_iter <= low_end + 5 and idx <= 1
            it.step(*batch, self.stage, warmup=warmup)
        if ba:
            return self._ba_end(it, optimize_frame, free, keyframe_dict, cur_c2w)
        return None

    def run(self):
        raise NotImplementedError('the Mapper is not a process of its own here: DF_Prior.run() calls map_frame for the frames the '
                                  "reference's Mapper.run would pick up under sync_method: strict")

    def map_frame(self, idx, gt_color, gt_depth, gt_c2w):
        """One pass of the reference's mapping loop for frame idx (src/Mapper.py:512-605); gt_color / gt_depth on the device, gt_c2w
        on the host.  Returns False for a frame it skipped (no finite entry in its ground-truth pose), else True."""
        cfg = self.cfg
        idx = int(idx)
        if idx == 0:
            self.estimate_c2w_list[0] = gt_c2w.cpu()
        tsdf_volume = self.tsdf_volume_shared

        if self.verbose:
            print("Mapping Frame ", idx)

        valid_c2w = gt_c2w.clone().cpu().numpy()
        if not np.isfinite(valid_c2w).any():
            self.mapping_idx[0] = idx
            return False

        if not self.init:
            lr_factor = cfg['mapping']['lr_factor']
            num_joint_iters = cfg['mapping']['iters']

            # here provides a color refinement postprocess
            if idx == self.n_img - 1 and self.color_refine:
                outer_joint_iters = 5
                self.mapping_window_size *= 2
                self.low_iter_ratio = 0.0
                self.high_iter_ratio = 0.0
                num_joint_iters *= 5
                self.fix_color = True
                self.frustum_feature_selection = False
            else:
                outer_joint_iters = 1
        else:
            outer_joint_iters = 1
            lr_factor = cfg['mapping']['lr_first_factor']
            num_joint_iters = cfg['mapping']['iters_first']

        cur_c2w = self.estimate_c2w_list[idx].to(self.device)
        num_joint_iters = num_joint_iters // outer_joint_iters

        if self.prior is not None:
            self._integrate_prior(idx, gt_color, gt_depth)

        for outer_joint_iter in range(outer_joint_iters):
            new_c2w = self.optimize_map(num_joint_iters, lr_factor, idx, gt_color, gt_depth, gt_c2w, self.keyframe_dict, self.keyframe_list,
                                        tsdf_volume, cur_c2w=cur_c2w)
            if new_c2w is not None:                           # bundle adjustment moved the frame's pose
                cur_c2w = new_c2w
                self.estimate_c2w_list[idx] = cur_c2w.detach().cpu()

            # add new frame to keyframe set
            if outer_joint_iter == outer_joint_iters - 1:
                if (idx % self.keyframe_every == 0 or (idx == self.n_img - 2)) and (idx not in self.keyframe_list):
                    self.keyframe_list.append(idx)
                    self.keyframe_dict.append({'gt_c2w': gt_c2w.cpu(), 'idx': idx, 'color': gt_color.cpu(), 'depth': gt_depth.cpu(),
                                               'est_c2w': cur_c2w.clone()})
                    self.keyframe_store.append(idx, gt_color, gt_depth, cur_c2w)

        if self.low_gpu_mem and torch.cuda.is_available():
            torch.cuda.empty_cache()

        if self.init:
            self.init = False
            # the first frame's iteration (lr_first_factor) is not used again: its moments, shadows and graphs go
            if cfg['mapping']['lr_first_factor'] != cfg['mapping']['lr_factor']:
                self._iterations.clear()
        self.mapping_first_frame[0] = 1

        last = idx == self.n_img - 1
        if ((not (idx == 0 and self.no_log_on_first_frame)) and idx % self.ckpt_freq == 0) or last:
            self.logger.log(idx, self.keyframe_dict, self.keyframe_list,
                            selected_keyframes=self.selected_keyframes if self.save_selected_keyframes_info else None)

        self.mapping_idx[0] = idx
        self.mapping_cnt[0] += 1

        def mesh(name, use_all):
            path = f'{self.output}/mesh/{name}'
            self.mesher.get_mesh(path, self.c, self.decoders, self.keyframe_dict, self.estimate_c2w_list, idx, tsdf_volume, self.device,
                                 clean_mesh=self.clean_mesh, get_mask_use_all_frames=use_all, keyframe_store=self.keyframe_store)
            return path

        if (idx % self.mesh_freq == 0) and (not (idx == 0 and self.no_mesh_on_first_frame)):
            mesh(f'{idx:05d}_mesh.ply', False)

        if last:
            final = mesh('final_mesh.ply', False)
            if os.path.exists(final):                         # an empty level set writes no file (the Mesher prints its notice)
                shutil.copyfile(final, f'{self.output}/mesh/{idx:05d}_mesh.ply')
            if self.eval_rec:
                mesh('final_mesh_eval_rec.ply', True)
        return True


class Tracker(object):
    """The tracking loop (src/Tracker.py:150-275).  ``track_frame`` is one pass of the reference's ``run`` loop body; the
    iterations are ``tracking.TrackerIteration.step`` replays, and ONE TrackerIteration lives for the whole run."""

    def __init__(self, cfg, args, slam):
        self.cfg = cfg
        self.args = args

        self.scale = cfg['scale']
        self.occupancy = cfg['occupancy']
        self.sync_method = cfg['sync_method']

        self.idx = slam.idx
        self.bound = slam.bound
        self.mesher = slam.mesher
        self.output = slam.output
        self.verbose = slam.verbose
        self.shared_c = slam.shared_c
        self.renderer = slam.renderer
        self.gt_c2w_list = slam.gt_c2w_list
        self.low_gpu_mem = slam.low_gpu_mem
        self.mapping_idx = slam.mapping_idx
        self.mapping_cnt = slam.mapping_cnt
        self.shared_decoders = slam.shared_decoders
        self.estimate_c2w_list = slam.estimate_c2w_list
        self.tsdf_volume_shared = slam.tsdf_volume_shared
        self.tsdf_bnds = slam.tsdf_bnds

        t = cfg['tracking']
        self.cam_lr = t['lr']
        self.device = t['device']
        self.num_cam_iters = t['iters']
        self.gt_camera = t['gt_camera']
        self.tracking_pixels = t['pixels']
        self.seperate_LR = t['seperate_LR']
        self.w_color_loss = t['w_color_loss']
        self.ignore_edge_W = t['ignore_edge_W']
        self.ignore_edge_H = t['ignore_edge_H']
        self.handle_dynamic = t['handle_dynamic']
        self.use_color_in_tracking = t['use_color_in_tracking']
        self.const_speed_assumption = t['const_speed_assumption']

        self.every_frame = cfg['mapping']['every_frame']
        self.no_vis_on_first_frame = cfg['mapping']['no_vis_on_first_frame']

        self.prev_mapping_idx = -1
        self.frame_reader = slam.frame_reader
        self.n_img = slam.n_img
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy
        # the Mapper's own grids and decoders, not copies: nothing maps while a frame is tracked
        self.c = self.shared_c
        self.decoders = self.shared_decoders
        self.visualizer = self._new_visualizer()
        self._it = None
        # tracking.init: icp -- the guess goes through icp.DepthICP first; one status per tracked frame (icp.OK ...)
        self.init = tracking_setting(cfg, 'init')
        if self.init not in TRACKING_INITS:
            raise ValueError(f'tracking.init {self.init!r}: one of {TRACKING_INITS}')
        self.icp_kwargs = dict(tracking_setting(cfg, 'icp') or {})
        # tracking.icp_rgb: {weight, tol} -- a weight > 0 adds the photometric term against the last tracked frame (icp.RgbdICP)
        rgb = dict(tracking_setting(cfg, 'icp_rgb') or {})
        unknown = set(rgb) - {'weight', 'tol'}
        if unknown:
            raise ValueError(f'tracking.icp_rgb: unknown keys {sorted(unknown)} (weight, tol)')
        self.icp_rgb_weight = float(rgb.get('weight') or 0.0)
        self.icp_rgb_tol = rgb.get('tol')
        if self.icp_rgb_weight < 0 or self.icp_rgb_weight != self.icp_rgb_weight:
            raise ValueError(f'tracking.icp_rgb.weight {self.icp_rgb_weight!r}: a number >= 0')
        if self.icp_rgb_weight > 0 and self.init != 'icp':
            raise ValueError('tracking.icp_rgb.weight > 0 needs tracking.init: icp')
        self.icp_rgb = self.init == 'icp' and self.icp_rgb_weight > 0
        self._icp = None
        self.icp_status = []

    # ---- the parts a test replaces with recording stand-ins ----------------------------------------------------------------
    def _new_icp(self):
        """The raycaster inside shares the Renderer's Engine: its empty-space bitmap is keyed on the prior volume's version counter
        (--prior online integrates through PyTorch, which bumps it) and dropped by the Renderer's invalidate_tsdf."""
        from .icp import DepthICP, RgbdICP
        if self.icp_rgb:
            kw = dict(self.icp_kwargs, rgb_weight=self.icp_rgb_weight)
            if self.icp_rgb_tol is not None:
                kw['rgb_tol'] = float(self.icp_rgb_tol)
            return RgbdICP(self.tsdf_volume_shared, self.tsdf_bnds, self.H, self.W, self.fx, self.fy, self.cx, self.cy,
                           engine=self.renderer._engine, **kw)
        return DepthICP(self.tsdf_volume_shared, self.tsdf_bnds, self.H, self.W, self.fx, self.fy, self.cx, self.cy,
                        engine=self.renderer._engine, **self.icp_kwargs)

    def _new_visualizer(self):
        from .visualizer import Visualizer
        t = self.cfg['tracking']
        vis_dir = os.path.join(self.output, 'vis' if 'Demo' in self.output else 'tracking_vis')
        os.makedirs(vis_dir, exist_ok=True)
        return Visualizer(freq=t['vis_freq'], inside_freq=t['vis_inside_freq'], vis_dir=vis_dir, renderer=self.renderer,
                          verbose=self.verbose, device=self.device)

    def _new_iteration(self):
        from .tracking import TrackerIteration
        return TrackerIteration(self.renderer, self.decoders, self.c, self.tsdf_volume_shared, self.tsdf_bnds, self.H, self.W,
                                self.fx, self.fy, self.cx, self.cy, self.ignore_edge_H, self.ignore_edge_W, cam_lr=self.cam_lr,
                                seperate_LR=self.seperate_LR, use_color=self.use_color_in_tracking, w_color_loss=self.w_color_loss,
                                handle_dynamic=self.handle_dynamic)

    # ---- the reference's methods -------------------------------------------------------------------------------------------
    @property
    def iteration(self):
        if self._it is None:
            self._it = self._new_iteration()
        return self._it

    @property
    def icp(self):
        if self._icp is None:
            self._icp = self._new_icp()
        return self._icp

    def optimize_cam_in_batch(self, camera_tensor, gt_color, gt_depth, batch_size, optimizer, tsdf_volume):
        """One iteration of camera optimisation (src/Tracker.py:75-134) on the frame and pose the iteration holds since its last
        ``new_frame``: the arguments are the reference's and are not read (`optimizer` may be None), the loss comes back as a float
        as the reference's does, which synchronises.  ``track_frame`` calls ``iteration.step`` itself and reads nothing back."""
        return float(self.iteration.step(batch_size))

    def update_para_from_mapping(self):
        """After a mapped frame the iteration re-reads the grids and decoders (src/Tracker.py:136-147 copies them)."""
        if self.mapping_idx[0] != self.prev_mapping_idx:
            if self.verbose:
                print('Tracking: update the parameters from mapping')
            if self._it is not None:
                self._it.update_para(self.decoders, self.c)
            self.prev_mapping_idx = self.mapping_idx[0].clone()

    def guess(self, idx):
        """The constant-speed guess for frame idx >= 1 from the two poses before it (src/Tracker.py:203-209), float32 on the host."""
        pre_c2w = self.estimate_c2w_list[idx - 1].float()
        if self.const_speed_assumption and idx - 2 >= 0:
            delta = pre_c2w @ self.estimate_c2w_list[idx - 2].float().inverse()
            return delta @ pre_c2w
        return pre_c2w

    def run(self):
        raise NotImplementedError('the Tracker is not a process of its own here: DF_Prior.run() calls track_frame for every frame')

    def track_frame(self, idx, gt_color, gt_depth, gt_c2w):
        """One pass of the reference's tracking loop for frame idx (src/Tracker.py:161-274)."""
        idx = int(idx)
        tsdf_volume, tsdf_bnds = self.tsdf_volume_shared, self.tsdf_bnds
        self.update_para_from_mapping()

        if self.verbose:
            print("Tracking Frame ", idx)

        if idx == 0 or self.gt_camera:
            c2w = gt_c2w.detach().cpu()
            if not self.no_vis_on_first_frame:
                self.visualizer.vis(idx, 0, gt_depth, gt_color, c2w.to(self.device), self.c, self.decoders, tsdf_volume, tsdf_bnds)
            if self.icp_rgb:
                self.icp.set_keyframe(c2w, gt_color, gt_depth)                           # what the next tracked frame is compared with
        else:
            if self.icp_rgb:
                # the same, with the photometric term against the last tracked frame in every step's normal equations
                camera_tensor = self.icp.refine(self.guess(idx).detach(), gt_depth, gt_color)
            elif self.init == 'icp':
                # the guess aligned with the prior's surface over the whole depth image; the guess itself when that fails.  On the
                # device, no read-back: the iterations below are queued behind it
                camera_tensor = self.icp.refine(self.guess(idx).detach(), gt_depth)
            else:
                camera_tensor = get_tensor_from_camera(self.guess(idx).detach())
            if self.num_cam_iters > 0:
                it = self.iteration
                it.new_frame(camera_tensor.to(self.device), gt_depth, gt_color)          # a fresh Adam, like :219-229
                for cam_iter in range(self.num_cam_iters):
                    self.visualizer.vis(idx, cam_iter, gt_depth, gt_color, it.camera_tensor, self.c, self.decoders, tsdf_volume, tsdf_bnds)
                    it.step(self.tracking_pixels)
                camera_tensor = it.best_camera_tensor                                    # the lowest-loss pose, kept on the device
            # tracking.iters: 0 keeps the guess (tracking.init: icp: what the ICP made of it)
            top = get_camera_from_tensor(camera_tensor.detach().clone()).cpu()           # the frame's one download
            c2w = torch.cat([top.float(), torch.tensor([[0., 0., 0., 1.]])], dim=0)
            if self.init == 'icp':
                stats = self.icp.last_stats()                                            # behind the download: nothing is waited for
                self.icp_status.append(int(stats[-1, 5].item()))
                if self.verbose:
                    from .icp import STATUS_NAMES
                    last = stats[:-1][stats[:-1, 0] > 0]
                    step = last[-1].tolist() if len(last) else [0.0] * 6
                    print(f'ICP frame {idx}: {STATUS_NAMES[self.icp_status[-1]]}, last step {step[0]:.0f} pairs, rmse {step[1]:.5f} m, '
                          f'pivot ratio {step[2]:.2e}; moved {stats[-1, 4].item():.4f} m {stats[-1, 3].item():.4f} rad from the guess')
                    if self.icp_rgb:
                        rgb = self.icp.last_rgb_stats()[:-1]
                        rgb = rgb[rgb[:, 0] > 0]
                        last_rgb = rgb[-1].tolist() if len(rgb) else [0.0, 0.0]
                        print(f'ICP frame {idx}: photometric term, last step {last_rgb[0]:.0f} pairs, rmse {last_rgb[1]:.5f}')
                if self.icp_rgb:
                    self.icp.promote(c2w)                                                # the pose is final: this frame is the next keyframe

        self.estimate_c2w_list[idx] = c2w.clone()
        self.gt_c2w_list[idx] = gt_c2w.clone().cpu()
        self.idx[0] = idx
        if self.low_gpu_mem and torch.cuda.is_available():
            torch.cuda.empty_cache()


class DF_Prior(object):
    """DF_Prior main class (src/DF_Prior.py): allocates the shared state and runs the Tracker and the Mapper.

    args: ``input_folder``, ``output`` (the reference's), and optionally ``tsdf_volume`` / ``tsdf_bounds`` (files of the prior
    volume and its bounds; default ``<dataset>_tsdf_volume/<scene>_tsdf_volume.pt`` and ``_bounds.pt``), ``prior`` ('file' |
    'online'), ``prior_voxel_size``, ``last_frame``, ``no_prefetch``."""

    def __init__(self, cfg, args):
        self.cfg = cfg
        self.args = args

        self.occupancy = cfg['occupancy']
        self.low_gpu_mem = cfg['low_gpu_mem']
        self.verbose = cfg['verbose']
        self.dataset = cfg['dataset']
        if getattr(args, 'output', None) is None:
            self.output = cfg['data']['output']
        else:
            self.output = args.output
        self.ckptsdir = os.path.join(self.output, 'ckpts')
        os.makedirs(self.output, exist_ok=True)
        os.makedirs(self.ckptsdir, exist_ok=True)
        os.makedirs(f'{self.output}/mesh', exist_ok=True)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = cfg['cam']['H'], cfg['cam'][
            'W'], cfg['cam']['fx'], cfg['cam']['fy'], cfg['cam']['cx'], cfg['cam']['cy']
        self.update_cam()

        model = get_model(cfg)
        self.shared_decoders = model

        self.scale = cfg['scale']

        self.load_bound(cfg)
        self.load_pretrain(cfg)
        self.grid_init(cfg)

        device = cfg['mapping']['device']
        self.frame_reader = self._get_dataset(cfg, args, self.scale, device)
        self.n_img = len(self.frame_reader)
        last_frame = getattr(args, 'last_frame', None)
        if last_frame is not None:
            self.n_img = max(1, min(self.n_img, int(last_frame) + 1))
        self.estimate_c2w_list = torch.zeros((self.n_img, 4, 4))
        self.gt_c2w_list = torch.zeros((self.n_img, 4, 4))

        dataset = cfg['data'].get('dataset', cfg['dataset'])
        scene_id = cfg['data'].get('id')
        self.scene_id = scene_id
        self.load_prior(cfg, args, dataset, scene_id, device)
        self.vol_bnds = self.tsdf_bnds

        self.idx = torch.zeros((1)).int()
        self.mapping_first_frame = torch.zeros((1)).int()
        self.mapping_idx = torch.zeros((1)).int()      # the id of the newest frame the Mapper has finished
        self.mapping_cnt = torch.zeros((1)).int()      # counter for mapping
        for key, val in self.shared_c.items():
            self.shared_c[key] = val.to(device)
        self.shared_decoders = self.shared_decoders.to(device)
        self.renderer = self._new_renderer(cfg, args)
        self.mesher = self._new_mesher(cfg, args)
        self.logger = self._new_logger(cfg, args)
        self.mapper = self._new_mapper(cfg, args)
        self.tracker = self._new_tracker(cfg, args)
        self.measure = False           # run(): synchronise at frame ends and keep per-frame wall times (tools/run_bench.py)
        self.frame_times = []
        self.ate = None
        self.print_output_desc()

    # ---- the parts a test replaces with recording stand-ins ----------------------------------------------------------------
    def _get_dataset(self, cfg, args, scale, device):
        from .datasets import get_dataset
        return get_dataset(cfg, args, scale, device=device)

    def _new_renderer(self, cfg, args):
        from .renderer import Renderer
        return Renderer(cfg, args, self)

    def _new_mesher(self, cfg, args):
        from .mesher import Mesher
        return Mesher(cfg, args, self)

    def _new_logger(self, cfg, args):
        return Logger(cfg, args, self)

    def _new_mapper(self, cfg, args):
        return Mapper(cfg, args, self)

    def _new_tracker(self, cfg, args):
        return Tracker(cfg, args, self)

    # ---- the reference's methods -------------------------------------------------------------------------------------------
    def print_output_desc(self):
        print(f"INFO: The output folder is {self.output}")
        if 'Demo' in self.output:
            print(f"INFO: The GT, generated and residual depth/color images can be found under {self.output}/vis/")
        else:
            print(f"INFO: The GT, generated and residual depth/color images can be found under "
                  f"{self.output}/tracking_vis/ and {self.output}/mapping_vis/")
        print(f"INFO: The mesh can be found under {self.output}/mesh/")
        print(f"INFO: The checkpoint can be found under {self.output}/ckpts/")

    def update_cam(self):
        """Update the camera intrinsics according to pre-processing config, such as resize or edge crop."""
        if 'crop_size' in self.cfg['cam']:
            crop_size = self.cfg['cam']['crop_size']
            sx = crop_size[1] / self.W
            sy = crop_size[0] / self.H
            self.fx = sx * self.fx
            self.fy = sy * self.fy
            self.cx = sx * self.cx
            self.cy = sy * self.cy
            self.W = crop_size[1]
            self.H = crop_size[0]

        # croping will change H, W, cx, cy, so need to change here
        if self.cfg['cam']['crop_edge'] > 0:
            self.H -= self.cfg['cam']['crop_edge'] * 2
            self.W -= self.cfg['cam']['crop_edge'] * 2
            self.cx -= self.cfg['cam']['crop_edge']
            self.cy -= self.cfg['cam']['crop_edge']

    def load_bound(self, cfg):
        """Pass the scene bound parameters to different decoders and self."""
        # scale the bound if there is a global scaling factor
        self.bound = torch.from_numpy(np.array(cfg['mapping']['bound']) * self.scale)
        bound_divisible = cfg['grid_len']['bound_divisible']
        # enlarge the bound a bit to allow it divisible by bound_divisible
        self.bound[:, 1] = (((self.bound[:, 1] - self.bound[:, 0]) / bound_divisible).int() + 1) * bound_divisible + self.bound[:, 0]
        self.shared_decoders.bound = self.bound
        self.shared_decoders.low_decoder.bound = self.bound
        self.shared_decoders.high_decoder.bound = self.bound
        self.shared_decoders.color_decoder.bound = self.bound

    def load_pretrain(self, cfg):
        """Load parameters of pretrained ConvOnet checkpoints to the decoders.  ``pretrained_decoders.low_high: null`` (not in the
        reference) leaves the decoders as their seeded initialisation made them."""
        path = (cfg.get('pretrained_decoders') or {}).get('low_high')
        if path is None:
            log.info('pretrained_decoders.low_high is null: the decoders keep their seeded initialisation')
            return
        ckpt = torch.load(path, map_location=cfg['mapping']['device'], weights_only=False)
        low_dict = {}
        high_dict = {}
        for key, val in ckpt['model'].items():
            if ('decoder' in key) and ('encoder' not in key):
                if 'coarse' in key:
                    key = key[8 + 7:]
                    low_dict[key] = val
                elif 'fine' in key:
                    key = key[8 + 5:]
                    high_dict[key] = val
        self.shared_decoders.low_decoder.load_state_dict(low_dict)
        self.shared_decoders.high_decoder.load_state_dict(high_dict)

    def grid_init(self, cfg):
        """Initialize the hierarchical feature grids."""
        self.low_grid_len = cfg['grid_len']['low']
        self.high_grid_len = cfg['grid_len']['high']
        self.color_grid_len = cfg['grid_len']['color']

        c = {}
        c_dim = cfg['model']['c_dim']
        xyz_len = self.bound[:, 1] - self.bound[:, 0]
        for key, grid_len, std in (('grid_low', self.low_grid_len, 0.01), ('grid_high', self.high_grid_len, 0.0001),
                                   ('grid_color', self.color_grid_len, 0.01)):
            val_shape = list(map(int, (xyz_len / grid_len).tolist()))
            val_shape[0], val_shape[2] = val_shape[2], val_shape[0]
            setattr(self, key[5:] + '_val_shape', val_shape)
            c[key] = torch.zeros([1, c_dim, *val_shape]).normal_(mean=0, std=std)
        self.shared_c = c

    def load_prior(self, cfg, args, dataset, scene_id, device):
        """The TSDF prior: ``tsdf_volume_shared`` [1,1,Z,Y,X] and ``tsdf_bnds`` on the device.  From the files get_tsdf wrote
        (src/DF_Prior.py:74-91), or with ``--prior online`` an empty fusion.TSDFVolume over the scene bound that the Mapper fills."""
        self.prior = None
        mode = getattr(args, 'prior', None) or 'file'
        if mode == 'online':
            from . import fusion
            voxel = getattr(args, 'prior_voxel_size', None) or 4.0 / 256
            self.prior = fusion.TSDFVolume(self.bound.numpy(), voxel_size=voxel, device=device)
            self.tsdf_volume_shared, bnds = self.prior.get_render_volume()
            self.tsdf_bnds = bnds.to(device)
            return
        if mode != 'file':
            raise ValueError(f"prior {mode!r}: 'file' or 'online'")
        stem = f'scene{scene_id}' if dataset == 'scannet' else f'{scene_id}'
        volume_path = getattr(args, 'tsdf_volume', None) or f'{dataset}_tsdf_volume/{stem}_tsdf_volume.pt'
        bounds_path = getattr(args, 'tsdf_bounds', None) or f'{dataset}_tsdf_volume/{stem}_bounds.pt'
        self.tsdf_volume_shared = torch.load(volume_path, map_location='cpu', weights_only=False).to(device)
        self.tsdf_bnds = torch.as_tensor(torch.load(bounds_path, map_location='cpu', weights_only=False)).to(device)

    def tracking(self, rank):
        raise NotImplementedError('the Tracker is not a process of its own here: run() tracks and maps in one process')

    def mapping(self, rank):
        raise NotImplementedError('the Mapper is not a process of its own here: run() tracks and maps in one process')

    def run(self):
        """Map frame 0, then for every frame: track it and, when ``idx % every_frame == 0`` or it is the last frame, map it -- the
        order the reference's ``sync_method: strict`` produces with its two processes.  Then the trajectory error."""
        sync = self.cfg['sync_method']
        if sync != 'strict':
            msg = f"sync_method {sync!r}: one process, so the frames are tracked and mapped in the order 'strict' produces"
            log.warning(msg)
            print(msg)
        every_frame = self.cfg['mapping']['every_frame']
        sync_dev = torch.cuda.synchronize if self.measure else (lambda: None)
        feed = self.feed = FrameFeed(self.frame_reader, self.n_img, prefetch=not getattr(self.args, 'no_prefetch', False))
        try:
            for idx in range(self.n_img):
                t0 = time.perf_counter()
                wait0, prior0 = feed.wait_s, self.mapper.prior_s
                gt_color, gt_depth, gt_c2w = feed.get(idx)
                sync_dev()
                t1 = time.perf_counter()
                mapped = False
                if idx == 0:
                    mapped = self.mapper.map_frame(0, gt_color, gt_depth, gt_c2w)
                    sync_dev()
                t2 = time.perf_counter()
                self.tracker.track_frame(idx, gt_color, gt_depth, gt_c2w)
                sync_dev()
                t3 = time.perf_counter()
                if idx > 0 and (idx % every_frame == 0 or idx == self.n_img - 1):
                    mapped = self.mapper.map_frame(idx, gt_color, gt_depth, gt_c2w)
                    sync_dev()
                t4 = time.perf_counter()
                if self.measure:
                    self.frame_times.append({'idx': idx, 'mapped': bool(mapped), 'fetch_s': t1 - t0, 'decode_wait_s': feed.wait_s - wait0,
                                             'track_s': t3 - t2, 'map_s': (t2 - t1) + (t4 - t3), 'prior_host_s': self.mapper.prior_s - prior0})
        finally:
            feed.close()
        self.ate = self.eval_ate()
        return self.ate

    def eval_ate(self):
        """Prints the trajectory error of the finished run and writes {output}/eval_ate.json (the reference runs
        src/tools/eval_ate.py on the newest checkpoint afterwards)."""
        import json
        from . import eval_ate
        res = eval_ate.ate_of_lists(self.gt_c2w_list, self.estimate_c2w_list, self.n_img - 1, self.scale)
        if res is None:
            print('ATE: fewer than two frames with a finite ground-truth pose, nothing to compare')
            return None
        res = {k: (int(v) if k == 'compared_pose_pairs' else float(v)) for k, v in res.items()}
        print(res)
        with open(os.path.join(self.output, 'eval_ate.json'), 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
        return res
