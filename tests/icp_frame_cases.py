"""Inputs of tests/test_gpu_icp_frame_sizes.py: depth (and colour) images of an analytic room at frame sizes where the launch arithmetic
of the ICP kernels (csrc/adfp_icp.h, adfp_rgbd.h) runs more than once -- a row of several workgroups in k_depth_normals and
k_rgbd_frame_map, more than 64 partial rows in k_icp_solve, more than one pass of the grid-stride loop in k_icp_step / k_rgbd_step.
Plain numpy in float64, no GPU, no raycaster: the room is the axis-aligned box [-ROOM, ROOM]^3 seen from inside, the depth of a pixel
the smallest positive plane parameter along its ray ((u - cx) / fx, -(v - cy) / fy, -1), which is icp_vertex's convention.

The launchers size the step's grid as blocks = min(ceil(n / 256), 2 CU, 1024) with n the strided pixel count and CU the device's
compute-unit count, so the shapes of the `pass*` cases follow from CU (256 on the MI355X: DEFAULT_CU).

What the last row costs.  A normal needs the pixel below and the pixel to the right, so the last row and the last column of a normal
map are zero.  At stride 1 the shapes H x W = 129 x 128, (CU + 1) x 512 and (2 CU + 1) x 512 put exactly their LAST ROW into the
65th partial row / the second / the third pass: those pixels carry no sensor normal, a correct step adds nothing for them, and a
step that drops them gives the same sums.  Each of the three therefore has a sibling one row taller (`solve_b`, `pass2_b`,
`pass3_b`) whose row H - 2 -- which has normals -- falls into the same partial row / pass; tests/test_icp_frame_cases.py asserts both
facts.  The one-row-short shapes stay: they hold the ragged tail (a last workgroup with 128 live lanes, a pass of 512 lanes)."""
import functools
import math

import numpy as np

import icp_ref as R
import rgbd_icp_ref as G

ROOM = 1.5
YAW, PITCH, AT = 0.7, -0.35, (0.2, -0.1, 0.3)
GUESS_SCALE = 0.5
THREADS, MAX_BLOCKS, SOLVE_LANES = 256, 1024, 64         # ADFP_ICP_THREADS, ADFP_ICP_MAX_BLOCKS, k_icp_solve's wave
DEFAULT_CU = 256
STRIDES = (1, 2, 3)
ROWS_SHAPES = ((3, 513), (4, 256), (4, 257))
MASKS = ('first', 'last', 'solve_second_pass', 'last_partial_row', 'second_pass', 'third_pass', 'corner')


def shapes(CU=DEFAULT_CU):
    """name -> (H, W) of the step cases"""
    return {'solve': (129, 128), 'solve_b': (130, 128), 'pass2': (CU + 1, 512), 'pass2_b': (CU + 2, 512), 'pass3': (2 * CU + 1, 512),
            'pass3_b': (2 * CU + 2, 512)}


def strided(H, W, stride):
    """-> (wn, hn, n): strided pixels per row, strided rows, strided pixels"""
    wn, hn = -(-W // stride), -(-H // stride)
    return wn, hn, wn * hn


def expected_blocks(H, W, stride, CU=DEFAULT_CU):
    """The workgroups adfp_icp_step / adfp_rgbd_step launch = the partial rows k_icp_solve adds."""
    n = strided(H, W, stride)[2]
    return min(-(-n // THREADS), 2 * CU, MAX_BLOCKS)


def passes(H, W, stride, CU=DEFAULT_CU):
    """-> (passes of lane 0 of workgroup 0, lanes of the grid that take that last pass)"""
    n, step = strided(H, W, stride)[2], expected_blocks(H, W, stride, CU) * THREADS
    full, rest = divmod(n, step)
    return (full + 1, rest) if rest else (full, step)


def intrinsics(H, W):
    return 0.9 * W, 0.9 * W, (W - 1) / 2, (H - 1) / 2


def true_pose():
    cy_, sy_, cp_, sp_ = math.cos(YAW), math.sin(YAW), math.cos(PITCH), math.sin(PITCH)
    Ry = np.array([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
    Rx = np.array([[1, 0, 0], [0, cp_, -sp_], [0, sp_, cp_]])
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = Ry @ Rx, AT
    return P.astype(np.float32)


def guess_pose(P):
    return (R.exp_se3(np.asarray(R.TWIST) * GUESS_SCALE) @ np.asarray(P, dtype=np.float64)).astype(np.float32)


def room_depth(c2w, H, W):
    """The room seen from the float32 pose c2w -> depth [H,W] float32 (computed in float64)"""
    fx, fy, cx, cy = intrinsics(H, W)
    M = np.asarray(c2w, dtype=np.float32).astype(np.float64)
    u, v = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    d = np.stack(np.broadcast_arrays((u - cx) / fx, -(v - cy) / fy, -1.0), -1) @ M[:3, :3].T
    o = M[:3, 3]
    assert (np.abs(o) < ROOM).all()
    with np.errstate(divide='ignore'):
        t = np.where(d > 0, (ROOM - o) / d, np.where(d < 0, (-ROOM - o) / d, np.inf))
    return t.min(-1).astype(np.float32)


class Case(object):
    """One frame: the sensor depth at the true pose P, the model depth at the guess G (p_ref = G), and on demand the colours and
    the keyframe of the RGB-D cases."""

    def __init__(self, name, H, W):
        self.name, self.H, self.W = name, H, W
        self.intr = intrinsics(H, W)
        self.cam = (H, W) + self.intr
        self.P = true_pose()
        self.G = guess_pose(self.P)
        self.depth_s, self.depth_m = room_depth(self.P, H, W), room_depth(self.G, H, W)

    @functools.cached_property
    def K(self):
        return G.key_pose(self.P)

    @functools.cached_property
    def color_s(self):
        return G.color_of(self.depth_s, self.P, *self.intr)

    @functools.cached_property
    def depth_k(self):
        return room_depth(self.K, self.H, self.W)

    @functools.cached_property
    def color_k(self):
        return G.color_of(self.depth_k, self.K, *self.intr)

    @functools.cached_property
    def ref_normals(self):
        """The float64 restatement's normal maps (sensor, model): what the CPU test of this file works on"""
        return R.normals(self.depth_s, *self.intr), R.normals(self.depth_m, *self.intr)


@functools.lru_cache(maxsize=None)
def case(name, CU=DEFAULT_CU):
    H, W = shapes(CU)[name]
    return Case(name, H, W)


@functools.lru_cache(maxsize=None)
def rows_case(H, W):
    return Case(f'rows {H} x {W}', H, W)


def pair_flags(c, normals_s, normals_m, stride=1, dist_tol=0.1, cos_tol=0.8):
    """[n] bool over the strided index i: the pixel forms a geometric pair in a step from the guess (icp_ref.step_sums' gates restated
    pixel by pixel in float64; tests/test_icp_frame_cases.py holds the count against step_sums' own)."""
    fx, fy, cx, cy = R.intrinsics(*c.intr, np.float64)
    H, W = c.H, c.W
    T = P = c.G.astype(np.float64)
    vs, us = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing='ij')
    vs, us = vs.reshape(-1), us.reshape(-1)
    Ns = np.asarray(normals_s, dtype=np.float32)[vs, us].astype(np.float64)
    ok = (Ns != 0).any(-1)
    x = R.vertices(c.depth_s, *c.intr, np.float64)[vs, us] @ T[:3, :3].T + T[:3, 3]
    nsw = Ns @ T[:3, :3].T
    xc = (x - P[:3, 3]) @ P[:3, :3]
    z = -xc[:, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        pu, pv = np.floor(fx * xc[:, 0] / z + cx + 0.5), np.floor(-fy * xc[:, 1] / z + cy + 0.5)
    ok &= (z > 0) & (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1)
    pu, pv = np.where(ok, pu, 0).astype(np.int64), np.where(ok, pv, 0).astype(np.int64)
    Nm = np.asarray(normals_m, dtype=np.float32)[pv, pu].astype(np.float64)
    ok &= (Nm != 0).any(-1)
    m = R.vertices(c.depth_m, *c.intr, np.float64)[pv, pu] @ P[:3, :3].T + P[:3, 3]
    n = Nm @ P[:3, :3].T
    ok &= (np.linalg.norm(m - x, axis=-1) <= dist_tol) & ((nsw * n).sum(-1) >= cos_tol)
    return ok


def nominal_mask(name, H, W, stride, CU=DEFAULT_CU):
    """The strided indices the issue lists for a mask, cut to [0, n); empty where the case does not reach that far."""
    wn, hn, n = strided(H, W, stride)
    blocks = expected_blocks(H, W, stride, CU)
    lo, hi = {'first': (0, 1), 'last': (n - 1, n), 'solve_second_pass': (SOLVE_LANES * THREADS, (SOLVE_LANES + 1) * THREADS),
              'last_partial_row': ((blocks - 1) * THREADS, blocks * THREADS), 'second_pass': (blocks * THREADS, blocks * THREADS + 1),
              'third_pass': (2 * blocks * THREADS + 511, 2 * blocks * THREADS + 512), 'corner': (n - 1, n)}[name]
    return np.arange(max(lo, 0), min(hi, n))


def mask_indices(name, c, flags, stride=1, CU=DEFAULT_CU):
    """The strided indices of a mask on a case, `flags` = pair_flags of the full normal maps at that stride.

    The row masks (solve_second_pass, last_partial_row) are the nominal index ranges.  A one-pixel mask is the nominal pixel when that
    forms a pair, else the nearest index that does and still crosses the same edge:
      first        the smallest pairing i < 64 (wave 0 of workgroup 0; with this pose pixel (0, 0) itself pairs, so it is i = 0)
      last         the largest pairing i of all (i = n - 1 lies on the last row wherever the stride divides H - 1)
      second_pass  the smallest pairing i in [blocks 256, blocks 256 + 64): wave 0 of workgroup 0 on its second pass
      third_pass   the largest pairing i in [2 blocks 256, n): a lane on its third pass, as far into it as a pair exists
      corner       the largest pairing i whose us is the last strided column THAT HAS A NORMAL (us <= W - 2) and whose vs is the last
                   such strided row on which that column pairs; the divide and the remainder of i by wn are both at their largest
    Empty when no index qualifies (the one-row-short shapes: see the module docstring)."""
    H, W = c.H, c.W
    wn, hn, n = strided(H, W, stride)
    blocks = expected_blocks(H, W, stride, CU)
    nom = nominal_mask(name, H, W, stride, CU)
    if name in ('solve_second_pass', 'last_partial_row'):
        return nom
    if len(nom) and flags[nom].all() and name != 'corner':
        return nom
    step = blocks * THREADS
    if name == 'first':
        lo, hi, pick = 0, min(64, n), 'min'
    elif name == 'last':
        lo, hi, pick = 0, n, 'max'
    elif name == 'second_pass':
        lo, hi, pick = step, min(step + 64, n), 'min'
    elif name == 'third_pass':
        lo, hi, pick = 2 * step, n, 'max'
    else:
        ucol = (W - 2) // stride
        cand = np.arange(hn) * wn + ucol
        cand = cand[flags[cand]]
        return cand[-1:]
    cand = np.arange(lo, hi) if hi > lo else np.arange(0)
    cand = cand[flags[cand]] if len(cand) else cand
    return cand[:1] if pick == 'min' else cand[-1:]


def one_hot(normals_s, idx, W, stride=1):
    """A copy of the sensor normals that is zero everywhere except at the strided pixels idx"""
    wn = -(-W // stride)
    idx = np.asarray(idx, dtype=np.int64)
    vs, us = (idx // wn) * stride, (idx % wn) * stride
    out = np.zeros_like(normals_s)
    out[vs, us] = normals_s[vs, us]
    return out
