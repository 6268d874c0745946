"""CPU: the TSDF raycast's restatement (tests/tsdfcast_ref.py) against itself in f64 and against the analytic box room, and the new
entries of the C ABI without a GPU: argument errors come back as their codes before any launch (null stream, dummy pointers)."""
import ctypes as C

import pytest
import torch

import tsdfcast_ref as R
from attentive_dfprior_amd import _lib, synthetic
from attentive_dfprior_amd.common import get_rays

ARG, UNSUPPORTED = -1, -2
DUMMY = 4096                                       # never dereferenced: every call below fails its host-side checks first
VOXEL = 0.04                                       # synthetic.mini_scene's TSDF voxel


@pytest.fixture(scope='module')
def scene():
    sc = synthetic.mini_scene()
    return sc, R.mini_poses(sc), (sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy)


@pytest.fixture(scope='module')
def casts(scene):
    sc, poses, cam = scene
    return {(frac, dt): R.raycast(sc.tsdf_volume, sc.tsdf_bnds, poses, *cam, step=frac * VOXEL, dtype=dt)
            for frac in (0.5, 0.25) for dt in (torch.float32, torch.float64)}


@pytest.mark.parametrize('frac', [0.5, 0.25])
def test_f32_and_f64_restatements_agree(casts, frac):
    """Fixes the GPU test's tolerance: f32 lookups move a depth by at most F32_VS_F64_M, no pixel hits in one and misses in the
    other, and every pixel of these poses (inside a closed room) hits."""
    a, b = casts[(frac, torch.float32)], casts[(frac, torch.float64)]
    diff = (a - b).abs().max().item()
    print(f'step {frac} voxel: f32 vs f64 max |diff| {diff:.3e} m (constant {R.F32_VS_F64_M:.1e})')
    assert int(((a > 0) != (b > 0)).sum()) == 0
    assert int((a == 0).sum()) == 0 and int((b == 0).sum()) == 0
    assert diff <= R.F32_VS_F64_M


@pytest.mark.parametrize('frac', [0.5, 0.25])
def test_restatement_finds_the_box_room_s_walls(scene, casts, frac):
    """A sanity check, not the parity check: within 3 voxels of the analytic wall, not within rounding.  The volume samples the
    room at lo + i voxel, while grid_sample with align_corners spreads the same samples over the SNAPPED tsdf_bnds, so voxel i sits
    at lo + i extent / (size - 1): the level set is displaced by up to one voxel across the volume, and by more along a grazing
    ray (measured: up to 2.0 voxels at these poses)."""
    sc, poses, cam = scene
    got = casts[(frac, torch.float32)]
    for v in range(poses.shape[0]):
        ro, rd = get_rays(*cam, poses[v], 'cpu')
        want = synthetic.box_depth(ro.reshape(-1, 3), rd.reshape(-1, 3), sc.lo_in, sc.hi_in).reshape(sc.H, sc.W)
        gap = ((got[v] - want).abs().max() / VOXEL).item()
        print(f'step {frac} voxel, pose {v}: max gap to the analytic wall {gap:.2f} voxels')
        assert gap <= 3.0


def test_near_and_far_cut_the_restatement(scene):
    sc, poses, cam = scene
    full = R.raycast(sc.tsdf_volume, sc.tsdf_bnds, poses[0], *cam, step=0.5 * VOXEL)
    near, far = R.NEAR_FAR
    cut = R.raycast(sc.tsdf_volume, sc.tsdf_bnds, poses[0], *cam, near=near, far=far, step=0.5 * VOXEL)
    assert int(((cut > 0) & ((cut < near) | (cut > far))).sum()) == 0
    assert int(((full < near) & (cut != 0)).sum()) == 0                    # a ray that starts behind the wall: 0 (the k = 0 rule)
    assert int((full < near).sum()) > 100 and int((full > far + VOXEL).sum()) > 100 and int((cut > 0).sum()) > 100
    keep = cut > 0
    assert float((cut[keep] - full[keep]).abs().max()) <= 0.5 * VOXEL      # the same wall, met by another sample pair


def tsdf(data=DUMMY, Z=32, Y=40, X=40):
    return _lib.AdfpTsdf(data, Z, Y, X, 1, Z, Z * Y, None)


def bound(lo=-1.0, hi=1.0):
    b = _lib.Bound()
    _lib.fill_bound(b, [[lo, hi]] * 3)
    return b


def cast(t='default', b='default', bricks=DUMMY, nbytes=None, c2w=DUMMY, V=1, H=48, W=64, near=0.0, far=0.0, step=0.02, options=0, depth=DUMMY):
    L = _lib.lib()
    t = tsdf() if t == 'default' else t
    b = bound() if b == 'default' else b
    if nbytes is None:
        nbytes = L.adfp_tsdf_bricks_bytes(t.Z, t.Y, t.X) if t is not None else 1 << 20
    return L.adfp_tsdf_raycast(C.byref(t) if t is not None else None, C.byref(b) if b is not None else None, bricks, nbytes, c2w, V, H, W,
                               57.76, 57.76, 31.5, 23.5, near, far, step, options, depth, None, None)


def test_version_is_unchanged():
    assert _lib.lib().adfp_version() == 134 == _lib.ABI_VERSION           # additive: the version stays
    assert _lib.CAST_NO_SKIP == 1


def test_bricks_bytes():
    L = _lib.lib()
    assert L.adfp_tsdf_bricks_bytes(32, 40, 40) == 4 * ((4 * 5 * 5 + 31) // 32)
    assert L.adfp_tsdf_bricks_bytes(10, 9, 17) == 4                        # 3 x 2 x 2 bricks: one word
    assert L.adfp_tsdf_bricks_bytes(451, 574, 758) == 4 * ((57 * 72 * 95 + 31) // 32)      # room0: 49 KB
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, -1), (32769, 8, 8)):
        assert L.adfp_tsdf_bricks_bytes(*bad) == 0


def test_argument_errors_need_no_gpu():
    L = _lib.lib()
    need = L.adfp_tsdf_bricks_bytes(32, 40, 40)
    # the bitmap's build
    assert L.adfp_tsdf_bricks_build(None, DUMMY, need, None) == ARG
    assert L.adfp_tsdf_bricks_build(C.byref(tsdf(data=None)), DUMMY, need, None) == ARG
    assert L.adfp_tsdf_bricks_build(C.byref(tsdf()), None, need, None) == ARG
    assert L.adfp_tsdf_bricks_build(C.byref(tsdf()), DUMMY, need - 1, None) == ARG
    assert L.adfp_tsdf_bricks_build(C.byref(tsdf()), DUMMY + 2, need, None) == ARG
    for dims in (dict(Z=0), dict(Y=0), dict(X=-4)):
        assert L.adfp_tsdf_bricks_build(C.byref(tsdf(**dims)), DUMMY, 1 << 20, None) == ARG, dims
    assert L.adfp_tsdf_bricks_build(C.byref(tsdf(X=32769)), DUMMY, 1 << 30, None) == UNSUPPORTED
    # the raycast
    assert cast(t=None) == ARG and cast(t=tsdf(data=None)) == ARG and cast(b=None) == ARG
    assert cast(c2w=None) == ARG and cast(depth=None) == ARG
    assert cast(bricks=None) == ARG                                        # only ADFP_CAST_NO_SKIP does without the bitmap
    assert cast(bricks=DUMMY + 1) == ARG and cast(nbytes=need - 1) == ARG and cast(nbytes=0) == ARG
    for dims in (dict(Z=0), dict(Y=-1), dict(X=0)):
        assert cast(t=tsdf(**dims), nbytes=1 << 20) == ARG, dims
    assert cast(V=0) == ARG and cast(V=-2) == ARG and cast(H=0) == ARG and cast(W=0) == ARG and cast(W=-7) == ARG
    assert cast(step=0.0) == ARG and cast(step=-0.02) == ARG and cast(step=float('nan')) == ARG
    assert cast(near=float('nan')) == ARG and cast(far=float('nan')) == ARG
    assert cast(options=2) == ARG and cast(options=-1) == ARG
    assert cast(b=bound(1.0, 1.0)) == ARG and cast(b=bound(1.0, -1.0)) == ARG
    assert cast(t=tsdf(Y=32769), nbytes=1 << 30) == UNSUPPORTED
    assert cast(H=32769) == UNSUPPORTED and cast(W=32769) == UNSUPPORTED and cast(V=65536) == UNSUPPORTED
    assert cast(step=1e-8) == UNSUPPORTED                                  # 3.5 m of diagonal in more than 2^24 samples
