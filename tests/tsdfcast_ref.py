"""The TSDF raycast (include/adfp.h "TSDF raycast", csrc/adfp_tsdfcast.h) restated with torch on the CPU: the marching loop over
F.grid_sample, every pixel of every view at once.  `dtype` is the precision of the LOOKUP (coordinates, volume, blend): float32 is
the rule the kernel implements, float64 is the yardstick that says how far f32 lookups move a depth.  Ray, interval and march are
f64 in both.  No skip here: the rule has none, the skip must not change a bit."""
import torch
import torch.nn.functional as F

from attentive_dfprior_amd.common import get_rays

# The largest depth difference between the f32 and the f64 restatement on the mini scene (three poses, steps of 1/2 and 1/4
# voxel): test_tsdfcast_host.py measures it (1.7e-7 m when this was written) and asserts it stays below this constant.  The GPU
# test allows the kernel 8 x the constant against the f32 restatement: the kernel's fmaf chain and ATen's blend order are two f32
# evaluations of the same trilinear form, each as far from f64 as the other, and the hit formula divides by f_{k-1} - f_k.
F32_VS_F64_M = 2.0e-7
KERNEL_TOL_M = 8 * F32_VS_F64_M
NEAR_FAR = (0.36, 0.43)          # cuts the first mini pose's room (depths 0.33 .. 0.51 m) on both sides


def mini_poses(sc):
    """Three poses inside the mini scene's room: different yaws and pitches, off-centre."""
    return torch.stack([sc.default_c2w(), sc.default_c2w(offset=(0.1, -0.15, 0.05), yaw=2.1, pitch=0.35),
                        sc.default_c2w(offset=(-0.2, 0.1, -0.1), yaw=-1.2, pitch=-0.5)])


def raycast(tsdf_volume, tsdf_bnds, c2w, H, W, fx, fy, cx, cy, near=0., far=0., step=None, dtype=torch.float32, device='cpu'):
    """tsdf_volume [1,1,Z,Y,X] (any strides), tsdf_bnds [3,2], c2w [V,4,4] or [4,4] -> depth [V,H,W] or [H,W] float32 on `device`
    (the tests run it on the CPU; tools/tsdfcast_bench.py times the same loop on the GPU as the torch baseline)."""
    c2w = torch.as_tensor(c2w).float().cpu()
    if c2w.dim() == 2:
        return raycast(tsdf_volume, tsdf_bnds, c2w[None], H, W, fx, fy, cx, cy, near, far, step, dtype, device)[0]
    vol = tsdf_volume.detach().to(device).to(dtype)
    bnds = tsdf_bnds.detach().to(device).double()
    lo, hi = bnds[:, 0], bnds[:, 1]
    Z, Y, X = vol.shape[2:]
    if step is None:
        step = 0.5 * float(((hi - lo).cpu() / torch.tensor([X, Y, Z], dtype=torch.float64)).min())
    inf = float('inf')
    out = []
    for m in c2w:
        ro, rd = get_rays(H, W, fx, fy, cx, cy, m, device)                    # f32, camera z = -1
        o, d = ro.reshape(-1, 3).double(), rd.reshape(-1, 3).double()
        n = o.shape[0]
        tn, tf = torch.full((n,), -inf, dtype=torch.float64, device=device), torch.full((n,), inf, dtype=torch.float64, device=device)
        for k in range(3):
            moving = d[:, k] != 0
            dk = torch.where(moving, d[:, k], torch.ones_like(d[:, k]))
            t1, t2 = (lo[k] - o[:, k]) / dk, (hi[k] - o[:, k]) / dk
            ta, tb = torch.where(t1 < t2, t1, t2), torch.where(t1 < t2, t2, t1)
            outside = ~moving & ~((o[:, k] >= lo[k]) & (o[:, k] <= hi[k]))
            tn = torch.where(moving, torch.where(ta > tn, ta, tn), tn)
            tf = torch.where(moving, torch.where(tb < tf, tb, tf), tf)
            tn = torch.where(outside, torch.full_like(tn, inf), tn)
            tf = torch.where(outside, torch.full_like(tf, -inf), tf)
        tn = torch.clamp(tn, min=max(float(near), 0.0))
        if far > 0:
            tf = torch.clamp(tf, max=float(far))
        dt = step / torch.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        depth = torch.zeros((n,), dtype=torch.float64, device=device)
        alive = ~(tf < tn)
        f_prev = torch.zeros((n,), dtype=dtype, device=device)
        k = 0
        while True:
            t = tn + k * dt
            alive = alive & (t <= tf)
            if not bool(alive.any()):
                break
            p = o + d * t[:, None]
            pn = ((p - lo) / (hi - lo)) * 2 - 1.0                           # common.normalize_3d_coordinate, f64
            f = F.grid_sample(vol, pn.to(dtype).reshape(1, 1, 1, n, 3), mode='bilinear', padding_mode='border',
                              align_corners=True).reshape(n)
            hit = alive & (f <= 0)
            if k > 0:
                fp, fk = f_prev.double(), f.double()
                d_hit = (tn + (k - 1) * dt) + (dt * fp) / (fp - fk)
                depth = torch.where(hit, d_hit, depth)
            alive = alive & ~hit
            f_prev = f
            k += 1
        out.append(depth.float().reshape(H, W))
    return torch.stack(out)


# ---- small volumes for the empty-space skip -------------------------------------------------------------------------------------
def as_view(phys):
    """[X,Y,Z] contiguous -> the reference's permuted view [1,1,Z,Y,X] (z fastest, get_tsdf.py:95-97)."""
    X, Y, Z = phys.shape
    return phys.reshape(1, 1, X, Y, Z).permute(0, 1, 4, 3, 2)


def bnds_of(phys, voxel=0.04):
    X, Y, Z = phys.shape
    return torch.tensor([[0.0, X * voxel], [0.0, Y * voxel], [0.0, Z * voxel]], dtype=torch.float64)


def one_voxel_volume():
    """3 x 2 x 2 bricks, + 1 everywhere but one solid voxel in the corner brick: every other brick is passed over."""
    phys = torch.ones((24, 16, 16), dtype=torch.float32)
    phys[1, 1, 1] = -1.0
    return phys


def plane_volume():
    """17 x 9 x 10: partial last bricks on every axis (the pad clipped at the volume's edge).  A slanted plane cuts off the corner at
    the origin: the bricks at x >= 8 and the partial ones at y = 8 and z >= 8 are clear, the rays pass over them to the surface."""
    x, y, z = torch.meshgrid(torch.arange(17.), torch.arange(9.), torch.arange(10.), indexing='ij')
    return torch.clamp((0.55 * x + 0.6 * y + 0.58 * z - 3.0) / 3.0, -1.0, 1.0).float()


def small_poses(phys, voxel=0.04):
    """Four poses at the far end of a small volume, on the positive side of both volumes above, fanned over the rest of it."""
    from attentive_dfprior_amd.synthetic import camera_c2w
    X, Y, Z = phys.shape
    ctr = (0.84 * X * voxel, 0.8 * Y * voxel, 0.8 * Z * voxel)
    return torch.stack([camera_c2w(ctr, 1.03, -0.48), camera_c2w(ctr, 1.5, -0.1), camera_c2w(ctr, 0.6, -0.7), camera_c2w(ctr, 1.2, 0.2)])
