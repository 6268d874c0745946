"""Inputs and runners shared by tests/test_gpu_tile_front.py and tools/gen_tile_front_golden.py (which recorded
tests/golden/tile_front.npz with the build BEFORE the tile fronts of k_decode_lc16 / k_decode_high_g / k_attention_g were reworked).

Everything is seeded and built on the CPU; a case is (rays, samples, which TSDF).  The 130 rays hold a ray with a NaN direction
(every point NaN: nan_point_outputs) and one that starts outside the bound heading away (every point out of bound: occupancy 100),
between ordinary rays.  `band32` / `band33` are subsets of the 130 rays whose in-band points number exactly 32 and 33 (a full last
tile of the in-band kernels, and one entry more): the far clamp is pinned to the whole batch's (depth_max), so a ray's samples do
not depend on the subset it is in, and the subset is found from the oracle's per-ray band counts."""
import hashlib

import numpy as np
import torch

from attentive_dfprior_amd import synthetic
from oracle import adfp_oracle as O

N = 130
I_NAN, I_OUT = 5, 7
CTR = [0.25, 0.125, 0.125]
MANY = 40000            # rays of the hash-only case: ~20 000 in-band tiles, more than the 2 048 waves of a launch


class Scene(object):
    def __init__(self):
        self.bound = torch.tensor([[-1.0, 1.5], [-1.0, 1.25], [-0.75, 1.0]], dtype=torch.float64)
        self.c = synthetic.make_grids(self.bound, seed=4, std_scale=30.0)
        self.c['grid_high'] = self.c['grid_high'] * 100.0
        self.tsdf_volume, self.tsdf_bnds, _ = synthetic.make_box_room_tsdf(self.bound, voxel=0.0625, inset=0.25, trunc_voxels=3.0)
        self.vol_bnds = self.tsdf_bnds
        self.tsdf_outside = torch.ones_like(self.tsdf_volume)          # every value 1: nothing inside the band
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = 48, 64, 57.76, 57.76, 31.5, 23.5
        self.sd = O.random_state_dict(seed=3)


def make_rays():
    g = torch.Generator().manual_seed(21)
    ro = torch.tensor(CTR, dtype=torch.float32).repeat(N, 1) + (torch.rand(N, 3, generator=g) - 0.5) * 0.2
    rd = torch.rand(N, 3, generator=g) * 2 - 1
    rd[:, 2] = -1.0
    gd = 0.3 + 0.5 * torch.rand(N, generator=g)
    gd[::9] = 0.0                                                        # no sensor depth: the surface list runs to the batch maximum
    rd[I_NAN, 1] = float('nan')
    ro[I_OUT] = torch.tensor([2.0, 0.125, 0.125])
    rd[I_OUT] = torch.tensor([0.5, 0.1, -1.0])
    return ro.float().contiguous(), rd.float().contiguous(), gd.float().contiguous()


def band_subset(counts, target):
    """Indices (ascending) of a subset of `counts` that sums to `target`: subset-sum by dynamic programming, smallest indices first."""
    reach = {0: []}
    for i, c in enumerate(counts):
        if c <= 0:
            continue
        for s, idx in sorted(reach.items()):
            if s + c <= target and s + c not in reach:
                reach[s + c] = idx + [i]
        if target in reach:
            return reach[target]
    raise AssertionError(f'no subset of the rays has {target} in-band points')


def cases(sc):
    """name -> dict(ro, rd, gd, ns, nf, tsdf, depth_max, band): band = the in-band count the case is built for, or None."""
    ro, rd, gd = make_rays()
    dmax = gd.max().reshape(1)
    out = {
        'r3x24': dict(rays=[1, 2, 3], ns=16, nf=8, tsdf='room', band=None),
        'r130x64': dict(rays=list(range(N)), ns=48, nf=16, tsdf='room', band=None),
        'noband': dict(rays=list(range(40)), ns=16, nf=8, tsdf='outside', band=0),
    }
    # per-ray in-band counts at 16 + 8 samples with the batch's far clamp
    ok = [i for i in range(N) if i not in (I_NAN, I_OUT)]
    aux = O.render_batch_ray(sc.sd, sc.c, rd[ok], ro[ok], sc.tsdf_volume, sc.tsdf_bnds, sc.bound, 'color', gd[ok], 16, 8,
                             return_aux=True, depth_max=dmax)[4]
    counts = aux['band'].reshape(len(ok), 24).sum(1).tolist()
    for target in (32, 33):
        sub = band_subset(counts, target)
        out[f'band{target}'] = dict(rays=[ok[i] for i in sub], ns=16, nf=8, tsdf='room', band=target)
    for k, v in out.items():
        idx = torch.tensor(v['rays'])
        v.update(ro=ro[idx].contiguous(), rd=rd[idx].contiguous(), gd=gd[idx].contiguous(), depth_max=dmax)
    rep = (MANY + N - 1) // N
    out['many'] = dict(ro=ro.repeat(rep, 1)[:MANY].contiguous(), rd=rd.repeat(rep, 1)[:MANY].contiguous(), gd=gd.repeat(rep)[:MANY].contiguous(),
                       ns=48, nf=16, tsdf='room', band=None, depth_max=dmax, rays=None)
    return out


def points70():
    """70 explicit points (f64): inside the room, a NaN point, points outside the bound."""
    g = torch.Generator().manual_seed(22)
    p = torch.tensor(CTR, dtype=torch.float64) + (torch.rand(70, 3, generator=g, dtype=torch.float64) - 0.5) * 1.6
    p[11, 2] = float('nan')
    p[12] = torch.tensor([3.0, 0.0, 0.0], dtype=torch.float64)
    return p


def canon(x):
    """The bits of a float array with every NaN replaced by ONE quiet NaN (sign and payload of an invalid operation's result are the
    processor's choice)."""
    x = np.ascontiguousarray(x).copy()
    x[np.isnan(x)] = np.nan
    return x.view(np.int64 if x.dtype == np.float64 else np.int32)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(canon(a).tobytes())
    return h.hexdigest()


def ws_offsets(lib, P):
    """Byte offsets of the in-band list and of att_occ in the forward workspace of a P-point call (csrc/adfp_kernels.hip layout_forward():
    counter block, per-segment maxima, z, raw, list, att_occ, att_u, flags, each rounded up to 256 bytes)."""
    al = lambda n: (n + 255) // 256 * 256
    seg = lib.adfp_workspace_bytes(256) - 256 - 37 * 256
    lst = 256 + seg + al(8 * P) + al(16 * P)
    return lst, lst + al(4 * P)


def run_rays(A, lib, sc_dev, dec, case, dev):
    """One render_forward of a case -> dict of numpy arrays: the frame's outputs, raw, the attention weights (weight) and the in-band
    att_occ values scattered to their points (NaN where a point is not in the band), plus the in-band count."""
    from conftest import make_cfg
    rend = A.Renderer(make_cfg(case['ns'], case['nf']), None, sc_dev['scene'], ray_batch_size=10 ** 9)
    eng = rend._engine
    vol = sc_dev['room'] if case['tsdf'] == 'room' else sc_dev['outside']
    with torch.no_grad():
        d, u, c, w, aux = eng.render_forward(dec, sc_dev['c'], case['ro'].to(dev), case['rd'].to(dev), case['gd'].to(dev), vol, sc_dev['bnds'],
                                             sc_dev['scene'].bound, 'color', case['ns'], case['nf'], depth_max=case['depth_max'], want_aux=True)
    torch.cuda.synchronize()
    P = case['ro'].shape[0] * (case['ns'] + case['nf'])
    ws = eng._ws
    count = int(ws[:4].view(torch.int32).item())
    o_list, o_occ = ws_offsets(lib, P)
    lst = ws[o_list:o_list + 4 * count].view(torch.int32).long()
    occ = ws[o_occ:o_occ + 4 * count].view(torch.float32)
    att_occ = torch.full((P,), float('nan'), dtype=torch.float32, device=ws.device)
    att_occ[lst] = occ
    assert lst.unique().numel() == count
    return dict(depth=d.cpu().numpy(), uncertainty=u.cpu().numpy(), color=c.cpu().numpy(), weight=w.cpu().numpy().reshape(-1),
                raw=aux['raw'].cpu().numpy().reshape(-1, 4), att_occ=att_occ.cpu().numpy(), z_vals=aux['z_vals'].cpu().numpy(), count=count)


def run_points(A, sc_dev, dec, dev):
    """The explicit-point entries on the 70 points: eval_points (f64 and f32 points) and every decoder alone (adfp_decode_single)."""
    from conftest import make_cfg
    rend = A.Renderer(make_cfg(16, 8), None, sc_dev['scene'])
    p = points70().to(dev)
    out = {}
    with torch.no_grad():
        for tag, pts in (('f64', p), ('f32', p.float())):
            raw, w = rend.eval_points(pts, dec, sc_dev['room'], sc_dev['bnds'], c=sc_dev['c'], stage='color')
            out[f'eval_{tag}_raw'], out[f'eval_{tag}_w'] = raw.cpu().numpy(), w.cpu().numpy()
            for name in ('low', 'high', 'color'):
                mlp = getattr(dec, name + '_decoder')
                mlp.bound = sc_dev['scene'].bound
                out[f'single_{tag}_{name}'] = mlp(pts.reshape(1, -1, 3), sc_dev['c']).cpu().numpy()
    torch.cuda.synchronize()
    return out


def device_scene(A, sc, dev):
    dec = A.DF()
    dec.load_state_dict(sc.sd)
    dec.bound = sc.bound
    dec = dec.to(dev)
    sc_dev = dict(scene=sc, c={k: v.to(dev) for k, v in sc.c.items()}, room=sc.tsdf_volume.to(dev), outside=sc.tsdf_outside.to(dev),
                  bnds=sc.tsdf_bnds.to(dev))
    return sc_dev, dec
