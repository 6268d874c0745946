"""GPU: the lane-per-ray sampler (k_sample: a wave takes 64 rays, every lane merges its ray's uniform and surface lists with two
pointers) against oracle.adfp_oracle.sample_z on the CPU, bit for bit.

130 rays = two full waves and a ragged third (130 is a multiple of neither 4 nor 64).  Batches below MERGE_MIN_RAYS
(ADFP_SAMPLE_MERGE_MIN_RAYS, csrc/adfp_kernels.hip) keep the wave-per-four-rays kernel, so every case runs twice: on the 130 rays
(k_sample_small) and on MERGE_MIN_RAYS + 130 rays, the same 130 rows over and over (k_sample: 627 full waves and a ragged one); one
case runs on both sides of the threshold itself.  The rows hold what the merge and its fall-back can get wrong:
  positive depths; depth 0 (the surface list runs from 0.001 to the batch maximum); rays whose far < near (a descending uniform list)
  BETWEEN ordinary rays, so that the O(S^2) recount runs inside a wave of merged rays; a zero direction component with the origin on
  that bound plane (NaN far plane: every uniform sample NaN); lindisp with a zero depth (inf * 0 in the last uniform sample); a depth at
  which a uniform and a surface sample are EXACTLY equal (the tie goes to the uniform element, like torch.sort's stable order -- only
  the values matter, and they are equal, but the merge must still emit both); N_surface = 0 (no sort); perturb = 1 with a fixed t_rand.

Every case also runs with rows above 64 samples (LONG_ROWS: S = 65, 129, 255, 256 = the ABI's maximum; 250 uniform samples alone):
k_sample's staging rounds of 8 slots end ragged at 65 and 255, its wave-wide recount of a degenerate row and k_sample_small's
lane-per-element loops take two to four passes, and k_sample_small's LDS row is full at 256.

The comparison is on the int64 view of the f64 rows.  Both sides' NaNs are first replaced by ONE quiet NaN: which sign and payload
an invalid operation returns is the processor's choice (x86 gives the negative default NaN, the GPU the positive one), not the
sampler's."""
import numpy as np
import pytest
import torch

import attentive_dfprior_amd as A
from attentive_dfprior_amd import synthetic
from oracle import adfp_oracle as O
from conftest import make_cfg, to_dev

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 130
MERGE_MIN_RAYS = 40000
SIZES = [N, MERGE_MIN_RAYS + N]
# f32 depths found by search: with the batch maximum DMAX the far plane of a ray that stays inside the bound is f32(1.2f * DMAX), and
# for N_samples 5 / N_surface 3 uniform sample 2 (t = 0.5: near / 2 + far / 2, exact in f64) of depth TIE equals surface sample 0
# (f32(0.95f * TIE)) to the last bit
DMAX = float.fromhex('0x1.0003bp-1')
TIE = float.fromhex('0x1.4519p-2')
CTR = [0.25, 0.125, 0.125]
I_DESC = (3, 70)            # far < near
I_NAN = (71, 128)           # NaN far plane
I_ZERO = (5, 64, 128, 129)  # zero depth
I_TIE = 66
# rows above 64 samples: S = 65 (a ragged last staging round of k_sample: 65 = 8 x 8 + 1; one element in the second pass of the lane-per-
# element loops), 129, 255 (ragged again) and 256 = ADFP_MAX_SAMPLES (k_sample_small's whole LDS row, four passes per lane in the
# recount of a degenerate row)
LONG_ROWS = [(48, 17), (100, 29), (200, 55), (224, 32)]
MAX_NS = 250            # test_no_surface_samples' longest row; t_rand has that many columns


class ExactScene(object):
    """A bound made of binary fractions: an f32 origin can sit exactly on an f64 bound plane."""

    def __init__(self):
        self.bound = torch.tensor([[-1.0, 1.5], [-1.0, 1.25], [-0.75, 1.0]], dtype=torch.float64)
        self.c = synthetic.make_grids(self.bound, seed=4, std_scale=30.0)
        self.tsdf_volume, self.tsdf_bnds, _ = synthetic.make_box_room_tsdf(self.bound, voxel=0.0625, inset=0.25, trunc_voxels=3.0)
        self.vol_bnds = self.tsdf_bnds
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = 48, 64, 57.76, 57.76, 31.5, 23.5


def make_rays():
    g = torch.Generator().manual_seed(11)
    ro = torch.tensor(CTR, dtype=torch.float32).repeat(N, 1)
    rd = torch.rand(N, 3, generator=g) * 2 - 1
    rd[:, 2] = -1.0
    rd[::3] *= 2.5                                   # these leave the bound before 1.2 x the depth maximum: far comes from the slab test
    gd = 0.1 + 0.35 * torch.rand(N, generator=g)
    gd[0] = DMAX
    for i in I_ZERO:
        gd[i] = 0.0
    for i in I_DESC:                                 # outside the bound and heading away: far_bb < 0, clamped to 0 < near
        ro[i] = torch.tensor([2.0, 0.125, 0.125])
        rd[i] = torch.tensor([0.5, 0.1, -1.0])
    ro[71] = torch.tensor([-1.0, 0.125, 0.125]); rd[71] = torch.tensor([0.0, 0.3, -1.0])      # 0 / 0 in the x slab
    ro[128] = torch.tensor([1.5, 0.125, 0.125]); rd[128] = torch.tensor([0.0, -0.2, -1.0])
    rd[I_TIE] = torch.tensor([0.1, 0.2, -1.0])
    gd[I_TIE] = TIE
    assert float(gd.max()) == DMAX
    return ro, rd.float(), gd.float()


@pytest.fixture(scope='module')
def setup():
    sc = ExactScene()
    dec = A.DF()
    dec.load_state_dict(O.random_state_dict(seed=3))
    dec.bound = sc.bound
    dec = dec.to(DEV)
    ro, rd, gd = make_rays()
    t_rand = torch.rand(MERGE_MIN_RAYS + N, MAX_NS, generator=torch.Generator().manual_seed(12))
    return dict(sc=sc, dec=dec, c=to_dev(sc.c, DEV), vol=sc.tsdf_volume.to(DEV), bnds=sc.tsdf_bnds.to(DEV),
                ro=ro, rd=rd, gd=gd, t_rand=t_rand)


def canon(z):
    z = np.ascontiguousarray(z, dtype=np.float64).copy()
    z[np.isnan(z)] = np.float64('nan')
    return z.view(np.int64)


def run(s, n, ns, nf, lindisp=False, perturb=0.0):
    """The first n rays of the 130 rows repeated; returns the oracle's rows."""
    rep = (n + N - 1) // N
    ro, rd, gd = (t.repeat(*((rep,) + (1,) * (t.dim() - 1)))[:n].contiguous() for t in (s['ro'], s['rd'], s['gd']))
    tr = s['t_rand'][:n, :ns].contiguous() if perturb > 0 else None
    ref = O.sample_z(ro, rd, gd, s['sc'].bound, ns, nf, lindisp=lindisp, perturb=perturb, t_rand=tr).numpy()
    rend = A.Renderer(make_cfg(ns, nf, lindisp=lindisp, perturb=perturb), None, s['sc'])
    with torch.no_grad():
        aux = rend._engine.render_forward(s['dec'], s['c'], ro.to(DEV), rd.to(DEV), gd.to(DEV), s['vol'], s['bnds'],
                                          s['sc'].bound, 'color', ns, nf, lindisp=lindisp, perturb=perturb,
                                          t_rand=tr.to(DEV) if tr is not None else None, want_aux=True)[4]
    z = aux['z_vals'].cpu().numpy()
    assert z.shape == ref.shape == (n, ns + nf) and z.dtype == np.float64
    a, b = canon(z), canon(ref)
    rows = np.nonzero((a != b).any(axis=1))[0]
    print(f'{n} rays, ns {ns} nf {nf} lindisp {lindisp} perturb {perturb}: {len(rows)} of {n} rows differ {rows[:10].tolist()}; '
          f'NaN rows {np.nonzero(np.isnan(ref).any(axis=1))[0][:8].tolist()}')
    assert len(rows) == 0, (rows.tolist(), z[rows[0]].tolist(), ref[rows[0]].tolist())
    return ref


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('ns,nf', [(48, 16), (5, 3)] + LONG_ROWS)
@pytest.mark.parametrize('lindisp', [False, True])
def test_merge_bit_exact(setup, n, ns, nf, lindisp):
    ref = run(setup, n, ns, nf, lindisp=lindisp)
    # the rows are what the docstring says they are
    for i in I_NAN:                                  # every uniform sample NaN, sorted behind the surface samples
        assert np.isnan(ref[i]).sum() == ns and np.isnan(ref[i, nf:]).all()
    ok = np.ones(n, dtype=bool)
    ok[[i + N * k for i in I_NAN for k in range(n // N + 1) if i + N * k < n]] = False
    if not lindisp:
        assert np.isfinite(ref[ok]).all()
        for i in I_DESC:                             # descending uniform list: far = 0 < near
            u = O.sample_z(setup['ro'][i:i + 1], setup['rd'][i:i + 1], setup['gd'][i:i + 1], setup['sc'].bound, ns, 0,
                           depth_max=torch.tensor(DMAX)).numpy()[0]
            assert u[0] > u[-1] == 0.0
    else:
        for i in I_ZERO:
            assert np.isnan(ref[i, -1])              # inf * 0 in the last uniform sample, sorted last
        assert np.isfinite(ref[5, :-1]).all()
    if (ns, nf, lindisp) == (5, 3, False):           # the tie: uniform sample 2 == surface sample 0, both in the row
        near, far, t = np.float32(TIE) * np.float32(0.01), np.float64(np.float32(DMAX) * np.float32(1.2)), np.float32(0.5)
        u2 = np.float64(near * (np.float32(1) - t)) + far * np.float64(t)
        s0 = np.float64(np.float32(0.95) * np.float32(TIE))
        assert u2 == s0 and (ref[I_TIE] == s0).sum() == 2


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('ns', [48, 5, 250])
def test_no_surface_samples(setup, n, ns):
    """N_surface = 0: the uniform list as it is, no sort (the descending rows stay descending)."""
    ref = run(setup, n, ns, 0)
    assert ref[I_DESC[1], 0] > ref[I_DESC[1], -1]


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('ns,nf', [(48, 16), (5, 3)] + LONG_ROWS)
def test_perturbed(setup, n, ns, nf):
    run(setup, n, ns, nf, perturb=1.0)


@pytest.mark.parametrize('n', [MERGE_MIN_RAYS - 1, MERGE_MIN_RAYS])
def test_both_sides_of_the_threshold(setup, n):
    run(setup, n, 48, 16)


def test_threshold_is_the_kernel_source_s():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'attentive_dfprior_amd', 'csrc', 'adfp_kernels.hip')).read()
    assert int(re.search(r'#define ADFP_SAMPLE_MERGE_MIN_RAYS (\d+)', src).group(1)) == MERGE_MIN_RAYS
