"""Inputs shared by the tests over the in-band count range (tests/test_inband_cases.py checks the builders on the CPU with the oracle,
tests/test_gpu_grad_inband_range.py runs the kernels on them).

The high decoder and the attention MLP run on the in-band list alone: the points whose TSDF value lies inside (-1 + 1e-4, 1 - 1e-4).
Its length is a device word; every launch is sized from the upper bound P and cut down by that word (k_outer_h's 16-row tiles and its
own row split, the 32-entry tiles of the chain kernels, the partial-sum slots k_reduce_partials_scaled reads: at most one per compute
unit, 256 here and 252 beside the side lane, so that the rows per slot step from 16 to 32 at a count of 16 * 252 + 1 resp.
16 * 256 + 1).  A case is (rays, TSDF volume, expected count) on the mini fixture's geometry at 16 + 8 samples a ray:

  none                 the volume is all 1.0: count 0
  few1, few2           all 1.0 except ONE voxel at 0.0, found by a search with the oracle: count 1 and 2
  edge15 .. edge65     the room volume, a subset of the rays found by subset-sum over the oracle's per-ray counts
  slot252 .. slot256p1 the same at counts 4 032, 4 033, 4 096, 4 097
  all41, all86         the volume is constant 0.25, every point is in the band: P = 984 (a whole number of neither tile) and
                       P = 2 064 (across k_tsdf's 2 048-point block)

Every batch ends with one ANCHOR ray (the four slot cases: with a few copies of it, so that they have one P) that starts outside the bound heading away, with 1.5 x the deepest sensor depth: it pins the
batch's far clamp (1.2 x the largest depth), so a ray's samples do not depend on the subset it is in, and on the border-clamped room
TSDF (-1 outside the wall) none of its own points is in the band.

No point sits near a band threshold.  With |t| the size of a point's oracle TSDF value, either |t| <= 1 - 1e-4 - MARGIN (in the band
by a thousand times what f32 rounding of the trilinear sum can move) or |t| >= 1 - SATURATED (all corners at the clamp value, or as
good as: out of the band by 1e-4 - 1e-6, a hundred times that rounding).  Rays with a point in between are removed before the
subset-sum, voxels that produce one are skipped.  So oracle.adfp_oracle.df_forward's complaint that the kernels and the oracle
disagree on the band is never rounding.  This is a condition on the inputs, met by choosing them; it is no tolerance on the kernels."""
import copy

import torch

from attentive_dfprior_amd import synthetic
from oracle import adfp_oracle as O
from tile_front_cases import band_subset

NS, NF = 16, 8
S = NS + NF
POOL = 340
MARGIN = 1e-3
SATURATED = 1e-6
BAND = 1.0 - 1e-4
ANCHOR_O = [5.0, 0.1, 0.1]
ANCHOR_D = [0.5, 0.1, -1.0]
EDGE_TARGETS = (15, 16, 17, 31, 32, 33, 63, 64, 65)
SLOT_TARGETS = {'slot252': 16 * 252, 'slot252p1': 16 * 252 + 1, 'slot256': 16 * 256, 'slot256p1': 16 * 256 + 1}
ALL_RAYS = {'all41': 41, 'all86': 86}
FEW_RAYS = 40
FEW_CANDIDATES = 100
NAMES = (['none', 'few1', 'few2'] + [f'edge{t}' for t in EDGE_TARGETS] + list(SLOT_TARGETS) + list(ALL_RAYS))
STAGE_HIGH = ('none', 'edge32', 'edge33', 'all41')
UNPRIMED = ('none', 'edge33')
TRACKER = ('none', 'edge33', 'all41')
FORWARD = ('none', 'few1', 'edge32', 'edge33', 'all41', 'all86')
# 4 096 in-band rows in 16-row blocks write every one of 256 slots (and of 252): the case that primes the slots of the other three
SLOT_PRIMER = 'slot256'


class Case(object):
    def __init__(self, name, pool, rows, volume, count, voxel=None):
        """rows: the rays' rows in the pool (pool_rays), ascending; the anchor, where there is one, is the last."""
        self.name, self.rows, self.volume, self.count, self.voxel = name, list(rows), volume, count, voxel
        self.rays = rays = subset(pool, self.rows)
        self.n_rays = rays[0].shape[0]
        self.P = self.n_rays * S


def subset(rays, rows):
    rows = torch.as_tensor(rows, dtype=torch.long)
    return tuple(t[rows].contiguous() for t in rays)


def pool_rays(scene, n=POOL, anchor=True):
    """n ordinary rays of three poses inside the room, none at zero depth, and (last row) the anchor."""
    ro, rd, gd, gc = synthetic.make_ray_batch(scene, n, seed=8, poses=3, zero_frac=0.0)
    if anchor:
        ro = torch.cat([ro, torch.tensor([ANCHOR_O], dtype=ro.dtype)])
        rd = torch.cat([rd, torch.tensor([ANCHOR_D], dtype=rd.dtype)])
        gd = torch.cat([gd, 1.5 * gd.max().reshape(1)])
        gc = torch.cat([gc, torch.full((1, 3), 0.5, dtype=gc.dtype)])
    return ro.contiguous(), rd.contiguous(), gd.contiguous(), gc.contiguous()


def oracle_tsdf(mini, volume, rays):
    """The oracle's TSDF value at every sample of the rays, [N, S]: its sampler, its points, its trilinear lookup."""
    ro, rd, gd, _ = rays
    z = O.sample_z(ro, rd, gd, mini.bound, NS, NF)
    pts = ro[..., None, :] + rd[..., None, :] * z[..., :, None]
    return O.trilerp(volume, pts.reshape(-1, 3), mini.tsdf_bnds).reshape(ro.shape[0], S)


def in_band(t):
    return (t > -1.0 + 1e-4) & (t < 1.0 - 1e-4)


def near_threshold(t):
    a = t.abs()
    return (a > BAND - MARGIN) & (a < 1.0 - SATURATED)


def with_volume(mini, volume):
    """A shallow copy of the mini fixture with another TSDF volume (test_gpu_grad.run / check_tight read mini.tsdf_volume)."""
    m = copy.copy(mini)
    m.tsdf_volume = volume
    return m


def constant_volume(mini, value):
    return torch.full_like(mini.tsdf_volume, value)


def voxel_volume(mini, voxel):
    """All 1.0 except the voxel (x, y, z) at 0.0, in the fixture's permuted [1, 1, Z, Y, X] view."""
    vol = constant_volume(mini, 1.0)
    x, y, z = voxel
    vol[0, 0, z, y, x] = 0.0
    return vol


def _voxel_candidates(mini, rays):
    """Up to FEW_CANDIDATES distinct interior voxels, each the cell of a sample of the ordinary rays."""
    ro, rd, gd, _ = rays
    z = O.sample_z(ro, rd, gd, mini.bound, NS, NF)
    pts = (ro[..., None, :] + rd[..., None, :] * z[..., :, None])[:-1].reshape(-1, 3)              # not the anchor's
    Z, Y, X = mini.tsdf_volume.shape[2:]
    dims = torch.tensor([X, Y, Z], dtype=torch.float64)
    lo, hi = mini.tsdf_bnds[:, 0].double(), mini.tsdf_bnds[:, 1].double()
    idx = torch.floor((pts.double() - lo) / (hi - lo) * (dims - 1)).long()
    ok = ((idx >= 1) & (idx <= dims.long() - 2)).all(dim=1)
    seen, out = set(), []
    for v in idx[ok][::5].tolist():
        if tuple(v) not in seen:
            seen.add(tuple(v))
            out.append(tuple(v))
        if len(out) == FEW_CANDIDATES:
            break
    return out


def find_voxels(mini, rays, wanted=(1, 2)):
    """count -> the first candidate voxel that puts exactly `count` samples of `rays` in the band, none of them near a threshold."""
    found = {}
    for voxel in _voxel_candidates(mini, rays):
        t = oracle_tsdf(mini, voxel_volume(mini, voxel), rays)
        if bool(near_threshold(t).any()):
            continue
        n = int(in_band(t).sum())
        if n in wanted and n not in found:
            found[n] = voxel
        if len(found) == len(wanted):
            break
    missing = [n for n in wanted if n not in found]
    assert not missing, f'no single voxel puts exactly {missing} samples in the band'
    return found


def pick(counts, usable, target, must=()):
    """Ascending pool rows, `must` among them, whose per-ray counts sum to `target` (tile_front_cases.band_subset over the usable
    rows)."""
    fixed = sum(counts[i] for i in must)
    rest = [i for i in usable if i not in must]
    sub = band_subset([counts[i] for i in rest], target - fixed)
    return sorted([rest[k] for k in sub] + list(must))


_BUILT = {}


def build(mini):
    """name -> Case, built once a process."""
    if 'cases' in _BUILT:
        return _BUILT['cases']
    scene = synthetic.mini_scene()
    pool = pool_rays(scene)
    anchor = POOL
    room = mini.tsdf_volume
    t = oracle_tsdf(mini, room, pool)
    counts = in_band(t).sum(dim=1).tolist()
    assert counts[anchor] == 0 and not bool(near_threshold(t[anchor]).any())
    usable = [i for i in range(POOL) if not bool(near_threshold(t[i]).any())]
    out = {}
    first = list(range(FEW_RAYS)) + [anchor]
    out['none'] = Case('none', pool, first, constant_volume(mini, 1.0), 0)
    for n, voxel in sorted(find_voxels(mini, subset(pool, first)).items()):
        out[f'few{n}'] = Case(f'few{n}', pool, first, voxel_volume(mini, voxel), n, voxel=voxel)
    targets = {f'edge{k}': k for k in EDGE_TARGETS}
    targets.update(SLOT_TARGETS)
    rows = {name: pick(counts, usable, target) for name, target in targets.items()}
    # the four slot cases get ONE ray count, made up with further copies of the anchor: the backward's scratch is carved by P, so
    # only a call of the same P leaves its partial sums where the next call's slots are (SLOT_PRIMER)
    n_slot = max(len(rows[name]) for name in SLOT_TARGETS)
    for name, target in targets.items():
        pad = n_slot - len(rows[name]) if name in SLOT_TARGETS else 0
        out[name] = Case(name, pool, rows[name] + [anchor] * (1 + pad), room, target)
    for name, n in ALL_RAYS.items():
        out[name] = Case(name, pool, list(range(n - 1)) + [anchor], constant_volume(mini, 0.25), n * S)
    _BUILT['cases'] = out
    return out


def build_tracker(mini):
    """The Tracker's cases: no anchor (none of its samples is inside, so its variance is 0, and the Tracker loss divides by the
    variance).  The far clamp is pinned by the deepest ordinary ray instead: the pool is cut down to the rays no deeper than one of
    its rays, which is then in every subset.  (Which one: the deepest whose own count leaves a remainder that the others can make up;
    two rays have 26 to 34 in-band points between them, so with the pool's very deepest ray 33 need not be within reach.)"""
    if 'tracker' in _BUILT:
        return _BUILT['tracker']
    full = pool_rays(synthetic.mini_scene(), anchor=False)
    room = mini.tsdf_volume
    for deepest in full[2].argsort(descending=True)[:20].tolist():
        rows = [i for i in range(POOL) if float(full[2][i]) <= float(full[2][deepest])]
        pool = subset(full, rows)
        at = rows.index(deepest)
        t = oracle_tsdf(mini, room, pool)
        counts = in_band(t).sum(dim=1).tolist()
        usable = [i for i in range(len(rows)) if not bool(near_threshold(t[i]).any())]
        if at not in usable:
            continue
        try:
            rows33 = pick(counts, usable, 33, must=(at,))
        except AssertionError:
            continue
        rows41 = sorted([i for i in range(len(rows)) if i != at][:40] + [at])
        out = {'none': Case('none', pool, rows41, constant_volume(mini, 1.0), 0),
               'edge33': Case('edge33', pool, rows33, room, 33),
               'all41': Case('all41', pool, rows41, constant_volume(mini, 0.25), 41 * S)}
        _BUILT['tracker'] = out
        return out
    raise AssertionError('no deepest ray leaves 33 in-band points within reach')
