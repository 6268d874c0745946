"""Inputs shared by the tests over the sample-count range (tests/test_sample_range_cases.py checks the builders on the CPU with the
oracle, tests/test_gpu_grad_sample_range.py runs the kernels on them).

S, the number of samples per ray, is N_samples + N_surface with sensor depth and N_samples alone without (N_surface is then
ignored and the far plane comes from the slab test alone).  The ABI takes 1 <= S <= 256; the ray-major kernels work in chunks of 64
samples (k_composite, composite_bwd_block: up to four chunks with a transmittance carried forwards and a suffix sum carried
backwards), k_tsdf packs RB rays into a block with RB * S <= 2048 (S = 128 and 256 fill it exactly, 129 halves RB), the samplers
stage 8 slots per round.  S_CASES sits on those edges: one sample, one chunk exactly, one sample into the second chunk, two chunks
exactly and one more, three chunks, one short of the maximum, the maximum.

leaving_rays: a batch whose rays leave the scene bound somewhere along the ray (occupancy 100 from there on: alpha = 1 exactly, f =
1e-10, the transmittance underflows after a few such samples) or lie outside altogether, with zero-depth rays among them."""
import torch

from attentive_dfprior_amd import synthetic

# (n_samples, n_surface, with_depth)
S_CASES = [
    (1, 0, False),        # S = 1
    (1, 1, True),         # S = 2
    (64, 16, False),      # S = 64: the surface count is ignored without sensor depth
    (48, 17, True),       # S = 65
    (96, 32, True),       # S = 128
    (100, 29, True),      # S = 129
    (160, 32, True),      # S = 192
    (200, 55, True),      # S = 255
    (224, 32, True),      # S = 256
]


def total(n_samples, n_surface, with_depth):
    return n_samples + (n_surface if with_depth else 0)


def case_id(case):
    return f'S{total(*case)}-{case[0]}+{case[1]}-{"depth" if case[2] else "nodepth"}'


def plain_rays(scene, n=24):
    """The 24 rays of the sweep: three poses inside the room, a tenth at zero depth."""
    return synthetic.make_ray_batch(scene, n, seed=8, poses=3)


def near_shift(n=24):
    """The rays leaving_rays moves by +0.45 m in x: they start inside and leave the bound early."""
    return torch.arange(n) % 4 == 1


def far_shift(n=24):
    """The rays leaving_rays moves by +5 m in x: every sample lies outside the bound."""
    return torch.arange(n) % 4 == 3


def leaving_rays(scene, n=24):
    """(rays_o, rays_d, gt_depth, gt_color): depths stretched by 1.8 (the surface samples and the far clamp reach beyond the wall, so
    the rays leave the bound late in the row), a quarter of the origins moved by 0.45 m, another quarter by 5 m."""
    ro, rd, gd, gc = synthetic.make_ray_batch(scene, n, seed=8, poses=3, zero_frac=0.2)
    gd = gd * 1.8
    ro = ro.clone()
    ro[near_shift(n), 0] += 0.45
    ro[far_shift(n), 0] += 5.0
    return ro.contiguous(), rd.contiguous(), gd.contiguous(), gc.contiguous()


def subset(rays, rows):
    return tuple(t[rows].contiguous() for t in rays)
