"""CPU, oracle only: the inputs of tests/sample_range_cases.py are what tests/test_gpu_grad_sample_range.py relies on -- an edit of
the builders that empties a condition fails here, not silently on the GPU."""
import torch

import sample_range_cases as SR
from attentive_dfprior_amd import synthetic
from oracle import adfp_oracle as O

NS, NF = 100, 29


def test_s_cases_cover_the_chunk_edges():
    assert [SR.total(*c) for c in SR.S_CASES] == [1, 2, 64, 65, 128, 129, 192, 255, 256]
    assert len({SR.case_id(c) for c in SR.S_CASES}) == len(SR.S_CASES)
    assert any(not c[2] and c[1] > 0 for c in SR.S_CASES)                  # a call without sensor depth that names surface samples


def test_leaving_rays_meet_the_conditions_the_gpu_tests_rely_on(mini):
    sc = synthetic.mini_scene()
    ro, rd, gd, gc = SR.leaving_rays(sc)
    n = ro.shape[0]
    assert n == 24 and int(SR.near_shift(n).sum()) == 6 and int(SR.far_shift(n).sum()) == 6
    sd = O.random_state_dict(seed=17)
    c_or = {k: v.clone().requires_grad_(True) for k, v in mini.c.items()}
    sd_or = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    d, u, col, w, aux = O.render_batch_ray(sd_or, c_or, rd, ro, mini.tsdf_volume, mini.tsdf_bnds, mini.bound, 'color', gd, NS, NF, return_aux=True)
    S = NS + NF
    out = aux['raw'].detach()[..., 3] == 100
    assert tuple(out.shape) == (n, S)
    frac = float(out.float().mean())
    assert 0.10 <= frac <= 0.60, frac
    whole = out.all(dim=1)
    assert int(whole.sum()) >= 3 and bool(whole[SR.far_shift(n)].all())     # the rays moved by 5 m lie outside altogether
    first = torch.where(out.any(dim=1), out.float().argmax(dim=1), torch.full((n,), -1))
    assert int((first >= 64).sum()) >= 6, first.tolist()                   # they leave the bound behind the first chunk
    assert int((gd == 0).sum()) >= 3
    assert int(((gd == 0) & ~whole).sum()) >= 1                            # a zero-depth ray that is not outside altogether
    assert int((~whole).sum()) >= 12                                       # what the Tracker comparison keeps
    O.mapper_loss(d, col, w, gd, gc, 'color', True).backward()
    for k, v in list(c_or.items()) + list(sd_or.items()):
        assert v.grad is None or bool(torch.isfinite(v.grad).all()), k
    assert float(c_or['grid_color'].grad.abs().max()) > 0
