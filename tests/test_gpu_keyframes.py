"""GPU: the Mapper's overlap keyframe selection (adfp_keyframe_overlap, attentive_dfprior_amd.keyframes) against the reference's own
method executed on the mini scene (mapper_keyframes.npz), against an f64 restatement at K = 2 000, and the KeyframeStore that
feeds get_samples_multi from device memory."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from attentive_dfprior_amd import common, keyframes as KF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = ('main', 'zeros', 'random')
SCANNET = dict(H=480, W=640, fx=577.590698, fy=578.729797, cx=318.905426, cy=242.683609)     # configs/ScanNet/scannet.yaml


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN, 'mapper_keyframes.npz'))
    return {k: z[k] for k in z.files}


def intr(g):
    H, W, fx, fy, cx, cy = g['intrinsics'].tolist()
    return int(H), int(W), fx, fy, cx, cy


def recorded_counts(g, c):
    total = int(g['pixels']) * int(g['n_samples'])
    return np.rint(g[f'{c}.percent'] * total).astype(np.int64), total


def device_counts(g, c, return_points=False):
    H, W, fx, fy, cx, cy = intr(g)
    t = lambda k: torch.from_numpy(g[f'{c}.{k}']).to(DEV)      # noqa: E731
    return KF.keyframe_overlap_counts(t('idx'), t('depth'), t('c2w'), t('poses'), int(g['n_samples']), H, W, fx, fy, cx, cy,
                                      return_points=return_points)


@pytest.mark.parametrize('case', CASES)
def test_points_bit_exact(gold, case):
    _, pts = device_counts(gold, case, return_points=True)
    torch.cuda.synchronize()
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), gold[f'{case}.points'].view(np.uint32))


@pytest.mark.parametrize('case', CASES)
def test_counts_match_reference(gold, case):
    got = device_counts(gold, case).cpu().numpy().astype(np.int64)
    want, _ = recorded_counts(gold, case)
    amb = gold[f'{case}.ambiguous']
    assert (np.abs(got - want) <= amb).all(), np.nonzero(np.abs(got - want) > amb)
    assert np.array_equal(got[amb == 0], want[amb == 0])


def test_selection_from_fixture_indices(gold):
    compared = 0
    for case in CASES + ('empty',):
        want, total = recorded_counts(gold, case)
        got = device_counts(gold, case).cpu().numpy() if len(want) else want
        if not np.array_equal(got, want):            # only possible through ambiguous points (test_counts_match_reference)
            assert gold[f'{case}.ambiguous'].sum() > 0
            continue
        for s in gold['np_seeds'].tolist():
            for k in (0, 3, 8, 1000):
                np.random.seed(s)
                assert [int(v) for v in KF.select_from_counts(got, total, k)] == gold[f'{case}.sel.{s}.{k}'].tolist(), (case, s, k)
                compared += 1
    assert compared >= 24


def restated_counts(idx, depth, c2w, poses, n_s, H, W, fx, fy, cx, cy, edge=20):
    """The selection's contract restated with torch on the GPU: the points with the reference's f32 torch ops, w2c = inv(pose) in
    f64 rounded to f32, camera coordinates in f32 in the contract's order, the projection and the inside test in f64."""
    i, j = (idx % W).float(), torch.div(idx, W, rounding_mode='floor').float()
    dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
    R = c2w[:3, :3]
    rays_d = (dirs[:, 0:1] * R[:, 0] + dirs[:, 1:2] * R[:, 1]) + dirs[:, 2:3] * R[:, 2]
    rays_o = c2w[:3, 3].expand(rays_d.shape)
    d = depth.reshape(-1)[idx].reshape(-1, 1).repeat(1, n_s)
    t = torch.linspace(0., 1., steps=n_s).to(DEV)
    z = (d * 0.8) * (1. - t) + (d + 0.5) * t
    pts = (rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]).reshape(-1, 3)
    w2c = torch.linalg.inv(poses.double()).float()[:, None, :3, :]                  # [K,1,3,4]
    x = pts[None]
    cam = ((w2c[..., 0] * x[..., 0:1] + w2c[..., 1] * x[..., 1:2]) + w2c[..., 2] * x[..., 2:3]) + w2c[..., 3]
    X, Y, Z = -cam[..., 0].double(), cam[..., 1].double(), cam[..., 2].double()
    zz = Z + 1e-5
    u, v = ((fx * X + cx * Z) / zz).float(), ((fy * Y + cy * Z) / zz).float()
    inside = (u < W - edge) & (u > edge) & (v < H - edge) & (v > edge) & (zz < 0)
    return inside.sum(1).cpu().numpy(), pts


def scannet_scene(K, seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W = SCANNET['H'], SCANNET['W']
    depth = (0.5 + 3.5 * torch.rand(H, W, generator=g)).float()
    depth[:, :40] = 0.0                                                                  # invalid pixels
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([1.0, 0.5, 1.2])
    poses = []
    for _ in range(K):
        a = (torch.rand(3, generator=g) - 0.5) * 1.2                                    # up to ~35 degrees per axis
        cx_, sx_, cy_, sy_, cz_, sz_ = a[0].cos(), a[0].sin(), a[1].cos(), a[1].sin(), a[2].cos(), a[2].sin()
        Rx = torch.tensor([[1, 0, 0], [0, cx_, -sx_], [0, sx_, cx_]])
        Ry = torch.tensor([[cy_, 0, sy_], [0, 1, 0], [-sy_, 0, cy_]])
        Rz = torch.tensor([[cz_, -sz_, 0], [sz_, cz_, 0], [0, 0, 1]])
        p = torch.eye(4)
        p[:3, :3] = Rz @ Ry @ Rx
        if len(poses) % 10 == 9:                                                         # facing away
            p[:3, :3] = p[:3, :3] @ torch.tensor([[-1., 0, 0], [0, 1, 0], [0, 0, -1]])
        p[:3, 3] = c2w[:3, 3] + (torch.rand(3, generator=g) - 0.5) * 1.0
        poses.append(p)
    return depth, c2w, torch.stack(poses).float()


def test_drop_in_end_to_end():
    H, W, fx, fy, cx, cy = (SCANNET[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    depth, c2w, poses = scannet_scene(60, seed=1)
    kd = [{'est_c2w': p.to(DEV), 'idx': 5 * n} for n, p in enumerate(poses)]
    color = torch.rand(H, W, 3, device=DEV)
    depth_d, c2w_d = depth.to(DEV), c2w.to(DEV)
    for seed, npseed, k in ((3, 0, 10), (4, 7, 3), (5, 1, 100)):
        torch.manual_seed(seed)
        np.random.seed(npseed)
        sel = KF.keyframe_selection_overlap(color, depth_d, c2w_d, kd, k, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, device=DEV)
        after = torch.rand(4, device=DEV)
        np_after = np.random.rand()
        torch.manual_seed(seed)
        idx = torch.randint(H * W, (100,), device=DEV)
        assert torch.equal(after, torch.rand(4, device=DEV))                             # one randint of the reference's shape
        got = KF.keyframe_overlap_counts(idx, depth_d, c2w_d, poses.to(DEV), 16, H, W, fx, fy, cx, cy).cpu().numpy()
        ref, pts = restated_counts(idx, depth_d, c2w_d, poses.to(DEV), 16, H, W, fx, fy, cx, cy)
        amb = KF.overlap_ambiguity(pts.cpu().numpy(), poses.numpy(), fx, fy, cx, cy, H, W)
        assert (np.abs(got - ref) <= amb).all()
        assert all(isinstance(v, np.integer) for v in sel) and len(sel) == min(k, int((got > 0).sum()))
        np.random.seed(npseed)
        want = KF.select_from_counts(ref if np.array_equal(got, ref) else got, 1600, k)
        assert np.random.rand() == np_after
        assert [int(v) for v in sel] == [int(v) for v in want]


def test_scale_2000_keyframes():
    H, W, fx, fy, cx, cy = (SCANNET[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    depth, c2w, poses = scannet_scene(2000, seed=2)
    torch.manual_seed(0)
    idx = torch.randint(H * W, (100,), device=DEV)
    got, pts = KF.keyframe_overlap_counts(idx, depth.to(DEV), c2w.to(DEV), poses.to(DEV), 16, H, W, fx, fy, cx, cy, return_points=True)
    got = got.cpu().numpy()
    ref, pts_ref = restated_counts(idx, depth.to(DEV), c2w.to(DEV), poses.to(DEV), 16, H, W, fx, fy, cx, cy)
    amb = KF.overlap_ambiguity(pts_ref.cpu().numpy(), poses.numpy(), fx, fy, cx, cy, H, W)
    assert (np.abs(got - ref) <= amb).all(), np.nonzero(np.abs(got - ref) > amb)
    assert (got > 0).sum() > 100 and (got == 0).sum() > 0                       # both outcomes occur
    # K = 1 and K = 0; poses and the current pose as host tensors
    one = KF.keyframe_overlap_counts(idx, depth, c2w, poses[:1], 16, H, W, fx, fy, cx, cy).cpu().numpy()
    assert one.tolist() == got[:1].tolist()
    host = KF.keyframe_overlap_counts(idx, depth, c2w, poses, 16, H, W, fx, fy, cx, cy).cpu().numpy()
    assert np.array_equal(host, got)
    none, p0 = KF.keyframe_overlap_counts(idx, depth, c2w, poses[:0], 16, H, W, fx, fy, cx, cy, return_points=True)
    assert none.shape == (0,) and p0 is None
    np.random.seed(0)
    assert KF.keyframe_selection_overlap(None, depth.to(DEV), c2w.to(DEV), [], 5, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy,
                                         device=DEV) == []


def test_more_points_than_one_chunk():
    """n N_samples = 6 400 points > the 4 096 held in LDS at a time: the counts add over the chunks."""
    H, W, fx, fy, cx, cy = (SCANNET[k] for k in ('H', 'W', 'fx', 'fy', 'cx', 'cy'))
    depth, c2w, poses = scannet_scene(300, seed=3)
    torch.manual_seed(1)
    idx = torch.randint(H * W, (400,), device=DEV)
    got = KF.keyframe_overlap_counts(idx, depth.to(DEV), c2w.to(DEV), poses.to(DEV), 16, H, W, fx, fy, cx, cy).cpu().numpy()
    ref, pts = restated_counts(idx, depth.to(DEV), c2w.to(DEV), poses.to(DEV), 16, H, W, fx, fy, cx, cy)
    amb = KF.overlap_ambiguity(pts.cpu().numpy(), poses.numpy(), fx, fy, cx, cy, H, W)
    assert (np.abs(got - ref) <= amb).all()
    assert got.max() > 1600


def frames(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for f in range(n):
        c2w = torch.eye(4)
        c2w[:3, 3] = torch.rand(3, generator=g)
        out.append((f * 5, torch.rand(H, W, 3, generator=g), 0.5 + 3 * torch.rand(H, W, generator=g), c2w))
    return out


def test_store_growth_and_views():
    H, W = 48, 64
    data = frames(7, H, W, seed=4)
    st = KF.KeyframeStore(H, W, DEV, capacity=2)
    for idx, color, depth, c2w in data:
        st.append(idx, color, depth, c2w)
    assert len(st) == 7 and st.capacity >= 7 and st.ids == [d[0] for d in data]
    for i, (_, color, depth, c2w) in enumerate(data):
        m, d, c = st.frame(i)
        assert d.is_cuda and tuple(d.shape) == (H, W) and tuple(c.shape) == (H, W, 3)
        assert torch.equal(m.cpu(), c2w) and torch.equal(d.cpu(), depth) and torch.equal(c.cpu(), color)
    P = st.poses()
    assert P.is_contiguous() and tuple(P.shape) == (7, 4, 4) and st[:-1].poses().shape[0] == 6 and len(st[:-1]) == 6
    # device inputs give the same store as host inputs
    st2 = KF.KeyframeStore(H, W, DEV, capacity=3)
    for idx, color, depth, c2w in data:
        st2.append(idx, color.to(DEV), depth.to(DEV), c2w.to(DEV))
    for i in range(7):
        assert all(torch.equal(a, b) for a, b in zip(st.frame(i), st2.frame(i)))
    st3 = KF.KeyframeStore.from_keyframe_dict([{'idx': i, 'color': c, 'depth': d, 'est_c2w': m} for i, c, d, m in data], H, W, DEV)
    assert st3.ids == st.ids and torch.equal(st3.poses(), st.poses())


def test_store_feeds_get_samples_multi_bit_exact():
    H, W = SCANNET['H'], SCANNET['W']
    fx, fy, cx, cy = SCANNET['fx'], SCANNET['fy'], SCANNET['cx'], SCANNET['cy']
    data = frames(10, H, W, seed=6)
    st = KF.KeyframeStore(H, W, DEV, capacity=4)
    for idx, color, depth, c2w in data:
        st.append(idx, color, depth, c2w)
    window = [0, 3, 4, 9, 7]
    torch.manual_seed(11)
    fast = common.get_samples_multi(0, H, 0, W, 1000, H, W, fx, fy, cx, cy, [st.frame(i) for i in window], DEV)
    torch.manual_seed(11)
    parts = []
    for i in window:                                   # the reference's pattern: host images uploaded, then get_samples per frame
        _, color, depth, c2w = data[i]
        parts.append(common.get_samples(0, H, 0, W, 1000, H, W, fx, fy, cx, cy, c2w.to(DEV), depth.to(DEV), color.to(DEV), DEV))
    slow = [torch.cat([p[k].float() for p in parts]) for k in range(4)]
    for a, b in zip(fast, slow):
        assert torch.equal(a, b)


def test_no_pixels_drawn_is_refused():
    with pytest.raises(ValueError, match='no pixels drawn'):
        KF.keyframe_overlap_counts(torch.zeros(0, dtype=torch.int64, device=DEV), torch.ones((4, 4)), torch.eye(4), torch.eye(4)[None], 16,
                                   4, 4, 4.0, 4.0, 1.5, 1.5)
