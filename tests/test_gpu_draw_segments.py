"""GPU: render_mesh.draw_segments (adfp_draw_segments, csrc/adfp_segments.h) against the numpy restatement of tests/segments_ref.py.
Both sides do the same correctly rounded f64 operations in the same order (include/adfp.h, "mesh views"), so rgb and seg are
compared EXACTLY: no tolerance anywhere in this file.  The random scenes are drawn from numpy's default_rng(SEED)."""
import functools

import numpy as np
import pytest
import torch

import segments_ref as SR
from attentive_dfprior_amd import render_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 20261020
NEAR_CLIP = 1e-3
PLANE = 2.5                                   # the constant depth image: random segments lie in z = 0.5 .. 5, on both sides of it
BIASES = ((0.0, 0.0), (0.0, 0.05))
ALPHAS = (0.0, 0.5, 1.0)


def camera(H, W):
    return 40.0, 38.0, (W - 1) / 2.0, (H - 1) / 2.0


def poses():
    """Three views: the identity (world = camera space: the named cases below are stated in it), a turned and shifted camera, and
    a pose with a NaN entry."""
    a, b = 0.3, -0.2
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    p = np.stack([np.eye(4)] * 3)
    p[1, :3, :3] = Ry @ Rx
    p[1, :3, 3] = (0.3, -0.2, -0.5)
    p[2, 1, 1] = np.nan
    return p


def named_segments():
    """The cases of the issue, in view 0's camera space."""
    dup = [[-0.6, -0.4, 1.5], [0.5, 0.45, 2.0]]
    return np.array([
        [[0.0, 0.0, -1.0], [1.0, 0.2, -2.0]],                    # fully behind the camera
        [[0.1, 0.1, -1.0], [-0.3, 0.2, 2.0]],                    # crossing the near plane
        [[0.0005, -0.0002, NEAR_CLIP], [0.5, 0.5, 2.0]],         # an endpoint at exactly z = near_clip
        [[0.125, 0.0, 1.0], [0.125, 0.0, 1.0]],                  # zero length, at the screen point (31, 18)
        dup, dup,                                                # coincident duplicates (their colours differ: all colours are random)
        [[50.0, 50.0, 1.0], [60.0, 50.0, 1.0]],                  # wholly off screen
        [[-1000.0, -700.0, 2.0], [1000.0, 700.0, 2.0]],          # crossing the whole screen from far outside, through the centre
        [[np.nan, 0.0, 1.0], [0.1, 0.2, 2.0]],                   # a NaN endpoint
        [[-0.5, 0.3, 1.0], [0.4, 0.35, 1.2]],                    # in front of the plane
        [[-0.5, -0.3, 4.0], [0.6, -0.2, 3.5]],                   # behind it
        [[-0.4, -0.1, 1.0], [0.5, 0.1, 4.5]],                    # crossing it
    ])


@functools.lru_cache(maxsize=None)
def scene(n):
    """(segments [n,2,3], colors uint8 [n,3]): n = 0 and 1 are what they say (1: the screen-crossing segment); the larger lists are
    random segments with the named ones mixed in at random places."""
    rng = np.random.default_rng(SEED + n)
    if n == 0:
        return np.zeros((0, 2, 3)), np.zeros((0, 3), np.uint8)
    if n == 1:
        return named_segments()[7:8], np.array([[10, 200, 30]], np.uint8)
    named = named_segments()
    segs = rng.uniform((-2.0, -1.5, 0.5), (2.0, 1.5, 5.0), size=(n - len(named), 2, 3))
    short = rng.random(len(segs)) < 0.5                           # half of them short: long ones alone would cover everything
    segs[short, 1] = segs[short, 0] + rng.uniform(-0.3, 0.3, size=(int(short.sum()), 3))
    segs = np.concatenate([segs, named])
    perm = rng.permutation(n)
    i5, i6 = sorted((int(np.nonzero(perm == len(segs) - len(named) + 4)[0][0]), int(np.nonzero(perm == len(segs) - len(named) + 5)[0][0])))
    colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    colors[i5], colors[i6] = (250, 10, 10), (10, 10, 250)        # the two duplicates
    return segs[perm], colors


def ranges_for(n):
    """Three ranges per view: two overlapping and an empty one; an inverted one and two overlapping ones that reach past both ends
    of the list; the last view's are never read for a pixel (its pose is not finite)."""
    return np.array([[[0, n // 2], [n // 3, (2 * n) // 3], [5, 5]],
                     [[n, 0], [-7, n // 4 + 1], [n // 5, n + 50]],
                     [[0, n], [0, n], [0, n]]], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def images(H, W):
    """(rgb uint8 [3,H,W,3], depth f32 [3,H,W]): a random picture and the constant plane with a fifth of its pixels 0."""
    rng = np.random.default_rng(SEED + 1000 * H + W)
    rgb = rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    depth = np.where(rng.random((3, H, W)) < 0.2, 0.0, PLANE).astype(np.float32)
    return rgb, depth


@functools.lru_cache(maxsize=None)
def reference(H, W, n, width, with_ranges):
    """The winners of one configuration, computed once and shared by the paint variants."""
    segs, _ = scene(n)
    return SR.winners(poses(), H, W, *camera(H, W), segs, ranges_for(n) if with_ranges else None, 0.5 * width, NEAR_CLIP)


def run(rgb, depth, H, W, n, width, with_ranges, bias=(0.0, 0.0), alpha=0.0, segs=None, colors=None):
    s, c = scene(n)
    s, c = (s if segs is None else segs), (c if colors is None else colors)
    out = torch.from_numpy(rgb).to(DEV)
    seg = render_mesh.draw_segments(out, None if depth is None else torch.from_numpy(depth).to(DEV), poses(), *camera(H, W), s, c,
                                    ranges_for(n) if with_ranges else None, width=width, near_clip=NEAR_CLIP, bias=bias, hidden_alpha=alpha,
                                    want_seg=True)
    return out.cpu().numpy(), seg.cpu().numpy()


def check_case(H, W, n, width, with_ranges):
    rgb, depth = images(H, W)
    want_seg, want_z = reference(H, W, n, width, with_ranges)
    _, colors = scene(n)
    variants = [(None, (0.0, 0.0), 0.0)] + [(depth, b, a) for b in BIASES for a in ALPHAS]
    for dep, bias, alpha in variants:
        got_rgb, got_seg = run(rgb, dep, H, W, n, width, with_ranges, bias, alpha)
        want_rgb = SR.paint(rgb, dep, want_seg, want_z, colors, bias[0], bias[1], alpha)
        what = (H, W, n, width, with_ranges, dep is not None, bias, alpha)
        bad = got_seg != want_seg
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got_seg[bad][:5], want_seg[bad][:5])
        bad = (got_rgb != want_rgb).any(-1)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5], got_rgb[bad][:5], want_rgb[bad][:5])
        assert np.array_equal(got_rgb[2], rgb[2]) and (got_seg[2] == -1).all()        # the NaN pose's view is left alone
    return want_seg, want_z


@pytest.mark.parametrize('with_ranges', [False, True])
@pytest.mark.parametrize('width', [0.5, 1.0, 2.5])
@pytest.mark.parametrize('n', [0, 1, 300, 600])
def test_equals_the_restatement_37x53(n, width, with_ranges):
    seg, z = check_case(37, 53, n, width, with_ranges)
    if n >= 300 and width >= 1.0:                                # the scene exercises what it is meant to
        _, depth = images(37, 53)
        won = seg[:2] >= 0
        assert won.mean() > 0.2 and (~won).any()
        assert (won & (depth[:2] > 0) & (z[:2] > PLANE)).any() and (won & (depth[:2] > 0) & (z[:2] <= PLANE)).any()
        assert len(np.unique(seg[0])) > 30


@pytest.mark.parametrize('with_ranges', [False, True])
@pytest.mark.parametrize('n', [0, 1, 300, 600])
@pytest.mark.parametrize('H,W', [(16, 16), (1, 1)])
def test_equals_the_restatement_one_tile_and_one_pixel(H, W, n, with_ranges):
    seg, _ = check_case(H, W, n, 1.0, with_ranges)
    if n == 1 and not with_ranges:
        assert (seg[0] == 0).any()                               # 1 x 1: the screen-crossing segment runs through the only pixel


def test_named_cases_in_the_identity_view():
    """What each named segment does alone, stated without the restatement: nothing for the four that must draw nothing."""
    H, W = 37, 53
    rgb, _ = images(H, W)
    named = named_segments()
    colors = np.full((len(named), 3), 7, np.uint8)
    for k in range(len(named)):
        r = np.array([[[k, k + 1]]] * 3, dtype=np.int64)
        out = torch.from_numpy(rgb).to(DEV)
        seg = render_mesh.draw_segments(out, None, poses(), *camera(H, W), named, colors, r, width=1.0, near_clip=NEAR_CLIP, want_seg=True)
        seg = seg.cpu().numpy()
        assert set(np.unique(seg)) <= {-1, k}
        if k in (0, 6, 8):                                       # behind the camera, off screen, a NaN endpoint
            assert (seg == -1).all() and np.array_equal(out.cpu().numpy(), rgb), k
        else:
            assert (seg[0] == k).any(), k
        if k == 3:                                               # zero length: a disc of radius 0.5 about the pixel centre (31, 18)
            assert int((seg[0] == k).sum()) == 1 and seg[0, 18, 31] == k
        if k == 7:                                               # a diagonal through the centre that leaves no column out
            assert seg[0, 18, 26] == k and (seg[0] == k).any(0).all()


def test_two_calls_give_the_same_bytes_and_the_order_of_the_list_does_not_matter():
    H, W, n = 37, 53, 300
    rgb, depth = images(H, W)
    a_rgb, a_seg = run(rgb, depth, H, W, n, 2.5, True, (0.0, 0.05), 0.5)
    b_rgb, b_seg = run(rgb, depth, H, W, n, 2.5, True, (0.0, 0.05), 0.5)
    assert np.array_equal(a_rgb, b_rgb) and np.array_equal(a_seg, b_seg)
    # a list without coincident segments (the random part alone), permuted: rgb keeps every byte, seg names the same segments
    rng = np.random.default_rng(SEED - 1)
    segs = rng.uniform((-2.0, -1.5, 0.5), (2.0, 1.5, 5.0), size=(n, 2, 3))
    colors = rng.integers(0, 256, size=(n, 3), dtype=np.uint8)
    perm = rng.permutation(n)
    p_rgb, p_seg = run(rgb, depth, H, W, n, 1.0, False, segs=segs, colors=colors)
    q_rgb, q_seg = run(rgb, depth, H, W, n, 1.0, False, segs=segs[perm], colors=colors[perm])
    assert np.array_equal(p_rgb, q_rgb)
    assert np.array_equal(p_seg, np.where(q_seg >= 0, perm[np.maximum(q_seg, 0)], -1))
    assert (p_rgb != rgb).any()


def test_views_go_through_in_chunks():
    H, W, n = 37, 53, 300
    rgb, depth = images(H, W)
    s, c = scene(n)
    whole, _ = run(rgb, depth, H, W, n, 1.0, True)
    out = torch.from_numpy(rgb).to(DEV)
    seg = render_mesh.draw_segments(out, torch.from_numpy(depth).to(DEV), poses(), *camera(H, W), s, c, ranges_for(n), width=1.0,
                                    near_clip=NEAR_CLIP, want_seg=True, chunk=1)
    assert np.array_equal(out.cpu().numpy(), whole) and seg.shape == (3, H, W)
    assert render_mesh.draw_segments(out, None, poses(), *camera(H, W), s, c) is None
    with pytest.raises(ValueError):
        render_mesh.draw_segments(out, None, poses()[:2], *camera(H, W), s, c)
    with pytest.raises(ValueError):
        render_mesh.draw_segments(out, None, poses(), *camera(H, W), s, c[:-1])
    with pytest.raises(ValueError):
        render_mesh.draw_segments(out, None, poses(), *camera(H, W), s, c, np.zeros((3, 9, 2), np.int64))
    with pytest.raises(RuntimeError):
        render_mesh.draw_segments(out, None, poses(), *camera(H, W), s, c, width=200.0)


CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (2.5, 3.5)], dtype=np.float64)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                   [1, 5, 7], [1, 7, 3]], dtype=np.int64)


def test_a_segment_through_a_cube_is_hidden_inside_and_behind_it():
    """Real mesh depth: a unit cube at z = 2.5 .. 3.5 seen from the origin through MeshViews.render, and a segment that starts beside
    and in front of it, enters it through its front face and ends behind it."""
    H, W = 37, 53
    fx, fy, cx, cy = camera(H, W)
    mv = render_mesh.MeshViews(CUBE_V, CUBE_F, None, DEV)
    r = mv.render(np.eye(4)[None], H, W, fx, fy, cx, cy)
    depth = r['depth'].cpu().numpy()
    before = r['rgb'].cpu().numpy()
    assert (depth[0, 14:23, 20:33] == 2.5).all() and (depth[0, :5] == 0).all()                # the front face; nothing above it
    segs = np.array([[[-0.4, 0.0, 1.5], [0.4, 0.0, 4.5]]])
    red = np.array([[255, 0, 0]], np.uint8)
    rgb = r['rgb'].clone()
    seg = render_mesh.draw_segments(rgb, r['depth'], np.eye(4)[None], fx, fy, cx, cy, segs, red, width=1.0, want_seg=True).cpu().numpy()
    got = rgb.cpu().numpy()
    want_rgb, want_seg = SR.draw_segments(before, depth, np.eye(4)[None], fx, fy, cx, cy, segs, red, None, 0.5)
    assert np.array_equal(seg, want_seg) and np.array_equal(got, want_rgb)
    _, z = SR.winners(np.eye(4)[None], H, W, fx, fy, cx, cy, segs, None, 0.5)
    on = seg[0] == 0
    is_red = (got[0] == (255, 0, 0)).all(-1)
    over_cube = on & (depth[0] > 0)
    assert (on & (depth[0] == 0)).any() and (is_red[on & (depth[0] == 0)]).all()              # beside the cube: drawn
    assert (over_cube & (z[0] <= 2.5)).any() and is_red[over_cube & (z[0] <= 2.5)].all()      # in front of its face: drawn
    assert (over_cube & (z[0] > 2.5)).any() and not is_red[over_cube & (z[0] > 2.5)].any()    # inside and behind: hidden
    assert np.array_equal(got[0][~is_red], before[0][~is_red])
    faint = r['rgb'].clone()
    render_mesh.draw_segments(faint, r['depth'], np.eye(4)[None], fx, fy, cx, cy, segs, red, width=1.0, hidden_alpha=0.5)
    f = faint.cpu().numpy()[0]
    hid = over_cube & (z[0] > 2.5)
    assert (f[hid, 0] > before[0][hid, 0]).all() and (f[hid, 1] < before[0][hid, 1]).all() and np.array_equal(f[is_red], got[0][is_red])
