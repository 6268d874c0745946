"""CPU: the numpy restatement of adfp_draw_segments (tests/segments_ref.py) on cases worked out by hand, the replay's geometry
helpers and its choice of a mesh per frame.  The GPU tests compare the kernels with the restatement exactly; this file pins the
restatement itself."""
import numpy as np
import pytest

import segments_ref as SR
from attentive_dfprior_amd import replay

H, W = 12, 16
FX = FY = 10.0
CX, CY = 7.5, 5.5
EYE = np.eye(4)[None]
WHITE = np.full((1, H, W, 3), 255, np.uint8)
RED, GREEN = (255, 0, 0), (0, 255, 0)


def draw(segments, colors, depth=None, ranges=None, c2w=EYE, **kw):
    return SR.draw_segments(WHITE, depth, c2w, FX, FY, CX, CY, np.asarray(segments, dtype=np.float64), np.asarray(colors, np.uint8),
                            ranges, **kw)


def at_pixel(u, v, z):
    """The camera-space point (identity pose: the world point) that projects to the screen point (u, v) at depth z."""
    return [(u - CX) / FX * z, (v - CY) / FY * z, z]


def test_fronto_parallel_segment_paints_the_rows_within_half_a_pixel():
    # depth 2, from screen (2, 5.25) to (13, 5.25), width 1: row 5 (0.25 away) is inside 0.5, rows 4 and 6 are not
    rgb, seg = draw([[at_pixel(2.0, 5.25, 2.0), at_pixel(13.0, 5.25, 2.0)]], [RED], half_width=0.5)
    want = np.zeros((H, W), bool)
    want[5, 2:14] = True                                       # columns 2 .. 13: the caps reach sqrt(0.25 - 0.0625) = 0.43 < 1 further
    assert np.array_equal(seg[0] == 0, want)
    assert (rgb[0][want] == RED).all() and (rgb[0][~want] == 255).all()
    assert (seg[0][~want] == -1).all()
    # exactly 0.5 away counts (<=): a segment on the line between rows 5 and 6 paints both
    _, seg = draw([[at_pixel(2.0, 5.5, 2.0), at_pixel(13.0, 5.5, 2.0)]], [RED], half_width=0.5)
    assert set(np.nonzero((seg[0] == 0).any(1))[0]) == {5, 6}


def test_depth_along_the_line_is_perspective_correct():
    # screen midpoint of a segment from z = 1 to z = 3: 1 / z is linear on the screen, so z = 1 / ((1 + 1/3) / 2) = 1.5, not 2
    rec = SR.project(np.eye(4)[:3].reshape(12), np.array([at_pixel(3.0, 5.0, 1.0), at_pixel(11.0, 5.0, 3.0)]), FX, FY, CX, CY, 1e-3)
    covered, z = SR.cover(rec, H, W, 0.5)
    assert covered[5, 7] and abs(z[5, 7] - 1.5) < 1e-12
    assert abs(z[5, 3] - 1.0) < 1e-12 and abs(z[5, 11] - 3.0) < 1e-12
    # a plane at 1.6 hides exactly the part of the line deeper than it: the midpoint (1.5) is drawn, the next pixels are not
    depth = np.full((1, H, W), 1.6, np.float32)
    rgb, seg = draw([[at_pixel(3.0, 5.0, 1.0), at_pixel(11.0, 5.0, 3.0)]], [RED], depth=depth, half_width=0.5)
    zs = z[5, 3:12]
    assert (seg[0][5, 3:12] == 0).all()
    assert np.array_equal((rgb[0][5, 3:12] == RED).all(1), zs <= np.float64(np.float32(1.6)))
    assert (rgb[0][5, 3:8] == RED).all() and (rgb[0][5, 8:12] == 255).all()


def test_endpoint_behind_the_camera_ends_at_the_near_plane():
    m = np.eye(4)[:3].reshape(12)
    rec = SR.project(m, np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 3.0]]), FX, FY, CX, CY, 0.5)
    assert rec[2] == 1.0 / 0.5 and rec[5] == 1.0 / 3.0          # w0 = 1 / near_clip
    rec = SR.project(m, np.array([[0.2, 0.0, 3.0], [-0.2, 0.0, -1.0]]), FX, FY, CX, CY, 0.5)
    assert rec[5] == 1.0 / 0.5                                   # the second endpoint clipped: t = (0.5 + 1) / 4, x = -0.2 + t 0.4
    assert abs(rec[3] - (FX * ((-0.2 + 0.375 * 0.4) / 0.5) + CX)) < 1e-12
    assert SR.project(m, np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.4]]), FX, FY, CX, CY, 0.5) is None      # both behind the plane
    assert SR.project(m, np.array([[0.0, 0.0, 0.5], [0.0, 0.0, 3.0]]), FX, FY, CX, CY, 0.5)[2] == 2.0     # exactly on it: not clipped
    assert SR.project(m, np.array([[np.nan, 0.0, 1.0], [0.0, 0.0, 3.0]]), FX, FY, CX, CY, 0.5) is None
    bad = np.eye(4)[None].copy()
    bad[0, 1, 2] = np.inf
    rgb, seg = draw([[at_pixel(2.0, 5.0, 2.0), at_pixel(13.0, 5.0, 2.0)]], [RED], c2w=bad)
    assert (seg == -1).all() and (rgb == 255).all()              # a view with a non-finite pose is left alone


def test_coincident_segments_the_smaller_index_wins():
    s = [at_pixel(2.0, 5.0, 2.0), at_pixel(13.0, 5.0, 2.0)]
    rgb, seg = draw([s, s], [RED, GREEN], half_width=0.5)
    assert set(np.unique(seg)) == {-1, 0} and (rgb[0][seg[0] == 0] == RED).all()
    rgb, seg = draw([s, s], [RED, GREEN], half_width=0.5, ranges=np.array([[[1, 2], [0, 1]]]))      # the order of the ranges does not matter
    assert set(np.unique(seg)) == {-1, 0}
    nearer = [at_pixel(2.0, 5.0, 1.0), at_pixel(13.0, 5.0, 1.0)]
    rgb, seg = draw([s, nearer], [RED, GREEN], half_width=0.5)
    assert set(np.unique(seg)) == {-1, 1} and (rgb[0][seg[0] == 1] == GREEN).all()                  # the nearer one wins whatever its index


def test_plane_hides_the_far_half_and_hidden_alpha_blends():
    s = [[at_pixel(2.0, 5.0, 1.0), at_pixel(13.0, 5.0, 3.0)]]
    depth = np.full((1, H, W), 2.0, np.float32)
    depth[0, 5, 13] = 0.0                                         # nothing hit there: visible whatever the line's depth
    rgb, seg = draw(s, [RED], depth=depth, half_width=0.5)
    z = SR.cover(SR.project(np.eye(4)[:3].reshape(12), np.array(s[0]), FX, FY, CX, CY, 1e-3), H, W, 0.5)[1][5]
    red = (rgb[0][5] == RED).all(1)
    assert np.array_equal(red[2:13], z[2:13] <= 2.0) and red[13] and red[2] and not red[12]
    assert (seg[0][5, 2:14] == 0).all()                           # seg names the segment where it is hidden, too
    rgb_h, _ = draw(s, [RED], depth=depth, half_width=0.5, hidden_alpha=0.5)
    assert (rgb_h[0][5, 12] == (255, 128, 128)).all()             # floor(0.5 * 0 + 0.5 * 255 + 0.5) = 128
    assert np.array_equal(rgb_h[0][5][red], rgb[0][5][red])
    rgb_1, _ = draw(s, [RED], depth=depth, half_width=0.5, hidden_alpha=1.0)
    assert (rgb_1[0][5, 2:14] == RED).all()
    # an absolute bias lifts the plane: 2 (1 + 0) + 0.5
    rgb_b, _ = draw(s, [RED], depth=depth, half_width=0.5, bias_abs=0.5)
    assert np.array_equal((rgb_b[0][5] == RED).all(1)[2:13], z[2:13] <= 2.5)


def test_ranges_clamp_drop_empty_and_count_a_segment_once():
    assert SR.listed(None, 4) == [0, 1, 2, 3]
    assert SR.listed([[-5, 2], [3, 3], [4, 1], [1, 3]], 4) == [0, 1, 2]
    assert SR.listed([[2, 100]], 4) == [2, 3]
    assert SR.n_listed(np.array([[[-5, 2], [3, 3], [4, 1], [1, 3]], [[0, 1], [0, 0], [0, 0], [0, 0]]]), 4) == 4
    s = [[at_pixel(2.0, 5.0, 2.0), at_pixel(13.0, 5.0, 2.0)], [at_pixel(2.0, 8.0, 2.0), at_pixel(13.0, 8.0, 2.0)]]
    depth = np.full((1, H, W), 1.0, np.float32)                   # everything hidden: a segment blended twice would show
    once, seg1 = draw(s, [RED, GREEN], depth=depth, half_width=0.5, hidden_alpha=0.5, ranges=np.array([[[0, 1]]]))
    twice, seg2 = draw(s, [RED, GREEN], depth=depth, half_width=0.5, hidden_alpha=0.5, ranges=np.array([[[0, 1], [0, 1], [2, 9]]]))
    assert np.array_equal(once, twice) and np.array_equal(seg1, seg2)
    assert (once[0][5, 4] == (255, 128, 128)).all() and (once[0][8] == 255).all()


# ---- the replay's helpers ----
CAM = (48, 64, 60.0, 55.0, 30.0, 25.0)


def project(c2w, P):
    cam = (np.asarray(P) - c2w[:3, 3]) @ c2w[:3, :3]
    return np.array([CAM[2] * cam[0] / cam[2] + CAM[4], CAM[3] * cam[1] / cam[2] + CAM[5], cam[2]])


def some_pose():
    c2w = np.eye(4)
    c2w[:3, :] = replay.viewmatrix(np.array([0.3, -0.5, 0.8]), np.array([0.1, 1.0, 0.2]), np.array([1.0, -2.0, 0.5]))
    return c2w


def test_frustum_rays_pass_through_the_image_corners():
    c2w = some_pose()
    seg = replay.frustum_segments(c2w, *CAM, 0.3)
    assert seg.shape == (8, 2, 3)
    Hh, Ww = CAM[:2]
    corners = [(-0.5, -0.5), (Ww - 0.5, -0.5), (Ww - 0.5, Hh - 0.5), (-0.5, Hh - 0.5)]
    for k, (u, v) in enumerate(corners):
        assert np.allclose(seg[k, 0], c2w[:3, 3])
        for t in (1.0, 0.4):                                        # the corner itself and a point part of the way along the ray
            p = project(c2w, c2w[:3, 3] + t * (seg[k, 1] - c2w[:3, 3]))
            assert np.allclose(p[:2], (u, v), atol=1e-9) and abs(p[2] - 0.3 * t) < 1e-12
        assert np.allclose(seg[4 + k, 0], seg[k, 1]) and np.allclose(seg[4 + k, 1], seg[(k + 1) % 4, 1])
    assert replay.trajectory_segments(np.stack([c2w, c2w, c2w])).shape == (2, 2, 3)
    assert replay.trajectory_segments(c2w[None]).shape == (0, 2, 3)
    inf = c2w.copy()
    inf[:3, 3] = -np.inf
    t = replay.trajectory_segments(np.stack([c2w, inf, c2w, c2w]))
    assert t.shape == (3, 2, 3) and not np.isfinite(t[0]).all() and not np.isfinite(t[1]).all() and np.isfinite(t[2]).all()


def test_follow_pose_looks_at_the_camera_centre():
    c2w = some_pose()
    f = replay.follow_pose(c2w, 1.5, 0.7)
    R = f[:3, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.999 and np.allclose(f[3], (0, 0, 0, 1))
    p = project(f, c2w[:3, 3])
    assert np.allclose(p[:2], (CAM[4], CAM[5]), atol=1e-9) and p[2] > 0            # the principal point, in front
    rel = (f[:3, 3] - c2w[:3, 3]) @ c2w[:3, :3]                                      # the follower in the followed camera's axes
    assert np.allclose(rel, (0.0, -0.7, -1.5), atol=1e-12)                           # above (y is down) and behind
    with pytest.raises(ValueError):
        replay.follow_pose(c2w, 0.0, 1.0)


@pytest.mark.parametrize('lo,hi', [((-1.0, -2.0, 0.0), (3.0, 1.0, 2.5)), ((0.0, 0.0, 0.0), (1.0, 6.0, 0.5)), ((-3.0, 2.0, -1.0), (-2.9, 2.1, 4.0))])
def test_overview_pose_holds_the_box_in_frame(lo, hi):
    o = replay.overview_pose(lo, hi, CAM)
    R = o[:3, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.999
    assert np.allclose(R[:, 2], (0, 0, -1))                                          # looking straight down
    for x in (lo[0], hi[0]):
        for y in (lo[1], hi[1]):
            for z in (lo[2], hi[2]):
                u, v, d = project(o, (x, y, z))
                assert d > 0 and 0 <= u <= CAM[1] - 1 and 0 <= v <= CAM[0] - 1, (x, y, z, u, v)


def test_mesh_per_frame():
    names = ['00008_mesh.ply', '00000_mesh.ply', 'final_mesh.ply', '00004_mesh.ply', '00004_mesh_culled.ply', 'notes.txt']
    assert replay.mesh_index(names) == [(0, '00000_mesh.ply'), (4, '00004_mesh.ply'), (8, '00008_mesh.ply')]
    got = replay.mesh_for_frames(names, range(0, 11, 2))
    assert got == ['00000_mesh.ply', '00000_mesh.ply', '00004_mesh.ply', '00004_mesh.ply', '00008_mesh.ply', '00008_mesh.ply']
    assert replay.mesh_for_frames(['00004_mesh.ply'], [0, 3, 4, 5]) == [None, None, '00004_mesh.ply', '00004_mesh.ply']
    assert replay.mesh_for_frames([], [0, 1]) == [None, None]
    assert replay.mesh_for_frames(['/run/mesh/00100_mesh.ply', '/run/mesh/00020_mesh.ply'], [50]) == ['/run/mesh/00020_mesh.ply']


def test_overlay_lists_grow_with_the_frame():
    poses = np.stack([np.eye(4)] * 6)
    poses[:, 0, 3] = np.arange(6)
    segs, colors, ranges = replay.overlay_lists(poses, poses, [0, 2, 4], CAM, 0.2)
    assert segs.shape == (5 + 5 + 3 * 16, 2, 3) and colors.shape == (58, 3) and ranges.shape == (3, 4, 2)
    assert ranges[0].tolist() == [[0, 0], [5, 5], [10, 18], [18, 26]]                # frame 0: no trajectory, its two frusta
    assert ranges[2].tolist() == [[0, 4], [5, 9], [42, 50], [50, 58]]
    assert (colors[:5] == RED).all() and (colors[5:10] == GREEN).all() and (colors[10:18] == RED).all() and (colors[18:26] == GREEN).all()
    _, colors, ranges = replay.overlay_lists(poses, poses, [0, 2, 4], CAM, 0.2, gt_traj=False)
    for i in range(3):
        assert not (colors[SR.listed(ranges[i], len(colors))] == GREEN).all(1).any()
