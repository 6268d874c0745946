"""GPU: mesh colours from the keyframes' images -- the kernel (mesh.project_colors, adfp_mesh_project_colors) against the f32 numpy
statement of its rule (tests/project_colors_ref.py), the Mesher's keyframe_projection colouring, and the color_mesh command line.

Kernel against statement: both carry out the same f32 operations, so on every vertex that the f64 statement does not mark as
ambiguous (within 1e-3 px of a frame bound, 1e-6 of zz = 0, 1e-4 of the depth tolerance at a corner, 1e-5 relative between the two
best weights) count and best are equal and rgb and wsum agree within 2e-6 relative; an ambiguous vertex -- at most 0.5 % of them --
may differ in count by one view.  The vertex subsets of the launch-geometry cases are drawn from the vertices that are not
ambiguous, so the cap is the full scene's to meet."""
import functools
import os

import numpy as np
import pytest
import torch

import project_colors_ref as R
from attentive_dfprior_amd import color_mesh, mesh as M
from attentive_dfprior_amd.keyframes import KeyframeStore

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 0.1
POSE_TILE = 32                     # ADFP_MPC_TILE of csrc/adfp_meshcolor.h
REL = 2e-6


@functools.lru_cache(maxsize=None)
def scene(K):
    """The cube scene with K keyframes: the four of the host tests, or K seeded cameras beyond four."""
    if K <= 4:
        return R.with_keyframes(R.cube_scene(), K)
    return R.cube_scene(R.many_cameras(K, seed=1))


@functools.lru_cache(maxsize=None)
def scene_device(K):
    s = scene(K)
    return {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ('depth', 'color')}


def kernel(s, verts, normals, tol, border, blend, images=None):
    """mesh.project_colors on a scene dict's arrays -> numpy (rgb, wsum, count, best) and the device tensors."""
    images = images or {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(DEV) for k in ('depth', 'color')}
    out = M.project_colors(torch.from_numpy(verts).to(DEV), None if normals is None else torch.from_numpy(normals).to(DEV),
                           images['depth'], images['color'], torch.from_numpy(s['c2w']), s['fx'], s['fy'], s['cx'], s['cy'], tol, border, blend)
    return tuple(t.cpu().numpy() for t in out), out


def statement(s, verts, normals, tol, border, blend):
    args = (verts, normals, s['w2c'], s['center'], s['depth'], s['color'], s['fx'], s['fy'], s['cx'], s['cy'], tol, border, blend)
    return R.project_colors_ref(*args), R.ambiguity_mask(*args)


def compare(got, ref, amb, what):
    (rgb, wsum, count, best), (rrgb, rwsum, rcount, rbest) = got, ref
    assert rgb.dtype == np.float32 and wsum.dtype == np.float32 and count.dtype == np.int32 and best.dtype == np.int32, what
    assert rgb.shape == rrgb.shape and wsum.shape == rwsum.shape and count.shape == rcount.shape and best.shape == rbest.shape, what
    ok = ~amb
    assert np.array_equal(count[ok], rcount[ok]), (what, int((count[ok] != rcount[ok]).sum()))
    assert np.array_equal(best[ok], rbest[ok]), (what, int((best[ok] != rbest[ok]).sum()))
    for name, a, b in (('rgb', rgb[ok], rrgb[ok]), ('wsum', wsum[ok], rwsum[ok])):
        a, b = a.astype(np.float64), b.astype(np.float64)
        excess = np.abs(a - b) - REL * np.abs(b)
        assert not np.isnan(a).any() and (excess <= 0).all(), (what, name, float(excess.max()))
    assert (np.abs(count[amb].astype(np.int64) - rcount[amb]) <= 1).all(), what


@pytest.mark.parametrize('K', [0, 1, 4, POSE_TILE + 1])
@pytest.mark.parametrize('blend', R.BLENDS)
def test_kernel_matches_statement_on_the_cube(K, blend):
    s, images = scene(K), scene_device(K)
    order = np.random.RandomState(5).permutation(len(s['verts']))
    covered = 0
    for border in (0, 2):
        for with_normals in (True, False):
            normals = s['normals'] if with_normals else None
            ref, amb = statement(s, s['verts'], normals, TOL, border, blend)
            assert amb.mean() <= 0.005, (K, border, with_normals, float(amb.mean()))
            got, _ = kernel(s, s['verts'], normals, TOL, border, blend, images)
            compare(got, ref, amb, (K, blend, border, with_normals, 'all'))
            covered += int((got[2] > 0).sum())
            clear = order[~amb[order]]
            for V in (0, 1, 63, 64, 65, 257):
                pick = clear[:V]
                sub_ref, sub_amb = statement(s, s['verts'][pick], None if normals is None else normals[pick], TOL, border, blend)
                assert not sub_amb.any()
                assert all(np.array_equal(a, b[pick]) for a, b in zip(sub_ref, ref))          # the statement is per vertex
                sub, _ = kernel(s, s['verts'][pick], None if normals is None else normals[pick], TOL, border, blend, images)
                compare(sub, sub_ref, sub_amb, (K, blend, border, with_normals, V))
    if K == 0:
        assert covered == 0
    else:
        assert covered > 400 * K ** 0.5                         # every configuration sees a fair part of the walls


@pytest.mark.parametrize('blend', R.BLENDS)
def test_two_runs_give_identical_bits(blend):
    s, images = scene(POSE_TILE + 1), scene_device(POSE_TILE + 1)
    _, a = kernel(s, s['verts'], s['normals'], TOL, 0, blend, images)
    _, b = kernel(s, s['verts'], s['normals'], TOL, 0, blend, images)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert (a[2] >= 2).sum() > 1000                              # sums of several views were formed


@pytest.mark.parametrize('blend', R.BLENDS)
@pytest.mark.parametrize('border', [0, 2])
@pytest.mark.parametrize('with_normals', [True, False])
def test_cases_by_construction(blend, border, with_normals):
    """Vertices exactly on the frame bounds, behind the camera, beside a hole and a depth edge, with bad normals: the kernel gives
    the constructed answer, not only the statement's."""
    s = R.constructed_scene()
    normals = s['normals'] if with_normals else None
    got, _ = kernel(s, s['verts'], normals, R.CASE_TOL, border, blend)
    ref, _ = statement(s, s['verts'], normals, R.CASE_TOL, border, blend)
    want = R.case_counts(border, with_normals)
    for i, case in enumerate(R.CASES):
        assert got[2][i] == want[i], (i, case[4], int(got[2][i]))
    assert np.array_equal(got[3], np.where(want > 0, 0, -1))
    compare(got, ref, np.zeros(len(want), bool), (blend, border, with_normals))
    assert not got[0][want == 0].any() and not got[1][want == 0].any()


@pytest.mark.parametrize('blend', R.BLENDS)
def test_two_identical_keyframes(blend):
    one, two = R.constructed_scene(1), R.constructed_scene(2)
    a, _ = kernel(one, one['verts'], one['normals'], R.CASE_TOL, 0, blend)
    b, _ = kernel(two, two['verts'], two['normals'], R.CASE_TOL, 0, blend)
    assert np.array_equal(a[0], b[0])                            # WEIGHTED: (w c + w c) / (w + w) is (w c) / w exactly
    assert np.array_equal(b[2], 2 * a[2]) and np.array_equal(b[3], a[3]) and set(b[3].tolist()) == {-1, 0}
    assert np.array_equal(b[1], a[1] * (2 if blend == 'weighted' else 1))


@pytest.mark.parametrize('blend', R.BLENDS)
@pytest.mark.parametrize('border', [0, 2])
def test_clamp_on_a_13_by_9_image(blend, border):
    """Every half pixel of a 13 x 9 image, the last column and row included: x0 = W - 2 and y0 = H - 2 clamp there."""
    s = R.clamp_scene()
    got, _ = kernel(s, s['verts'], s['normals'], TOL, border, blend)
    ref, _ = statement(s, s['verts'], s['normals'], TOL, border, blend)
    want = R.clamp_counts(s, border)
    assert want.sum() == (425 if border == 0 else 17 * 9)
    assert np.array_equal(got[2], want) and np.array_equal(got[3], want - 1)
    compare(got, ref, np.zeros(len(want), bool), (blend, border))
    seen = want > 0
    assert np.abs(got[0][seen] - R.texture(s['verts'][seen])).max() <= 0.01


def test_wrapper_refuses_what_the_contract_refuses():
    s = R.constructed_scene()
    v, d, c, m = (torch.from_numpy(s[k]).to(DEV) for k in ('verts', 'depth', 'color', 'c2w'))
    with pytest.raises(ValueError, match='blend'):
        M.project_colors(v, None, d, c, m, 8, 8, 7.5, 5.5, 0.1, 0, 'mean')
    with pytest.raises(ValueError, match='depth_tol'):
        M.project_colors(v, None, d, c, m, 8, 8, 7.5, 5.5, float('nan'), 0, 'best')
    with pytest.raises(ValueError, match='border'):
        M.project_colors(v, None, d, c, m, 8, 8, 7.5, 5.5, 0.1, 6, 'best')
    with pytest.raises(ValueError, match='color'):
        M.project_colors(v, None, d, c[:, :, :, :2], m, 8, 8, 7.5, 5.5, 0.1, 0, 'best')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        M.project_colors(v.cpu(), None, d, c, m, 8, 8, 7.5, 5.5, 0.1, 0, 'best')


# ---- the Mesher ----------------------------------------------------------------------------------------------------------
def mesher_setup(**meshing):
    import test_gpu_mesher as TM
    from attentive_dfprior_amd.mesher import Mesher
    sc, sd, dec, cfg, slam, kfs, est, c = TM.setup(resolution=32)
    v, u = np.meshgrid(np.arange(sc.H), np.arange(sc.W), indexing='ij')
    for k, kf in enumerate(kfs):                                 # smooth images, one per keyframe (the set-up's are black)
        kf['color'] = torch.from_numpy(np.stack([0.5 + 0.4 * np.sin(0.11 * u + k), 0.5 + 0.4 * np.cos(0.13 * v - k),
                                                 np.full(u.shape, 0.2 + 0.3 * k)], -1).astype(np.float32))
    direct = Mesher(cfg, None, slam)
    cfg_p = dict(cfg, meshing=dict(cfg['meshing'], color_mesh_extraction_method='keyframe_projection', **meshing))
    return sc, dec, c, kfs, est, direct, Mesher(cfg_p, None, slam)


def marching_cubes_of(m, sc, dec, c, kfs):
    xyz = m.get_grid_uniform(m.resolution)['xyz']
    z, ax = m.lattice(c, dec, sc.tsdf_volume.to(DEV), xyz, DEV)
    M.hull_fill(z, ax, m.bound_planes(kfs, m.scale, DEV), 100.)
    spacing, origin = m.marching_cubes_geometry(xyz)
    verts, faces, _ = M.marching_cubes(z, level=m.level_set, spacing=spacing, origin=origin, outward='lower')
    assert faces.shape[0] > 0
    return verts, faces


@pytest.mark.parametrize('blend', R.BLENDS)
def test_mesher_keyframe_projection(blend):
    """Without clean-up or simplification the vertices the Mesher colours are marching cubes' own: covered vertices carry the
    bytes of the statement's colour, the others the direct point query's, through the same merge of coincident vertices."""
    from attentive_dfprior_amd.mesher import merge_coincident
    tol = 0.3
    sc, dec, c, kfs, est, direct, proj = mesher_setup(projection_depth_tol=tol, projection_blend=blend, projection_border=1)
    assert (proj.projection_depth_tol, proj.projection_blend, proj.projection_border) == (tol, blend, 1)
    assert (direct.projection_depth_tol, direct.projection_blend, direct.projection_border) == (0.05, 'weighted', 0)      # the defaults
    verts, faces = marching_cubes_of(direct, sc, dec, c, kfs)
    tsdf = sc.tsdf_volume.to(DEV)
    vd, fd, cd = direct.mesh_arrays(verts, faces, c, dec, kfs, est, 2, tsdf, DEV, clean_mesh=False)
    vp, fp, cp = proj.mesh_arrays(verts, faces, c, dec, kfs, est, 2, tsdf, DEV, clean_mesh=False)
    assert np.array_equal(vd, vp) and np.array_equal(fd, fp) and cp.dtype == np.uint8 and cp.shape == cd.shape

    normals = M.vertex_normals(verts, faces).to(torch.float32).cpu().numpy()
    w2c, center = R.invert_poses(torch.stack([kf['est_c2w'] for kf in kfs]).numpy())
    args = (verts.cpu().numpy(), normals, w2c, center, torch.stack([kf['depth'] for kf in kfs]).numpy(),
            torch.stack([kf['color'] for kf in kfs]).numpy(), sc.fx, sc.fy, sc.cx, sc.cy, tol, 1, blend)
    rgb, _, count, _ = R.project_colors_ref(*args)
    amb = R.ambiguity_mask(*args)
    assert amb.mean() <= 0.005
    scaled = np.clip(rgb, np.float32(0), np.float32(1)) * np.float32(255)
    # the statement's vertices through the host merge, with what each one must carry
    carried = np.concatenate([scaled, (count > 0)[:, None], amb[:, None]], 1)                # float32 [V,5]: what survives a merge
    _, _, carried = merge_coincident(verts.cpu().numpy(), faces.cpu().numpy(), carried)
    exact, covered, amb_m = carried[:, :3], carried[:, 3] > 0, carried[:, 4] > 0
    want = exact.astype(np.uint8)
    assert len(carried) == len(vp)
    print(f'{blend}: {len(vp)} vertices, {covered.mean():.3f} covered, {amb_m.sum()} ambiguous')
    assert 0.02 < covered.mean() < 0.98
    sure = covered & ~amb_m
    step = np.abs(cp[sure].astype(int) - want[sure].astype(int))
    near_integer = np.abs(exact[sure] - np.rint(exact[sure])) <= REL * 255
    assert (step <= near_integer).all(), int((step > near_integer).sum())
    plain = ~covered & ~amb_m
    assert np.array_equal(cp[plain], cd[plain])
    assert not np.array_equal(cp[sure], cd[sure])


def test_mesher_store_and_dict_agree_and_the_file_is_written(tmp_path):
    sc, dec, c, kfs, est, direct, proj = mesher_setup(projection_depth_tol=0.3)
    verts, faces = marching_cubes_of(direct, sc, dec, c, kfs)
    tsdf = sc.tsdf_volume.to(DEV)
    store = KeyframeStore.from_keyframe_dict(kfs, sc.H, sc.W, DEV)
    a = proj.mesh_arrays(verts, faces, c, dec, kfs, est, 2, tsdf, DEV, clean_mesh=True)
    b = proj.mesh_arrays(verts, faces, c, dec, kfs, est, 2, tsdf, DEV, clean_mesh=True, keyframe_store=store)
    assert len(a[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    d = direct.mesh_arrays(verts, faces, c, dec, kfs, est, 2, tsdf, DEV, clean_mesh=True)
    assert np.array_equal(a[0], d[0]) and np.array_equal(a[1], d[1]) and not np.array_equal(a[2], d[2])
    out = tmp_path / 'projected.ply'
    assert proj.get_mesh(str(out), c, dec, kfs, est, 2, tsdf, DEV, keyframe_store=store) is not None
    m = M.read_ply(str(out))
    assert np.array_equal(m.colors, a[2]) and np.array_equal(m.faces, a[1])
    proj.color_mesh_extraction_method = 'render_ray'              # a value of the key that nobody offers is still refused
    with pytest.raises(NotImplementedError, match='render_ray'):
        proj.get_mesh(str(out), c, dec, kfs, est, 2, tsdf, DEV)


# ---- the command line ----------------------------------------------------------------------------------------------------
N_FRAMES = 12


@pytest.fixture(scope='module')
def finished_run(tmp_path_factory):
    """A 12-frame run of tests/test_gpu_slam_run.py's kind (its box room, files, prior and config) with the true poses and
    keyframe_projection as the Mesher's colour method; returns (config path, output directory, slam)."""
    from types import SimpleNamespace
    from PIL import Image
    import test_gpu_slam_run as SR
    from attentive_dfprior_amd import datasets, run, synthetic
    base = tmp_path_factory.mktemp('color_mesh')
    root = str(base / 'box')
    os.makedirs(os.path.join(root, 'results'))
    lines = []
    for k in range(N_FRAMES):
        c2w = SR.pose_cv(k)
        depth, color = SR.frame_images(c2w)
        Image.fromarray(color).save(os.path.join(root, 'results', f'frame{k:06d}.jpg'), quality=95)
        Image.fromarray(np.clip(np.rint(depth * SR.PNG), 0, 65535).astype(np.uint16)).save(os.path.join(root, 'results', f'depth{k:06d}.png'))
        lines.append(' '.join(repr(float(x)) for x in c2w.reshape(-1)))
    with open(os.path.join(root, 'traj.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    cfg = SR.full_cfg(base, SR.scene_cfg(root, str(base / 'unused')), 'world')[0]
    ds = datasets.get_dataset(cfg, SimpleNamespace(input_folder=None), 1, device=DEV)
    colors, depths, _ = ds.frames(range(N_FRAMES))
    bound = synthetic.scene_bound(SR.BOUND, 0.32, 1).numpy()
    tsdf, bnds = SR.prior_of(bound, [(colors[k], depths[k], ds.pose(k)) for k in range(N_FRAMES)]).get_render_volume()
    vol_path, bnds_path = str(base / 'box_tsdf_volume.pt'), str(base / 'box_bounds.pt')
    torch.save(tsdf.cpu(), vol_path)
    torch.save(bnds.numpy(), bnds_path)
    out = str(base / 'run')
    over = dict(tracking={'gt_camera': True, 'iters': 0}, mapping={'mesh_freq': 100, 'color_refine': False},
                meshing={'eval_rec': False, 'color_mesh_extraction_method': 'keyframe_projection'})
    _, path = SR.full_cfg(base, SR.scene_cfg(root, out, **over), 'run')
    slam = run.main([path, '--default_config', SR.DEFAULT, '--seed', '0', '--tsdf_volume', vol_path, '--tsdf_bounds', bnds_path])
    torch.cuda.synchronize()
    return path, out, slam


def room_mesh(n=16):
    """The box room's six walls as a mesh: n x n vertices per wall of [0, 3]^3."""
    t = np.linspace(0.0, 3.0, n)
    a, b = (g.reshape(-1) for g in np.meshgrid(t, t, indexing='ij'))
    i, j = (g.reshape(-1) for g in np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing='ij'))
    quad = np.stack([i * n + j, (i + 1) * n + j, i * n + j + 1, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1], 1).reshape(-1, 3)
    verts, faces = [], []
    for axis in range(3):
        for side in (0.0, 3.0):
            p = np.empty((a.size, 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side, a, b
            faces.append(quad + len(verts) * n * n)
            verts.append(p)
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces).astype(np.int32)


def test_color_mesh_command_line(finished_run, tmp_path, capsys):
    import test_gpu_slam_run as SR
    path, out, slam = finished_run
    assert slam.mapper.keyframe_list == [0, 4, 8, 10]
    assert sorted(os.listdir(os.path.join(out, 'ckpts')))[-1] == '00011.tar'
    final = os.path.join(out, 'mesh', 'final_mesh.ply')
    if os.path.exists(final):                                     # the run's own mesh went through keyframe_projection
        assert M.read_ply(final).colors is not None
    verts, faces = room_mesh()
    old = np.tile(np.array([[10, 20, 30]], np.uint8), (len(verts), 1))
    with_colors, without = str(tmp_path / 'room.ply'), str(tmp_path / 'bare.ply')
    M.write_ply(with_colors, verts, faces, colors=old)
    M.write_ply(without, verts, faces)

    kfd = torch.load(os.path.join(out, 'ckpts', '00011.tar'), map_location='cpu', weights_only=False)['keyframe_dict']
    assert [kf['idx'] for kf in kfd] == [0, 4, 8, 10]
    v, f = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    depth, color, poses = (torch.stack([kf[k].cpu().float() for kf in kfd]) for k in ('depth', 'color', 'est_c2w'))
    for blend, border, tol, src, fallback in (('weighted', 0, None, with_colors, old), ('best', 2, 0.1, without, np.full_like(old, 128))):
        dst = str(tmp_path / f'out_{blend}.ply')
        argv = [path, '--default_config', SR.DEFAULT, '--input_mesh', src, '--output_mesh', dst, '--blend', blend, '--border', str(border)]
        argv += ['--depth_tol', str(tol)] if tol is not None else []
        covered, V = color_mesh.main(argv)
        printed = capsys.readouterr().out
        assert V == len(verts) and f'{covered} of {V} vertices' in printed and '% covered' in printed
        m = M.read_ply(dst)
        assert np.array_equal(m.verts.astype(np.float32), verts) and np.array_equal(m.faces, faces)
        rgb, _, count, _ = M.project_colors(v, M.vertex_normals(v, f), depth.to(DEV), color.to(DEV), poses, SR.FX, SR.FY, SR.CX, SR.CY,
                                            0.05 if tol is None else tol, border, blend)
        seen = (count > 0).cpu().numpy()
        assert covered == seen.sum() and 0.03 * V < covered < V
        assert np.array_equal(m.colors[seen], M.color_bytes(rgb).cpu().numpy()[seen])
        assert np.array_equal(m.colors[~seen], fallback[~seen])
    # the default output name, the newest checkpoint by default (it is the one used above)
    covered, V = color_mesh.main([path, '--default_config', SR.DEFAULT, '--input_mesh', with_colors])
    assert os.path.exists(str(tmp_path / 'room_projected.ply')) and '00011.tar' in capsys.readouterr().out


def test_no_vertices_and_no_keyframes():
    d = torch.ones((2, 8, 8), dtype=torch.float32, device=DEV)
    c = torch.ones((2, 8, 8, 3), dtype=torch.float32, device=DEV)
    m = torch.eye(4)[None].repeat(2, 1, 1)
    v = torch.tensor([[0.0, 0.0, 1.0], [0.1, 0.0, 1.0]], device=DEV)
    rgb, wsum, count, best = M.project_colors(v[:0], None, d, c, m, 8, 8, 3.5, 3.5, 0.1)
    assert rgb.shape == (0, 3) and wsum.shape == (0,) and count.shape == (0,) and best.shape == (0,)
    assert (rgb.dtype, wsum.dtype, count.dtype, best.dtype) == (torch.float32, torch.float32, torch.int32, torch.int32)
    rgb, wsum, count, best = M.project_colors(v, None, d[:0], c[:0], m[:0], 8, 8, 3.5, 3.5, 0.1)
    assert rgb.shape == (2, 3) and (rgb == 0).all() and (wsum == 0).all() and (count == 0).all() and (best == -1).all()
