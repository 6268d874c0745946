"""GPU, end to end: python -m attentive_dfprior_amd.render_mesh on a small coloured room written with write_ply, a two-pose
trajectory and a 32 x 24 camera, once per mode, each in a fresh child process.  The PNGs are MeshViews.render's bytes for the same
inputs and the depth files are render_depth's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import depth_ref as D
import shade_cases as SC
import soup_meshes as S
from conftest import ROOT
from attentive_dfprior_amd import mesh, raycast, render_mesh

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CAM = dict(H=24, W=32, fx=20.0, fy=20.0, cx=15.5, cy=11.5)


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    d = tmp_path_factory.mktemp('render_mesh')
    verts, faces = D.box_room(inner=((-0.6, -0.4, -1.2), (0.3, 0.5, 0.2)))
    ply = str(d / 'room.ply')
    mesh.write_ply(ply, verts, faces, SC.colors_of(len(verts), 11))
    poses = [SC.cases()[2].c2w, SC.rolled(S.look((-1.0, -0.5, -0.2), (1.2, 0.9, -0.3)), -0.4)]
    traj = str(d / 'traj.txt')
    with open(traj, 'w') as f:
        for p in poses:
            f.write(' '.join(repr(float(x)) for x in np.asarray(p).reshape(-1)) + '\n')
    return d, ply, traj


@pytest.mark.parametrize('mode', ['shaded', 'color', 'normal'])
def test_command_line(scene, mode):
    d, ply, traj = scene
    out = str(d / mode)
    cmd = [sys.executable, '-m', 'attentive_dfprior_amd.render_mesh', '--input_mesh', ply, '--traj', traj, '--mode', mode, '--depth',
           '--out', out] + [a for k, v in CAM.items() for a in ('--' + k, str(v))]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    run = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert run.returncode == 0, run.stdout.decode()[-2000:]
    # the same inputs: the mesh as the file holds it (f32 vertices), the poses as the reader returns them
    m = mesh.read_ply(ply)
    from attentive_dfprior_amd.cull_mesh import load_poses
    poses = render_mesh.opencv_poses(load_poses(traj))
    assert poses.shape == (2, 4, 4)
    want = render_mesh.MeshViews(m.verts, m.faces, m.colors, DEV).render(poses, *CAM.values(), mode=mode)
    depth = raycast.MeshBVH(m.verts, m.faces, DEV).render_depth(poses, *CAM.values(), D.near_of(m.verts), 20.0)
    assert sorted(os.listdir(out)) == sorted([f'{mode}_{k:05d}.png' for k in range(2)] + [f'depth_{k:05d}.npy' for k in range(2)])
    for k in range(2):
        img = np.asarray(Image.open(os.path.join(out, f'{mode}_{k:05d}.png')))
        assert img.shape == (24, 32, 3) and img.dtype == np.uint8
        assert np.array_equal(img, want['rgb'][k].cpu().numpy()), (mode, k)
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 8                       # a picture, not a flat fill
        got = np.load(os.path.join(out, f'depth_{k:05d}.npy'))
        assert got.dtype == np.float32 and np.array_equal(got, depth[k].cpu().numpy())
        assert torch.equal(want['depth'][k], depth[k]) and (got > 0).mean() > 0.5
