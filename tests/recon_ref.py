"""CPU oracle of reconstruction evaluation (numpy / scipy / torch on the host), restating what the reference's
src/tools/eval_recon.py and src/tools/cull_mesh.py compute through trimesh, open3d and scipy:

  * sample_surface: trimesh.sample.sample_surface on given uniforms (numpy f64, trimesh's order of operations);
  * cull_mask: cull_mesh.py's per-pose loop in the same torch f32 ops, on the CPU;
  * icp: open3d's point-to-point registration_icp loop (cKDTree with distance_upper_bound for the correspondences, Umeyama
    without scaling on the centred correspondences);
  * metrics: cKDTree queries and np.mean, as eval_recon.py:32-50;
  * room_mesh: the synthetic test scene, a box room with a ball in it, through the numpy marching cubes of mesh_ref.
"""
import numpy as np
import torch
from scipy.spatial import cKDTree

import mesh_ref


def room_mesh(voxel=0.05):
    """(verts f64 [V,3], faces int64 [F,3]): the synthetic box room (synthetic.make_box_room_tsdf) with a ball of radius 0.45 at
    (0.6, -0.3, -0.2), meshed at the zero level."""
    from attentive_dfprior_amd import synthetic
    b = torch.tensor([[-2.0, 2.0], [-1.5, 1.5], [-1.2, 1.3]], dtype=torch.float64)
    tv, bn, _ = synthetic.make_box_room_tsdf(b, voxel=voxel, inset=0.4)
    vol = tv[0, 0].permute(2, 1, 0).contiguous().numpy()
    X, Y, Z = vol.shape
    lo = bn[:, 0].numpy()
    ax = [(lo[i] + np.arange(n) * voxel).astype(np.float32) for i, n in enumerate((X, Y, Z))]
    gx, gy, gz = np.meshgrid(*ax, indexing='ij')
    ball = (np.sqrt((gx - 0.6) ** 2 + (gy + 0.3) ** 2 + (gz + 0.2) ** 2) - 0.45) / (5 * voxel)
    vol = np.minimum(vol, np.clip(ball, -1, 1)).astype(np.float32)
    v, f, _ = mesh_ref.marching_cubes(vol, 0.0, (voxel,) * 3, tuple(float(x) for x in lo))
    return v.astype(np.float64), f.astype(np.int64)


def areas(verts, faces):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    a, b = v1 - v0, v2 - v0
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) * 0.5


def sample_surface(verts, faces, u_face, u_bary):
    """trimesh.sample.sample_surface with its random draws replaced by u_face [n], u_bary [n,2]: (points [n,3], face_index [n],
    cum [F])."""
    verts = np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64)
    cum = np.cumsum(areas(verts, faces))
    face_index = np.searchsorted(cum, np.asarray(u_face) * cum[-1])
    o = verts[faces[:, 0]][face_index]
    e1 = (verts[faces[:, 1]] - verts[faces[:, 0]])[face_index]
    e2 = (verts[faces[:, 2]] - verts[faces[:, 0]])[face_index]
    r = np.array(u_bary, dtype=np.float64).reshape(-1, 2).copy()
    fold = r.sum(1) > 1.0
    r[fold] -= 1.0
    r = np.abs(r)
    return (e1 * r[:, :1] + e2 * r[:, 1:]) + o, face_index, cum


def nn(ref, query, radius=np.inf):
    d, i = cKDTree(ref).query(query, distance_upper_bound=radius)
    return d, np.where(np.isfinite(d), i, -1)


def accuracy(gt, rec):
    return np.mean(cKDTree(gt).query(rec)[0])


def completion(gt, rec):
    return np.mean(cKDTree(rec).query(gt)[0])


def completion_ratio(gt, rec, dist_th=0.05):
    return np.mean((cKDTree(rec).query(gt)[0] < dist_th).astype(float))


def apply_transform(verts, T):
    x, y, z = verts[:, 0], verts[:, 1], verts[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def umeyama(p, q):
    """Rigid 4x4 taking p [n,3] onto q [n,3] (Eigen::umeyama, no scaling); identity for no points."""
    T = np.eye(4)
    if len(p) == 0:
        return T
    mp, mq = p.mean(0), q.mean(0)
    sigma = (q - mq).T @ (p - mp) / len(p)
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    T[:3, :3] = R
    T[:3, 3] = mq - R @ mp
    return T


def icp(src, tgt, threshold=0.1, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """open3d registration_icp (point-to-point, identity init) from the untouched source: (T, fitness, rmse, iterations)."""
    tree = cKDTree(tgt)

    def corr(T):
        d, i = tree.query(apply_transform(src, T), distance_upper_bound=threshold)
        ok = np.isfinite(d)
        n = int(ok.sum())
        p, q = apply_transform(src[ok], T), tgt[i[ok]]
        dd = q - p
        d2 = ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).sum()
        return (p, q), n / len(src), (np.sqrt(d2 / n) if n else 0.0)

    T = np.eye(4)
    res = corr(T)
    it = 0
    for it in range(1, max_iteration + 1):
        T = umeyama(*res[0]) @ T
        prev = res
        res = corr(T)
        if abs(prev[1] - res[1]) < relative_fitness and abs(prev[2] - res[2]) < relative_rmse:
            break
    return T, res[1], res[2], it


def metric_3d(rec_v, rec_f, gt_v, gt_f, u_rec, u_gt, T=None):
    """calc_3d_metric's three numbers (x100) on given uniforms ((u_face, u_bary) per mesh) and alignment."""
    rv = rec_v if T is None else apply_transform(rec_v, T)
    rp = sample_surface(rv, rec_f, *u_rec)[0]
    gp = sample_surface(gt_v, gt_f, *u_gt)[0]
    return {'accuracy': accuracy(gp, rp) * 100, 'completion': completion(gp, rp) * 100,
            'completion_ratio': completion_ratio(gp, rp) * 100}


def w2c_list(c2w_list):
    return [np.linalg.inv(c2w) for c2w in c2w_list]


def cull_mask(verts, faces, c2w_list, H=680, W=1200, fx=600.0, fy=600.0, cx=599.5, cy=339.5):
    """cull_mesh.py:48-74 on the CPU in the same torch ops: (keep [F] bool, seen [V] bool)."""
    pc = np.asarray(verts, np.float64)
    whole = np.ones(pc.shape[0]).astype(bool)
    K = torch.from_numpy(np.array([[fx, .0, cx], [.0, fy, cy], [.0, .0, 1.0]]).reshape(3, 3))
    for c2w in c2w_list:
        points = torch.from_numpy(pc.copy())
        w2c = torch.from_numpy(np.linalg.inv(c2w)).float()
        ones = torch.ones_like(points[:, 0]).reshape(-1, 1)
        homo = torch.cat([points, ones], dim=1).reshape(-1, 4, 1).float()
        cam = (w2c @ homo)[:, :3]
        cam[:, 0] *= -1
        uv = K.float() @ cam.float()
        z = uv[:, -1:] + 1e-5
        uv = (uv[:, :2] / z).float().squeeze(-1).numpy()
        mask = (0 <= -z[:, 0, 0].numpy()) & (uv[:, 0] < W) & (uv[:, 0] > 0) & (uv[:, 1] < H) & (uv[:, 1] > 0)
        whole &= ~mask
    face_mask = whole[np.asarray(faces)].all(axis=1)
    return ~face_mask, ~whole


def projections_f64(verts, c2w_list, fx=600.0, fy=600.0, cx=599.5, cy=339.5):
    """Per vertex and pose, (u, v, z) recomputed in f64: for listing vertices whose f32 test lies within rounding of a border."""
    v = np.asarray(verts, np.float64)
    out = []
    for c2w in c2w_list:
        w2c = np.linalg.inv(np.asarray(c2w, np.float64))
        cam = v @ w2c[:3, :3].T + w2c[:3, 3]
        X, Y, Z = -cam[:, 0], cam[:, 1], cam[:, 2]
        z = Z + 1e-5
        out.append((fx * X + cx * Z) / z)
        out.append((fy * Y + cy * Z) / z)
        out.append(z)
    return np.stack(out, 1).reshape(len(v), len(c2w_list), 3)


def near_border(verts, c2w_list, H=680, W=1200, rel=1e-5, **k):
    """Vertices some pose projects within `rel` (relative) of a frustum border or of z = 0."""
    p = projections_f64(verts, c2w_list, **k)
    u, v, z = p[..., 0], p[..., 1], p[..., 2]
    near = (np.abs(z) <= rel * (np.abs(z).max() + 1e-30))
    for val, lim in ((u, 0.0), (u, W), (v, 0.0), (v, H)):
        near |= np.abs(val - lim) <= rel * np.maximum(np.abs(val), 1.0) + 1e-3 * rel
    return near.any(1)
