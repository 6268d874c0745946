"""The numpy f64 statement of include/adfp.h's "mesh simplification" (vertex clustering), which the device kernels are tested
against: np.unique on the cell keys, np.bincount / np.add.at in input order, np.linalg.eigh.  No GPU, no package import."""
import itertools

import numpy as np

TAU = 1e-3
CONTRACTIONS = ('average', 'quadric')


def clusters(verts, voxel_size):
    """(p f64 [V,3], cluster of every vertex, number of clusters): adfp_voxel_down_sample's cells, ascending key order."""
    p = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    vmin = p.min(0) - voxel_size * 0.5
    N = np.floor((p.max(0) - vmin) / voxel_size).astype(np.int64) + 1
    i = np.floor((p - vmin) / voxel_size).astype(np.int64)
    key = (i[:, 0] * N[1] + i[:, 1]) * N[2] + i[:, 2]
    uk, cl = np.unique(key, return_inverse=True)
    return p, cl.reshape(-1), len(uk)


def quadrics(p, faces, cl, K, voxel_size):
    """Per cluster: the average m, the counts, A, b (relative to m, summed in (face, corner) order), eigh's (lam, E), the truncated
    solve x, and ok = the placement guard passes."""
    n_in = np.bincount(cl, minlength=K)
    m = np.stack([np.bincount(cl, weights=p[:, c], minlength=K) for c in range(3)], 1) / n_in[:, None]
    p0, p1, p2 = (p[faces[:, c]] for c in range(3))
    g = np.cross(p1 - p0, p2 - p0)
    ell = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    valid = np.isfinite(ell) & (ell > 0)
    rep = np.repeat(np.arange(len(faces)), 3)                # contributions in face-major order: (face, corner)
    k = cl[faces].reshape(-1)
    rep, k = rep[valid[rep]], k[valid[rep]]
    nrm = g[rep] / ell[rep, None]
    w = ell[rep] / 2
    d = -np.einsum('ij,ij->i', nrm, p0[rep] - m[k])
    A = np.zeros((K, 3, 3))
    b = np.zeros((K, 3))
    np.add.at(A, k, w[:, None, None] * nrm[:, :, None] * nrm[:, None, :])
    np.add.at(b, k, (w * d)[:, None] * nrm)
    lam, E = np.linalg.eigh(A)
    x = solve(lam, E, b, lam > TAU * lam[:, -1:])
    ok = (lam[:, -1] > 0) & ~(np.abs(x).max(1) > voxel_size)
    return dict(m=m, n=n_in, A=A, b=b, lam=lam, E=E, x=x, ok=ok)


def solve(lam, E, b, sel):
    coef = np.where(sel, np.einsum('kji,kj->ki', E, -b) / np.where(sel, lam, 1.0), 0.0)
    return np.einsum('kji,ki->kj', E, coef)


def simplify(verts, faces, voxel_size, contraction='quadric', colors=None, detail=False):
    """(verts f32 [V',3], faces int32 [F',3], colors uint8 [V',3] or None) by the contract's rules; detail=True appends a dict
    with the per-cluster quantities and `used` (the cluster of every output vertex)."""
    assert contraction in CONTRACTIONS
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p, cl, K = clusters(verts, voxel_size)
    q = quadrics(p, faces, cl, K, voxel_size)
    pos = q['m'] + (np.where(q['ok'][:, None], q['x'], 0.0) if contraction == 'quadric' else 0.0)
    col = None
    if colors is not None:
        S = np.zeros((K, 3), np.int64)
        np.add.at(S, cl, np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.int64))
        col = ((2 * S + q['n'][:, None]) // (2 * q['n'][:, None])).astype(np.uint8)
    t = cl[faces]
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    rot = (np.argmin(t, 1)[:, None] + np.arange(3)[None, :]) % 3
    t = np.take_along_axis(t, rot, 1)
    idx = np.flatnonzero(alive)
    if len(idx):
        _, first = np.unique(t[idx], axis=0, return_index=True)          # the earliest input face of every rotated triple
        idx = idx[np.sort(first)]
    t = t[idx]
    used = np.unique(t)
    remap = np.full(K, -1, np.int64)
    remap[used] = np.arange(len(used))
    out = (pos[used].astype(np.float32), remap[t].astype(np.int32).reshape(-1, 3), col[used] if col is not None else None)
    if detail:
        q.update(used=used, cl=cl, K=K)
        return out + (q,)
    return out


def marginal(q):
    """bool [K,3]: eigenvalue i of the cluster has lam_i / lam_max within 1e-6 relative of TAU."""
    lmax = q['lam'][:, -1:]
    r = q['lam'] / np.where(lmax > 0, lmax, 1.0)
    return (lmax > 0) & (np.abs(r - TAU) <= 1e-6 * TAU)


def ambiguous(verts, faces, voxel_size):
    """bool per cluster: the placement rule can fall either way between two correct evaluations -- an eigenvalue ratio at TAU, or
    max |x_c| within 1e-9 relative of the voxel."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    p, cl, K = clusters(verts, voxel_size)
    q = quadrics(p, faces, cl, K, voxel_size)
    return marginal(q).any(1) | (np.abs(np.abs(q['x']).max(1) - voxel_size) <= 1e-9 * voxel_size)


def candidates(q, k):
    """The positions (f64 [n,3]) an ambiguous cluster k may take: m_k, and m_k + x with every choice of its marginal directions."""
    lam, E, b = q['lam'][k:k + 1], q['E'][k:k + 1], q['b'][k:k + 1]
    mg = np.flatnonzero(marginal(q)[k])
    base = lam > TAU * lam[:, -1:]
    out = [q['m'][k]]
    for bits in itertools.product((False, True), repeat=len(mg)):
        sel = base.copy()
        sel[0, mg] = bits
        out.append(q['m'][k] + solve(lam, E, b, sel)[0])
    return np.stack(out)
