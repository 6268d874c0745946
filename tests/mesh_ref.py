"""CPU oracle of the marching cubes of include/adfp.h (numpy, float32 arithmetic in the kernels' order).

The case table is rebuilt here from the ambiguity rule alone, in a formulation of its own (runs of inside corners walked
counter-clockwise around each face), so that it checks the table tools/gen_mc_table.py wrote into the header rather than
copying it.  Conventions: corner c = (c & 1, c >> 1 & 1, c >> 2 & 1); edge e = 4 * axis + the other two corner bits (lower axis
first); inside iff v > level; vertices in ascending edge key 3 p + axis; triangles by cell index, then table order;
winding 'lower' = normals toward lower values.
"""
import numpy as np


def _edge(c0, c1):
    a = (c0 ^ c1).bit_length() - 1
    lo = min(c0, c1)
    others = [b for b in range(3) if b != a]
    return 4 * a + ((lo >> others[0]) & 1) + 2 * ((lo >> others[1]) & 1)


def _faces_ccw():
    """Each face's corners in counter-clockwise order seen from outside (u x v = outward normal)."""
    out = []
    for axis in range(3):
        for side in (0, 1):
            u, v = (axis + 1) % 3, (axis + 2) % 3                # e_u x e_v = +e_axis
            if side == 0:
                u, v = v, u                                      # outward normal -e_axis
            base = side << axis
            out.append([base, base | 1 << u, base | 1 << u | 1 << v, base | 1 << v])
    return out


def _case(case):
    inside = [bool(case >> c & 1) for c in range(8)]
    succ = {}
    for cyc in _faces_ccw():
        ins = [inside[c] for c in cyc]
        if all(ins) or not any(ins):
            continue
        # every maximal run of inside corners (CCW) enters through edge (prev, first) and leaves through (last, next); on a face
        # with diagonal inside corners each run is a single corner: the inside corners are separated
        for k in range(4):
            if ins[k] and not ins[k - 1]:
                m = k
                while ins[(m + 1) % 4]:
                    m = (m + 1) % 4
                enter = _edge(cyc[k - 1], cyc[k])
                leave = _edge(cyc[m], cyc[(m + 1) % 4])
                succ[enter] = leave
    tris, seen = [], set()
    loops = []
    for e0 in sorted(succ):
        if e0 in seen:
            continue
        loop = [e0]
        while succ[loop[-1]] != e0:
            loop.append(succ[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    for loop in loops:                                           # found in order of their lowest edge, starting there
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


TABLE = [_case(c) for c in range(256)]
MAX_TRI = max(len(t) for t in TABLE)


def _edge_offsets():
    """edge id -> (axis, dx, dy, dz) of its lower corner"""
    out = []
    for e in range(12):
        a, r = divmod(e, 4)
        o = [b for b in range(3) if b != a]
        d = [0, 0, 0]
        d[o[0]], d[o[1]] = r & 1, r >> 1 & 1
        out.append((a, d[0], d[1], d[2]))
    return out


EDGES = _edge_offsets()


def _grad(v, sp):
    g = []
    for a in range(3):
        n = v.shape[a]
        if n < 2:
            g.append(np.zeros_like(v))
            continue
        sl = lambda s: tuple(s if b == a else slice(None) for b in range(3))     # noqa: E731
        d = np.empty_like(v)
        d[sl(slice(1, -1))] = (v[sl(slice(2, None))] - v[sl(slice(None, -2))]) / (np.float32(2) * sp[a])
        d[sl(slice(0, 1))] = (v[sl(slice(1, 2))] - v[sl(slice(0, 1))]) / (np.float32(1) * sp[a])
        d[sl(slice(-1, None))] = (v[sl(slice(-1, None))] - v[sl(slice(-2, -1))]) / (np.float32(1) * sp[a])
        g.append(d)
    return g


def marching_cubes(values, level=0., spacing=(1, 1, 1), origin=(0, 0, 0), normals=False, outward='lower'):
    """numpy: (verts f32 [V,3], faces int32 [F,3], normals f32 [V,3] or None), same conventions and order as the kernel."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    X, Y, Z = v.shape
    lev = np.float32(level)
    sp = np.asarray(spacing, dtype=np.float32)
    org = np.asarray(origin, dtype=np.float32)
    fin = np.isfinite(v)
    ins = v > lev
    lin = np.arange(v.size, dtype=np.int64).reshape(v.shape)
    keys, pos, nrm = [], [], []
    grads = _grad(v, sp) if normals else None
    for a in range(3):
        n = v.shape[a]
        if n < 2:
            continue
        lo = tuple(slice(0, n - 1) if b == a else slice(None) for b in range(3))
        hi = tuple(slice(1, n) if b == a else slice(None) for b in range(3))
        m = fin[lo] & fin[hi] & (ins[lo] != ins[hi])
        p = lin[lo][m]
        keys.append(3 * p + a)
        v0, v1 = v[lo][m], v[hi][m]
        t = (lev - v0) / (v1 - v0)
        ijk = np.stack(np.unravel_index(p, v.shape), 1).astype(np.float32)
        ijk[:, a] = ijk[:, a] + t
        pos.append(org + ijk * sp)
        if normals:
            g0 = np.stack([grads[b][lo][m] for b in range(3)], 1)
            g1 = np.stack([grads[b][hi][m] for b in range(3)], 1)
            nv = g0 + t[:, None] * (g1 - g0)
            nn = nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2]
            inv = np.where(nn > 0, np.float32(1) / np.sqrt(np.maximum(nn, np.float32(1e-38))), np.float32(0)).astype(np.float32)
            sgn = np.float32(1 if outward == 'higher' else -1)
            nrm.append(sgn * (nv * inv[:, None]))
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    order = np.argsort(keys, kind='stable')
    keys = keys[order]
    verts = (np.concatenate(pos) if pos else np.zeros((0, 3), np.float32))[order].astype(np.float32)
    nrms = ((np.concatenate(nrm) if nrm else np.zeros((0, 3), np.float32))[order].astype(np.float32)) if normals else None

    if min(X, Y, Z) < 2:
        return verts, np.zeros((0, 3), np.int32), nrms
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    ok = np.ones((X - 1, Y - 1, Z - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, c >> 1 & 1, c >> 2 & 1
        sl = (slice(dx, X - 1 + dx), slice(dy, Y - 1 + dy), slice(dz, Z - 1 + dz))
        case |= ins[sl].astype(np.int64) << c
        ok &= fin[sl]
    cells = lin[:-1, :-1, :-1][ok]
    cases = case[ok]
    cnt = np.array([len(t) for t in TABLE])[cases]
    cell_of = np.repeat(cells, cnt)
    case_of = np.repeat(cases, cnt)
    slot = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    tab = np.full((256, MAX_TRI, 3), -1, np.int64)
    for c, tris in enumerate(TABLE):
        for m, t in enumerate(tris):
            tab[c, m] = t
    edges = tab[case_of, slot]                                                    # [F,3] local edge ids
    eo = np.array(EDGES, np.int64)
    owner = cell_of[:, None] + eo[edges, 1] * (Y * Z) + eo[edges, 2] * Z + eo[edges, 3]
    ekeys = 3 * owner + eo[edges, 0]
    idx = np.searchsorted(keys, ekeys)
    assert (keys[np.minimum(idx, len(keys) - 1)] == ekeys).all()
    faces = idx.astype(np.int32)
    if outward == 'higher':
        faces = faces[:, [0, 2, 1]]
    return verts, np.ascontiguousarray(faces), nrms


# ---- mesh properties -------------------------------------------------------------------------------------------------------
def edge_use(faces):
    """(undirected edge -> count, directed edge -> count)"""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, 1)
    _, uc = np.unique(und, axis=0, return_counts=True)
    _, dc = np.unique(d, axis=0, return_counts=True)
    return uc, dc


def is_watertight_oriented(faces):
    uc, dc = edge_use(faces)
    return bool((uc == 2).all() and (dc == 1).all())


def is_closed_oriented(faces):
    """Every undirected edge is used by an even number of faces, half of them in each direction: a closed, consistently
    oriented surface that may touch itself along an edge.  That happens where an ambiguous face's four crossings are joined by
    the fan diagonals of BOTH cells sharing the face (the fan starts at each loop's lowest edge id): the two cells' triangles
    meet along the diagonal -- a non-manifold edge, never a crack."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = d[:, 0] < d[:, 1]
    und = np.sort(d, 1)
    u, inv = np.unique(und, axis=0, return_inverse=True)
    n_fwd = np.bincount(inv.reshape(-1), weights=fwd, minlength=len(u))
    n_all = np.bincount(inv.reshape(-1), minlength=len(u))
    return bool((n_all % 2 == 0).all() and (2 * n_fwd == n_all).all())


def euler(verts, faces):
    f = np.asarray(faces, np.int64)
    used = np.unique(f)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    ne = len(np.unique(d, axis=0))
    return len(used) - ne + len(f)


def face_normals(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def area(verts, faces):
    return 0.5 * np.linalg.norm(face_normals(verts, faces), axis=1).sum()


def volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return np.einsum('ij,ij->i', v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0


def read_ply(path):
    """Small PLY reader (ascii / binary_little_endian, float / uchar vertex properties, uchar-int face lists)."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    head = data[:end].decode('ascii').splitlines()
    fmt = head[1].split()[1]
    props, nv, nf, cur = [], 0, 0, None
    for line in head:
        w = line.split()
        if w[0] == 'element':
            cur = w[1]
            if cur == 'vertex':
                nv = int(w[2])
            else:
                nf = int(w[2])
        elif w[0] == 'property' and cur == 'vertex':
            props.append((w[2], {'float': '<f4', 'uchar': 'u1'}[w[1]]))
    body = data[end:]
    if fmt == 'ascii':
        lines = body.decode('ascii').split('\n')
        rec = np.zeros(nv, dtype=props)
        for i in range(nv):
            vals = lines[i].split()
            rec[i] = tuple(float(x) if t == '<f4' else int(x) for x, (_, t) in zip(vals, props))
        faces = np.array([[int(x) for x in lines[nv + i].split()[1:]] for i in range(nf)], np.int32).reshape(-1, 3)
    else:
        rec = np.frombuffer(body, dtype=props, count=nv)
        fr = np.frombuffer(body, dtype=[('n', 'u1'), ('i', '<i4', (3,))], count=nf, offset=rec.nbytes)
        assert (fr['n'] == 3).all()
        faces = fr['i'].copy()
    return rec, faces
