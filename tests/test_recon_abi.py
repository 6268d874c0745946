"""CPU: the reconstruction-evaluation entries of the C ABI without a GPU -- argument errors come back as negative codes before
any launch, empty inputs return 0 or an error as include/adfp.h defines them, and the workspace sizes follow their formulas."""
import ctypes as C
import math

from attentive_dfprior_amd import _lib

D = C.c_void_p(16)                                  # never dereferenced: every call below fails (or returns) before any launch
BIG = 2 ** 31


def al256(b):
    return (b + 255) // 256 * 256


def test_workspace_formulas():
    L = _lib.lib()
    for n in (1, 15, 16, 17, 1000, 200000):
        leaves = -(-n // 16)
        P = 1
        while P < leaves:
            P *= 2
        assert L.adfp_nn_index_bytes(n) == al256(24 * n) + al256(4 * n) + 2 * P * 48
        sort = (-(-n // 1024) + 1) * 256 * 4
        assert L.adfp_nn_build_workspace_bytes(n) == al256(256 * 48) + 4 * al256(4 * n) + al256(sort)
        assert L.adfp_nn_query_workspace_bytes(n, 1) == L.adfp_nn_build_workspace_bytes(n)
        assert L.adfp_nn_query_workspace_bytes(n, 0) == 0
        assert L.adfp_recon_reduce_workspace_bytes(n) == 8 * 17 * min(max(-(-n // 256), 1), 1024)
        assert L.adfp_sample_surface_workspace_bytes(n) == al256(8 * n) + 8 * (2 * -(-n // 2048) + 1)
    for fn in (L.adfp_nn_index_bytes, L.adfp_nn_build_workspace_bytes, L.adfp_sample_surface_workspace_bytes):
        assert fn(0) == 0 and fn(-1) == 0 and fn(BIG) == 0
    assert L.adfp_recon_reduce_workspace_bytes(0) == 8 * 17
    assert L.adfp_nn_index_bytes(10 ** 6) < 64 * 10 ** 6


def test_nn_argument_errors():
    L = _lib.lib()
    ib, wb = L.adfp_nn_index_bytes(100), L.adfp_nn_build_workspace_bytes(100)
    assert L.adfp_nn_build(None, 100, D, ib, D, wb, None) == -1
    assert L.adfp_nn_build(D, 100, None, ib, D, wb, None) == -1
    assert L.adfp_nn_build(D, 100, D, ib, None, wb, None) == -1
    assert L.adfp_nn_build(D, -1, D, ib, D, wb, None) == -1
    assert L.adfp_nn_build(D, BIG, D, ib, D, wb, None) == -2
    assert L.adfp_nn_build(D, 100, D, ib - 1, D, wb, None) == -3
    assert L.adfp_nn_build(D, 100, D, ib, D, wb - 1, None) == -3
    assert L.adfp_nn_build(None, 0, None, 0, None, 0, None) == 0          # an empty cloud: nothing to build

    def q(index=D, ib=ib, n_ref=100, query=D, nq=50, radius=math.inf, flags=0, ws=None, wsb=0, dist=D, idx=D):
        return L.adfp_nn_query(index, ib, n_ref, query, nq, None, radius, flags, ws, wsb, dist, idx, None)
    assert q(index=None) == -1
    assert q(query=None) == -1
    assert q(dist=None) == -1
    assert q(idx=None) == -1
    assert q(n_ref=0) == -1                                 # queries against an empty index
    assert q(nq=-1) == -1
    assert q(radius=0.0) == -1
    assert q(radius=-1.0) == -1
    assert q(radius=float('nan')) == -1
    assert q(flags=2) == -1
    assert q(flags=1) == -1                                 # sorting the queries needs a workspace
    assert q(flags=1, ws=D, wsb=L.adfp_nn_query_workspace_bytes(50, 1) - 1) == -3
    assert q(ib=ib - 1) == -3
    assert q(n_ref=BIG) == -2
    assert q(nq=BIG) == -2
    assert q(index=None, query=None, dist=None, idx=None, nq=0) == 0          # no queries: nothing to do
    assert q(n_ref=0, nq=0) == 0


def test_reduction_argument_errors():
    L = _lib.lib()
    wb = L.adfp_recon_reduce_workspace_bytes(1000)
    assert L.adfp_nn_metric_sums(None, 1000, 0.05, D, wb, D, None) == -1
    assert L.adfp_nn_metric_sums(D, 1000, 0.05, None, wb, D, None) == -1
    assert L.adfp_nn_metric_sums(D, 1000, 0.05, D, wb, None, None) == -1
    assert L.adfp_nn_metric_sums(D, -1, 0.05, D, wb, D, None) == -1
    assert L.adfp_nn_metric_sums(D, BIG, 0.05, D, wb, D, None) == -2
    assert L.adfp_nn_metric_sums(D, 1000, 0.05, D, wb - 1, D, None) == -3
    t = (C.c_double * 12)()
    o = (C.c_double * 3)()

    def m(src=D, n=1000, tr=C.byref(t), org=C.byref(o), tgt=D, nt=10, idx=D, ws=D, wsb=wb, out=D):
        return L.adfp_icp_moments(src, n, tr, org, tgt, nt, idx, ws, wsb, out, None)
    assert m(src=None) == -1
    assert m(idx=None) == -1
    assert m(tgt=None) == -1
    assert m(tr=None) == -1
    assert m(org=None) == -1
    assert m(out=None) == -1
    assert m(ws=None) == -1
    assert m(n=-1) == -1
    assert m(nt=-1) == -1
    assert m(n=BIG) == -2
    assert m(wsb=wb - 1) == -3


def test_sample_and_cull_argument_errors():
    L = _lib.lib()
    wb = L.adfp_sample_surface_workspace_bytes(10)

    def s(v=D, nv=8, f=D, nf=10, uf=D, ub=D, n=100, ws=D, wsb=wb, pts=D, fi=D):
        return L.adfp_sample_surface(v, nv, f, nf, uf, ub, n, ws, wsb, pts, fi, None)
    for k in ('v', 'f', 'uf', 'ub', 'ws', 'pts', 'fi'):
        assert s(**{k: None}) == -1, k
    assert s(nf=0) == -1                                    # draws from a mesh without faces
    assert s(nv=-1) == -1 and s(nf=-1) == -1 and s(n=-1) == -1
    assert s(n=BIG) == -2 and s(nf=BIG) == -2
    assert s(wsb=wb - 1) == -3
    assert s(n=0, v=None, f=None, uf=None, ub=None, ws=None, pts=None, fi=None) == 0

    def cv(v=D, nv=100, w=D, npose=5, seen=D):
        return L.adfp_cull_vertices(v, nv, w, npose, 600.0, 600.0, 599.5, 339.5, 1200, 680, seen, None)
    assert cv(v=None) == -1 and cv(w=None) == -1 and cv(seen=None) == -1
    assert cv(nv=-1) == -1 and cv(npose=-1) == -1
    assert cv(nv=BIG) == -2
    assert cv(nv=0, v=None, seen=None) == 0

    def cf(seen=D, nv=100, f=D, nf=10, keep=D):
        return L.adfp_cull_faces(seen, nv, f, nf, keep, None)
    assert cf(seen=None) == -1 and cf(f=None) == -1 and cf(keep=None) == -1
    assert cf(nv=-1) == -1 and cf(nf=-1) == -1
    assert cf(nf=BIG) == -2
    assert cf(nf=0, f=None, keep=None) == 0
