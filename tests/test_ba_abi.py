"""CPU: the three bundle-adjustment entries of the C ABI (adfp_ba_head, adfp_ba_tail, adfp_cameras_from_tensors) return ADFP_E_ARG
(-1) before any launch for null pointers, a frame count outside [1, ADFP_KEYFRAMES_MAX] and a ray count below 1, as include/adfp.h
states.  No GPU: nothing is dereferenced on an argument error, so any non-null address stands in for device memory; every call here
is an error case, so nothing is ever launched (the suite also runs on machines with a GPU)."""
import ctypes as C

from attentive_dfprior_amd import _lib

P = 4096                                         # any non-null address
KM = _lib.KEYFRAMES_MAX


def head_args(F=3, n=70, **kw):
    a = _lib.AdfpBaHeadArgs()
    a.n_frames, a.n, a.H0, a.H1, a.W0, a.W1, a.H, a.W = F, n, 0, 48, 0, 64, 48, 64
    a.fx, a.fy, a.cx, a.cy = 50.0, 50.0, 31.5, 23.5
    for name in ('cam', 'c2w', 'pix_i', 'pix_j', 'rays_o', 'rays_d', 'gt_depth', 'gt_color'):
        setattr(a, name, P)
    for f in range(KM):
        j = a.frames[f]
        j.idx, j.c2w, j.depth_img, j.color_img, j.free_pose = P, P, P, P, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def tail_args(F=3, n=70, **kw):
    a = _lib.AdfpBaTailArgs()
    a.n_frames, a.n = F, n
    a.fx, a.fy, a.cx, a.cy = 50.0, 50.0, 31.5, 23.5
    for name in ('pix_i', 'pix_j', 'g_rays_o', 'g_rays_d', 'cam', 'g_c2w', 'g_cam', 'free_flags', 'exp_avg', 'exp_avg_sq', 'derived'):
        setattr(a, name, P)
    a.step, a.beta1, a.beta2, a.eps = 1, 0.9, 0.999, 1e-8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_are_bound():
    names = [n for n, _, _ in _lib.SYMBOLS]
    assert all(n in names for n in ('adfp_ba_head', 'adfp_ba_tail', 'adfp_cameras_from_tensors'))
    assert KM == 16


def test_ba_head_argument_errors():
    f = _lib.lib().adfp_ba_head
    assert f(None, None) == -1
    for bad in (dict(n_frames=0), dict(n_frames=-1), dict(n_frames=KM + 1), dict(n=0), dict(n=-5), dict(H1=0), dict(W1=65), dict(H0=-1)):
        assert f(C.byref(head_args(**bad)), None) == -1, bad
    for name in ('cam', 'c2w', 'pix_i', 'pix_j', 'rays_o', 'rays_d', 'gt_depth', 'gt_color'):
        assert f(C.byref(head_args(**{name: None})), None) == -1, name
    for field in ('idx', 'depth_img', 'color_img'):
        a = head_args()
        setattr(a.frames[2], field, None)
        assert f(C.byref(a), None) == -1, field
    a = head_args()
    a.frames[1].c2w, a.frames[1].free_pose = None, 0         # the fixed frame's stored pose is read
    assert f(C.byref(a), None) == -1


def test_ba_tail_argument_errors():
    f = _lib.lib().adfp_ba_tail
    assert f(None, None) == -1
    for bad in (dict(n_frames=0), dict(n_frames=KM + 1), dict(n=0), dict(n=-1)):
        assert f(C.byref(tail_args(**bad)), None) == -1, bad
    for name in ('pix_i', 'pix_j', 'g_rays_o', 'g_rays_d', 'cam', 'g_c2w', 'g_cam', 'free_flags'):
        assert f(C.byref(tail_args(**{name: None})), None) == -1, name
    for name in ('exp_avg', 'exp_avg_sq', 'derived'):
        assert f(C.byref(tail_args(**{name: None})), None) == -1, name              # needed by the step


def test_cameras_from_tensors_argument_errors():
    f = _lib.lib().adfp_cameras_from_tensors
    dst = (C.c_void_p * KM)(*([P] * KM))
    assert f(0, P, dst, None) == -1 and f(-2, P, dst, None) == -1 and f(KM + 1, P, dst, None) == -1
    assert f(3, None, dst, None) == -1 and f(3, P, None, None) == -1
