"""CPU: adfp_depth_bilateral returns its error code before any launch, as include/adfp.h states ("Depth bilateral filter").  No GPU:
nothing is dereferenced on an argument error, so any non-null address stands in for device memory; every call here is an error case,
so nothing is ever launched (the suite also runs on machines with a GPU)."""
from attentive_dfprior_amd import _lib

P, Q = 4096, 8192                                # two different non-null addresses
NAN, INF = float('nan'), float('inf')


def test_symbol_and_version():
    entry = [(n, r, a) for n, r, a in _lib.SYMBOLS if n == 'adfp_depth_bilateral']
    assert len(entry) == 1 and len(entry[0][2]) == 10
    assert hasattr(_lib.lib(), 'adfp_depth_bilateral')
    assert _lib.lib().adfp_version() == _lib.ABI_VERSION              # additive: the version stays


def call(**kw):
    a = dict(depth=P, V=1, H=48, W=64, radius=2, sigma_space=1.5, sigma_depth=0.05, sigma_depth_z2=0.0, out=Q, stream=None)
    a.update(kw)
    return _lib.lib().adfp_depth_bilateral(a['depth'], a['V'], a['H'], a['W'], a['radius'], a['sigma_space'], a['sigma_depth'],
                                           a['sigma_depth_z2'], a['out'], a['stream'])


def test_argument_errors():
    for bad in (dict(depth=None), dict(out=None), dict(out=P), dict(V=0), dict(V=-1), dict(H=0), dict(W=0), dict(W=-3), dict(radius=0),
                dict(radius=-1), dict(sigma_space=NAN), dict(sigma_space=0.0), dict(sigma_space=-1.5), dict(sigma_depth=NAN),
                dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth_z2=NAN), dict(sigma_depth_z2=-1e-9)):
        assert call(**bad) == -1, bad


def test_unsupported_sizes():
    for bad in (dict(radius=9), dict(radius=1000), dict(H=32769), dict(W=32769), dict(V=65536)):
        assert call(**bad) == -2, bad


def test_an_argument_error_comes_before_unsupported():
    assert call(radius=9, depth=None) == -1 and call(H=32769, sigma_space=NAN) == -1 and call(V=65536, out=P) == -1
