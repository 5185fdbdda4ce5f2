"""CPU-side checks of the resampler (MATLAB's resample(x, p, q), N = 10, bta = 5): the NumPy restatement of resample.m that the
GPU tests compare against, checked against scipy.signal.resample_poly and against a property that needs
neither; the exported entry points; the argument checks that come before the library is called."""
import ctypes as C
import math

import numpy as np
import pytest

NEW = ["emagls_resample_length", "emagls_resample", "emagls_resample_device", "emagls_binaural_decode_render_fs",
       "emagls_binaural_decode_render_fs_device"]
RATIOS = [(147, 160), (160, 147), (1, 6), (3, 1), (441, 320), (2, 3)]


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def reduce(p, q):
    g = math.gcd(p, q)
    return p // g, q // g


def design(p, q):
    """(h, h0.sum()): h = p h0 / sum(h0), h0 the Kaiser-windowed (bta 5) sinc of L = 2 * 10 * max(p, q) + 1 taps, fc = 1/(2m)."""
    m = max(p, q)
    fc, L = 1.0 / (2 * m), 2 * 10 * m + 1
    n = np.arange(L)
    h0 = 2 * fc * np.sinc(2 * fc * (n - (L - 1) / 2)) * np.kaiser(L, 5.0)
    return p * h0 / h0.sum(), h0.sum()


def upfirdn(x, h, p, q):
    """Upsample by p, filter by h, keep every q-th sample: length ceil(((len(x) - 1) p + len(h)) / q)."""
    u = np.zeros((len(x) - 1) * p + 1, dtype=x.dtype)
    u[::p] = x
    return np.convolve(u, h)[::q]


def matlab_resample(x, p, q):
    """resample.m restated, per column; 1-D input is one column."""
    p, q = reduce(p, q)
    x = np.asarray(x)
    if p == 1 and q == 1:
        return x.copy()
    h, _ = design(p, q)
    half = (len(h) - 1) // 2
    nz = q - half % q
    h = np.concatenate([np.zeros(nz), h])
    half += nz
    delay = half // q
    cols = x.reshape(x.shape[0], -1)
    Lx = cols.shape[0]
    Ly = -(-Lx * p // q)
    nz1 = 0
    while -(-((Lx - 1) * p + len(h) + nz1) // q) - delay < Ly:
        nz1 += 1
    h = np.concatenate([h, np.zeros(nz1)])
    y = np.column_stack([upfirdn(cols[:, c], h, p, q)[delay:delay + Ly] for c in range(cols.shape[1])])
    return y.reshape(Ly) if x.ndim == 1 else y


def polyphase_resample(x, p, q):
    """The same values by the polyphase sum y[k] = sum_r h[ph + p r] x[t0 - r] (the kernel's form), fast enough for long inputs."""
    p, q = reduce(p, q)
    x = np.asarray(x)
    if p == 1 and q == 1:
        return x.copy()
    h, _ = design(p, q)
    half = (len(h) - 1) // 2
    nz = q - half % q
    h = np.concatenate([np.zeros(nz), h])
    delay = (half + nz) // q
    R = -(-len(h) // p)
    h = np.concatenate([h, np.zeros(R * p - len(h))])
    cols = x.reshape(x.shape[0], -1)
    Lx = cols.shape[0]
    Ly = -(-Lx * p // q)
    nq = (np.arange(Ly, dtype=np.int64) + delay) * q
    t0, ph = nq // p, nq % p
    y = np.zeros((Ly, cols.shape[1]), dtype=np.result_type(cols.dtype, np.float64))
    for r in range(R):
        t = t0 - r
        ok = (t >= 0) & (t < Lx)
        y[ok] += h[ph[ok] + p * r][:, None] * cols[t[ok]]
    return y.reshape(Ly) if x.ndim == 1 else y


def test_restatement_matches_scipy():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(1)
    for p, q in RATIOS:
        for n in (1, 2, 7, 100, 1000):
            x = rng.standard_normal(n)
            want = sig.resample_poly(x, p, q, window=("kaiser", 5.0))
            got = matlab_resample(x, p, q)
            assert got.shape == want.shape == (-(-n * p // q),)
            assert np.abs(got - want).max() <= 1e-14 * max(np.abs(want).max(), 1e-300), (p, q, n)


def test_q1_property():
    """q = 1: the filter's centre tap lands on the input samples and its other taps of that phase on zeros of the sinc, so
    y[p t] = x[t] / sum(h0)."""
    rng = np.random.default_rng(2)
    for p in (2, 3, 5):
        x = rng.standard_normal(300)
        y = matlab_resample(x, p, 1)
        _, s0 = design(p, 1)
        assert np.abs(y[::p] - x / s0).max() <= 1e-14 * np.abs(x).max(), p


def test_polyphase_form_equals_restatement():
    rng = np.random.default_rng(3)
    for p, q in RATIOS + [(1, 2), (2, 1), (80, 441)]:
        for n in (1, 2, 5, 333):
            x = rng.standard_normal((n, 2)) + 1j * rng.standard_normal((n, 2))
            want = matlab_resample(x, p, q)
            assert np.abs(polyphase_resample(x, p, q) - want).max() <= 1e-14 * max(np.abs(want).max(), 1e-300), (p, q, n)


# ---------------------------------------------------------------------------------------------------------------------------
# the library boundary
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from emagls_amd import build, _lib
    build.build(jobs=4, verbose=False)
    return _lib.load()


def test_new_symbols_are_exported(lib):
    from emagls_amd import _lib as L
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS


def test_resample_length(lib):
    for n in (0, 1, 2, 17, 1000, 4_800_000):
        for p, q in [(44100, 48000), (48000, 44100), (147, 160), (1, 6), (6, 2), (3, 1), (5, 5), (1, 65537)]:
            gp, gq = reduce(p, q)
            assert lib.emagls_resample_length(n, p, q) == -(-n * gp // gq) == math.ceil(n * p / q), (n, p, q)
    assert lib.emagls_resample_length(-1, 2, 3) == -1
    assert lib.emagls_resample_length(10, 0, 3) == -1
    assert lib.emagls_resample_length(10, 3, -1) == -1


def test_entry_point_argument_errors(lib):
    """Checked before any device work."""
    from emagls_amd import _lib as L
    x, y = np.zeros(8), np.zeros(64)
    px, py = x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)
    assert lib.emagls_resample(px, 0, 8, 1, 0, 3, py) == L.ERR_ARG
    assert lib.emagls_resample(px, 0, 8, 1, 3, -2, py) == L.ERR_ARG
    assert lib.emagls_resample(px, 0, -1, 1, 2, 3, py) == L.ERR_ARG
    assert lib.emagls_resample(None, 0, 8, 1, 2, 3, py) == L.ERR_ARG
    assert lib.emagls_resample(px, 0, 8, 1, 65537, 1, py) == L.ERR_UNSUPPORTED
    assert lib.emagls_resample(px, 0, 8, 1, 2 * 65537, 2, py) == L.ERR_UNSUPPORTED
    w = np.zeros((16, 4))
    pw = w.ctypes.data_as(C.c_void_p)
    for fs in [(48000.0, 44100.5, 48000.0), (48000.0, 0.0, 48000.0), (-48000.0, 44100.0, 48000.0), (48000.0, float("nan"), 48000.0)]:
        assert lib.emagls_binaural_decode_render_fs(px, 0, 2, 4, pw, pw, 0, 16, 0, 0, 0, None, 0, None, 0, None, 0, None, 0, *fs, py,
                                                    None) == L.ERR_ARG, fs
    assert lib.emagls_binaural_decode_render_fs(px, 0, 2, 4, pw, pw, 0, 16, 0, 0, 0, None, 0, None, 0, None, 0, None, 0,
                                                 100000.0, 65537.0, 100000.0, py, None) == L.ERR_UNSUPPORTED


@pytest.fixture
def no_library(monkeypatch):
    """Any call into the library fails the test: the argument checks must come first."""
    from emagls_amd import _lib as L

    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(L, "load", boom)


def test_python_rejects_bad_rates(no_library):
    import emagls_amd as E
    x = np.zeros(10)
    for p, q in [(44100.5, 48000), (0, 3), (3, 0), (-2, 3), (2, -3), (float("nan"), 2), (float("inf"), 2), ("a", 2)]:
        with pytest.raises(ValueError, match="positive integer"):
            E.resample(x, p, q)
    with pytest.raises(ValueError, match="vector or a"):
        E.resample(np.zeros((2, 2, 2)), 2, 3)
    s, w = np.zeros((10, 4)), np.zeros((8, 4))
    with pytest.raises(ValueError, match="positive integer"):
        E.binauralDecode(s, 48000, w, w, 44100.5, allowResampling=True)
    with pytest.raises(ValueError, match="positive integer"):
        E.binauralDecode(s, 48000, w, w, 48000, signal=np.ones(5), signalFs=-44100, allowResampling=True)
    with pytest.raises(ValueError, match="positive integer"):
        E.binauralDecode(s, 48000.5, w, w, 44100, allowResampling=True)
    # the default call keeps refusing, and says how to opt in
    with pytest.raises(NotImplementedError, match="allowResampling"):
        E.binauralDecode(s, 48000, w, w, 44100)
