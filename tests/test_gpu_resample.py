"""The GPU resampler (MATLAB's resample(x, p, q), N = 10, bta = 5) against the NumPy restatement of test_resample_host.py
(DESIGN.md section 7), and properties that need no restatement: the q = 1 identity and a sine resampled to another rate."""
import ctypes as C

import numpy as np
import pytest

from test_resample_host import design, matlab_resample, polyphase_resample

gpu = pytest.mark.gpu
RATIOS = [(147, 160), (160, 147), (1, 2), (2, 1), (1, 6), (3, 1), (441, 320), (80, 441), (47999, 48000)]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@gpu
@pytest.mark.parametrize("p,q", RATIOS)
def test_against_restatement(p, q):
    import emagls_amd as E
    rng = np.random.default_rng(p * 7 + q)
    L = 20 * max(p, q) + 1
    lengths = [1, 2, max(3, L // (3 * max(1, q // p))), 5000]
    for n in lengths:
        for nch in (1, 3):
            for cplx in (False, True):
                x = rng.standard_normal((n, nch)) + (1j * rng.standard_normal((n, nch)) if cplx else 0)
                # (the restatement convolves the upsampled input directly; the polyphase form, equal to it on the host, for big ones)
                want = matlab_resample(x, p, q) if n * p * L < 300_000_000 else polyphase_resample(x, p, q)
                got = E.resample(x, p, q)
                if n == 1:      # (a 1 x nch matrix is a row vector to MATLAB, resampled along its length: one column at a time)
                    got = np.column_stack([E.resample(x[:, c], p, q) for c in range(nch)])
                assert got.shape == want.shape == (-(-n * p // q), nch) and np.iscomplexobj(got) == cplx
                assert rel(got, want) <= 1e-12, (p, q, n, nch, cplx, rel(got, want))


@gpu
def test_long_and_wide():
    """10^6 samples, and 32 channels (the array-recording case)."""
    import emagls_amd as E
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1_000_000)
    for p, q in [(147, 160), (160, 147), (1, 6)]:
        assert rel(E.resample(x, p, q), polyphase_resample(x, p, q)) <= 1e-12, (p, q)
    X = rng.standard_normal((20000, 32)) + 1j * rng.standard_normal((20000, 32))
    assert rel(E.resample(X, 147, 160), polyphase_resample(X, 147, 160)) <= 1e-12


@gpu
def test_shapes():
    """1-D and 1 x n rows along their length, matrices per column; p == q after reduction copies."""
    import emagls_amd as E
    rng = np.random.default_rng(6)
    v = rng.standard_normal(1000)
    y = E.resample(v, 160, 147)
    assert y.shape == (1089,)
    assert np.array_equal(E.resample(v.reshape(1, -1), 160, 147), y.reshape(1, -1))
    assert np.array_equal(E.resample(v.reshape(-1, 1), 160, 147), y.reshape(-1, 1))
    assert np.array_equal(E.resample(v, 44100 * 2, 48000 * 2), E.resample(v, 147, 160))
    assert np.array_equal(E.resample(v, 48000.0, 48000), v)
    assert E.resample(np.zeros((0, 2)), 2, 3).shape == (0, 2)


@gpu
def test_q1_property_on_gpu():
    import emagls_amd as E
    rng = np.random.default_rng(7)
    x = rng.standard_normal(4000)
    for p in (2, 3, 5):
        _, s0 = design(p, 1)
        assert np.abs(E.resample(x, p, 1)[::p] - x / s0).max() <= 1e-13 * np.abs(x).max(), p


@gpu
def test_sine_48k_to_44k1():
    """A 1 kHz sine at 48 kHz, resampled to 44.1 kHz, is the 1 kHz sine at 44.1 kHz away from the ends."""
    import emagls_amd as E
    t = np.arange(48000) / 48000.0
    y = E.resample(np.sin(2 * np.pi * 1000 * t), 44100, 48000)
    want = np.sin(2 * np.pi * 1000 * np.arange(y.size) / 44100.0)
    assert y.size == 44100
    assert np.abs(y[500:-500] - want[500:-500]).max() < 1e-3


@gpu
def test_repeatable_and_device_entry():
    """Repeated calls are bit-identical, and the device entry equals the host entry bit for bit."""
    import torch

    import emagls_amd as E
    from emagls_amd import _lib as L
    rng = np.random.default_rng(8)
    for p, q, cplx in [(147, 160, False), (1, 6, True), (441, 320, False), (47999, 48000, True)]:
        x = np.asfortranarray(rng.standard_normal((30000, 3)) + (1j * rng.standard_normal((30000, 3)) if cplx else 0))
        a = E.resample(x, p, q)
        assert np.array_equal(a, E.resample(x, p, q))
        dt = torch.complex128 if cplx else torch.float64
        dx = torch.from_numpy(np.ascontiguousarray(x.T)).to("cuda")      # [nch][n]: the column-major buffer
        ny = int(L.load().emagls_resample_length(30000, p, q))
        dy = torch.empty((3, ny), dtype=dt, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        L.check(L.load().emagls_resample_device(C.c_void_p(dx.data_ptr()), int(cplx), 30000, 3, p, q, C.c_void_p(dy.data_ptr()),
                                                C.c_void_p(st)))
        torch.cuda.synchronize()
        assert np.array_equal(dy.cpu().numpy().T, a), (p, q)


@gpu
def test_unsupported_ratio():
    import emagls_amd as E
    from emagls_amd import _lib as L
    from emagls_amd._lib import EmaglsError
    with pytest.raises(EmaglsError) as e:
        E.resample(np.ones(100), 65537, 65536)
    assert e.value.code == L.ERR_UNSUPPORTED
    assert E.resample(np.ones(100), 2 * 65536, 2 * 65535).shape == (101,)     # 65536 / 65535 after reduction: supported
