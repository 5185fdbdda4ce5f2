"""binauralDecode with the resampling of dependencies/binauralDecode.m:12-23 (allowResampling=True) against the NumPy chain: the
restatement of MATLAB's resample (test_resample_host.py), then the oracle's decode as test_gpu_decode_render.py builds it.  Also
the MEX gateway's 'resample' command."""
import ctypes as C
import warnings

import numpy as np
import pytest

from test_gpu_decode_render import fitted_rot_t, oracle_render, rand, rel, rot_closed_form
from test_resample_host import matlab_resample

gpu = pytest.mark.gpu


def render_fs(x, wL, wR, comp, in_fs, filter_fs, signal_fs, yaw=None, signal=None, basis="real"):
    """emagls_binaural_decode_render_fs through ctypes: (out, imag_abs_sum)."""
    from emagls_amd import _lib as L
    ic, wc = np.iscomplexobj(x), np.iscomplexobj(wL)
    x = np.asfortranarray(x, dtype=np.complex128 if ic else np.float64)
    wL = np.asfortranarray(wL, dtype=np.complex128 if wc else np.float64)
    wR = np.asfortranarray(wR, dtype=np.complex128 if wc else np.float64)
    n, Cc = x.shape
    ln = wL.shape[0]
    ln2 = int(L.load().emagls_resample_length(ln, int(in_fs), int(filter_fs)))
    yaw = None if yaw is None else np.ascontiguousarray(np.asarray(yaw, dtype=np.float64).reshape(-1))
    sig = None if signal is None else np.ascontiguousarray(signal, dtype=np.float64)
    nsig = 0 if sig is None else int(L.load().emagls_resample_length(sig.size, int(in_fs), int(signal_fs)))
    nout = (nsig if sig is not None else n) - ((ln2 // 2 - 1) if comp else 0)
    out = np.zeros((nout, 2), order="F")
    im = (C.c_double * 2)()
    L.check(L.load().emagls_binaural_decode_render_fs(
        x.ctypes.data_as(C.c_void_p), int(ic), n, Cc, wL.ctypes.data_as(C.c_void_p), wR.ctypes.data_as(C.c_void_p), int(wc), ln,
        int(comp), L.LAYOUT["sh"], L.BASIS[basis], None if yaw is None else yaw.ctypes.data_as(C.c_void_p), 0 if yaw is None else yaw.size,
        None, 0, None, 0, None if sig is None else sig.ctypes.data_as(C.c_void_p), 0 if sig is None else sig.size,
        float(in_fs), float(filter_fs), float(signal_fs), out.ctypes.data_as(C.c_void_p), im))
    return out, np.array([im[0], im[1]])


@gpu
def test_filters_48k_to_44k1(capsys):
    """512 taps at 48 kHz become 471 at 44.1 kHz (odd), so compensateDelay cuts 471 // 2 - 1 = 234 samples."""
    import emagls_amd as E
    rng = np.random.default_rng(1)
    x = rng.standard_normal((4000, 9))
    wL, wR = rng.standard_normal((512, 9)), rng.standard_normal((512, 9))
    rL, rR = matlab_resample(wL, 44100, 48000), matlab_resample(wR, 44100, 48000)
    assert rL.shape == (471, 9)
    for comp in (False, True):
        want, _ = oracle_render(x, rL, rR, comp)
        got = E.binauralDecode(x, 44100, wL, wR, 48000, comp, allowResampling=True)
        assert got.shape == want.shape == (4000 - (234 if comp else 0), 2)
        assert rel(got, want) <= 1e-12, (comp, rel(got, want))
    assert capsys.readouterr().out.count("binauralDecode: resampling decoding filter") == 2


@gpu
def test_signal_44k1_to_48k(capsys):
    import emagls_amd as E
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3000, 9))
    wL, wR = rng.standard_normal((256, 9)), rng.standard_normal((256, 9))
    sig = rng.standard_normal((9000, 2))
    s2 = matlab_resample(sig, 48000, 44100)[:, 0]         # the reference's order: resample, then signal(:, 1)
    for comp in (False, True):
        want, _ = oracle_render(x, wL, wR, comp, signal=s2)
        got = E.binauralDecode(x, 48000, wL, wR, 48000, comp, sig, 44100, allowResampling=True)
        assert got.shape == want.shape == (s2.size - (127 if comp else 0), 2) and s2.size == 9796
        assert rel(got, want) <= 1e-12
    out = capsys.readouterr().out
    assert out.count("binauralDecode: resampling signal") == 2 and "decoding filter" not in out


@gpu
def test_filters_and_signal(capsys):
    import emagls_amd as E
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2500, 16))
    wL, wR = rng.standard_normal((300, 16)), rng.standard_normal((300, 16))
    sig = rng.standard_normal(7000)
    rL, rR = matlab_resample(wL, 44100, 48000), matlab_resample(wR, 44100, 48000)
    want, _ = oracle_render(x, rL, rR, True, signal=matlab_resample(sig, 44100, 32000))
    got = E.binauralDecode(x, 44100, wL, wR, 48000, True, sig, 32000, allowResampling=True)
    assert got.shape == want.shape and rel(got, want) <= 1e-12
    assert capsys.readouterr().out.splitlines() == ["binauralDecode: resampling signal", "binauralDecode: resampling decoding filter"]


@gpu
def test_complex_sh_warning_sums():
    """Complex filters are resampled as complex; the imaginary-part sums run over the returned samples."""
    import emagls_amd as E
    rng = np.random.default_rng(4)
    x = rand(rng, (2500, 9), True)
    wL, wR = rand(rng, (512, 9), True), rand(rng, (512, 9), True)
    sig = rng.standard_normal(5000)
    rL, rR = matlab_resample(wL, 44100, 48000), matlab_resample(wR, 44100, 48000)
    for comp in (False, True):
        for s in (None, sig):
            want, want_im = oracle_render(x, rL, rR, comp, signal=None if s is None else matlab_resample(s, 44100, 48000))
            got, im = render_fs(x, wL, wR, comp, 44100, 48000, 48000, signal=s, basis="complex")
            assert rel(got, want) <= 1e-12
            assert np.all(np.abs(im - want_im) <= 1e-12 * want_im), (im, want_im)
    with pytest.warns(UserWarning, match="discarding imaginary part"):
        E.binauralDecode(x, 44100, wL, wR, 48000, True, allowResampling=True)


@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_rotation_after_resampling(basis):
    """A fixed rotation turns the resampled filters; a trajectory (one angle per input sample) turns the signal."""
    rng = np.random.default_rng(5)
    N, n = 2, 3000
    x = rand(rng, (n, 9), basis == "complex")
    wL, wR = rng.standard_normal((512, 9)), rng.standard_normal((512, 9))
    rL, rR = matlab_resample(wL, 44100, 48000), matlab_resample(wR, 44100, 48000)
    got, _ = render_fs(x, wL, wR, True, 44100, 48000, 44100, yaw=0.7, basis=basis)
    assert rel(got, oracle_render(x @ fitted_rot_t(N, 0.7, basis, "sh"), rL, rR, True)[0]) <= 1e-12
    th = np.cumsum(rng.normal(0, 1e-2, n))
    got, _ = render_fs(x, wL, wR, True, 44100, 48000, 44100, yaw=th, basis=basis)
    assert rel(got, oracle_render(rot_closed_form(x, th, N, basis, "sh"), rL, rR, True)[0]) <= 1e-12


@gpu
def test_matched_rates_are_bit_identical(capsys):
    import emagls_amd as E
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5000, 9))
    wL, wR = rng.standard_normal((512, 9)), rng.standard_normal((512, 9))
    sig = rng.standard_normal(6000)
    for args in [(), (sig, 48000), (sig, 48000, 0.4)]:
        assert np.array_equal(E.binauralDecode(x, 48000, wL, wR, 48000, True, *args, allowResampling=True),
                              E.binauralDecode(x, 48000, wL, wR, 48000, True, *args))
    # the C entry with matched rates is the _ypr entry
    from test_gpu_decode_render import render
    assert np.array_equal(render_fs(x, wL, wR, True, 48000, 48000, 48000, yaw=0.4, signal=sig)[0],
                          render(x, wL, wR, True, yaw=0.4, signal=sig)[0])
    assert capsys.readouterr().out == ""


@gpu
def test_device_entry_matches_host():
    import torch
    from emagls_amd import _lib as L
    rng = np.random.default_rng(7)
    n, ln = 3000, 512
    x = np.asfortranarray(rng.standard_normal((n, 9)))
    wL, wR = np.asfortranarray(rng.standard_normal((ln, 9))), np.asfortranarray(rng.standard_normal((ln, 9)))
    sig = rng.standard_normal(4000)
    host, _ = render_fs(x, wL, wR, False, 44100, 48000, 48000, signal=sig)
    dev = "cuda"

    def d(a):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a).T).reshape(-1)).to(dev)
    dx, dL, dR, ds = d(x), d(wL), d(wR), torch.from_numpy(sig).to(dev)
    dout = torch.zeros(2 * host.shape[0], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    L.check(L.load().emagls_binaural_decode_render_fs_device(
        C.c_void_p(dx.data_ptr()), 0, n, 9, C.c_void_p(dL.data_ptr()), C.c_void_p(dR.data_ptr()), 0, ln, L.LAYOUT["sh"], L.BASIS["real"],
        None, 0, None, 0, None, 0, C.c_void_p(ds.data_ptr()), sig.size, 44100.0, 48000.0, 48000.0, C.c_void_p(dout.data_ptr()), None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(dout.cpu().numpy().reshape(2, -1).T, host)


@gpu
def test_default_still_refuses():
    import emagls_amd as E
    x, w = np.zeros((100, 9)), np.zeros((16, 9))
    with pytest.raises(NotImplementedError, match="resampling"):
        E.binauralDecode(x, 48000, w, w, 44100)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert E.binauralDecode(x, 48000, w, w, 44100, allowResampling=True).shape == (100, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# the MEX gateway
# ---------------------------------------------------------------------------------------------------------------------------
from test_mex_gateway import mex  # noqa: E402,F401  (the stub mex.h harness)


@gpu
def test_mex_resample(mex):
    import emagls_amd as E
    rng = np.random.default_rng(8)
    X = rng.standard_normal((3000, 3))
    Z = X + 1j * rng.standard_normal((3000, 3))
    for p, q in [(147, 160), (160, 147), (1, 6), (3, 1)]:
        assert np.array_equal(mex(1, "resample", X, p, q)[0], E.resample(X, p, q))
        assert np.array_equal(mex(1, "resample", Z, p, q)[0], E.resample(Z, p, q))
        row = X[:, :1].T
        got = mex(1, "resample", row, p, q)[0]
        assert got.shape == (1, -(-3000 * p // q)) and np.array_equal(got, E.resample(row, p, q))
    with pytest.raises(mex.Error, match="positive integer"):
        mex(1, "resample", X, 44100.5, 48000)
    with pytest.raises(mex.Error, match="65536"):
        mex(1, "resample", X, 65537, 2)
