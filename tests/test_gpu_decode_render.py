"""binauralDecode with head rotation and source-signal convolution (dependencies/binauralDecode.m:27-31,44-48) against NumPy
built on oracle.binauralDecode / oracle.fftfilt.  The rotation matrix the expected values use is fitted independently of the
kernel: Rot^T = pinv(S(a)) S(a + theta), S = conj(getSH) / conj(getCH) of the oracle on a point set that resolves order N.
The argument checks that need no device run without a GPU."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
TWO_PI = 2.0 * np.pi


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def signals(N, azi, zen, basis, layout):
    """Rows: the signal of a plane wave from each direction, conj(Y)."""
    if layout == "sh":
        return np.conj(O.getSH(N, np.column_stack([azi, zen]), basis))
    return np.conj(O.getCH(N, azi, basis))


def fitted_rot_t(N, theta, basis, layout):
    """Rot^T with S(a) Rot^T = S(a + theta), theta reduced modulo 2 pi in FP64 as the specification says."""
    th = math.fmod(theta, TWO_PI)
    if layout == "sh":    # a Fibonacci lattice of 3 (N+1)^2 points
        i = np.arange(3 * (N + 1) ** 2) + 0.5
        azi, zen = np.mod(np.pi * (1 + 5 ** 0.5) * i, TWO_PI), np.arccos(1 - 2 * i / i.size)
    else:                 # 4N + 4 equiangular azimuths
        azi, zen = np.arange(4 * N + 4) * TWO_PI / (4 * N + 4), None
    return np.linalg.pinv(signals(N, azi, zen, basis, layout)) @ signals(N, azi + th, zen, basis, layout)


def rot_closed_form(x, theta, N, basis, layout):
    """Per-sample rotation in NumPy (the closed form of the specification; anchored to fitted_rot_t by a test below)."""
    th = np.fmod(np.broadcast_to(np.asarray(theta, dtype=np.float64), (x.shape[0],)), TWO_PI)
    y = x.astype(np.complex128 if (np.iscomplexobj(x) or basis == "complex") else np.float64, copy=True)
    pairs = [(n * n + n + m, n * n + n - m, m) for n in range(N + 1) for m in range(1, n + 1)] if layout == "sh" else \
            [(2 * m, 2 * m - 1, m) for m in range(1, N + 1)]
    for p, q, m in pairs:
        c, s = np.cos(m * th), np.sin(m * th)
        if basis == "complex":
            y[:, p] = np.exp(-1j * m * th) * x[:, p]
            y[:, q] = np.exp(1j * m * th) * x[:, q]
        else:
            y[:, p] = c * x[:, p] - s * x[:, q]
            y[:, q] = c * x[:, q] + s * x[:, p]
    return y


def nch(N, layout):
    return (N + 1) ** 2 if layout == "sh" else 2 * N + 1


def oracle_render(x, wL, wR, comp=False, signal=None):
    """binauralDecode.m:33-64 in NumPy on the oracle's fftfilt: (real output, the two imaginary-part sums)."""
    n, Cc = x.shape
    ear = np.zeros((n, 2), dtype=np.complex128)
    for c in range(Cc):
        ear[:, 0] += O.fftfilt(wL[:, c], x[:, c])
        ear[:, 1] += O.fftfilt(wR[:, c], x[:, c])
    if signal is not None:
        ear = np.column_stack([O.fftfilt(ear[:, 0], signal), O.fftfilt(ear[:, 1], signal)])
    if comp:
        ear = ear[wL.shape[0] // 2 - 1:]
    return ear.real, np.abs(ear.imag).sum(axis=0)


def render(x, wL, wR, comp=False, yaw=None, signal=None, basis="real", layout="sh"):
    """emagls_binaural_decode_render through ctypes: (out, imag_abs_sum)."""
    from emagls_amd import _lib as L
    ic, wc = np.iscomplexobj(x), np.iscomplexobj(wL)
    x = np.asfortranarray(x, dtype=np.complex128 if ic else np.float64)
    wL = np.asfortranarray(wL, dtype=np.complex128 if wc else np.float64)
    wR = np.asfortranarray(wR, dtype=np.complex128 if wc else np.float64)
    n, Cc = x.shape
    ln = wL.shape[0]
    yaw = None if yaw is None else np.ascontiguousarray(np.asarray(yaw, dtype=np.float64).reshape(-1))
    sig = None if signal is None else np.ascontiguousarray(signal, dtype=np.float64)
    nout = (sig.size if sig is not None else n) - ((ln // 2 - 1) if comp else 0)
    out = np.zeros((nout, 2), order="F")
    im = (C.c_double * 2)()
    L.check(L.load().emagls_binaural_decode_render(
        x.ctypes.data_as(C.c_void_p), int(ic), n, Cc, wL.ctypes.data_as(C.c_void_p), wR.ctypes.data_as(C.c_void_p), int(wc), ln,
        int(comp), L.LAYOUT[layout], L.BASIS[basis], None if yaw is None else yaw.ctypes.data_as(C.c_void_p),
        0 if yaw is None else yaw.size, None if sig is None else sig.ctypes.data_as(C.c_void_p), 0 if sig is None else sig.size,
        out.ctypes.data_as(C.c_void_p), im))
    return out, np.array([im[0], im[1]])


def rand(rng, shape, cplx):
    return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rotation on its own
# ---------------------------------------------------------------------------------------------------------------------------
ANGLES = [0.0, 0.3, -2.0, np.pi, TWO_PI, 400.0]


@gpu
@pytest.mark.parametrize("layout,N", [("sh", 1), ("sh", 4), ("sh", 7), ("sh", 15), ("ch", 1), ("ch", 10)])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_rotation_invariant(layout, N, basis):
    """rotateYaw(conj(Y(a, z)), theta) == conj(Y(a + theta, z)): a fixed angle, then one angle per sample."""
    import emagls_amd as E
    rng = np.random.default_rng(N)
    azi = rng.uniform(0, TWO_PI, 64)
    zen = rng.uniform(0, np.pi, 64)
    x = signals(N, azi, zen, basis, layout)
    for th in ANGLES:
        got = E.rotateYaw(x, th, basis, layout)
        want = signals(N, azi + math.fmod(th, TWO_PI), zen, basis, layout)
        assert got.shape == want.shape and np.abs(got - want).max() < 1e-13, (th, np.abs(got - want).max())
    th = rng.choice(ANGLES, azi.size) + rng.uniform(-1, 1, azi.size)
    got = E.rotateYaw(x, th, basis, layout)
    want = signals(N, azi + np.fmod(th, TWO_PI), zen, basis, layout)
    assert np.abs(got - want).max() < 1e-13


@gpu
@pytest.mark.parametrize("layout,N", [("sh", 3), ("ch", 4)])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_rotation_matches_fitted_matrix(layout, N, basis):
    """The kernel and the NumPy closed form the longer tests use both equal x Rot^T with the fitted Rot, complex input too."""
    import emagls_amd as E
    rng = np.random.default_rng(7)
    x = rand(rng, (200, nch(N, layout)), True)
    for th in ANGLES:
        want = x @ fitted_rot_t(N, th, basis, layout)
        assert np.abs(rot_closed_form(x, th, N, basis, layout) - want).max() < 1e-12
        assert np.abs(E.rotateYaw(x, th, basis, layout) - want).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 2. a fixed angle in the render (the filters are rotated)
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("length", [64, 256, 512, 1000, 3000])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_fixed_angle_render(length, basis):
    rng = np.random.default_rng(length)
    N, n, th = 2, 4000, 0.7
    rt = fitted_rot_t(N, th, basis, "sh")
    for ic, wc in [(False, False), (True, True), (False, True), (True, False)]:
        x = rand(rng, (n, 9), ic)
        wL, wR = rand(rng, (length, 9), wc), rand(rng, (length, 9), wc)
        for comp in (False, True):
            out, im = render(x, wL, wR, comp, yaw=th, basis=basis)
            ref, ref_im = oracle_render(x @ rt, wL, wR, comp)
            assert out.shape == ref.shape and rel(out, ref) < 1e-12, (ic, wc, comp, rel(out, ref))
            if ic or wc or basis == "complex":
                assert np.all(np.abs(im - ref_im) <= 1e-12 * ref_im), (im, ref_im)


@gpu
def test_fixed_angle_render_ch():
    """The EMAinCH renderer's layout: 2N + 1 circular-harmonic channels."""
    rng = np.random.default_rng(3)
    for basis in ("real", "complex"):
        x = signals(5, rng.uniform(0, TWO_PI, 3000), None, basis, "ch") * rng.standard_normal((3000, 1))
        wL, wR = rand(rng, (512, 11), basis == "complex"), rand(rng, (512, 11), basis == "complex")
        out, _ = render(x, wL, wR, True, yaw=-1.2, basis=basis, layout="ch")
        ref, _ = oracle_render(x @ fitted_rot_t(5, -1.2, basis, "ch"), wL, wR, True)
        assert rel(out, ref) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 3. one angle per sample (the signal is rotated)
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_trajectory_render(basis):
    rng = np.random.default_rng(11)
    N, n = 2, 600_000
    x = rand(rng, (n, 9), basis == "complex")
    wL, wR = rand(rng, (512, 9), False), rand(rng, (512, 9), False)
    th = 300.0 + np.cumsum(rng.normal(0, 2e-3, n))      # an unwrapped head-tracker angle
    out, im = render(x, wL, wR, True, yaw=th, basis=basis)
    ref, ref_im = oracle_render(rot_closed_form(x, th, N, basis, "sh"), wL, wR, True)
    assert rel(out, ref) < 1e-12
    if basis == "complex":
        assert np.all(np.abs(im - ref_im) <= 1e-12 * ref_im)


@gpu
def test_trajectory_other_forms():
    """The trajectory through every decode form: register-resident (64 taps), LDS passes (1000 taps), hipFFT (3000 taps)."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((20000, 16))
    th = np.cumsum(rng.normal(0, 1e-2, x.shape[0]))
    xr = rot_closed_form(x, th, 3, "real", "sh")
    for length in (64, 1000, 3000):
        wL, wR = rng.standard_normal((length, 16)), rng.standard_normal((length, 16))
        out, _ = render(x, wL, wR, False, yaw=th)
        assert rel(out, oracle_render(xr, wL, wR)[0]) < 1e-12, length


@gpu
def test_zero_trajectory_is_exact():
    import emagls_amd as E
    rng = np.random.default_rng(13)
    x = rng.standard_normal((50000, 25))
    wL, wR = rng.standard_normal((512, 25)), rng.standard_normal((512, 25))
    assert np.array_equal(render(x, wL, wR, True, yaw=np.zeros(x.shape[0]))[0], E.binauralDecode(x, 48000, wL, wR, 48000, True))
    xc = rand(rng, (20000, 9), True)
    cL, cR = rand(rng, (300, 9), True), rand(rng, (300, 9), True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.array_equal(E.binauralDecode(xc, 48000, cL, cR, 48000, horRotAngleRad=np.zeros(20000), shDefinition="complex"),
                              E.binauralDecode(xc, 48000, cL, cR, 48000))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. end to end: a rotated plane wave renders like the plane wave from the rotated direction
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_plane_wave_end_to_end(basis):
    import emagls_amd as E
    from emagls_amd import synth
    azi, zen = synth.fibonacci_grid(400)
    hL, hR = synth.rigid_sphere_hrirs(azi, zen, taps=256)
    wL, wR = E.getLsFilters(hL, hR, azi, zen, 4, basis)
    rng = np.random.default_rng(4)
    s = rng.standard_normal((8000, 1))
    a, z, th = 0.4, 1.1, 2.5
    x = s * signals(4, np.array([a]), np.array([z]), basis, "sh")
    xt = s * signals(4, np.array([a + th]), np.array([z]), basis, "sh")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=th, shDefinition=basis)
        want = E.binauralDecode(xt, 48000, wL, wR, 48000, True)
        traj = E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=np.full(8000, th), shDefinition=basis)
    assert rel(got, want) < 1e-12 and rel(traj, want) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the source-signal convolution
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nsamp", [1000, 3000])          # a rendered response below 2048 samples (fused forms) and above (hipFFT)
@pytest.mark.parametrize("nsig", [700, 9000])            # a signal shorter and one longer than the response
def test_source_signal(nsamp, nsig):
    import emagls_amd as E
    rng = np.random.default_rng(nsamp + nsig)
    x = rng.standard_normal((nsamp, 9))
    wL, wR = rng.standard_normal((256, 9)), rng.standard_normal((256, 9))
    sig = rng.standard_normal((nsig, 2))
    for comp in (False, True):
        ref, _ = oracle_render(x, wL, wR, comp, signal=sig[:, 0])
        out = E.binauralDecode(x, 48000, wL, wR, 48000, comp, sig, 48000)
        assert out.shape == ref.shape == (nsig - (127 if comp else 0), 2) and rel(out, ref) < 1e-12
        assert np.array_equal(out, E.binauralDecode(x, 48000, wL, wR, 48000, comp, sig[:, :1]))   # only the first column counts
    # with a rotation in front of it
    out = E.binauralDecode(x, 48000, wL, wR, 48000, True, sig[:, 0], None, -0.9)
    assert rel(out, oracle_render(x @ fitted_rot_t(2, -0.9, "real", "sh"), wL, wR, True, signal=sig[:, 0])[0]) < 1e-12
    # an empty signal skips the step
    assert np.array_equal(E.binauralDecode(x, 48000, wL, wR, 48000, True, np.zeros((0, 1))), E.binauralDecode(x, 48000, wL, wR, 48000, True))


@gpu
def test_source_signal_complex_sh():
    """Complex SH: the response stays complex until the end; the warning sums are taken after the delay cut."""
    rng = np.random.default_rng(21)
    x = rand(rng, (2500, 9), True)
    wL, wR = rand(rng, (512, 9), True), rand(rng, (512, 9), True)
    sig = rng.standard_normal(6000)
    for comp in (False, True):
        for yaw in (None, 1.3, np.linspace(0, 3, 2500)):
            xr = x if yaw is None else rot_closed_form(x, yaw, 2, "complex", "sh")
            ref, ref_im = oracle_render(xr, wL, wR, comp, signal=sig)
            out, im = render(x, wL, wR, comp, yaw=yaw, signal=sig, basis="complex")
            assert rel(out, ref) < 1e-12
            assert np.all(np.abs(im - ref_im) <= 1e-12 * ref_im), (im, ref_im)
    import emagls_amd as E
    with pytest.warns(UserWarning, match="discarding imaginary part"):
        E.binauralDecode(x, 48000, wL, wR, 48000, True, sig)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. old calls are unchanged
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_old_calls_bit_identical():
    import emagls_amd as E
    from emagls_amd import _lib as L
    rng = np.random.default_rng(31)
    for ic, wc, length in [(False, False, 512), (True, False, 300), (False, True, 3000), (True, True, 64)]:
        x = np.asfortranarray(rand(rng, (7000, 9), ic))
        wL, wR = np.asfortranarray(rand(rng, (length, 9), wc)), np.asfortranarray(rand(rng, (length, 9), wc))
        for comp in (False, True):
            want = np.zeros((7000 - ((length // 2 - 1) if comp else 0), 2), order="F")
            im = (C.c_double * 2)()
            p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
            if ic or wc:
                L.check(L.load().emagls_binaural_decode_complex(p(x), int(ic), 7000, 9, p(wL), p(wR), int(wc), length, int(comp), p(want), im))
            else:
                L.check(L.load().emagls_binaural_decode(p(x), 7000, 9, p(wL), p(wR), length, int(comp), p(want)))
            got, gim = render(x, wL, wR, comp)
            assert np.array_equal(got, want) and (not (ic or wc) or np.array_equal(gim, [im[0], im[1]]))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(E.binauralDecode(x, 48000, wL, wR, 48000, comp, None, None, 0), want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the MEX gateway
# ---------------------------------------------------------------------------------------------------------------------------
from test_mex_gateway import mex  # noqa: E402,F401  (the stub mex.h harness)


@gpu
def test_mex_decode_and_rotate(mex):
    import emagls_amd as E
    rng = np.random.default_rng(41)
    x = rng.standard_normal((3000, 9))
    wL, wR = rng.standard_normal((512, 9)), rng.standard_normal((512, 9))
    sig = rng.standard_normal((5000, 2))
    th = np.cumsum(rng.normal(0, 1e-2, 3000))
    # the old form is untouched
    assert np.array_equal(mex(1, "decode", x, wL, wR, True)[0], E.binauralDecode(x, 48000, wL, wR, 48000, True))
    assert np.array_equal(mex(1, "decode", x, wL, wR, True, 0.5, np.zeros((0, 0)), "real", "sh")[0],
                          E.binauralDecode(x, 48000, wL, wR, 48000, True, horRotAngleRad=0.5))
    assert np.array_equal(mex(1, "decode", x, wL, wR, False, th.reshape(-1, 1), sig)[0],
                          E.binauralDecode(x, 48000, wL, wR, 48000, False, sig, 48000, th))
    assert np.array_equal(mex(1, "decode", x, wL, wR, True, np.zeros((0, 0)), sig)[0], E.binauralDecode(x, 48000, wL, wR, 48000, True, sig))
    xc = rand(rng, (3000, 9), True)
    cL, cR = rand(rng, (512, 9), True), rand(rng, (512, 9), True)
    out, imag = mex(2, "decode", xc, cL, cR, True, 2.0, sig, "complex", "sh")
    ref, ref_im = render(xc, cL, cR, True, yaw=2.0, signal=sig[:, 0], basis="complex")
    assert np.array_equal(out, ref) and np.array_equal(imag.ravel(), ref_im)
    xh = rng.standard_normal((100, 7))
    assert np.array_equal(mex(1, "decode", xh, wL[:, :7], wR[:, :7], False, 1.0, np.zeros((0, 0)), "real", "ch")[0],
                          E.binauralDecode(xh, 48000, wL[:, :7], wR[:, :7], 48000, horRotAngleRad=1.0, rotationDomain="ch"))
    for basis in ("real", "complex"):
        assert np.array_equal(mex(1, "rotate", x, 0.3, basis)[0], E.rotateYaw(x, 0.3, basis))
        assert np.array_equal(mex(1, "rotate", xh, th[:100].reshape(-1, 1), basis, "ch")[0], E.rotateYaw(xh, th[:100], basis, "ch"))
    with pytest.raises(mex.Error, match="2N\\+1 CH channels"):
        mex(1, "rotate", x[:, :8], 0.3, "real", "ch")


# ---------------------------------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_without_device():
    """Checked before anything reaches the library: trajectory length, resampling, rotation domain."""
    import emagls_amd as E
    x = np.zeros((100, 9))
    w = np.zeros((16, 9))
    with pytest.raises(ValueError, match="one angle per input sample"):
        E.binauralDecode(x, 48000, w, w, 48000, horRotAngleRad=np.zeros(99))
    with pytest.raises(ValueError, match="one angle per sample"):
        E.rotateYaw(x, np.zeros(7))
    with pytest.raises(NotImplementedError, match="resampling"):
        E.binauralDecode(x, 48000, w, w, 44100)
    with pytest.raises(NotImplementedError, match="resampling"):
        E.binauralDecode(x, 48000, w, w, 48000, signal=np.ones(10), signalFs=44100)
    with pytest.raises(ValueError, match="'sh' or 'ch'"):
        E.rotateYaw(x, 0.1, domain="xyz")


@gpu
def test_argument_errors_from_the_library():
    import emagls_amd as E
    from emagls_amd._lib import EmaglsError
    x8 = np.zeros((100, 8))
    w8 = np.zeros((16, 8))
    with pytest.raises(EmaglsError, match=r"\(N\+1\)\^2 SH channels"):
        E.binauralDecode(x8, 48000, w8, w8, 48000, horRotAngleRad=0.2)
    with pytest.raises(EmaglsError, match="2N\\+1 CH channels"):
        E.rotateYaw(x8, 0.2, domain="ch")
    x = np.zeros((100, 9))
    with pytest.raises(EmaglsError, match="one angle or one angle per input sample"):
        render(x, np.zeros((16, 9)), np.zeros((16, 9)), yaw=np.zeros(50))
