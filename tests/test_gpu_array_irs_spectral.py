"""Array impulse responses with a spectral gain (getArrayIrs with surfaceReflection / exponents / airAttenuation / pathLength,
emagls_array_irs_spectral) on the GPU.  The definition is restated here in NumPy: the Legendre form of
tests/test_gpu_array_irs.py, evaluated per component and extended by

    G_j(k) = g_j prod_w R_w(k) ** e_jw exp(-alpha(k) l_j)

with direct powers (numpy: 0.0 ** 0 = 1) -- never the logarithms of the code under test.  Errors are relative to the largest
magnitude of the expected array; every test prints its figure before it asserts.

Bounds: ten times the figure measured on an MI355X, and in no case above 1e-11.

    test                                              measured    bound
    1  listed form, W = 0, 1, 3, 6, 8, air or not     1.33e-14    1.33e-13
    2  encoder real and complex; nfft 8192 (hipFFT)   1.44e-15    1.44e-14

One assertion departs from its issue's wording.  "The response is exactly 0 in the zero bins" cannot be read off an impulse
response: the entry returns taps, and the transform back of taps whose spectrum had an exact zero is zero to rounding, not in
bits.  The test asserts (a) that the expected spectrum of that source is exactly 0 in the two bins, (b) that the spectrum of the
returned taps is below 16 eps of its largest magnitude there (measured: 1.6e-16 at most, 0.7 eps), and (c) the exact statement where it can
be observed: a surface that is 0 in every bin gives a response that is 0 in every bit, while a component with exponent 0 on it is
not touched by it.
"""
import functools

import numpy as np
import pytest

from test_gpu_array_irs import legendre_spectra, random_dirs  # noqa: E402  (the Legendre form of the definition of section 11)

gpu = pytest.mark.gpu

FS, RADIUS, NFFT, PRE = 16000.0, 0.042, 256, 8.0
COUNTS = (0, 7, 16, 17, 40, 70)          # both forms, the threshold (16 / 17) and more than one lane round (70 > 64)
ZERO_BINS = (5, 77)
ALL_POSITIVE = 3                          # the source whose every component has a positive exponent on the surface with the zeros
BOUND = {1: 1.33e-13, 2: 1.44e-14}


def spectral_legendre(fs, r, mics, sources, order, nfft, pre, refl=None, exps=None, att=None, paths=None):
    """legendre_spectra extended by G: [Q x P x M].  Each component goes through legendre_spectra on its own (with its gain), is
    multiplied by its factor over the bins, and the components are added; the last bin is the real part of the sum."""
    P = nfft // 2 + 1
    out = np.zeros((len(sources), P, mics.shape[0]), dtype=complex)
    for q, s in enumerate(sources):
        if s.shape[0] == 0:
            continue
        each = legendre_spectra(fs, r, mics, [s[j:j + 1] for j in range(s.shape[0])], order, nfft, pre)      # [J x P x M]
        fac = np.ones((s.shape[0], P))
        if refl is not None:
            for w in range(refl.shape[0]):
                fac = fac * refl[w][None, :] ** exps[q][:, w][:, None]
        if att is not None:
            fac = fac * np.exp(-att[None, :] * paths[q][:, None])
        out[q] = (each * fac[:, :, None]).sum(axis=0)
        out[q, -1] = out[q, -1].real
    return out


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check(family, what, got, want):
    e = rel(got, want)
    print("array_irs_spectral test %d %s: %.3g (bound %.3g)" % (family, what, e, BOUND[family]))
    assert e < BOUND[family], (what, e)


@functools.lru_cache(maxsize=None)
def case(W, air, nfft=NFFT, counts=COUNTS):
    """Microphones, sources [J x 4] with fractional delays, W spectra, exponents 0 .. 5, attenuation and paths."""
    rng = np.random.default_rng(100 + 10 * W + int(air))
    P = nfft // 2 + 1
    mics = random_dirs(rng, 5)
    sources = [np.column_stack([random_dirs(rng, J), rng.uniform(0.0, 0.7 * nfft, J), rng.uniform(-1.0, 1.0, J)]) for J in counts]
    refl = exps = att = paths = None
    if W:
        refl = rng.uniform(-1.0, 1.0, (W, P))
        refl[0] = -np.abs(refl[0])                               # one surface negative throughout
        zs = min(1, W - 1)
        refl[zs, list(ZERO_BINS)] = 0.0                          # one with an exact 0 at two bins
        exps = [rng.integers(0, 6, (J, W)).astype(np.int32) for J in counts]
        for q, e in enumerate(exps):
            if e.shape[0]:
                e[0, zs] = 0                                     # exponent 0 on the zero bins: the factor there is 1
                e[-1, zs] = 3
        if len(counts) > ALL_POSITIVE:
            exps[ALL_POSITIVE][:, zs] = rng.integers(1, 6, counts[ALL_POSITIVE])
    if air:
        att = rng.uniform(0.0, 0.05, P)
        paths = [rng.uniform(1.0, 30.0, J) for J in counts]
    return mics, sources, refl, exps, att, paths


def library(c, sources=None, exps=None, paths=None, nfft=NFFT, ir_len=None, **kw):
    import emagls_amd as E
    mics, src, refl, ex, att, pa = c
    return E.getArrayIrs(src if sources is None else sources, FS, nfft if ir_len is None else ir_len, PRE, RADIUS, mics, nfft=nfft,
                         surfaceReflection=refl, exponents=(ex if exps is None else exps) if refl is not None else None, airAttenuation=att,
                         pathLength=(pa if paths is None else paths) if att is not None else None, **kw)


@functools.lru_cache(maxsize=None)
def expected(W, air):
    mics, src, refl, ex, att, pa = case(W, air)
    H = spectral_legendre(FS, RADIUS, mics, src, 4, NFFT, PRE, refl, ex, att, pa)
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def call_of_test_1():
    got = library(case(3, True))
    got.setflags(write=False)
    return got


# ---- 1. the listed form against the definition
@gpu
@pytest.mark.parametrize("W,air", [(3, True), (1, True), (6, True), (8, True), (0, True), (3, False)])
def test_listed_form_against_the_definition(W, air):
    H = expected(W, air)
    got = call_of_test_1() if (W, air) == (3, True) else library(case(W, air))
    assert got.shape == (len(COUNTS), NFFT, 5) and got.dtype == np.float64
    assert not got[0].any()                                       # the empty source
    check(1, "W = %d, air %s" % (W, air), got, np.fft.irfft(H, n=NFFT, axis=1))
    if W:
        # the zero bins of the source whose every component has a positive exponent there (see the head of this file)
        assert not H[ALL_POSITIVE][list(ZERO_BINS)].any() and np.abs(H[1][list(ZERO_BINS)]).min() > 0
        S = np.fft.rfft(got[ALL_POSITIVE], axis=0)
        z = float(np.abs(S[list(ZERO_BINS)]).max() / np.abs(S).max())
        print("array_irs_spectral zero bins, W = %d: %.3g of the largest bin" % (W, z))
        assert z < 16 * np.finfo(float).eps


@gpu
def test_a_surface_that_is_zero_in_every_bin():
    """G is exactly 0 where R = 0 meets e > 0, and R ** 0 = 1 also for R = 0."""
    mics, src, _r, _e, _a, _p = case(0, False)
    P = NFFT // 2 + 1
    refl = np.vstack([np.zeros(P), np.full(P, -0.5)])
    s = src[4]                                                      # 40 components
    dead = np.column_stack([np.arange(1, 41) % 5 + 1, np.arange(40) % 3]).astype(np.int32)
    c = (mics, [s, s], refl, [dead, dead * np.array([0, 1], dtype=np.int32)], None, None)
    got = library(c)
    assert not got[0].any() and got[1].any()
    want = spectral_legendre(FS, RADIUS, mics, [s], 4, NFFT, PRE, refl[1:], [dead[:, 1:]])
    check(1, "exponent 0 on a surface of zeros", got[1:], np.fft.irfft(want, n=NFFT, axis=1))


# ---- 2. encoders, and the long transform
@gpu
@pytest.mark.parametrize("encoder", ["real", "complex"])
def test_encoders(encoder):
    rng = np.random.default_rng(5)
    enc = rng.standard_normal((4, 5)) + (1j * rng.standard_normal((4, 5)) if encoder == "complex" else 0.0)
    mics, src, refl, ex, att, pa = case(3, True)
    got = library((mics, src[4:5], refl, ex[4:5], att, pa[4:5]), encoder=enc)
    assert got.shape == (1, NFFT, 4) and np.iscomplexobj(got) == (encoder == "complex")
    taps = lambda e: np.fft.irfft(np.einsum("cm,qkm->qkc", e, expected(3, True)[4:5]), n=NFFT, axis=1)   # noqa: E731
    want = taps(enc.real) + 1j * taps(enc.imag) if encoder == "complex" else taps(enc)   # (the two parts of enc transformed separately)
    check(2, "%s encoder" % encoder, got, want)


@gpu
def test_long_transform_through_hipfft():
    c = case(3, True, 8192, (40,))
    mics, src, refl, ex, att, pa = c
    got = library(c, nfft=8192, ir_len=600)
    assert got.shape == (1, 600, 5)
    want = np.fft.irfft(spectral_legendre(FS, RADIUS, mics, src, 4, 8192, PRE, refl, ex, att, pa), n=8192, axis=1)[:, :600]
    check(2, "nfft = 8192", got, want)


# ---- 3. no surfaces and no air: the flat kernels
@gpu
def test_no_surfaces_and_no_air_is_the_flat_call_bit_for_bit():
    import emagls_amd as E
    mics, src, _r, _e, _a, _p = case(3, True)
    flat = E.getArrayIrs(src, FS, NFFT, PRE, RADIUS, mics, nfft=NFFT)
    got = E.getArrayIrs(src, FS, NFFT, PRE, RADIUS, mics, nfft=NFFT, surfaceReflection=np.zeros((0, NFFT // 2 + 1)),
                        exponents=[np.zeros((J, 0), dtype=np.int32) for J in COUNTS])
    assert flat.any() and np.array_equal(got, flat)


# ---- 4. a source alone
@gpu
@pytest.mark.parametrize("q", range(len(COUNTS)))
def test_source_alone_equals_source_in_the_call(q):
    mics, src, refl, ex, att, pa = case(3, True)
    alone = library((mics, src[q:q + 1], refl, ex[q:q + 1], att, pa[q:q + 1]))
    assert np.array_equal(alone[0], call_of_test_1()[q])
    if q == 4:
        assert np.array_equal(library(case(3, True)), call_of_test_1())     # and equal calls give equal bits
