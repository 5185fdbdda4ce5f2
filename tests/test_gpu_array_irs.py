"""Array impulse responses (getArrayIrs, emagls_array_irs) on the GPU.  Expected values are written out here in
NumPy from oracle.emagls_oracle (getSMAIRMatrix, getSH, sphModalCoeffs) in two forms that do not share an algorithm: the SH product
smairMat(:, :, k) conj(getSH(N, dir)).' and the Legendre sum of the definition.  Errors are relative to the largest magnitude of the
expected array; every test prints its figure before it asserts.

Bounds: ten times the largest error seen per test family on an MI355X (the margin is for another machine's NumPy / libm on the
expected side: the kernels are deterministic).  On the CPU the two NumPy forms agree to 7e-15 at N = 7, 2.8e-14 at N = 44 and
6.5e-14 at N = 85.

    family                                     measured    bound
    1  one plane wave, SH product (N = 7, 9)   6.95e-15    6.95e-14
    2  high orders, Legendre (N = 44, 85)      2.83e-15    2.83e-14
    3  many components, fractional delays      2.80e-15    2.80e-14
    4  encoder, real and complex               4.17e-15    4.17e-14
    5  long transform (hipFFT, nfft = 8192)    5.59e-16    5.59e-15
    7  against getRenderedHrtfs                3.83e-15    3.83e-14
    8  through the streams                     4.13e-16    the streams' own 1e-12 (tests/test_gpu_decode_stream.py)
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import emagls_oracle as O

gpu = pytest.mark.gpu
BOUND = {1: 6.95e-14, 2: 2.83e-14, 3: 2.80e-14, 4: 4.17e-14, 5: 5.59e-15, 7: 3.83e-14, 8: 1e-12}


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def check(family, what, got, want):
    e = rel(got, want)
    print("array_irs family %d %s: %.3g (bound %.3g)" % (family, what, e, BOUND[family]))
    assert e < BOUND[family], (what, e)


def random_dirs(rng, n):
    return np.column_stack([rng.uniform(0, 2 * np.pi, n), np.arccos(rng.uniform(-1, 1, n))])


def unit(d):
    return np.column_stack([np.sin(d[:, 1]) * np.cos(d[:, 0]), np.sin(d[:, 1]) * np.sin(d[:, 0]), np.cos(d[:, 1])])


def sh_spectra(fs, r, mics, dirs, order, nfft):
    """[P x M x Q]: smairMat(:, :, k) conj(getSH(N, dirs)).' on raw microphones (the last bin as getSMAIRMatrix leaves it)."""
    smair, N = O.getSMAIRMatrix(order, fs, nfft, r, mics, returnRawMicSigs=True)
    Yc = np.conj(O.getSH(N, dirs)).T
    return np.stack([smair[:, :, k] @ Yc for k in range(smair.shape[2])])


def legendre_spectra(fs, r, mics, sources, order, nfft, pre):
    """The definition: [Q x P x M].  sources: list of [J x 4] (azi, zen, delay, gain).  The phase's argument is reduced exactly
    (the integer part of the delay times k modulo nfft in integers), so that the expected values stay good at long delays."""
    N = O.simulation_order(order, fs, r)
    P = nfft // 2 + 1
    k = np.arange(P)
    bn = -O.sphModalCoeffs(N, 2 * np.pi * (k * fs / nfft) / 343.0 * r).T * ((2 * np.arange(N + 1) + 1) / (4 * np.pi))[:, None]
    bn[:, -1] = bn[:, -1].real
    v = unit(mics)
    out = np.zeros((len(sources), P, mics.shape[0]), dtype=complex)
    for q, s in enumerate(sources):
        if s.shape[0] == 0:
            continue
        x = unit(s[:, :2]) @ v.T                                   # [J x M]
        p0, p1 = np.ones_like(x), x
        A = bn[0][:, None, None] * p0                                # [P x J x M]
        for n in range(1, N + 1):
            A = A + bn[n][:, None, None] * p1
            p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
        d = s[:, 2] + pre
        di = np.floor(d)
        turns = ((k[:, None] * di[None, :].astype(np.int64)) % nfft + k[:, None] * (d - di)[None, :]) / nfft
        ph = s[:, 3][None, :] * np.exp(-2j * np.pi * turns)          # [P x J]
        out[q] = np.einsum("kj,kjm->km", ph, A)
        out[q, -1] = out[q, -1].real
    return out


# ---- 1. one plane wave per source, against the SH product
@functools.lru_cache(maxsize=None)
def case_plane(order):
    rng = np.random.default_rng(11)
    mics, dirs = random_dirs(rng, 11), random_dirs(rng, 67)
    want = sh_spectra(16000.0, 0.042, mics, dirs, order, 64)      # [P x M x Q]
    for a in (mics, dirs, want):
        a.setflags(write=False)
    return mics, dirs, want


@gpu
@pytest.mark.parametrize("order,N", [(4, 7), (9, 9)])
def test_one_plane_wave_against_the_sh_product(order, N):
    import emagls_amd as E
    mics, dirs, want = case_plane(order)
    assert O.simulation_order(order, 16000.0, 0.042) == N
    ir = E.getArrayIrs(dirs, 16000.0, 64, 8, 0.042, mics, order=order, nfft=64)
    assert ir.shape == (67, 64, 11) and ir.dtype == np.float64
    got = np.fft.rfft(ir, axis=1) * np.exp(2j * np.pi * np.arange(33) * 8 / 64)[None, :, None]
    got, want = got.transpose(1, 2, 0).copy(), want.copy()
    got[-1], want[-1] = got[-1].real, want[-1].real
    check(1, "N = %d" % N, got, want)


# ---- 2. high orders, against the Legendre form
@gpu
@pytest.mark.parametrize("fs,r,M,Q,nfft,N", [(48000.0, 0.10, 5, 3, 256, 44), (48000.0, 0.193, 3, 2, 64, 85)])
def test_high_orders_against_the_legendre_form(fs, r, M, Q, nfft, N):
    import emagls_amd as E
    assert O.simulation_order(4, fs, r) == N
    rng = np.random.default_rng(N)
    mics, dirs = random_dirs(rng, M), random_dirs(rng, Q)
    pre = nfft // 4
    want = np.fft.irfft(legendre_spectra(fs, r, mics, [np.array([[d[0], d[1], 0.0, 1.0]]) for d in dirs], 4, nfft, pre), n=nfft, axis=1)
    got = E.getArrayIrs(dirs, fs, nfft, pre, r, mics, nfft=nfft)
    check(2, "N = %d" % N, got, want)


# ---- 3. many components, fractional delays, truncation
COUNTS = (200, 1, 0, 64, 65)
FS3, R3, NFFT3, NR3, PRE3 = 16000.0, 0.042, 128, 100, 5.5


@functools.lru_cache(maxsize=None)
def case_rooms():
    rng = np.random.default_rng(3)
    mics = random_dirs(rng, 7)
    sources = [np.column_stack([random_dirs(rng, J), rng.uniform(0, 40, J), rng.standard_normal(J)]) for J in COUNTS]
    want = np.fft.irfft(legendre_spectra(FS3, R3, mics, sources, 4, NFFT3, PRE3), n=NFFT3, axis=1)[:, :NR3]
    for a in (mics, want, *sources):
        a.setflags(write=False)
    return mics, sources, want


@functools.lru_cache(maxsize=None)
def rooms_on_the_gpu():
    import emagls_amd as E
    mics, sources, _ = case_rooms()
    got = E.getArrayIrs(list(sources), FS3, NR3, PRE3, R3, mics, nfft=NFFT3)
    got.setflags(write=False)
    return got


@gpu
def test_many_components_fractional_delays_truncation():
    _, _, want = case_rooms()
    got = rooms_on_the_gpu()
    assert got.shape == (5, NR3, 7)
    assert not got[2].any()                                         # no components: zeros
    for q, J in enumerate(COUNTS):
        if J:
            check(3, "%d components" % J, got[q], want[q])


# ---- 4. encoder
@gpu
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_encoder(basis):
    import emagls_amd as E
    rng = np.random.default_rng(4)
    mics, dirs = random_dirs(rng, 6), random_dirs(rng, 9)
    fs, r, nfft, pre = 16000.0, 0.042, 64, 8
    smair, N = O.getSMAIRMatrix(1, fs, nfft, r, mics, shDefinition=basis, returnRawMicSigs=False)     # [4 x S x P]: pinv(Y_lo) inside
    Yc = np.conj(O.getSH(N, dirs, basis)).T
    X = np.stack([smair[:, :, k] @ Yc for k in range(33)]) * np.exp(-2j * np.pi * np.arange(33) * pre / nfft)[:, None, None]   # [P x 4 x Q]
    # a complex encoder: the real and the imaginary part of enc transformed separately (include/emagls.h)
    enc = O.pinv(O.getSH(1, mics, basis))
    raw = sh_spectra(fs, r, mics, dirs, 1, nfft) * np.exp(-2j * np.pi * np.arange(33) * pre / nfft)[:, None, None]              # [P x M x Q]
    raw[-1] = raw[-1].real
    parts = [np.fft.irfft(np.einsum("cm,kmq->kcq", e, raw), n=nfft, axis=0) for e in (enc.real, enc.imag)]
    want = (parts[0] + 1j * parts[1] if basis == "complex" else parts[0]).transpose(2, 0, 1)
    got = E.getArrayIrs(dirs, fs, nfft, pre, r, mics, order=1, encoder=enc, nfft=nfft)
    assert got.shape == (9, 64, 4) and np.iscomplexobj(got) == (basis == "complex")
    check(4, basis + " basis, against the raw responses encoded in NumPy", got, want)
    # the oracle's SH-domain matrix on every bin 0 .. nfft/2 (with a whole pre-delay the last bin's phase is +-1, and the raw
    # responses are real there by the addition theorem, so the bin's real-part rule changes nothing beyond rounding)
    G = np.fft.fft(got, axis=1)[:, :33].transpose(1, 2, 0)
    check(4, basis + " basis, against getSMAIRMatrix(returnRawMicSigs=False)", G, X)


# ---- 5. long transform
@gpu
def test_long_transform():
    import emagls_amd as E
    rng = np.random.default_rng(5)
    mics = random_dirs(rng, 2)
    src = np.column_stack([random_dirs(rng, 3), [6000.0, 3210.25, 17.5], [1.0, -0.5, 0.25]])
    want = np.fft.irfft(legendre_spectra(16000.0, 0.042, mics, [src], 4, 8192, 20.0), n=8192, axis=1)
    got = E.getArrayIrs([src], 16000.0, 8192, 20.0, 0.042, mics, nfft=8192)
    assert got.shape == (1, 8192, 2)
    check(5, "nfft = 8192", got, want)
    # and behind a complex encoder on that path
    enc = rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2))
    got_e = E.getArrayIrs([src], 16000.0, 500, 20.0, 0.042, mics, nfft=8192, encoder=enc)
    check(5, "nfft = 8192, complex encoder", got_e, (want @ enc.T)[:, :500])


# ---- 6. bits
@gpu
def test_equal_calls_give_equal_bits_and_a_source_does_not_depend_on_its_neighbours():
    import emagls_amd as E
    mics, sources, _ = case_rooms()
    got = rooms_on_the_gpu()
    again = E.getArrayIrs(list(sources), FS3, NR3, PRE3, R3, mics, nfft=NFFT3)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    ms = ctypes.c_double(-1.0)                                      # the main kernel's device-event time of that call
    assert E._lib.load().emagls_array_irs_kernel_time(ctypes.byref(ms)) == 0 and 0.0 < ms.value < 1e3
    for q in range(len(COUNTS)):
        alone = E.getArrayIrs([sources[q]], FS3, NR3, PRE3, R3, mics, nfft=NFFT3)
        assert np.array_equal(alone[0].view(np.uint64), got[q].view(np.uint64)), q


# ---- 7. against getRenderedHrtfs
@gpu
def test_against_rendered_hrtfs():
    import emagls_amd as E
    rng = np.random.default_rng(7)
    mics, dirs = random_dirs(rng, 8), random_dirs(rng, 5)
    fs, r, nfft, pre = 16000.0, 0.042, 64, 8
    wL, wR = rng.standard_normal((32, 8)), rng.standard_normal((32, 8))
    ir = E.getArrayIrs(dirs, fs, nfft, pre, r, mics, order=4, nfft=nfft)                      # order 4: the emagls2 model's own rule
    want = E.getRenderedHrtfs(wL, wR, "emagls2", dirs, fs, micRadius=r, micGridAziZenRad=mics, nfft=nfft, returnResponse=True).H
    want = want * np.exp(-2j * np.pi * np.arange(33) * pre / nfft)[:, None, None]              # [P x D x 2]
    S = np.fft.rfft(ir, axis=1)                                                                 # [D x P x M]
    got = np.stack([np.einsum("dkc,kc->kd", S, np.fft.rfft(w, nfft, axis=0)) for w in (wL, wR)], axis=2)
    check(7, "emagls2", got, want)


# ---- 8. as the streams read it
@gpu
def test_as_the_streams_read_it():
    import emagls_amd as E
    rng = np.random.default_rng(8)
    mics = random_dirs(rng, 6)
    src = np.column_stack([random_dirs(rng, 4), rng.uniform(0, 30, 4), rng.standard_normal(4)])
    enc = E.arrayEncoder("sma", 1, mics[:, 0], mics[:, 1])
    ir = E.getArrayIrs([src], 16000.0, 100, 8, 0.042, mics, order=1, encoder=enc, nfft=256)    # [1 x 100 x 4]
    wL, wR = rng.standard_normal((32, 4)), rng.standard_normal((32, 4))
    n = 192
    impulse = np.zeros((n, 1))
    impulse[0] = 1.0
    with E.SourceFieldStream(ir, 64) as f, E.BinauralDecodeStream(wL, wR, 64) as d:
        field = f.push(impulse)
        got = d.push(field)
    padded = np.vstack([ir[0], np.zeros((n - 100, 4))])
    check(8, "field", field, padded)
    check(8, "ears", got, O.binauralDecode(padded, wL, wR))
