"""Array impulse responses to point sources at a finite distance on the GPU (getArrayIrs with distance=, getArrayRoomIrs with
waveModel='pointSource', getShoeboxComponents with returnDistance).

The truth is tests/point_reference.py: the product b'_n F_n evaluated directly from the oracle's sphModalCoeffs and scipy's spherical
Bessel functions (N = 19 and below, where neither factor leaves FP64), and the multiprecision fixture tests/golden/point_truth.npz
(written by tests/golden/make_point_truth.py) at N = 44 and 85 -- never the scaled recurrence of the code under test.  Errors are
relative to the largest magnitude of the expected array; every test prints its figure before it asserts.

Bounds: ten times the figure measured on an MI355X, and in no case above 1e-11.  The far-field bound is derived: N (N+1) / (kappa_1 rho),
the first-order term of F_n - 1 doubled.

    test                                                   measured    bound
    1  listed form, 0 .. 200 components, three encoders    6.65e-15    6.65e-14
    2  order 85 and 44 against the multiprecision fixture  1.05e-15    1.05e-14
    3  nfft 65536 (hipFFT, exact integer phase)            1.75e-16    1.75e-15
    4  sum of the taps against the closed form at DC       3.87e-15    3.87e-14
    5  rho = 1e7 m against the plane-wave call             6.21e-09    3.32e-05 (derived)
    6  three surfaces and air with distances               3.23e-15    3.23e-14
    7  room A as point sources, flat and data-sheet walls  1.23e-14    1.23e-13
    8  room A against its mirror image in y                1.88e-14    1.88e-13
"""
import functools
import os

import numpy as np
import pytest

from point_reference import dc_closed_form, point_legendre  # noqa: E402
from test_gpu_array_irs import random_dirs  # noqa: E402
from test_gpu_array_room_irs import A, BETA, RADIUS, mics5, shoebox_numpy  # noqa: E402
from test_gpu_array_room_spectral import ONES, data_sheet_room, images_numpy  # noqa: E402

gpu = pytest.mark.gpu

FS, NFFT, PRE, ORDER = 16000.0, 256, 8.0, 19            # order 19: N = max(19, ceil(16000 pi r / 343) = 7)
COUNTS = (0, 1, 16, 17, 64, 65, 200)                    # both forms, the threshold (16 / 17), one lane round and one more (64 / 65)
BOUND = {1: 6.65e-14, 2: 1.05e-14, 3: 1.75e-15, 4: 3.87e-14, 6: 3.23e-14, 7: 1.23e-13, 8: 1.88e-13}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_truth.npz")


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check(family, what, got, want, bound=None):
    e = rel(got, want)
    bound = BOUND[family] if bound is None else bound
    print("array_point test %d %s: %.3g (bound %.3g)" % (family, what, e, bound))
    assert np.isfinite(got).all(), what
    assert e < bound, (what, e)


def taps(H, n):
    return np.fft.irfft(H, n=n, axis=1)


@functools.lru_cache(maxsize=None)
def listed_case():
    """Seven sources [J x 4] with fractional delays and gains of both signs; distances from 1.05 r to 30 m, log-uniform, the two ends
    present."""
    rng = np.random.default_rng(1405)
    sources = [np.column_stack([random_dirs(rng, J), rng.uniform(0.0, 0.7 * NFFT, J), rng.uniform(-1.0, 1.0, J)]) for J in COUNTS]
    dists = [np.exp(rng.uniform(np.log(1.05 * RADIUS), np.log(30.0), J)) for J in COUNTS]
    dists[-1][0], dists[-1][-1], dists[1][0] = 1.05 * RADIUS, 30.0, 1.05 * RADIUS
    H = point_legendre(FS, RADIUS, mics5(), sources, dists, ORDER, NFFT, PRE)
    H.setflags(write=False)
    return sources, dists, H


# ---- 1. the listed form: both kernel forms and their seams
@gpu
@pytest.mark.parametrize("encoder", ["raw", "real", "complex"])
def test_listed_form_against_the_definition(encoder):
    import emagls_amd as E
    sources, dists, H = listed_case()
    rng = np.random.default_rng(7)
    enc = {"raw": None, "real": rng.standard_normal((4, 5)), "complex": rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))}[encoder]
    got = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, encoder=enc, distance=dists)
    assert got.shape == (7, NFFT, 5 if enc is None else 4) and np.iscomplexobj(got) == (encoder == "complex")
    assert not got[0].any()                                                   # the empty source
    if enc is None:
        want = taps(H, NFFT)
    elif encoder == "real":
        want = taps(H @ enc.T, NFFT)
    else:
        want = taps(H @ enc.real.T, NFFT) + 1j * taps(H @ enc.imag.T, NFFT)
    check(1, "listed form, %s encoder" % encoder, got, want)
    for q in (1, 3, 6):                                                       # source q of a call gives the bits of the call with it alone
        alone = E.getArrayIrs([sources[q]], FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, encoder=enc, distance=[dists[q]])
        assert np.array_equal(alone[0], got[q]), q


@gpu
def test_one_component_form_takes_a_vector_of_distances():
    import emagls_amd as E
    rng = np.random.default_rng(3)
    dirs, rho = random_dirs(rng, 9), rng.uniform(0.1, 3.0, 9)
    got = E.getArrayIrs(dirs, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, distance=rho)
    srcs = [np.array([[d[0], d[1], 0.0, 1.0]]) for d in dirs]
    assert np.array_equal(got, E.getArrayIrs(srcs, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, distance=[rho[q:q + 1] for q in range(9)]))
    check(1, "one component per source", got, taps(point_legendre(FS, RADIUS, mics5(), srcs, rho[:, None], ORDER, NFFT, PRE), NFFT))


# ---- 2. the extreme orders against the multiprecision fixture
@gpu
@pytest.mark.parametrize("order", [85, 44])
def test_extreme_orders_against_the_multiprecision_fixture(order):
    """fs 8000: N = order.  In the low bins F_n and b'_n leave FP64 on their own (bin 1 at n = 85: 1e+370 times 1e-390); a kernel that
    multiplies them unscaled, or inherits the zeroed b_n of modal.hip, gives zeros, infinities or NaN here."""
    import emagls_amd as E
    t = np.load(GOLDEN)
    fs, r, nfft, rho = float(t["fs"]), float(t["r"]), int(t["nfft"]), t["rho"]
    assert nfft == 1024 and np.array_equal(rho, [1.2 * r, 3 * r, 1.0, 20.0])
    src = np.column_stack([t["dirs"], [0.0, 3.25, 17.5, 466.5], [1.0, -0.7, 0.4, 5.0]])
    got = E.getArrayIrs([src], fs, nfft, PRE, r, t["mics"], order=order, nfft=nfft, distance=[rho])
    assert got.shape == (1, nfft, 2) and np.isfinite(got).all()
    k = np.arange(nfft // 2 + 1)
    d = src[:, 2] + PRE
    di = np.floor(d).astype(np.int64)                                         # (the integer part times k modulo nfft in integers: exact)
    ph = src[:, 3][:, None] * np.exp(-2j * np.pi * ((di[:, None] * k[None, :]) % nfft + (d - di)[:, None] * k[None, :]) / nfft)     # [4 x P]
    want = np.einsum("jk,jkm->km", ph, t["resp%d" % order])
    want[0], want[-1] = want[0].real, want[-1].real
    low = np.abs(want[1:6]).min()
    assert low > 0.1 * np.abs(want).max()                                                  # the low bins carry the answer
    check(2, "order %d, all 513 bins" % order, np.fft.rfft(got[0], axis=0), want)


# ---- 3. the long transform
@gpu
def test_long_transform_through_hipfft():
    """nfft 65536: bin 1 has kappa r = 5.6e-4, the direct product stays inside FP64 at N = 19.  Delays beyond 2^15 samples: the
    integer part of the phase is exact."""
    import emagls_amd as E
    n = 65536
    mics = mics5()[:2]
    src = np.array([[0.3, 1.2, 40000.25, 1.0], [2.0, 0.7, 123.5, -0.6], [-1.0, 2.2, 60001.75, 0.8]])
    rho = np.array([0.06, 1.5, 25.0])
    got = E.getArrayIrs([src], FS, n, PRE, RADIUS, mics, order=ORDER, nfft=n, distance=[rho])
    assert got.shape == (1, n, 2)
    check(3, "nfft 65536", got, taps(point_legendre(FS, RADIUS, mics, [src], [rho], ORDER, n, PRE), n))


# ---- 4. bin 0 in closed form
@gpu
def test_sum_of_the_taps_is_the_closed_form_at_dc():
    import emagls_amd as E
    sources, dists, _H = listed_case()
    got = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, distance=dists)
    check(4, "sum of the taps", got.sum(axis=1), dc_closed_form(RADIUS, mics5(), sources, dists, ORDER))


# ---- 5. the far field
@gpu
def test_far_field_is_the_plane_wave():
    import emagls_amd as E
    sources, _d, _H = listed_case()
    far = [np.full(s.shape[0], 1.0e7) for s in sources]
    got = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, distance=far)
    plane = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT)
    kappa1 = 2 * np.pi * (FS / NFFT) / 343.0
    check(5, "rho = 1e7 m against the plane wave (x up to 1.5e9)", got, plane, bound=ORDER * (ORDER + 1) / (kappa1 * 1.0e7))


# ---- 6. the spectral gain together with distances
@gpu
def test_spectral_gain_with_distances():
    import emagls_amd as E
    rng = np.random.default_rng(66)
    P = NFFT // 2 + 1
    counts = (5, 0, 40, 70)
    sources = [np.column_stack([random_dirs(rng, J), rng.uniform(0.0, 0.7 * NFFT, J), rng.uniform(-1.0, 1.0, J)]) for J in counts]
    dists = [rng.uniform(1.05 * RADIUS, 30.0, J) for J in counts]
    refl = rng.uniform(-1.0, 1.0, (3, P))
    refl[0] = -np.abs(refl[0])                                  # one surface negative throughout
    refl[1, [5, 77]] = 0.0                                      # an exact zero at two bins
    exps = [rng.integers(0, 6, (J, 3)).astype(np.int32) for J in counts]
    att, paths = rng.uniform(0.0, 0.05, P), [rng.uniform(1.0, 30.0, J) for J in counts]
    got = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, surfaceReflection=refl, exponents=exps, airAttenuation=att,
                        pathLength=paths, distance=dists)
    check(6, "3 surfaces and air", got, taps(point_legendre(FS, RADIUS, mics5(), sources, dists, ORDER, NFFT, PRE, refl, exps, att, paths), NFFT))
    got = E.getArrayIrs(sources, FS, NFFT, PRE, RADIUS, mics5(), order=ORDER, nfft=NFFT, surfaceReflection=refl, exponents=exps, distance=dists)
    check(6, "3 surfaces, no air", got, taps(point_legendre(FS, RADIUS, mics5(), sources, dists, ORDER, NFFT, PRE, refl, exps), NFFT))


# ---- 7. the room
def room_point(walls, air, src=None, pos=None, mics=None, ir_len=1024, pre=16.0, max_delay=400.0, nfft=1024, **kw):
    import emagls_amd as E
    return E.getArrayRoomIrs(A["room"], walls, A["src"] if src is None else src, A["pos"] if pos is None else pos, A["fs"], ir_len, pre, RADIUS,
                             mics5() if mics is None else mics, maxDelay=max_delay, nfft=nfft, airAttenuation=air, waveModel="pointSource", **kw)


@functools.lru_cache(maxsize=None)
def a_point_spectral():
    got = room_point(*data_sheet_room())
    got.setflags(write=False)
    return got


@gpu
def test_room_a_as_point_sources_against_the_definition():
    comps, exps, paths = images_numpy(A["room"], A["src"], A["pos"], A["fs"], 400.0)
    flat, _ = shoebox_numpy(A["room"], BETA, A["src"], A["pos"], A["fs"], 400.0)
    assert flat.shape == comps.shape == (136, 4) and np.array_equal(flat[:, 2], comps[:, 2])       # no wall of BETA is 0: the same list
    got, counts = room_point(BETA, None, returnCounts=True)
    assert list(counts) == [136] and got.shape == (1, 1024, 5)
    check(7, "A at 400, flat walls", got, taps(point_legendre(A["fs"], RADIUS, mics5(), [flat], [paths], 4, 1024, 16.0), 1024))
    walls, air = data_sheet_room()
    want = point_legendre(A["fs"], RADIUS, mics5(), [comps], [paths], 4, 1024, 16.0, walls, [exps], air, [paths])
    check(7, "A at 400, data-sheet walls and air", a_point_spectral(), taps(want, 1024))
    import emagls_amd as E
    plane = E.getArrayRoomIrs(A["room"], BETA, A["src"], A["pos"], A["fs"], 1024, 16.0, RADIUS, mics5(), maxDelay=400.0, nfft=1024)
    assert rel(got, plane) > 1e-3                                             # the direct sound at 1.18 m is not a plane wave


@gpu
def test_room_mirror_image_in_y():
    walls, air = data_sheet_room()
    Ly = A["room"][1]
    flip = lambda p: (p[0], Ly - p[1], p[2])   # noqa: E731
    got = room_point(walls[[0, 1, 3, 2, 4, 5]], air, src=flip(A["src"]), pos=flip(A["pos"]), mics=mics5() * np.array([-1.0, 1.0]))
    check(8, "A against its mirror image in y", got, a_point_spectral())


def fused_and_listed(walls, air, src, pos=None, **kw):
    """The fused room call against the listed one on the lists the library returns; bit for bit."""
    import emagls_amd as E
    pos = A["pos"] if pos is None else pos
    fused, counts = room_point(walls, air, src=src, pos=pos, returnCounts=True, **kw)
    again = room_point(walls, air, src=src, pos=pos, **kw)
    assert np.array_equal(fused, again)                                       # two equal calls give equal bits
    lk = {k: v for k, v in kw.items() if k in ("encoder", "nfft")}
    md, n, pre = kw.get("max_delay", 400.0), kw.get("ir_len", 1024), kw.get("pre", 16.0)
    if np.ndim(walls) == 2 or air is not None:
        cs, es, ps = E.getShoeboxImages(A["room"], src, pos, A["fs"], md)
        w = walls if np.ndim(walls) == 2 else np.repeat(np.array(walls)[:, None], lk["nfft"] // 2 + 1, axis=1)
        listed = E.getArrayIrs(cs, A["fs"], n, pre, RADIUS, kw.get("mics", mics5()), surfaceReflection=w, exponents=es, airAttenuation=air,
                               pathLength=ps if air is not None else None, distance=ps, **lk)
    else:
        cs, ps = E.getShoeboxComponents(A["room"], walls, src, pos, A["fs"], md, returnDistance=True)
        listed = E.getArrayIrs(cs, A["fs"], n, pre, RADIUS, kw.get("mics", mics5()), distance=ps, **lk)
    assert list(counts) == [c.shape[0] for c in cs]
    assert fused.shape == listed.shape and fused.dtype == listed.dtype and np.abs(listed).max() > 0
    assert np.array_equal(fused, listed)
    return fused, counts


@gpu
@pytest.mark.parametrize("encoder", ["raw", "complex"])
@pytest.mark.parametrize("nfft", [1024, 8192])                               # the LDS transform and hipFFT
def test_fused_equals_listed_on_room_a(encoder, nfft):
    rng = np.random.default_rng(41)
    enc = None if encoder == "raw" else rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))
    import emagls_amd as E
    walls, air = E.wallReflectionSpectra(np.linspace(0.02, 0.6, 36).reshape(6, 6), (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0), A["fs"], nfft), \
        E.airAttenuation(A["fs"], nfft)
    fused, counts = fused_and_listed(BETA, None, [A["src"]], ir_len=512, nfft=nfft, encoder=enc)
    assert list(counts) == [136] and fused.shape == (1, 512, 5 if enc is None else 4) and np.iscomplexobj(fused) == (encoder == "complex")
    fused_and_listed(walls, air, [A["src"]], ir_len=512, nfft=nfft, encoder=enc)
    fused_and_listed(BETA, air, [A["src"]], ir_len=512, nfft=nfft, encoder=enc)                  # six coefficients repeated over the bins


@gpu
@pytest.mark.parametrize("spectral", [False, True])
def test_both_kernel_forms_and_an_empty_source_in_one_call(spectral):
    """The array in the corner of room A (the head of tests/test_gpu_array_room_irs.py): 8, 0 and 32 components.  And source q of a
    call equals the call with it alone."""
    import emagls_amd as E
    walls, air = (E.wallReflectionSpectra(np.linspace(0.02, 0.6, 36).reshape(6, 6), (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0), A["fs"], 512),
                  E.airAttenuation(A["fs"], 512)) if spectral else (BETA, None)
    src, pos = [(0.75, 0.3, 0.75), (3.0, 2.2, 2.6), (0.3, 1.9, 2.55), A["src"]], (0.1, 0.1, 0.1)
    kw = dict(ir_len=256, pre=8.0, max_delay=200.0, nfft=512)
    fused, counts = fused_and_listed(walls, air, src, pos=pos, **kw)
    assert list(counts[:3]) == [8, 0, 32] and 0 < counts[0] <= 16 < counts[2]
    assert not fused[1].any() and fused[0].any() and fused[2].any()
    for q in range(4):
        alone = room_point(walls, air, src=src[q], pos=pos, **kw)
        assert np.array_equal(alone[0], fused[q]), q


@gpu
def test_return_distance_is_the_images_path_and_keeps_the_columns():
    import emagls_amd as E
    src = [A["src"], (0.15, 0.2, 2.5), (2.5, 1.0, 1.0)]
    cs, ds = E.getShoeboxComponents(A["room"], ONES, src, A["pos"], A["fs"], 400.0, returnDistance=True)
    ic, _ie, ip = E.getShoeboxImages(A["room"], src, A["pos"], A["fs"], 400.0)
    plain = E.getShoeboxComponents(A["room"], ONES, src, A["pos"], A["fs"], 400.0)
    for q in range(3):
        assert ds[q].shape == (cs[q].shape[0],) and np.array_equal(ds[q], ip[q]) and np.array_equal(cs[q], ic[q]) and np.array_equal(cs[q], plain[q])
    cs, ds = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], A["fs"], 400.0, returnDistance=True)
    plain = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], A["fs"], 400.0)
    for q in range(3):
        assert np.array_equal(cs[q], plain[q])                                # the four columns keep their bits
        assert cs[q].shape[0] == 0 or np.abs(ds[q] / (cs[q][:, 2] * 343.0 / A["fs"]) - 1).max() < 1e-15
    e0, d0 = E.getShoeboxComponents(A["room"], BETA, (0.15, 0.2, 2.5), A["pos"], A["fs"], 100.0, returnDistance=True)
    assert e0[0].shape == (0, 4) and d0[0].shape == (0,)                      # a source without a component
