"""The spectral shoebox room on the GPU (getShoeboxImages, getArrayRoomIrs with wallReflection [6 x P] and airAttenuation;
DESIGN.md section 13).  Rooms A and B, the walls BETA, the five microphones and the radius are those of
tests/test_gpu_array_room_irs.py.  The images are restated here in NumPy (images_numpy): shoebox_numpy with all six coefficients 1
gives the four columns and asserts that no candidate lies within 1e-9 relative of the cut-off (with walls of 1 no gain is 0, so its
"gain != 0" rule drops nothing), and the exponents and the kept set are enumerated again beside it.  Counts with the gain rule
dropped: A at 400 samples 136 (largest exponent 2), the corner case of A at 200 samples 8 / 0 / 32, B at 6000 samples 5346
(largest exponent 7, longest path 42.9 m).

The NumPy side of the responses forms G with direct powers (spectral_legendre of tests/test_gpu_array_irs_spectral.py).  Bounds:
ten times the figure measured on an MI355X, relative to the largest expected magnitude, and in no case above 1e-11.

    test                                              measured    bound
    6  flat spectra against the flat room             2.18e-16    2.18e-15
    7  A at 400, nfft 1024, data-sheet walls and air  1.24e-14    1.24e-13
    8  A against its mirror image in y                1.90e-14    1.90e-13
    10 one reflecting wall, R rising 0.2 to 0.9       2.71e-14    2.71e-13
"""
import functools

import numpy as np
import pytest

from test_gpu_array_irs_spectral import spectral_legendre  # noqa: E402
from test_gpu_array_room_irs import A, A_BANK, A_BY_ORDER, B, BETA, MIRRORS, RADIUS, mics5, shoebox_numpy  # noqa: E402

gpu = pytest.mark.gpu
ONES = (1.0,) * 6
BOUND = {6: 2.18e-15, 7: 1.24e-13, 8: 1.90e-13, 10: 2.71e-13}
BANDS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
ABSORPTION = np.array([[0.02, 0.03, 0.04, 0.05, 0.07, 0.09],       # six different rows: painted concrete, carpet, glass, panel, ...
                       [0.08, 0.24, 0.57, 0.69, 0.71, 0.73],
                       [0.35, 0.25, 0.18, 0.12, 0.07, 0.04],
                       [0.28, 0.22, 0.17, 0.09, 0.10, 0.11],
                       [0.01, 0.02, 0.06, 0.15, 0.25, 0.45],
                       [0.45, 0.55, 0.60, 0.90, 0.86, 0.75]])


def images_numpy(room, src, pos, fs, max_delay, max_order=None):
    """The images of one source: ([J x 4] (azi, zen, delay, 1 / d), [J x 6] exponents, [J] paths) in the definition's order."""
    comps, _ = shoebox_numpy(room, ONES, src, pos, fs, max_delay, max_order)        # (asserts the cut-off margin)
    L, s, a = (np.asarray(v, dtype=np.float64) for v in (room, src, pos))
    box = [int(np.floor(max_delay * 343.0 / fs / (2 * L[i]))) + 1 for i in range(3)]
    if max_order is not None:
        box = [min(b, (max_order + 1) // 2) for b in box]
    ax = [np.arange(-b, b + 1) for b in box]
    nz, ny, nx, pz, py, px = (g.ravel() for g in np.meshgrid(ax[2], ax[1], ax[0], [0, 1], [0, 1], [0, 1], indexing="ij"))
    e, v = [], []
    for i, (n, p) in enumerate(((nx, px), (ny, py), (nz, pz))):
        e += [np.abs(n - p), np.abs(n)]
        v.append(((1 - 2 * p) * s[i] + 2 * n * L[i]) - a[i])
    d = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    e = np.column_stack(e)
    keep = d / 343.0 * fs <= max_delay
    if max_order is not None:
        keep &= e.sum(axis=1) <= max_order
    assert keep.sum() == comps.shape[0]
    return comps, e[keep].astype(np.int32), d[keep]


def check(family, what, got, want):
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print("array_room_spectral test %s: %.3g (bound %.3g)" % (what, e, BOUND[family]))
    assert e < BOUND[family], (what, e)


@functools.lru_cache(maxsize=None)
def data_sheet_room():
    """Walls from absorption rows and the air of 20 degrees and 50 percent, at fs 16000 and nfft 1024."""
    import emagls_amd as E
    w, a = E.wallReflectionSpectra(ABSORPTION, BANDS, 16000.0, 1024), E.airAttenuation(16000.0, 1024)
    assert w.shape == (6, 513) and a.shape == (513,) and len({tuple(r) for r in w}) == 6
    w.setflags(write=False)
    a.setflags(write=False)
    return w, a


def room_irs(case, walls, air, src=None, pos=None, mics=None, ir_len=1024, pre=16.0, max_delay=400.0, nfft=1024, **kw):
    import emagls_amd as E
    return E.getArrayRoomIrs(case["room"], walls, case["src"] if src is None else src, case["pos"] if pos is None else pos, case["fs"], ir_len,
                             pre, RADIUS, mics5() if mics is None else mics, maxDelay=max_delay, nfft=nfft, airAttenuation=air, **kw)


@functools.lru_cache(maxsize=None)
def a_spectral():
    got = room_irs(A, *data_sheet_room())
    got.setflags(write=False)
    return got


# ---- 5. images
@gpu
def test_images_of_room_a():
    import emagls_amd as E
    (c,), (e,), (p,) = E.getShoeboxImages(A["room"], A["src"], A["pos"], A["fs"], 400.0)
    want_c, want_e, want_p = images_numpy(A["room"], A["src"], A["pos"], A["fs"], 400.0)
    assert c.shape == (136, 4) and e.shape == (136, 6) and e.dtype == np.int32 and p.shape == (136,)
    flat, = E.getShoeboxComponents(A["room"], ONES, A["src"], A["pos"], A["fs"], 400.0)
    assert np.array_equal(c, flat)                                   # the bits of today's list with walls of 1
    assert np.array_equal(e, want_e) and e.max() == 2
    assert np.array_equal(c[:, 2], p / 343.0 * A["fs"]) and np.array_equal(c[:, 3], 1.0 / p)
    assert np.abs(p / want_p - 1).max() < 1e-13 and np.abs(c[:, 2] / want_c[:, 2] - 1).max() < 1e-13


@gpu
@pytest.mark.parametrize("max_order,count", sorted(A_BY_ORDER.items()))
def test_images_of_room_a_by_order(max_order, count):
    import emagls_amd as E
    (c,), (e,), (p,) = E.getShoeboxImages(A["room"], A["src"], A["pos"], A["fs"], 400.0, maxOrder=max_order)
    _c, want_e, _p = images_numpy(A["room"], A["src"], A["pos"], A["fs"], 400.0, max_order)
    assert c.shape[0] == count and np.array_equal(e, want_e) and e.sum(axis=1).max() == max_order


@gpu
def test_images_of_several_sources_and_an_empty_one_between_them():
    """Room A at 100 samples (2.14 m): the source (0.15, 0.2, 2.5) is 2.59 m from the array and has no image."""
    import emagls_amd as E
    src = [A["src"], (0.15, 0.2, 2.5), (2.5, 1.0, 1.0), A_BANK[3]]
    cs, es, ps = E.getShoeboxImages(A["room"], src, A["pos"], A["fs"], 100.0)
    assert [c.shape[0] for c in cs][:3] == [1, 0, 2] and es[1].shape == (0, 6) and ps[1].shape == (0,)
    for q in range(4):
        want_c, want_e, want_p = images_numpy(A["room"], src[q], A["pos"], A["fs"], 100.0)
        assert np.array_equal(es[q], want_e) and cs[q].shape == want_c.shape
        (c,), (e,), (p,) = E.getShoeboxImages(A["room"], src[q], A["pos"], A["fs"], 100.0)                # the source alone
        assert np.array_equal(c, cs[q]) and np.array_equal(e, es[q]) and np.array_equal(p, ps[q])


# ---- 6. flat spectra reproduce the flat room
@gpu
def test_flat_spectra_reproduce_the_flat_room():
    import emagls_amd as E
    flat = E.getArrayRoomIrs(A["room"], BETA, A["src"], A["pos"], A["fs"], 1024, 16.0, RADIUS, mics5(), maxDelay=400.0, nfft=1024)
    got, counts = room_irs(A, np.repeat(np.array(BETA)[:, None], 513, axis=1), None, returnCounts=True)
    assert list(counts) == [136] and got.shape == flat.shape == (1, 1024, 5)
    check(6, "6 flat spectra against the flat room", got, flat)


# ---- 7. the spectral room against the definition
@gpu
def test_spectral_room_against_the_definition():
    walls, air = data_sheet_room()
    comps, exps, paths = images_numpy(A["room"], A["src"], A["pos"], A["fs"], 400.0)
    want = np.fft.irfft(spectral_legendre(A["fs"], RADIUS, mics5(), [comps], 4, 1024, 16.0, walls, [exps], air, [paths]), n=1024, axis=1)
    check(7, "7 A at 400 against the definition", a_spectral(), want)


@gpu
def test_six_coefficients_with_air_are_repeated_over_the_bins():
    _w, air = data_sheet_room()
    got = room_irs(A, BETA, air)
    assert np.array_equal(got, room_irs(A, np.repeat(np.array(BETA)[:, None], 513, axis=1), air))
    comps, exps, paths = images_numpy(A["room"], A["src"], A["pos"], A["fs"], 400.0)
    walls = np.repeat(np.array(BETA)[:, None], 513, axis=1)
    want = np.fft.irfft(spectral_legendre(A["fs"], RADIUS, mics5(), [comps], 4, 1024, 16.0, walls, [exps], air, [paths]), n=1024, axis=1)
    check(7, "7 flat walls with air", got, want)


# ---- 8. mirror symmetry
@gpu
def test_mirror_image_in_y():
    """Room A mirrored in y: the two y walls' spectra swap, y -> Ly - y for source and array, the microphones' azimuths change sign.
    An exponent assigned to the wrong wall shows here."""
    walls, air = data_sheet_room()
    Ly = A["room"][1]
    flip = lambda p: (p[0], Ly - p[1], p[2])   # noqa: E731
    got = room_irs(A, walls[[0, 1, 3, 2, 4, 5]], air, src=flip(A["src"]), pos=flip(A["pos"]), mics=mics5() * np.array([-1.0, 1.0]))
    check(8, "8 A against its mirror image in y", got, a_spectral())


# ---- 9. fused equals listed, bit for bit
def fused_and_listed(case, walls, air, src, max_delay, ir_len, pre, mics, nfft, pos=None, **kw):
    import emagls_amd as E
    pos = case["pos"] if pos is None else pos
    fused, counts = room_irs(case, walls, air, src=src, pos=pos, mics=mics, ir_len=ir_len, pre=pre, max_delay=max_delay, nfft=nfft,
                             returnCounts=True, **kw)
    cs, es, ps = E.getShoeboxImages(case["room"], src, pos, case["fs"], max_delay)
    listed = E.getArrayIrs(cs, case["fs"], ir_len, pre, RADIUS, mics, nfft=nfft, surfaceReflection=walls, exponents=es, airAttenuation=air,
                           pathLength=ps if air is not None else None, **kw)
    assert list(counts) == [c.shape[0] for c in cs]
    assert fused.shape == listed.shape and fused.dtype == listed.dtype and np.abs(listed).max() > 0
    assert np.array_equal(fused, listed)
    return fused, counts, es, ps


@gpu
@pytest.mark.parametrize("encoder", ["raw", "complex"])
def test_fused_equals_listed_on_room_a(encoder):
    rng = np.random.default_rng(41)
    enc = None if encoder == "raw" else rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))
    walls, air = data_sheet_room()
    fused, counts, _e, _p = fused_and_listed(A, walls, air, [A["src"]], 400.0, 512, 16.0, mics5(), 1024, encoder=enc)
    assert list(counts) == [136] and fused.shape == (1, 512, 5 if enc is None else 4) and np.iscomplexobj(fused) == (encoder == "complex")
    fused_and_listed(A, walls, None, [A["src"]], 400.0, 512, 16.0, mics5(), 1024, encoder=enc)              # and without the air term


@gpu
def test_fused_equals_listed_on_room_b_through_hipfft():
    import emagls_amd as E
    walls, air = E.wallReflectionSpectra(ABSORPTION, BANDS, B["fs"], 8192), E.airAttenuation(B["fs"], 8192)
    src = [B["src"], (2.1, 3.3, 1.9), (4.6, 0.8, 0.7)]
    fused, counts, es, ps = fused_and_listed(B, walls, air, src, 6000.0, 6100, 64.0, mics5()[:4], 8192)
    assert list(counts) == [5346, 5330, 5314] and fused.shape == (3, 6100, 4)
    assert es[0].max() == 7 and 42.8 < ps[0].max() < 43.0


@gpu
def test_both_kernel_forms_and_an_empty_source_in_one_call():
    """The array in the corner of room A (the head of tests/test_gpu_array_room_irs.py).  And source q of a call equals the call
    with it alone."""
    import emagls_amd as E
    walls, air = E.wallReflectionSpectra(ABSORPTION, BANDS, A["fs"], 512), E.airAttenuation(A["fs"], 512)
    src, pos = [(0.75, 0.3, 0.75), (3.0, 2.2, 2.6), (0.3, 1.9, 2.55), A["src"]], (0.1, 0.1, 0.1)
    fused, counts, _e, _p = fused_and_listed(A, walls, air, src, 200.0, 256, 8.0, mics5(), 512, pos=pos)
    assert list(counts[:3]) == [8, 0, 32] and 0 < counts[0] <= 16 < counts[2]
    assert not fused[1].any() and fused[0].any() and fused[2].any()
    for q in range(4):
        alone = room_irs(A, walls, air, src=src[q], pos=pos, ir_len=256, pre=8.0, max_delay=200.0, nfft=512)
        assert np.array_equal(alone[0], fused[q]), q


# ---- 10. one reflecting wall
@gpu
@pytest.mark.parametrize("wall,image", MIRRORS)
def test_one_reflecting_wall(wall, image):
    """Five walls are 0 in every bin, one rises linearly from 0.2 to 0.9: the direct sound and one reflection (every image is
    enumerated -- 136 of them -- and all but two have a gain of exactly 0)."""
    walls = np.zeros((6, 513))
    walls[wall] = np.linspace(0.2, 0.9, 513)
    got, counts = room_irs(A, walls, None, returnCounts=True)
    assert list(counts) == [136]

    def comp(p):
        v = np.array(p) - np.array(A["pos"])
        d = float(np.sqrt(v @ v))
        return [np.arctan2(v[1], v[0]), np.arccos(v[2] / d), d / 343.0 * A["fs"], 1.0 / d]

    two = np.array([comp(A["src"]), comp(image)])
    want = spectral_legendre(A["fs"], RADIUS, mics5(), [two], 4, 1024, 16.0, walls[wall:wall + 1], [np.array([[0], [1]])])
    check(10, "10 wall %d alone" % wall, got, np.fft.irfft(want, n=1024, axis=1))
