"""Shoebox image sources on the GPU (getShoeboxComponents, getArrayRoomIrs).  The definition is restated
here in NumPy (shoebox_numpy); every comparison with it first asserts, on the NumPy side, that no candidate's delay lies within
1e-9 relative of max_delay, so that device and NumPy cannot disagree about a candidate on the cut-off (measured margins: 3.65e-4
for room A at 400 samples, 1.19e-6 for room B at 6000).

    room A   (3.1, 2.3, 2.7) m, source (1.13, 0.71, 1.52), array (2.02, 1.41, 1.17), fs 16000
    room B   (5.2, 4.1, 2.9) m, source (1.3, 2.2, 1.1),    array (3.4, 1.7, 1.6),    fs 48000
    walls    0.9, 0.85, 0.8, 0.75, 0.7, 0.6 (x=0, x=Lx, y=0, y=Ly, z=0, z=Lz); microphones at 4.2 cm

Bounds.  Lists: delay and gain 1e-13 relative, azi (modulo 2 pi) and zen 1e-12 absolute; counts and order exact.  Fused against
listed, source alone against source in a call, and the chain of streams: bit for bit.  Responses against NumPy (tests 5 and 6):
ten times the figure measured on an MI355X, relative to the largest expected magnitude, and in no case above 1e-11 (a delay off
by a few ulp at 400 samples, 6e-14, times pi per sample at the last bin is some 5e-13 per component).

    test                                              measured    bound
    5  room A at 400, nfft 1024, Legendre form        1.05e-14    1.05e-13
    6  room A against its mirror image in y           9.84e-15    the bound of test 5

One case departs from its issue's wording.  "One call on A with max_delay near 190 and an empty source next to sources of at most
16 and of more than 16 components" cannot be had with A's array: no point of room A is farther than 2.90 m (135 samples) from
(2.02, 1.41, 1.17), and the direct sound is the earliest component.  The case keeps A's room and walls and moves the array into
the corner (0.1, 0.1, 0.1), at max_delay 200: the source (3.0, 2.2, 2.6) is 203.7 samples away (empty), (0.75, 0.3, 0.75) has 8
components and (0.3, 1.9, 2.55) has 32.  The test asserts these counts from the library's own return, so both kernel forms and
the empty source do meet in that call.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

from test_gpu_array_irs import legendre_spectra, random_dirs  # noqa: E402  (the Legendre form of the definition of section 11)

gpu = pytest.mark.gpu

BETA = (0.9, 0.85, 0.8, 0.75, 0.7, 0.6)
A = dict(room=(3.1, 2.3, 2.7), beta=BETA, src=(1.13, 0.71, 1.52), pos=(2.02, 1.41, 1.17), fs=16000.0)
B = dict(room=(5.2, 4.1, 2.9), beta=BETA, src=(1.3, 2.2, 1.1), pos=(3.4, 1.7, 1.6), fs=48000.0)
RADIUS = 0.042
BOUND_RESPONSES = 1.05e-13
A_BY_DELAY = {40: 0, 60: 1, 130: 3, 150: 6, 180: 13, 200: 20, 400: 136}
A_BY_ORDER = {0: 1, 1: 7, 2: 25, 3: 61}
A_BANK = ((1.13, 0.71, 1.52), (1.4, 0.9, 1.3), (1.7, 1.1, 1.1), (2.3, 1.9, 2.0))      # 136, 132, 138, 135 components at 400


def shoebox_numpy(room, beta, src, pos, fs, max_delay, max_order=None):
    """The definition of DESIGN.md section 12 for one source: ([J x 4] (azi, zen, delay, gain) in the definition's order, the
    number of candidates).  Asserts that no candidate lies within 1e-9 relative of the cut-off."""
    L, beta, s, a = (np.asarray(v, dtype=np.float64) for v in (room, beta, src, pos))
    reach = max_delay * 343.0 / fs
    box = [int(np.floor(reach / (2 * L[i]))) + 1 for i in range(3)]
    if max_order is not None:
        box = [min(b, (max_order + 1) // 2) for b in box]
    ax = [np.arange(-b, b + 1) for b in box]
    nz, ny, nx, pz, py, px = (g.ravel() for g in np.meshgrid(ax[2], ax[1], ax[0], [0, 1], [0, 1], [0, 1], indexing="ij"))   # ascending (nz, ny, nx, pz, py, px)
    g, order, v = np.ones(nx.size), np.zeros(nx.size, dtype=np.int64), []
    for i, (n, p) in enumerate(((nx, px), (ny, py), (nz, pz))):
        e0, e1 = np.abs(n - p), np.abs(n)
        order += e0 + e1
        g = g * beta[2 * i] ** e0 * beta[2 * i + 1] ** e1             # (numpy: 0.0 ** 0 = 1)
        v.append(((1 - 2 * p) * s[i] + 2 * n * L[i]) - a[i])
    d = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    tau, g = d / 343.0 * fs, g / d
    margin = float(np.abs(tau / max_delay - 1.0).min())
    assert margin > 1e-9, "a candidate on the cut-off (%.3g relative): move max_delay" % margin
    keep = (g != 0.0) & (tau <= max_delay)
    if max_order is not None:
        keep &= order <= max_order
    return np.column_stack([np.arctan2(v[1], v[0]), np.arccos(v[2] / d), tau, g])[keep], nx.size


def compare_lists(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)     # the count; the order follows from the values below
    if want.shape[0] == 0:
        return
    e_d, e_g = np.abs(got[:, 2] / want[:, 2] - 1).max(), np.abs(got[:, 3] / want[:, 3] - 1).max()
    e_a = np.abs(np.angle(np.exp(1j * (got[:, 0] - want[:, 0])))).max()
    e_z = np.abs(got[:, 1] - want[:, 1]).max()
    print("shoebox %s: %d components, delay %.3g gain %.3g (rel), azi %.3g zen %.3g (abs)" % (what, want.shape[0], e_d, e_g, e_a, e_z))
    assert e_d < 1e-13 and e_g < 1e-13 and e_a < 1e-12 and e_z < 1e-12, what


def components(case, max_delay, max_order=None, src=None, pos=None):
    import emagls_amd as E
    return E.getShoeboxComponents(case["room"], case["beta"], case["src"] if src is None else src, case["pos"] if pos is None else pos,
                                  case["fs"], max_delay, maxOrder=max_order)


@functools.lru_cache(maxsize=None)
def a_at_400():
    """The library's list of room A at 400 samples (tests 3 and 4 share it)."""
    c, = components(A, 400.0)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def mics5():
    m = random_dirs(np.random.default_rng(12), 5)
    m.setflags(write=False)
    return m


# ---- 1. components against NumPy
@gpu
@pytest.mark.parametrize("max_delay,count", sorted(A_BY_DELAY.items()))
def test_components_of_room_a_by_delay(max_delay, count):
    want, ncand = shoebox_numpy(max_delay=float(max_delay), **A)
    assert want.shape[0] == count and ncand == (1000 if max_delay == 400 else 216)
    got, = components(A, float(max_delay))
    compare_lists("A at %d" % max_delay, got, want)


@gpu
@pytest.mark.parametrize("max_order,count", sorted(A_BY_ORDER.items()))
def test_components_of_room_a_by_order(max_order, count):
    want, _ = shoebox_numpy(max_delay=400.0, max_order=max_order, **A)
    assert want.shape[0] == count
    got, = components(A, 400.0, max_order)
    compare_lists("A at 400, order <= %d" % max_order, got, want)


@gpu
def test_components_of_room_b():
    want, ncand = shoebox_numpy(max_delay=6000.0, **B)
    assert want.shape[0] == 5346 and ncand == 19448
    got, = components(B, 6000.0)
    compare_lists("B at 6000", got, want)


@gpu
def test_several_sources_and_an_empty_one_between_them():
    """Room A at 100 samples (2.14 m): the source (0.15, 0.2, 2.5) is 2.59 m from the array and has no component."""
    src = [A["src"], (0.15, 0.2, 2.5), (2.5, 1.0, 1.0), A_BANK[3]]
    want = [shoebox_numpy(**dict(A, src=s), max_delay=100.0)[0] for s in src]
    assert [w.shape[0] for w in want][:3] == [1, 0, 2]
    got = components(A, 100.0, src=src)
    assert len(got) == 4
    for q in range(4):
        compare_lists("A at 100, source %d" % q, got[q], want[q])
    at_400 = components(A, 400.0, src=A_BANK)                      # and four full lists in one call
    for q in range(4):
        compare_lists("A at 400, source %d" % q, at_400[q], shoebox_numpy(**dict(A, src=A_BANK[q]), max_delay=400.0)[0])
    assert np.array_equal(at_400[0], a_at_400())                    # source 0 of the call: the bits of the call with it alone


# ---- 2. walls by closed form
#                wall    the source's mirror image across it (written out by hand from source (1.13, 0.71, 1.52) and room (3.1, 2.3, 2.7))
MIRRORS = [(0, (-1.13, 0.71, 1.52)), (1, (5.07, 0.71, 1.52)), (2, (1.13, -0.71, 1.52)), (3, (1.13, 3.89, 1.52)), (4, (1.13, 0.71, -1.52)),
           (5, (1.13, 0.71, 3.88))]


def by_hand(image, gain):
    v = [image[i] - A["pos"][i] for i in range(3)]
    d = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return [math.atan2(v[1], v[0]), math.acos(v[2] / d), d / 343.0 * 16000.0, gain / d]


@gpu
@pytest.mark.parametrize("wall,image", MIRRORS)
@pytest.mark.parametrize("coeff", [0.5, -0.5])
def test_one_reflecting_wall(wall, image, coeff):
    import emagls_amd as E
    beta = [0.0] * 6
    beta[wall] = coeff
    got, = E.getShoeboxComponents(A["room"], beta, A["src"], A["pos"], A["fs"], 400.0)
    want = np.array([by_hand(A["src"], 1.0), by_hand(image, coeff)])         # the direct sound comes first: n = 0, p = 0
    compare_lists("wall %d at %g" % (wall, coeff), got, want)
    assert np.sign(got[1, 3]) == np.sign(coeff)


@gpu
def test_no_reflecting_wall():
    import emagls_amd as E
    got, = E.getShoeboxComponents(A["room"], [0.0] * 6, A["src"], A["pos"], A["fs"], 400.0)
    compare_lists("all walls at 0", got, np.array([by_hand(A["src"], 1.0)]))


# ---- 3. a delay on the cut-off
def count_only(case, max_delay):
    """emagls_shoebox_components with null arrays and capacity 0."""
    from emagls_amd import _lib as L
    vp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    keep = [np.ascontiguousarray(case[k], dtype=np.float64) for k in ("room", "beta", "pos", "src")]
    ptr = np.zeros(2, dtype=np.int64)
    L.check(L.load().emagls_shoebox_components(vp(keep[0]), vp(keep[1]), vp(keep[2]), 1, vp(keep[3]), case["fs"], float(max_delay), -1, 0,
                                               ptr.ctypes.data_as(ctypes.c_void_p), None, None, None, None))
    return int(ptr[1])


@gpu
@pytest.mark.parametrize("k", [0, 1, 50, 135])
def test_a_delay_on_the_cut_off(k):
    """max_delay equal to the delay of the k-th earliest component: that component is kept (<=), and the count is the number of
    delays up to it -- in the count-only call and in the call that fills."""
    delays = a_at_400()[:, 2]
    cut = float(np.sort(delays)[k])
    n = int((delays <= cut).sum())
    assert n >= k + 1
    got, = components(A, cut)
    assert got.shape[0] == n and count_only(A, cut) == n
    assert got[:, 2].max() == cut
    assert np.array_equal(got, a_at_400()[delays <= cut])          # the same components, in the same order, with the same bits


# ---- 4. fused equals listed, bit for bit
def fused_and_listed(case, src, max_delay, ir_len, pre, mics, pos=None, **kw):
    import emagls_amd as E
    pos = case["pos"] if pos is None else pos
    fused, counts = E.getArrayRoomIrs(case["room"], case["beta"], src, pos, case["fs"], ir_len, pre, RADIUS, mics, maxDelay=max_delay,
                                      returnCounts=True, **kw)
    lists = E.getShoeboxComponents(case["room"], case["beta"], src, pos, case["fs"], max_delay)
    listed = E.getArrayIrs(lists, case["fs"], ir_len, pre, RADIUS, mics, **kw)
    assert list(counts) == [c.shape[0] for c in lists]
    assert fused.shape == listed.shape and fused.dtype == listed.dtype and np.abs(listed).max() > 0
    assert np.array_equal(fused, listed)
    return fused, counts


@gpu
@pytest.mark.parametrize("encoder", ["raw", "real", "complex"])
def test_fused_equals_listed_on_room_a(encoder):
    rng = np.random.default_rng(41)
    enc = {"raw": None, "real": rng.standard_normal((4, 5)), "complex": rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))}[encoder]
    fused, counts = fused_and_listed(A, [A["src"]], 400.0, 512, 16.0, mics5(), nfft=1024, encoder=enc)
    assert list(counts) == [136] and fused.shape == (1, 512, 5 if enc is None else 4) and np.iscomplexobj(fused) == (encoder == "complex")


@gpu
def test_fused_equals_listed_on_room_b_through_hipfft():
    src = [B["src"], (2.1, 3.3, 1.9), (4.6, 0.8, 0.7)]
    fused, counts = fused_and_listed(B, src, 6000.0, 6100, 64.0, mics5()[:4], nfft=8192)
    assert list(counts) == [5346, 5330, 5314] and fused.shape == (3, 6100, 4)


@gpu
def test_both_kernel_forms_and_an_empty_source_in_one_call():
    """(The array in the corner of room A: see the head of this file.)  And source q of a call equals the call with it alone."""
    import emagls_amd as E
    src, pos = [(0.75, 0.3, 0.75), (3.0, 2.2, 2.6), (0.3, 1.9, 2.55), A["src"]], (0.1, 0.1, 0.1)
    fused, counts = fused_and_listed(A, src, 200.0, 256, 8.0, mics5(), pos=pos, nfft=512)
    assert list(counts[:3]) == [8, 0, 32] and 0 < counts[0] <= 16 < counts[2]
    assert not fused[1].any() and fused[0].any() and fused[2].any()
    for q in range(4):
        alone = E.getArrayRoomIrs(A["room"], A["beta"], src[q], pos, A["fs"], 256, 8.0, RADIUS, mics5(), maxDelay=200.0, nfft=512)
        assert np.array_equal(alone[0], fused[q]), q


# ---- 5. responses against NumPy
def check_responses(what, got, want):
    e = float(np.abs(got - want).max() / np.abs(want).max())
    print("array_room_irs %s: %.3g (bound %.3g)" % (what, e, BOUND_RESPONSES))
    assert e < BOUND_RESPONSES, (what, e)


@functools.lru_cache(maxsize=None)
def a_responses():
    import emagls_amd as E
    got = E.getArrayRoomIrs(A["room"], A["beta"], A["src"], A["pos"], A["fs"], 1024, 16.0, RADIUS, mics5(), maxDelay=400.0, nfft=1024)
    got.setflags(write=False)
    return got


@gpu
def test_responses_against_the_legendre_form():
    comps, _ = shoebox_numpy(max_delay=400.0, **A)
    want = np.fft.irfft(legendre_spectra(A["fs"], RADIUS, mics5(), [comps], 4, 1024, 16.0), n=1024, axis=1)
    got = a_responses()
    assert got.shape == (1, 1024, 5)
    check_responses("A at 400 against the Legendre form", got, want)


# ---- 6. mirror symmetry
@gpu
def test_mirror_image_in_y():
    """Room A mirrored in y: the two y walls swap, y -> Ly - y for source and array, the microphones' azimuths change sign.  The
    responses are the same up to the order of the sums.  A wall assigned to the wrong parity would show here, where a restatement
    by the same hand would share it."""
    import emagls_amd as E
    Ly = A["room"][1]
    beta = (BETA[0], BETA[1], BETA[3], BETA[2], BETA[4], BETA[5])
    flip = lambda p: (p[0], Ly - p[1], p[2])   # noqa: E731
    mics = mics5() * np.array([-1.0, 1.0])
    got = E.getArrayRoomIrs(A["room"], beta, flip(A["src"]), flip(A["pos"]), A["fs"], 1024, 16.0, RADIUS, mics, maxDelay=400.0, nfft=1024)
    check_responses("A against its mirror image in y", got, a_responses())


# ---- 7. through the chain
@gpu
def test_through_the_streams():
    """A bank of four source positions in room A, raw microphones: SourceFieldStream (one set per position, the index changing from
    block to block) and a BinauralDecodeStream with the encoder inside.  Fed by the fused call and by the listed one, the chain
    gives the same bits."""
    import emagls_amd as E
    rng = np.random.default_rng(7)
    mics = mics5()
    fused = E.getArrayRoomIrs(A["room"], A["beta"], A_BANK, A["pos"], A["fs"], 448, 16.0, RADIUS, mics, maxDelay=400.0, nfft=1024)
    listed = E.getArrayIrs(E.getShoeboxComponents(A["room"], A["beta"], A_BANK, A["pos"], A["fs"], 400.0), A["fs"], 448, 16.0, RADIUS, mics,
                           nfft=1024)
    assert fused.shape == (4, 448, 5)
    enc = E.arrayEncoder("sma", 1, mics[:, 0], mics[:, 1])
    wL, wR = rng.standard_normal((32, 4)), rng.standard_normal((32, 4))
    sig, sets = rng.standard_normal(64 * 8), np.array([0, 1, 1, 2, 3, 3, 0, 2])
    ears = []
    for irs in (fused, listed):
        with E.SourceFieldStream(irs[:, None], 64) as f, E.BinauralDecodeStream(wL, wR, 64, encoder=enc) as d:
            ears.append(d.push(f.push(sig, setIndex=sets)))
    assert ears[0].shape == (512, 2) and np.abs(ears[0]).max() > 0
    assert np.array_equal(ears[0], ears[1])
