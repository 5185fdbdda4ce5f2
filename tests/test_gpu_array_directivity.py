"""Source directivity and orientation of the array room responses on the GPU (getArrayIrs with emission=, sourceOrientation=,
directivity=; getArrayRoomIrs with the last two; returnEmission of the list functions).

The truth is tests/directivity_reference.py: the enumeration of shoebox_numpy with the parities kept, and the undirected
restatements of sections 11, 13 and 14 per component times D from oracle.getSH(Nd, ., 'real').  Everything runs on room A of
tests/test_gpu_array_room_irs.py (3.1 x 2.3 x 2.7 m, fs 16000, nfft 1024, 136 components at 400 samples, N = 7) with its five random
microphones: an odd count that is no multiple of the four microphones of a wave.  Errors are relative to the largest magnitude of
the expected array; every test prints its figure before it asserts.

Bounds: ten times the figure measured on an MI355X (the table), and emission vectors the lists' existing 1e-13 (measured: 0, the
bits of the NumPy restatement).  The direct-sound
cases of test 3 are the omni case's computation times one real number and hold its bound; their null is held to that bound times
the free-field response's largest tap.

    test                                                     measured    bound
    2  omni, Nd = 0 and padded to Nd = 3                     2.20e-16    2.2e-15 
    4  room A against directive_spectra, 4 models x 2 orders 1.49e-14    1.49e-13
    5  listed call, 0 .. 65 components, the pole             7.93e-15    7.93e-14
    8  quarter turn about z and mirror image in y            2.07e-14    2.07e-13

The mirrored case also negates the sine coefficients (m < 0): the mirror image of a source carries the mirror image of its
pattern, and R' = S R S turns w = R^T e into S w, whose azimuth has the other sign.
"""
import functools

import numpy as np
import pytest

from directivity_reference import directive_spectra, shoebox_emission_numpy
from point_reference import point_legendre
from test_array_directivity_host import ARGS, call
from test_gpu_array_irs import legendre_spectra, random_dirs
from test_gpu_array_irs_spectral import spectral_legendre
from test_gpu_array_room_irs import A, BETA, RADIUS, mics5, shoebox_numpy
from test_gpu_array_room_spectral import ONES, data_sheet_room, images_numpy

gpu = pytest.mark.gpu

FS, NFFT, P, PRE, LEN, DELAY = A["fs"], 1024, 513, 16.0, 1024, 400.0
BOUND = {2: 2.2e-15, 4: 1.49e-13, 5: 7.93e-14, 8: 2.07e-13}
MODELS = ("flat", "spectral", "point", "point_spectral")
CORNER = dict(src=[(0.75, 0.3, 0.75), (3.0, 2.2, 2.6), (0.3, 1.9, 2.55)], pos=(0.1, 0.1, 0.1), max_delay=200.0, nfft=512, ir_len=256, pre=8.0)


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check(family, what, got, want, test=None):
    """family: whose bound holds; test: the number printed, where it is another test's (test 3 holds the bound of test 2)."""
    e = rel(got, want)
    bound = BOUND[family]
    print("array_directivity test %d %s: %.3g (bound %.3g)" % (family if test is None else test, what, e, bound))
    assert np.isfinite(got).all(), what
    assert e < bound, (what, e)


def taps(H, n=NFFT):
    return np.fft.irfft(H, n=n, axis=1)


def rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q if np.linalg.det(q) > 0 else q * np.array([1.0, 1.0, -1.0])


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def coefficients(rng, Q, Nd, nbins=P):
    return rng.standard_normal((Q, (Nd + 1) ** 2, nbins)) + 1j * rng.standard_normal((Q, (Nd + 1) ** 2, nbins))


def walls_of(model, nfft=NFFT):
    """(walls, air, waveModel) of a model."""
    import emagls_amd as E
    wave = "pointSource" if model.startswith("point") else "planeWave"
    if model in ("flat", "point"):
        return BETA, None, wave
    if nfft == NFFT:
        return data_sheet_room() + (wave,)
    return (E.wallReflectionSpectra(np.linspace(0.02, 0.6, 36).reshape(6, 6), (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0), FS, nfft),
            E.airAttenuation(FS, nfft), wave)


def room_irs(model, src=None, pos=None, mics=None, room=None, walls=None, ir_len=LEN, pre=PRE, max_delay=DELAY, nfft=NFFT, **kw):
    import emagls_amd as E
    w, air, wave = walls_of(model, nfft)
    return E.getArrayRoomIrs(A["room"] if room is None else room, w if walls is None else walls, A["src"] if src is None else src,
                             A["pos"] if pos is None else pos, FS, ir_len, pre, RADIUS, mics5() if mics is None else mics, maxDelay=max_delay,
                             nfft=nfft, airAttenuation=air, waveModel=wave, **kw)


def lists_of(model, src, pos, max_delay):
    """The library's lists of a model as the keywords of getArrayIrs: (sources, keywords with emission)."""
    import emagls_amd as E
    if model in ("spectral", "point_spectral"):
        cs, es, ps, em = E.getShoeboxImages(A["room"], src, pos, FS, max_delay, returnEmission=True)
        kw = dict(exponents=es, pathLength=ps, emission=em)
        if model == "point_spectral":
            kw["distance"] = ps
        return cs, kw
    if model == "point":
        cs, ps, em = E.getShoeboxComponents(A["room"], BETA, src, pos, FS, max_delay, returnDistance=True, returnEmission=True)
        return cs, dict(distance=ps, emission=em)
    cs, em = E.getShoeboxComponents(A["room"], BETA, src, pos, FS, max_delay, returnEmission=True)
    return cs, dict(emission=em)


@functools.lru_cache(maxsize=None)
def a_lists():
    """Room A at 400 in NumPy: the flat list (no wall of BETA is 0: also the images), exponents, paths, emission vectors."""
    comps, emit = shoebox_emission_numpy(A["room"], BETA, A["src"], A["pos"], FS, DELAY)
    images, exps, paths = images_numpy(A["room"], A["src"], A["pos"], FS, DELAY)
    _ones, emit1 = shoebox_emission_numpy(A["room"], ONES, A["src"], A["pos"], FS, DELAY)
    assert comps.shape == images.shape == (136, 4) and np.array_equal(comps[:, :3], images[:, :3]) and np.array_equal(emit, emit1)
    return comps, images, exps, paths, emit


def reference(model, sources, emits, rots, coefs, nfft=NFFT, pre=PRE, exps=None, paths=None, dists=None):
    """directive_spectra of a model on given lists (walls and air of the model)."""
    w, air, _wave = walls_of(model, nfft)
    kw = {}
    if model in ("spectral", "point_spectral"):
        kw.update(refl=np.asarray(w), exps=exps, att=air, paths=paths)
    if model.startswith("point"):
        kw.update(dists=dists)
    return directive_spectra(FS, RADIUS, mics5(), sources, emits, rots, coefs, 4, nfft, pre, **kw)


@functools.lru_cache(maxsize=None)
def a_undirected(model):
    """The undirected restatement of room A under a model: [1 x P x 5]."""
    comps, images, exps, paths, _emit = a_lists()
    w, air, _wave = walls_of(model)
    if model == "flat":
        return legendre_spectra(FS, RADIUS, mics5(), [comps], 4, NFFT, PRE)
    if model == "spectral":
        return spectral_legendre(FS, RADIUS, mics5(), [images], 4, NFFT, PRE, np.asarray(w), [exps], air, [paths])
    if model == "point":
        return point_legendre(FS, RADIUS, mics5(), [comps], [paths], 4, NFFT, PRE)
    return point_legendre(FS, RADIUS, mics5(), [images], [paths], 4, NFFT, PRE, np.asarray(w), [exps], air, [paths])


# ---- 1. emission lists
@gpu
def test_emission_lists_against_numpy():
    import emagls_amd as E
    src = [A["src"], (0.15, 0.2, 2.5), (2.5, 1.0, 1.0)]             # at 100 samples: 1, 0 and 2 components
    for max_delay in (100.0, DELAY):
        cs, em = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], FS, max_delay, returnEmission=True)
        plain = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], FS, max_delay)
        cd, dd, ed = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], FS, max_delay, returnDistance=True, returnEmission=True)
        _pc, pd = E.getShoeboxComponents(A["room"], BETA, src, A["pos"], FS, max_delay, returnDistance=True)
        ic, ie, ip, iem = E.getShoeboxImages(A["room"], src, A["pos"], FS, max_delay, returnEmission=True)
        jc, je, jp = E.getShoeboxImages(A["room"], src, A["pos"], FS, max_delay)
        worst = 0.0
        for q in range(3):
            want_c, want_e = shoebox_emission_numpy(A["room"], BETA, src[q], A["pos"], FS, max_delay)
            J = want_c.shape[0]
            assert cs[q].shape == (J, 4) and em[q].shape == (J, 3) and em[q].dtype == np.float64            # counts; the order follows from the values
            assert np.array_equal(cs[q], plain[q]) and np.array_equal(cd[q], plain[q]) and np.array_equal(dd[q], pd[q])      # today's bits
            assert np.array_equal(ed[q], em[q]) and np.array_equal(iem[q], em[q])                              # one emission list whatever goes with it
            assert np.array_equal(ic[q], jc[q]) and np.array_equal(ie[q], je[q]) and np.array_equal(ip[q], jp[q])
            if J:
                worst = max(worst, float(np.abs(em[q] - want_e).max()))
                assert np.abs((em[q] ** 2).sum(axis=1) - 1.0).max() < 1e-12                                    # what emagls_array_irs_directive asks
        print("array_directivity test 1 emission vectors at %g: %.3g (bound 1e-13)" % (max_delay, worst))
        assert worst < 1e-13
        if max_delay == 100.0:
            assert [c.shape[0] for c in cs] == [1, 0, 2]
    direct = np.subtract(A["pos"], A["src"])
    first = int(np.argmin(cs[0][:, 2]))                                                                       # the direct sound is the earliest component
    assert np.abs(em[0][first] - direct / np.linalg.norm(direct)).max() < 1e-15 * 4                           # from the source to the array
    no_walls, e0 = E.getShoeboxComponents(A["room"], [0.0] * 6, A["src"], A["pos"], FS, DELAY, returnEmission=True)
    assert no_walls[0].shape == (1, 4) and np.array_equal(e0[0], em[0][first:first + 1])
    (ic,), _e, _p, (iem,) = E.getShoeboxImages(A["room"], A["src"], A["pos"], FS, DELAY, maxOrder=1, returnEmission=True)
    assert ic.shape == (7, 4) and np.abs(iem - shoebox_emission_numpy(A["room"], ONES, A["src"], A["pos"], FS, DELAY, 1)[1]).max() < 1e-13


# ---- 2. omni
@gpu
@pytest.mark.parametrize("model", MODELS)
def test_omni_is_the_undirected_call(model):
    import emagls_amd as E
    want = room_irs(model)
    omni = E.firstOrderDirectivity(1.0)[:1]
    padded = np.zeros(16)
    padded[0] = omni[0]
    R = rotation(np.random.default_rng(21))[None]
    assert np.abs(want).max() > 0
    check(2, "%s, Nd = 0" % model, room_irs(model, directivity=omni), want)
    check(2, "%s, Nd = 3 padded, turned" % model, room_irs(model, directivity=padded, sourceOrientation=R), want)


# ---- 3. direct sound only
@gpu
@pytest.mark.parametrize("wave", ["planeWave", "pointSource"])
def test_direct_sound_through_a_cardioid(wave):
    import emagls_amd as E
    args = (A["room"], [0.0] * 6, A["src"], A["pos"], FS, LEN, PRE, RADIUS, mics5())
    kw = dict(maxDelay=DELAY, nfft=NFFT, waveModel=wave)
    free, counts = E.getArrayRoomIrs(*args, returnCounts=True, **kw)
    assert list(counts) == [1] and np.abs(free).max() > 0
    e = np.subtract(A["pos"], A["src"])
    e = e / np.linalg.norm(e)
    azi, zen = np.arctan2(e[1], e[0]), np.arccos(e[2])
    card = E.firstOrderDirectivity(0.5)
    facing = E.getArrayRoomIrs(*args, directivity=card, sourceOrientation=np.array([[azi, zen]]), **kw)
    away = E.getArrayRoomIrs(*args, directivity=card, sourceOrientation=np.array([[azi + np.pi, np.pi - zen]]), **kw)
    side = E.getArrayRoomIrs(*args, directivity=card, sourceOrientation=np.array([[azi + np.pi / 2, np.pi / 2]]), **kw)
    check(2, "%s, cardioid facing the array" % wave, facing, free, test=3)
    check(2, "%s, cardioid sideways" % wave, side, 0.5 * free, test=3)
    null = float(np.abs(away).max() / np.abs(free).max())
    print("array_directivity test 3 %s, cardioid facing away: %.3g of the free field (bound %.3g)" % (wave, null, BOUND[2]))
    assert null < BOUND[2]


# ---- 4. room A against the definition
@functools.lru_cache(maxsize=None)
def a_case(model, Nd):
    """Coefficients, a rotation, and the expected taps [1 x 1024 x 5] of room A under a model."""
    rng = np.random.default_rng(400 + 10 * MODELS.index(model) + Nd)
    coef, R = coefficients(rng, 1, Nd), rotation(rng)
    comps, images, exps, paths, emit = a_lists()
    src = images if model in ("spectral", "point_spectral") else comps
    H = reference(model, [src], [emit], [R], [coef[0]], exps=[exps], paths=[paths], dists=[paths])
    H.setflags(write=False)
    return coef, R, H


@gpu
@pytest.mark.parametrize("Nd", [1, 3])
@pytest.mark.parametrize("model", MODELS)
def test_room_a_against_the_definition(model, Nd):
    coef, R, H = a_case(model, Nd)
    want, plain = taps(H), taps(a_undirected(model))
    assert np.abs(want - plain).max() > 0.1 * np.abs(want).max()            # on the reference: the directivity changes the response
    got, counts = room_irs(model, directivity=coef, sourceOrientation=R[None], returnCounts=True)
    assert list(counts) == [136] and got.shape == (1, LEN, 5)
    check(4, "room A, %s, Nd = %d" % (model, Nd), got, want)


@gpu
def test_room_a_behind_a_complex_encoder():
    coef, R, H = a_case("spectral", 3)
    rng = np.random.default_rng(41)
    enc = rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))
    got = room_irs("spectral", directivity=coef, sourceOrientation=R[None], encoder=enc)
    assert got.shape == (1, LEN, 4) and np.iscomplexobj(got)
    check(4, "room A, spectral, Nd = 3, complex encoder", got, taps(H @ enc.real.T) + 1j * taps(H @ enc.imag.T))


# ---- 5. a listed call: both forms, the threshold, an empty source, the pole
COUNTS = (0, 1, 16, 17, 64, 65)
LISTED_NFFT = 256


@functools.lru_cache(maxsize=None)
def listed_case():
    rng = np.random.default_rng(1505)
    P2 = LISTED_NFFT // 2 + 1
    sources = [np.column_stack([random_dirs(rng, J), rng.uniform(0.0, 0.7 * LISTED_NFFT, J), rng.uniform(-1.0, 1.0, J)]) for J in COUNTS]
    emits = []
    for J in COUNTS:
        e = rng.standard_normal((J, 3))
        emits.append(e / np.sqrt((e * e).sum(axis=1))[:, None])
    rots = [rotation(rng) for _ in COUNTS]
    rots[3] = rot_z(0.7)                                             # its up axis is (0, 0, 1) to the bit, and so is R^T e there:
    emits[3][5] = (0.0, 0.0, 1.0)                                    # the pole of the basis (zen = 0, the azimuth atan2(0, 0))
    emits[5][64] = (0.0, 0.0, -1.0)
    rots[5] = rot_z(-2.1)
    dists = [np.exp(rng.uniform(np.log(1.05 * RADIUS), np.log(30.0), J)) for J in COUNTS]
    refl = rng.uniform(-1.0, 1.0, (3, P2))
    refl[0] = -np.abs(refl[0])
    refl[1, [5, 77]] = 0.0
    exps = [rng.integers(0, 6, (J, 3)).astype(np.int32) for J in COUNTS]
    att, paths = rng.uniform(0.0, 0.05, P2), [rng.uniform(1.0, 30.0, J) for J in COUNTS]
    coef = coefficients(rng, len(COUNTS), 2, P2)
    return sources, emits, rots, dists, refl, exps, att, paths, coef


@gpu
@pytest.mark.parametrize("model", MODELS)
def test_listed_call_in_both_forms(model):
    import emagls_amd as E
    sources, emits, rots, dists, refl, exps, att, paths, coef = listed_case()
    kw, rk = {}, {}
    if model in ("spectral", "point_spectral"):
        kw.update(surfaceReflection=refl, exponents=exps, airAttenuation=att, pathLength=paths)
        rk.update(refl=refl, exps=exps, att=att, paths=paths)
    if model.startswith("point"):
        kw.update(distance=dists)
        rk.update(dists=dists)
    got = E.getArrayIrs(sources, FS, LISTED_NFFT, 8.0, RADIUS, mics5(), order=4, nfft=LISTED_NFFT, emission=emits, sourceOrientation=np.array(rots),
                        directivity=coef, **kw)
    assert got.shape == (6, LISTED_NFFT, 5) and not got[0].any()
    want = directive_spectra(FS, RADIUS, mics5(), sources, emits, rots, list(coef), 4, LISTED_NFFT, 8.0, **rk)
    check(5, "listed, %s" % model, got, taps(want, LISTED_NFFT))
    for q in (1, 2, 3, 5):                                           # source q of a call gives the bits of the call with it alone
        one = {k: ([v[q]] if isinstance(v, list) else v) for k, v in kw.items()}
        alone = E.getArrayIrs([sources[q]], FS, LISTED_NFFT, 8.0, RADIUS, mics5(), order=4, nfft=LISTED_NFFT, emission=[emits[q]],
                              sourceOrientation=rots[q][None], directivity=coef[q:q + 1], **one)
        assert np.array_equal(alone[0], got[q]), q


# ---- 6. fused equals listed, bit for bit
@gpu
@pytest.mark.parametrize("encoder", ["raw", "complex"])
@pytest.mark.parametrize("model", MODELS)
def test_fused_equals_listed(model, encoder):
    """The array in the corner of room A (the head of tests/test_gpu_array_room_irs.py): 8, 0 and 32 components, counted here in NumPy."""
    import emagls_amd as E
    c = CORNER
    counts_np = [shoebox_numpy(A["room"], ONES if "spectral" in model else BETA, s, c["pos"], FS, c["max_delay"])[0].shape[0] for s in c["src"]]
    assert counts_np == [8, 0, 32] and 0 < counts_np[0] <= 16 < counts_np[2]
    rng = np.random.default_rng(61)
    enc = None if encoder == "raw" else rng.standard_normal((4, 5)) + 1j * rng.standard_normal((4, 5))
    coef, R = coefficients(rng, 3, 2, c["nfft"] // 2 + 1), np.array([rotation(rng) for _ in range(3)])
    kw = dict(ir_len=c["ir_len"], pre=c["pre"], max_delay=c["max_delay"], nfft=c["nfft"], pos=c["pos"])
    fused, counts = room_irs(model, src=c["src"], directivity=coef, sourceOrientation=R, encoder=enc, returnCounts=True, **kw)
    assert list(counts) == counts_np
    assert np.array_equal(fused, room_irs(model, src=c["src"], directivity=coef, sourceOrientation=R, encoder=enc, **kw))    # equal calls, equal bits
    cs, lk = lists_of(model, c["src"], c["pos"], c["max_delay"])
    w, air, _wave = walls_of(model, c["nfft"])
    if "spectral" in model:
        lk.update(surfaceReflection=w, airAttenuation=air)
    listed = E.getArrayIrs(cs, FS, c["ir_len"], c["pre"], RADIUS, mics5(), nfft=c["nfft"], encoder=enc, directivity=coef, sourceOrientation=R, **lk)
    assert fused.shape == listed.shape and fused.dtype == listed.dtype and np.abs(listed).max() > 0 and not fused[1].any()
    assert np.array_equal(fused, listed)
    for q in range(3):
        alone = room_irs(model, src=c["src"][q], directivity=coef[q:q + 1], sourceOrientation=R[q:q + 1], encoder=enc, **kw)
        assert np.array_equal(alone[0], fused[q]), q


# ---- 7. no directivity: today's entries
@gpu
@pytest.mark.parametrize("model", ["flat", "spectral", "point"])
def test_null_coefficients_are_todays_entries(model):
    import emagls_amd as E
    from emagls_amd import _lib as L
    lib = L.load()
    sources, _emits, _rots, dists, refl, exps, att, paths, _coef = listed_case()
    ptr = np.zeros(7, dtype=np.int64)
    ptr[1:] = np.cumsum(COUNTS)
    flat = np.ascontiguousarray(np.concatenate(sources))
    col = lambda i: np.ascontiguousarray(flat[:, i])   # noqa: E731
    M = 5
    out = np.zeros((6, M, LISTED_NFFT))
    a = dict(fs=FS, mic_radius=RADIUS, order=4, mic_azi=np.ascontiguousarray(mics5()[:, 0]), mic_zen=np.ascontiguousarray(mics5()[:, 1]), nmics=M,
             enc=None, enc_is_complex=0, nch=M, nsrc=6, comp_ptr=ptr, comp_azi=col(0), comp_zen=col(1), comp_delay=col(2), comp_gain=col(3), nsurf=0,
             surf_refl=None, comp_exp=None, air_atten=None, comp_path=None, comp_dist=None, comp_emit=None, src_rot=None, dir_order=0, dir_coef=None,
             pre_delay=8.0, nfft=LISTED_NFFT, nr=LISTED_NFFT, out=out)
    kw = {}
    if model == "spectral":
        a.update(nsurf=3, surf_refl=np.ascontiguousarray(refl), comp_exp=np.ascontiguousarray(np.concatenate(exps)), air_atten=att,
                 comp_path=np.concatenate(paths))
        kw = dict(surfaceReflection=refl, exponents=exps, airAttenuation=att, pathLength=paths)
    if model == "point":
        a.update(comp_dist=np.concatenate(dists))
        kw = dict(distance=dists)
    L.check(call(lib, "emagls_array_irs_directive", a))
    today = E.getArrayIrs(sources, FS, LISTED_NFFT, 8.0, RADIUS, mics5(), order=4, nfft=LISTED_NFFT, **kw)
    assert np.abs(today).max() > 0 and np.array_equal(out.transpose(0, 2, 1), today)
    # and the room entry
    w, air, wave = walls_of(model)
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = np.zeros((1, M, LEN))
    r = dict(a, room_dim=np.array(A["room"]), wall_refl=w, wall_is_spectral=1 if w.ndim == 2 else 0, air_atten=air, array_pos=np.array(A["pos"]), nsrc=1,
             src_pos=np.array(A["src"]), max_delay=DELAY, max_order=-1, point_source=1 if wave == "pointSource" else 0, pre_delay=PRE, nfft=NFFT, nr=LEN,
             comp_count=None, out=out)
    assert set(ARGS["emagls_array_room_irs_directive"]) <= set(r)
    L.check(call(lib, "emagls_array_room_irs_directive", r))
    assert np.array_equal(out.transpose(0, 2, 1), room_irs(model))


# ---- 8. the room turned and mirrored
@gpu
@pytest.mark.parametrize("model", ["flat", "point_spectral"])
def test_quarter_turn_and_mirror_image(model):
    rng = np.random.default_rng(88)
    coef, R = coefficients(rng, 1, 3), rotation(rng)
    w, _air, _wave = walls_of(model)
    w = np.asarray(w)
    Lx, Ly, Lz = A["room"]
    got = room_irs(model, directivity=coef, sourceOrientation=R[None])
    # a quarter turn about z: (x, y) -> (Ly - y, x); the wall at x' = 0 was the one at y = Ly, x' = Ly: y = 0, y' = 0: x = 0, y' = Lx: x = Lx
    turn = lambda p: (Ly - p[1], p[0], p[2])   # noqa: E731
    turned = room_irs(model, room=(Ly, Lx, Lz), walls=w[[3, 2, 0, 1, 4, 5]], src=turn(A["src"]), pos=turn(A["pos"]),
                      mics=mics5() + np.array([np.pi / 2, 0.0]), directivity=coef, sourceOrientation=(rot_z(np.pi / 2) @ R)[None])
    check(8, "%s, quarter turn about z" % model, turned, got)
    # the mirror image in y: the pattern is mirrored with its source (the sine coefficients change sign)
    S = np.diag([1.0, -1.0, 1.0])
    sine = np.array([m < 0 for n in range(4) for m in range(-n, n + 1)])
    mirrored_coef = np.where(sine[None, :, None], -coef, coef)
    flip = lambda p: (p[0], Ly - p[1], p[2])   # noqa: E731
    mirrored = room_irs(model, walls=w[[0, 1, 3, 2, 4, 5]], src=flip(A["src"]), pos=flip(A["pos"]), mics=mics5() * np.array([-1.0, 1.0]),
                        directivity=mirrored_coef, sourceOrientation=(S @ R @ S)[None])
    check(8, "%s, mirror image in y" % model, mirrored, got)
