"""GPU parity of getRenderedHrtfs (emagls_rendered_hrtfs).  The expected response is written out here:
fft(w) times the oracle's getSMAIRMatrix times conj(getSH) (or getSH alone, or the ATF spectra); the expected metrics are the NumPy
statement of tests/test_rendered_hrtfs_host.py applied to that expected response.  Random filters of the right shape: the response is
linear in them.  fs 48 kHz, len 128, nfft 256 unless a case says otherwise; the fixture grid thinned to every third direction (901).
Pass or fail: max abs difference over max abs value below 1e-6, per array.

The radii 4.2 cm and 8.75 cm give simulation orders 19 and 39 at 48 kHz (S = 400 and 1600); the inner dimension that is no multiple
of 4 (S = 49, simulation order 6) comes from the third radius, 1.3 cm.

The thinned grid starts at direction 1, not 0: both give 901 directions, but with directions 0, 3, 6, ... two Nyquist-bin values of the
synthetic HRTFs lie below 1e-6 of the largest magnitude (min / max = 9.1e-8), and ref_spectra() asserts that none does.  From
direction 1 the ratio is 1.13e-6 at nfft 256 and 1024, and 1.4e-5 or more on the first 67 directions at every nfft used here."""
import functools

import numpy as np
import pytest

from oracle import emagls_oracle as O
from test_rendered_hrtfs_host import rendered_metrics

pytestmark = pytest.mark.gpu
TOL = 1e-6
FS, LEN, NFFT = 48000.0, 128, 256
METRICS = ("mag_err_db", "ild_err_db", "cov_hat", "cov_ref", "coherence_hat", "coherence_ref")


def report(name, got, want):
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    print(f"{name}: max|diff|/max|ref| = {err:.3e}")
    return err


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(1, 2702, 3)      # directions 1, 4, 7, ...: see the module docstring
    hL, hR = hrirs
    return dict(dirs=np.column_stack([grids["azi"][sub], grids["zen"][sub]]), hL=np.ascontiguousarray(hL[:, sub]),
                hR=np.ascontiguousarray(hR[:, sub]), mics=np.column_stack([grids["mic_azi"], grids["mic_zen"]]))


def ref_spectra(hL, hR, nfft):
    """H [P x D x 2]; asserts that no logarithm of the metrics sits on a spectral zero."""
    H = np.stack([np.fft.rfft(hL, nfft, axis=0), np.fft.rfft(hR, nfft, axis=0)], axis=2)
    a = np.abs(H)
    assert a.min() / a.max() > 1e-6
    return H


def mic_grid(thin, M):
    from emagls_amd import synth
    return thin["mics"] if M == 32 else np.column_stack(synth.fibonacci_grid(M))


@functools.lru_cache(maxsize=None)
def _smair(order, nfft, radius, M, basis, raw, mics_key):
    mics = np.frombuffer(mics_key).reshape(-1, 2)
    return O.getSMAIRMatrix(order, FS, nfft, radius, mics, basis, returnRawMicSigs=raw)


def expected_array(w, dirs, mics, radius, order, basis, raw, nfft):
    """Hhat [P x D] of one ear: W(k,:) smairMat(:,:,k) getSH(simOrder, dirs)'  (lib/getEMagLsFilters.m:51-68, :87-103)."""
    sm, sim = _smair(order, nfft, radius, mics.shape[0], basis, raw, np.ascontiguousarray(mics).tobytes())
    W = np.fft.fft(w, nfft, axis=0)[:nfft // 2 + 1]
    Y = O.getSH(sim, dirs, basis)
    return np.einsum("ks,ds->kd", np.einsum("kc,csk->ks", W, sm), np.conj(Y))


def filters(rng, n, C, cplx=False):
    w = rng.standard_normal((n, C))
    return w + 1j * rng.standard_normal((n, C)) if cplx else w


def check(name, res, Hexp, Href, weights):
    errs = {"H": report(name + " H", res.H, Hexp)}
    want = rendered_metrics(Hexp, Href, weights)
    for k in METRICS:
        errs[k] = report(name + " " + k, getattr(res, k), want[k])
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("radius", [0.042, 0.0875, 0.013])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_emagls_model(thin, basis, radius):
    import emagls_amd as E
    rng = np.random.default_rng(41)
    wL, wR = filters(rng, LEN, 25, basis == "complex"), filters(rng, LEN, 25, basis == "complex")
    weights = rng.uniform(0.1, 1.0, 901) if basis == "complex" else None
    res = E.getRenderedHrtfs(wL, wR, "emagls", thin["dirs"], FS, order=4, micRadius=radius, micGridAziZenRad=thin["mics"], nfft=NFFT,
                             shDefinition=basis, hL=thin["hL"], hR=thin["hR"], weights=weights)
    Hexp = np.stack([expected_array(w, thin["dirs"], thin["mics"], radius, 4, basis, False, NFFT) for w in (wL, wR)], axis=2)
    assert res.H.shape == (129, 901, 2)
    check(f"emagls r={radius} {basis}", res, Hexp, ref_spectra(thin["hL"], thin["hR"], NFFT), weights)


@pytest.mark.parametrize("M,radius", [(32, 0.042), (64, 0.07)])
def test_emagls2_model(thin, M, radius):
    import emagls_amd as E
    rng = np.random.default_rng(42)
    mics = mic_grid(thin, M)
    wL, wR = filters(rng, LEN, M), filters(rng, LEN, M)
    weights = rng.uniform(0.1, 1.0, 901) if M == 32 else None
    res = E.getRenderedHrtfs(wL, wR, "emagls2", thin["dirs"], FS, micRadius=radius, micGridAziZenRad=mics, nfft=NFFT, hL=thin["hL"],
                             hR=thin["hR"], weights=weights)
    Hexp = np.stack([expected_array(w, thin["dirs"], mics, radius, 4, "real", True, NFFT) for w in (wL, wR)], axis=2)
    check(f"emagls2 M={M}", res, Hexp, ref_spectra(thin["hL"], thin["hR"], NFFT), weights)


@pytest.mark.parametrize("order", [1, 7, 15])
@pytest.mark.parametrize("basis", ["real", "complex"])
def test_sh_model(thin, basis, order):
    """D = 67: fewer directions than one tile is wide, and no multiple of 16."""
    import emagls_amd as E
    rng = np.random.default_rng(43)
    C = (order + 1) ** 2
    dirs, hL, hR = thin["dirs"][:67], thin["hL"][:, :67], thin["hR"][:, :67]
    wL, wR = filters(rng, LEN, C, basis == "complex"), filters(rng, LEN, C, basis == "complex")
    res = E.getRenderedHrtfs(wL, wR, "sh", dirs, FS, order=order, nfft=NFFT, shDefinition=basis, hL=hL, hR=hR)
    Yc = np.conj(O.getSH(order, dirs, basis))                                       # pwGrid = getSH(order, dirs, shDefinition)'
    Hexp = np.stack([np.fft.fft(w, NFFT, axis=0)[:129] @ Yc.T for w in (wL, wR)], axis=2)
    check(f"sh N={order} {basis}", res, Hexp, ref_spectra(hL, hR, NFFT), None)


@pytest.mark.parametrize("M,D,taps", [(6, 300, 96), (33, 901, 128)])
def test_atf_model(thin, M, D, taps):
    import emagls_amd as E
    rng = np.random.default_rng(44)
    atf = rng.standard_normal((taps, M, D)) * np.exp(-np.arange(taps) / 20.0)[:, None, None]
    wL, wR = filters(rng, LEN, M), filters(rng, LEN, M)
    hL, hR = thin["hL"][:, :D], thin["hR"][:, :D]
    weights = rng.uniform(0.1, 1.0, D)
    res = E.getRenderedHrtfs(wL, wR, "atf", thin["dirs"][:D], FS, atfIrs=atf, nfft=NFFT, hL=hL, hR=hR, weights=weights)
    A = np.fft.fft(atf, NFFT, axis=0)[:129]                                         # pwGrid_k(m, d) = fft(atfIrs, nfft)(k, m, d)
    Hexp = np.stack([np.einsum("km,kmd->kd", np.fft.fft(w, NFFT, axis=0)[:129], A) for w in (wL, wR)], axis=2)
    check(f"atf M={M} D={D}", res, Hexp, ref_spectra(hL, hR, NFFT), weights)


@pytest.mark.parametrize("nfft", [2048, 600])
def test_other_fft_lengths(thin, nfft):
    """nfft = 2048 (the designs' longest) and 600 (an even length that is no power of two), D = 67."""
    import emagls_amd as E
    rng = np.random.default_rng(45)
    dirs, hL, hR = thin["dirs"][:67], thin["hL"][:, :67], thin["hR"][:, :67]
    wL, wR = filters(rng, LEN, 25), filters(rng, LEN, 25)
    res = E.getRenderedHrtfs(wL, wR, "emagls", dirs, FS, order=4, micRadius=0.042, micGridAziZenRad=thin["mics"], nfft=nfft, hL=hL, hR=hR)
    Hexp = np.stack([expected_array(w, dirs, thin["mics"], 0.042, 4, "real", False, nfft) for w in (wL, wR)], axis=2)
    assert res.H.shape == (nfft // 2 + 1, 67, 2) and res.nfft == nfft
    check(f"emagls nfft={nfft}", res, Hexp, ref_spectra(hL, hR, nfft), None)


def test_default_nfft_is_twice_the_length(thin):
    import emagls_amd as E
    w = filters(np.random.default_rng(46), 100, 4)
    res = E.getRenderedHrtfs(w, w, "sh", thin["dirs"][:67], FS, order=1)
    assert res.nfft == 200 and res.H.shape == (101, 67, 2) and res.mag_err_db is None
    Hexp = np.fft.fft(w, 200, axis=0)[:101] @ O.getSH(1, thin["dirs"][:67], "real").T
    assert report("default nfft", res.H[..., 0], Hexp) < TOL


@pytest.fixture(scope="module")
def three_sets(thin):
    rng = np.random.default_rng(47)
    ws = [(filters(rng, LEN, 25), filters(rng, LEN, 25)) for _ in range(3)]
    hs = [(thin["hL"] * g, thin["hR"][::-1] * g) for g in (1.0, 0.5, 2.0)]
    kw = dict(order=4, micRadius=0.042, micGridAziZenRad=thin["mics"], nfft=NFFT, weights=rng.uniform(0.1, 1.0, 901))
    return ws, hs, kw


def same_bits(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in METRICS + ("H",) if getattr(a, k) is not None)


def test_three_sets_equal_three_single_calls_bit_for_bit(thin, three_sets):
    import emagls_amd as E
    ws, hs, kw = three_sets
    res = E.getRenderedHrtfs([w[0] for w in ws], [w[1] for w in ws], "emagls", thin["dirs"], FS, hL=[h[0] for h in hs], hR=[h[1] for h in hs], **kw)
    assert res.H.shape == (3, 129, 901, 2) and res.mag_err_db.shape == (3, 129, 2) and res.coherence_hat.shape == (3, 129)
    for i in range(3):
        one = E.getRenderedHrtfs(ws[i][0], ws[i][1], "emagls", thin["dirs"], FS, hL=hs[i][0], hR=hs[i][1], **kw)
        for k in METRICS + ("H",):
            assert np.array_equal(getattr(res, k)[i], getattr(one, k)), (i, k)
    assert not np.array_equal(res.mag_err_db[0], res.mag_err_db[1])
    # one HRIR pair shared by all sets
    shared = E.getRenderedHrtfs([w[0] for w in ws], [w[1] for w in ws], "emagls", thin["dirs"], FS, hL=hs[0][0], hR=hs[0][1], **kw)
    assert np.array_equal(shared.mag_err_db[0], res.mag_err_db[0]) and np.array_equal(shared.cov_ref[2], res.cov_ref[0])


def test_equal_calls_give_equal_bits_with_and_without_the_response(thin, three_sets):
    import emagls_amd as E
    ws, hs, kw = three_sets
    for model, w, extra in (("emagls", ws[0], kw), ("atf", (ws[0][0][:, :6], ws[0][1][:, :6]),
                                                   dict(atfIrs=np.random.default_rng(48).standard_normal((64, 6, 901)), nfft=NFFT))):
        a = E.getRenderedHrtfs(w[0], w[1], model, thin["dirs"], FS, hL=hs[0][0], hR=hs[0][1], **extra)
        b = E.getRenderedHrtfs(w[0], w[1], model, thin["dirs"], FS, hL=hs[0][0], hR=hs[0][1], **extra)
        c = E.getRenderedHrtfs(w[0], w[1], model, thin["dirs"], FS, hL=hs[0][0], hR=hs[0][1], returnResponse=False, **extra)
        assert same_bits(a, b), model
        assert c.H is None and all(np.array_equal(getattr(a, k), getattr(c, k)) for k in METRICS), model


def test_emagls_filters_render_closer_magnitudes_than_ls_filters(thin, grids):
    """A physical check without the oracle: above the cut the eMagLS design (len 512), evaluated through the model it was designed
    on, has a smaller mean magnitude error than the LS design evaluated through the SH model, on the same HRIRs.  Two measured
    values are compared; no threshold."""
    import emagls_amd as E
    azi, zen = thin["dirs"][:, 0], thin["dirs"][:, 1]
    nfft = 1024
    eL, eR = E.getEMagLsFilters(thin["hL"], thin["hR"], azi, zen, grids["mic_radius"], grids["mic_azi"], grids["mic_zen"], 4, FS, 512)
    lL, lR = E.getLsFilters(thin["hL"], thin["hR"], azi, zen, 4)
    em = E.getRenderedHrtfs(eL, eR, "emagls", thin["dirs"], FS, order=4, micRadius=grids["mic_radius"], micGridAziZenRad=thin["mics"], nfft=nfft,
                            hL=thin["hL"], hR=thin["hR"], returnResponse=False)
    ls = E.getRenderedHrtfs(lL, lR, "sh", thin["dirs"], FS, order=4, nfft=nfft, hL=thin["hL"], hR=thin["hR"], returnResponse=False)
    f = np.arange(nfft // 2 + 1) * FS / nfft
    k_cut = int(np.ceil(500.0 * 4 / f[1]))                   # the designs' cut (lib/getEMagLsFilters.m:47) on this bin grid
    band = slice(k_cut, int(np.floor(16000.0 / f[1])) + 1)
    e_mean, l_mean = float(em.mag_err_db[band].mean()), float(ls.mag_err_db[band].mean())
    print(f"mean |dB| error, bins {band.start}..{band.stop - 1}: eMagLS {e_mean:.3f} dB, LS {l_mean:.3f} dB")
    assert e_mean < l_mean
