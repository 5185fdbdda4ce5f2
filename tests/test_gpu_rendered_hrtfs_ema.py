"""GPU parity of the two equatorial-array models of getRenderedHrtfs ('ema_ch', 'ema_sh').  The expected response
is written out here in NumPy from the oracle's pieces -- getSMAIRMatrix (raw microphone signals, microphones at zenith pi/2), getSH,
getCH, getChToShExpansionMatrix -- as lib/getEMagLsFiltersEMAinCH.m:52-75 and lib/getEMagLsFiltersEMAinSH.m:66-100 state the operand;
the per-direction SH rotations are the oracle's least-squares fit (shRotationForElevation), vectorised over the directions with ONE
pinv of the fixed point matrix, and compared with the oracle's own function on a handful of directions.  Random filters of the
right shape: the response is linear in them.  The helpers, the grid (901 directions), fs 48 kHz, len 128, nfft 256 and the pass mark
-- max abs difference over max abs value below 1e-6, per array -- are those of tests/test_gpu_rendered_hrtfs.py.

The zeniths of the first three directions are overwritten with pi/2 (the identity rotation the reference takes there), 0 and pi (the
poles, a quarter turn up and down); their HRIR columns stay.  Microphones are uniformly spaced on the equator."""
import functools

import numpy as np
import pytest

from oracle import emagls_oracle as O
from test_gpu_rendered_hrtfs import FS, LEN, METRICS, NFFT, TOL, check, filters, ref_spectra, report, same_bits, thin  # noqa: F401

pytestmark = pytest.mark.gpu


def mic_azi(M):
    return 2.0 * np.pi * np.arange(M) / M


@pytest.fixture(scope="module")
def ema(thin):  # noqa: F811
    dirs = thin["dirs"].copy()
    dirs[:3, 1] = [np.pi / 2, 0.0, np.pi]
    return dict(dirs=dirs, hL=thin["hL"], hR=thin["hR"])


def n_channels(model, order):
    return 2 * order + 1 if model == "ema_ch" else (order + 1) ** 2


@functools.lru_cache(maxsize=None)
def _array(order, nfft, radius, M, basis):
    """pinv(getCH(order, micAzi)) smairMat(:,:,k) for every k: [P x 2 order + 1 x S], and the simulation order."""
    azi = mic_azi(M)
    sm, sim = O.getSMAIRMatrix(order, FS, nfft, radius, np.column_stack([azi, np.full(M, np.pi / 2)]), basis, returnRawMicSigs=True)
    return O.pinv(O.getCH(order, azi, basis)) @ sm.transpose(2, 0, 1), sim


def rotations(dirs, order, basis):
    """Rot_d [D x C x C] of oracle.shRotationForElevation for every direction at once (identity where zen == pi/2 exactly, as
    lib/getEMagLsFiltersEMAinSH.m:92 skips those): the same point set, the same rotation, one pinv of the fixed point matrix."""
    azi, zen = dirs[:, 0], dirs[:, 1]
    alpha = np.pi / 2 - zen
    ax = np.stack([np.sin(azi), -np.cos(azi), np.zeros_like(azi)], axis=1)
    K = np.zeros((azi.size, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -ax[:, 2], ax[:, 1], ax[:, 2], -ax[:, 0], -ax[:, 1], ax[:, 0]
    R = np.eye(3) + np.sin(alpha)[:, None, None] * K + (1 - np.cos(alpha))[:, None, None] * (K @ K)
    n = 4 * (order + 1) ** 2 + 8
    i = np.arange(n) + 0.5
    pz, pa = np.arccos(1 - 2 * i / n), np.mod(np.pi * (1 + 5 ** 0.5) * i, 2 * np.pi)
    X = np.column_stack([np.sin(pz) * np.cos(pa), np.sin(pz) * np.sin(pa), np.cos(pz)])
    Xr = X @ R                                                                       # [D x n x 3], rows R_d^-1 x_p
    pts = np.column_stack([np.arctan2(Xr[..., 1], Xr[..., 0]).ravel(), np.arccos(np.clip(Xr[..., 2], -1, 1)).ravel()])
    A = O.getSH(order, pts, basis).reshape(azi.size, n, -1)                          # Y_i(R_d^-1 x_p)
    rot = (O.pinv(O.getSH(order, np.column_stack([pa, pz]), basis)) @ A).transpose(0, 2, 1)
    rot[zen == np.pi / 2] = np.eye(rot.shape[1])
    return rot


@functools.lru_cache(maxsize=None)
def _rotations(order, basis, dirs_key):
    return rotations(np.frombuffer(dirs_key).reshape(-1, 2), order, basis)


def operand(model, dirs, radius, order, basis, M, nfft):
    """pwGrid [P x C x D] (EMAinCH.m:70-75, EMAinSH.m:66-100), each stage one batched matrix product."""
    A, sim = _array(order, nfft, radius, M, basis)
    if model == "ema_ch":
        return A @ np.conj(O.getSH(sim, dirs, basis)).T
    Yh = O.getSH(sim, np.column_stack([dirs[:, 0], np.full(dirs.shape[0], np.pi / 2)]), basis)
    V = (O.getChToShExpansionMatrix(order, basis) @ A) @ np.conj(Yh).T              # [P x C x D], unrotated
    rot = _rotations(order, basis, np.ascontiguousarray(dirs).tobytes())
    return (rot.transpose(0, 2, 1) @ V.transpose(2, 1, 0)).transpose(2, 1, 0)      # column d: Rot_d.' V(:, d)


def expected(model, wL, wR, dirs, radius, order, basis, M, nfft):
    pw = operand(model, dirs, radius, order, basis, M, nfft)
    return np.stack([np.einsum("kc,kcd->kd", np.fft.fft(w, nfft, axis=0)[:nfft // 2 + 1], pw) for w in (wL, wR)], axis=2)


def run_case(ema, model, order, radius, basis, M, seed, weighted=False):  # noqa: F811
    import emagls_amd as E
    rng = np.random.default_rng(seed)
    cplx = basis == "complex"
    C = n_channels(model, order)
    wL, wR = filters(rng, LEN, C, cplx), filters(rng, LEN, C, cplx)
    weights = rng.uniform(0.1, 1.0, 901) if weighted else None
    res = E.getRenderedHrtfs(wL, wR, model, ema["dirs"], FS, order=order, micRadius=radius, micGridAziZenRad=mic_azi(M), nfft=NFFT,
                             shDefinition=basis, hL=ema["hL"], hR=ema["hR"], weights=weights)
    assert res.H.shape == (129, 901, 2)
    Hexp = expected(model, wL, wR, ema["dirs"], radius, order, basis, M, NFFT)
    check(f"{model} N={order} r={radius} M={M} {basis}", res, Hexp, ref_spectra(ema["hL"], ema["hR"], NFFT), weights)


def test_vectorised_rotation_fit_agrees_with_the_oracle(ema):
    """Both solve the same least-squares problem on the same points in double precision; the entries are at most 1 in magnitude and
    the point matrix has a condition number below 2, so they differ by rounding in sums of 4 C + 8 <= 108 terms: 1e-13 is a hundred
    times that.  Directions: the three overwritten ones, two of the grid, real and complex basis, orders 2 and 4."""
    for order in (2, 4):
        for basis in ("real", "complex"):
            idx = [0, 1, 2, 3, 450, 900]
            got = rotations(ema["dirs"][idx], order, basis)
            for j, d in enumerate(idx):
                azi, zen = ema["dirs"][d]
                want = np.eye((order + 1) ** 2) if zen == np.pi / 2 else O.shRotationForElevation(azi, zen, order, basis)
                err = float(np.abs(got[j] - want).max())
                print(f"rotation fit N={order} {basis} d={d}: max abs diff {err:.2e}")
                assert err < 1e-13


@pytest.mark.parametrize("order,radius,basis,M", [(1, 0.042, "real", 3), (4, 0.042, "real", 16), (4, 0.042, "complex", 16),
                                                  (4, 0.013, "real", 16), (4, 0.013, "complex", 16), (15, 0.042, "real", 31),
                                                  (15, 0.042, "real", 64)])
def test_ema_ch_model(ema, order, radius, basis, M):
    """Order 1 on the fewest microphones; S = 400 and S = 49 (no multiple of 4) in both bases, the complex ones with complex filters and
    random direction weights; order 15 (31 channels: all the columns the factorisation takes) on 31 and on 64 microphones."""
    run_case(ema, "ema_ch", order, radius, basis, M, 61, weighted=basis == "complex")


@pytest.mark.parametrize("order,radius,basis", [(1, 0.042, "real"), (4, 0.042, "real"), (4, 0.042, "complex"), (5, 0.042, "real"),
                                                (5, 0.042, "complex"), (7, 0.042, "real"), (7, 0.013, "real")])
def test_ema_sh_model(ema, order, radius, basis):
    """16 microphones.  Orders 1 and 4 (rotations from one workgroup per direction), 5 (the first with per-order rotation blocks and
    the wide pinv of the point matrix, in both bases) and 7; the complex basis with complex filters and random weights; 1.3 cm at order 7: the
    simulation order is the order itself."""
    run_case(ema, "ema_sh", order, radius, basis, 16, 62, weighted=basis == "complex")


@pytest.mark.parametrize("model", ["ema_ch", "ema_sh"])
def test_non_power_of_two_nfft(ema, model):
    """len 100, nfft 200 (the default), D = 67: fewer directions than one tile is wide."""
    import emagls_amd as E
    rng = np.random.default_rng(63)
    dirs, hL, hR = ema["dirs"][:67], ema["hL"][:, :67], ema["hR"][:, :67]
    C = n_channels(model, 4)
    wL, wR = filters(rng, 100, C), filters(rng, 100, C)
    res = E.getRenderedHrtfs(wL, wR, model, dirs, FS, order=4, micRadius=0.042, micGridAziZenRad=mic_azi(16), hL=hL, hR=hR)
    assert res.nfft == 200 and res.H.shape == (101, 67, 2)
    check(f"{model} nfft=200", res, expected(model, wL, wR, dirs, 0.042, 4, "real", 16, 200), ref_spectra(hL, hR, 200), None)


@pytest.mark.parametrize("model", ["ema_ch", "ema_sh"])
def test_three_sets_equal_three_single_calls_and_equal_calls_give_equal_bits(ema, model):
    import emagls_amd as E
    rng = np.random.default_rng(64)
    C = n_channels(model, 4)
    ws = [(filters(rng, LEN, C), filters(rng, LEN, C)) for _ in range(3)]
    hs = [(ema["hL"] * g, ema["hR"][::-1] * g) for g in (1.0, 0.5, 2.0)]
    kw = dict(order=4, micRadius=0.042, micGridAziZenRad=mic_azi(16), nfft=NFFT, weights=rng.uniform(0.1, 1.0, 901))
    res = E.getRenderedHrtfs([w[0] for w in ws], [w[1] for w in ws], model, ema["dirs"], FS, hL=[h[0] for h in hs], hR=[h[1] for h in hs], **kw)
    assert res.H.shape == (3, 129, 901, 2) and res.mag_err_db.shape == (3, 129, 2)
    ones = [E.getRenderedHrtfs(ws[i][0], ws[i][1], model, ema["dirs"], FS, hL=hs[i][0], hR=hs[i][1], **kw) for i in range(3)]
    for i in range(3):
        for k in METRICS + ("H",):
            assert np.array_equal(getattr(res, k)[i], getattr(ones[i], k)), (i, k)
    assert not np.array_equal(res.mag_err_db[0], res.mag_err_db[1]) and np.abs(res.H).max() > 0
    # one HRIR pair shared by all sets
    shared = E.getRenderedHrtfs([w[0] for w in ws], [w[1] for w in ws], model, ema["dirs"], FS, hL=hs[0][0], hR=hs[0][1], **kw)
    assert np.array_equal(shared.mag_err_db[0], res.mag_err_db[0]) and np.array_equal(shared.cov_ref[2], res.cov_ref[0])
    assert np.array_equal(shared.H, res.H)
    # equal calls, with and without the response
    b = E.getRenderedHrtfs(ws[0][0], ws[0][1], model, ema["dirs"], FS, hL=hs[0][0], hR=hs[0][1], **kw)
    c = E.getRenderedHrtfs(ws[0][0], ws[0][1], model, ema["dirs"], FS, hL=hs[0][0], hR=hs[0][1], returnResponse=False, **kw)
    assert same_bits(ones[0], b)
    assert c.H is None and all(np.array_equal(getattr(b, k), getattr(c, k)) for k in METRICS)


@pytest.mark.parametrize("basis", ["real", "complex"])
def test_on_the_equator_ema_sh_is_ema_ch_behind_the_expansion_matrix(ema, basis):
    """A cross-check that needs no expected response: where every zenith is pi/2 exactly no direction is rotated, so
    pwGrid_sh = J pwGrid_ch and SH filters w through 'ema_sh' render what the CH filters w J render through 'ema_ch'.  67 directions."""
    import emagls_amd as E
    rng = np.random.default_rng(65)
    dirs = np.column_stack([ema["dirs"][:67, 0], np.full(67, np.pi / 2)])
    J = O.getChToShExpansionMatrix(4, basis)
    wL, wR = filters(rng, LEN, 25, basis == "complex"), filters(rng, LEN, 25, basis == "complex")
    kw = dict(order=4, micRadius=0.042, micGridAziZenRad=mic_azi(16), nfft=NFFT, shDefinition=basis)
    sh = E.getRenderedHrtfs(wL, wR, "ema_sh", dirs, FS, **kw)
    ch = E.getRenderedHrtfs(wL @ J, wR @ J, "ema_ch", dirs, FS, **kw)
    assert np.abs(ch.H).max() > 0
    assert report(f"ema_sh against ema_ch on the equator, {basis}", sh.H, ch.H) < TOL


def test_ema_in_sh_filters_render_closer_magnitudes_than_ls_filters(thin):  # noqa: F811
    """A physical check without the oracle: above the cut the EMAinSH design, evaluated through the model it was designed on, has a
    smaller mean magnitude error than the LS design (plain SH filters of the same order) evaluated through that same model, on the
    same HRIRs.  Order 4, 16 microphones at 4.2 cm, len 256.  A NumPy run of the two designs on a 301-point grid gave 0.9 dB against
    20.7 dB; the GPU design needs as many directions as simulated SH channels (400 here), so the grid is the 901 thinned
    directions with their own zeniths.  Two measured values are compared; no threshold."""
    import emagls_amd as E
    dirs, hL, hR = thin["dirs"], thin["hL"], thin["hR"]
    azi, zen, m_azi, nfft = dirs[:, 0], dirs[:, 1], mic_azi(16), 512
    eL, eR = E.getEMagLsFiltersEMAinSH(hL, hR, azi, zen, 0.042, m_azi, 4, FS, 256)
    lL, lR = E.getLsFilters(hL, hR, azi, zen, 4)
    kw = dict(order=4, micRadius=0.042, micGridAziZenRad=m_azi, nfft=nfft, hL=hL, hR=hR, returnResponse=False)
    em = E.getRenderedHrtfs(eL, eR, "ema_sh", dirs, FS, **kw)
    ls = E.getRenderedHrtfs(lL, lR, "ema_sh", dirs, FS, **kw)
    f1 = FS / nfft
    band = slice(int(np.ceil(500.0 * 4 / f1)), int(np.floor(16000.0 / f1)) + 1)     # from the designs' cut (lib/getEMagLsFiltersEMAinSH.m:47)
    e_mean, l_mean = float(em.mag_err_db[band].mean()), float(ls.mag_err_db[band].mean())
    print(f"mean |dB| error, bins {band.start}..{band.stop - 1}: EMAinSH {e_mean:.3f} dB, LS {l_mean:.3f} dB")
    assert e_mean < l_mean
