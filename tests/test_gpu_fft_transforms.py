"""The transforms at both ends of a design (emagls_amd/csrc/fft.hip) against a longdouble direct transform: the launchers the designs use,
run by the debug entries of fft_debug.hip on the inputs of tests/fft_reference.py and held, element by element, to the a-priori bounds
derived there (tests/test_fft_reference_host.py checks reference and bounds on the host).  Every case prints its largest error / bound.
What the kernels leave alone -- the gaps of ldD, ldT and ld_inner -- keeps the sentinel the entries fill the outputs with."""
import ctypes as C

import numpy as np
import pytest

import fft_reference as R

pytestmark = pytest.mark.gpu
LD = R.LD


def lib():
    from emagls_amd import _lib as L
    return L, L.load()


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def is_sentinel(a):
    from emagls_amd import _lib as L
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(L.DEBUG_SENTINEL_BITS)


def nan_filled(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.fill(np.nan)
    return a


@pytest.fixture(scope="module", autouse=True)
def _longdouble():
    R.require_longdouble()


# ---- the twiddle table -------------------------------------------------------------------------------------------------------------

def debug_twiddles(nfft):
    L, lb = lib()
    tw = nan_filled(nfft, np.complex128)
    L.check(lb.emagls_debug_twiddles(nfft, ptr(tw)))
    return tw


@pytest.mark.parametrize("nfft", sorted(set(R.EPI_POW2 + R.EPI_DFT + (1024, 2048, 600, 6))))
def test_twiddle_table(nfft):
    """launch_twiddles entry by entry within tw_bound; the four entries on the axes exact"""
    tw = debug_twiddles(nfft)
    ref, tb = R.twiddle_ref(nfft)
    err = R.f64(np.abs(R.to_cld(tw) - ref))
    print(f"twiddles nfft {nfft}: largest error {err.max() / R.U:.2f} u, largest error / bound {R.ratio(tw, ref, tb).max():.3f}")
    assert np.all(err <= tb)
    for j in {0, nfft // 2} | ({nfft // 4, 3 * nfft // 4} if nfft % 4 == 0 else set()):
        assert tw[j] == R.c128(ref[j])


# ---- filter epilogue ---------------------------------------------------------------------------------------------------------------

def debug_epilogue(W, nfft, length, grpd, conj_mode, dc_rule, shift_mode, out_cplx, n_ears, fade_rel):
    L, lb = lib()
    Cn = W.shape[2]
    dt = np.complex128 if out_cplx else np.float64
    out = [nan_filled((Cn, length), dt) for _ in range(n_ears)]
    g = np.array(grpd, dtype=np.float64) if grpd is not None else None
    L.check(lb.emagls_debug_filter_epilogue(ptr(W), Cn, nfft, length, ptr(g), conj_mode, dc_rule, shift_mode, out_cplx, n_ears, float(fade_rel),
                                            ptr(out[0]), ptr(out[1]) if n_ears == 2 else None))
    return out


@pytest.mark.parametrize("case", R.epilogue_cases(), ids=R.case_id)
def test_filter_epilogue(case):
    c = case
    W = R.epilogue_input(c)
    got = debug_epilogue(W, c["nfft"], c["len"], c["grpd"] if c["n_ears"] == 2 else None, c["conj_mode"], c["dc_rule"], c["shift_mode"], c["out_cplx"],
                         c["n_ears"], c["fade_rel"])
    ref = R.epilogue_ref(W, c["nfft"], c["len"], c["grpd"], c["conj_mode"], c["dc_rule"], c["shift_mode"], c["out_cplx"], c["n_ears"], c["fade_rel"])
    worst = 0.0
    for g, (val, bound) in zip(got, ref):
        assert not is_sentinel(g).any() and np.isfinite(g).all()
        worst = max(worst, float(R.ratio(g, val, bound).max()))
    print(f"epilogue ({c['cls']}) {R.case_id(c)}: largest error / bound = {worst:.4f}")
    assert worst <= 1.0


# ---- HRIR prologue -----------------------------------------------------------------------------------------------------------------

def debug_hrir(hL, hR, nfft, D=0, didx=None, mode=0, n_c=0, kabs0=0, grpd_in=None, ldD=0, ldT=0, spectra=True, hct=False):
    """returns grpd_out [2], phs [2][P], Hc [2][n_c][ldD], Habs [2][P - kabs0][ldD], HcT [D][ldT] or None"""
    L, lb = lib()
    P = nfft // 2 + 1
    go, phs = nan_filled(2, np.float64), nan_filled((2, P), np.complex128)
    Hc = nan_filled((2, n_c, ldD), np.complex128) if spectra else None
    Ha = nan_filled((2, P - kabs0, ldD), np.float64) if spectra else None
    HT = nan_filled((D, ldT), np.float64) if spectra and hct else None
    gi = np.array(grpd_in, dtype=np.float64) if grpd_in is not None else None
    L.check(lb.emagls_debug_hrir_spectra(ptr(hL), ptr(hR), hL.shape[1], hL.shape[0], D, ptr(didx), nfft, mode, n_c, kabs0, ptr(gi), ldD, ldT if HT is not None else 0,
                                         ptr(go), ptr(phs), ptr(Hc), ptr(Ha), ptr(HT)))
    return go, phs, Hc, Ha, HT


def check_delays(hL, hR, nfft, go, phs):
    """the two delays within the bound of the median, and the phase table behind them within the phase bound at the kernel's own delays"""
    worst = 0.0
    for e, ref in enumerate(R.grpdelay_ref(hL, hR, nfft)):
        assert np.isfinite(ref["delay_bound"]) and ref["delay_bound"] < 1e-4      # (the input is conditioned well enough for the bound to say something)
        worst = max(worst, abs(float(LD(float(go[e])) - ref["delay"])) / max(ref["delay_bound"], 1e-300) if go[e] != float(ref["delay"]) else 0.0)
        E, pb = R.phase_ref(nfft, go[e], +1)
        assert float(R.ratio(phs[e], E, pb).max()) <= 1.0 and phs[e, -1].imag == 0.0
    return worst


@pytest.mark.parametrize("case", R.spectra_cases(), ids=R.case_id)
def test_hrir_spectra(case, monkeypatch):
    c = case
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    hL, hR, didx = R.hrir_input(c)
    nfft, D, P = c["nfft"], c["D"], c["nfft"] // 2 + 1
    n_c, kabs0 = R.spectra_split(P, c["split"])
    ldD = -(-D // 8) * 8 + 8
    ldT = 4 * n_c + 2
    go, phs, Hc, Ha, HT = debug_hrir(hL, hR, nfft, D, didx, c["mode"], n_c, kabs0, c["grpd"], ldD, ldT, hct=c["hct"])
    rd = 0.0
    if c["grpd"] is None:
        rd = check_delays(hL, hR, nfft, go, phs)
        assert rd <= 1.0
    else:
        assert tuple(go) == tuple(c["grpd"]) and is_sentinel(phs).all()
    Hr, bc, Har, ba = R.hrir_spectra_ref(hL, hR, nfft, c["mode"], go, didx, D)
    rc = float(R.ratio(Hc[:, :, :D], Hr[:, :n_c], bc[:, :n_c]).max()) if n_c else 0.0
    ra = float(R.ratio(Ha[:, :, :D], Har[:, kabs0:], ba[:, kabs0:]).max()) if kabs0 < P else 0.0
    print(f"HRIR spectra {R.case_id(c)}: largest error / bound = {rc:.4f} (complex rows), {ra:.4f} (|H|), {rd:.4f} (delays)")
    assert rc <= 1.0 and ra <= 1.0
    # what lies beyond the D directions and beyond the rows' 4 n_c doubles is left alone; the direction-major copy is the same numbers
    assert is_sentinel(Hc[:, :, D:]).all() and is_sentinel(Ha[:, :, D:]).all()
    assert not is_sentinel(Hc[:, :, :D]).any() and not is_sentinel(Ha[:, :, :D]).any()
    if HT is not None:
        assert is_sentinel(HT[:, 4 * n_c:]).all()
        assert np.array_equal(HT[:, :4 * n_c].reshape(D, 2, n_c, 2), np.moveaxis(Hc[:, :, :D], 2, 0).copy().view(np.float64).reshape(D, 2, n_c, 2))
    if c["scale"]:                     # a power of two on the input is the same power of two on every output
        u = R.hrir_input(c, scaled=False)
        _, _, Hc1, Ha1, _ = debug_hrir(u[0], u[1], nfft, D, didx, c["mode"], n_c, kabs0, c["grpd"], ldD, ldT)
        s = 2.0 ** c["scale"]
        assert np.array_equal(Hc[:, :, :D], Hc1[:, :, :D] * s) and np.array_equal(Ha[:, :, :D], Ha1[:, :, :D] * s)


@pytest.mark.parametrize("case", [c for c in R.spectra_cases() if c["zero_ear"] is not None], ids=R.case_id)
def test_silent_ear_has_no_spectrum(case):
    """One ear all zeros: its |H| and its complex rows are exactly 0, in every form and both modes.  (The LDS and the wave form pack both
    ears into one complex transform and separate them as (z_k +- conj z_{nfft-k}) / 2; the computed transform of a real input is not
    exactly Hermitian, and before the kernels wrote a silent ear's rows as zeros this test found 1.05 ... 3.49 u of the other ear's sum of
    moduli there, in 93 ... 99 % of the bins.  The direct form sums each ear on its own.)"""
    c = case
    hL, hR, didx = R.hrir_input(c)
    nfft, D, P = c["nfft"], c["D"], c["nfft"] // 2 + 1
    go, _, Hc, Ha, _ = debug_hrir(hL, hR, nfft, D, didx, c["mode"], P, 0, c["grpd"], 16, 0)
    _, bc, _, _ = R.hrir_spectra_ref(hL, hR, nfft, c["mode"], go, didx, D)
    e = c["zero_ear"]
    other = float(np.abs((hR if e == 0 else hL)).sum(axis=1).max())
    print(f"silent ear {R.case_id(c)}: largest |H| of the silent ear = {Ha[e, :, :D].max():.3e} = {Ha[e, :, :D].max() / other / R.U:.2f} u of the other ear's sum of "
          f"moduli, {float((Ha[e, :, :D] / bc[e]).max()):.4f} of the bound; bins that are not exactly 0: {int((Ha[e, :, :D] != 0).sum())} of {P * D}")
    assert np.all(Ha[e, :, :D] == 0.0) and np.all(Hc[e, :, :D] == 0.0)


@pytest.mark.parametrize("case", R.grpdelay_cases(), ids=R.case_id)
def test_group_delay(case):
    """the direction sum, the per-bin delays and their median (more taps than threads, the bin beyond the workgroup at nfft 2048, chunks of 64
    directions, a median that averages two values): the delay within the largest per-bin bound, the phase table within the phase bound"""
    hL, hR = R.grpdelay_input(case)
    go, phs, _, _, _ = debug_hrir(hL, hR, case["nfft"], spectra=False)
    r = check_delays(hL, hR, case["nfft"], go, phs)
    print(f"group delay {R.case_id(case)}: delays {go[0]!r}, {go[1]!r}; largest error / bound = {r:.4f}")
    assert r <= 1.0
    if case["kind"] == "impulse":
        assert abs(go[0] - 7 % case["L"]) < 1e-9 and abs(go[1] - 11 % case["L"]) < 1e-9
    if case["kind"] == "twotap":       # gd = 1 at every bin but nfft / 4, where den = 0 takes the branch
        assert abs(go[0] - 1.0) < 1e-9


# ---- ATF spectra -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", R.real_cases(), ids=R.case_id)
def test_atf_spectra(case):
    L, lb = lib()
    x, colidx, (ldo, inner, ld_inner) = R.real_input(case)
    nfft, nc, P = case["nfft"], case["ncols"], case["nfft"] // 2 + 1
    out = nan_filled((P, ldo), np.complex128)
    L.check(lb.emagls_debug_real_spectra(ptr(x), x.shape[1], x.shape[0], nc, ptr(colidx), nfft, ldo, inner, ld_inner, ptr(out)))
    X, b = R.real_spectra_ref(x, nfft, nc, colidx)
    at = R.place_columns(nc, inner, ld_inner)
    r = float(R.ratio(out[:, at], X, b).max())
    print(f"ATF spectra {R.case_id(case)}: largest error / bound = {r:.4f}")
    assert r <= 1.0
    rest = np.ones(ldo, dtype=bool)
    rest[at] = False
    assert is_sentinel(out[:, rest]).all() and not is_sentinel(out[:, at]).any()


# ---- the modes tested are the modes used: the epilogue of five designs, from the plan's own W and delays ---------------------------

@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


def design_plan(kind, thin, grids):
    """(plan, the arguments plan_run.hip hands launch_filter_epilogue: conj_mode, dc_rule, shift_mode)"""
    from emagls_amd import Plan, synth, _lib as L
    nsamp, nd = thin["hL"].shape
    if kind == "emagls_real":
        p, args = Plan(L.KIND_EMAGLS, "real", 4, 48000.0, 128, nsamp, nd, grids["mic_radius"], 32), (0, 1, 0)
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
    elif kind == "emagls_complex":
        p, args = Plan(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, nsamp, nd, grids["mic_radius"], 32), (1, 1, 0)
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
    elif kind == "ema_ch_complex":
        p, args = Plan(L.KIND_EMA_CH, "complex", 4, 48000.0, 128, nsamp, nd, 0.042, 16), (2, 1, 0)
        p.set_mic_grid(np.linspace(0.0, 2 * np.pi, 16, endpoint=False) + 0.1)
    elif kind == "magls_real":
        p, args = Plan(L.KIND_MAGLS, "real", 4, 48000.0, 128, nsamp, nd), (0, 0, 0)
    else:
        atf, aazi, azen = synth.glasses_atfs(natf=512, nmics=4, taps=64)
        p, args = Plan(L.KIND_FROM_ATF, "real", 0, 48000.0, 128, nsamp, nd, nmics=4, f_trans=1500.0, atf_taps=64, natf=512), (0, 1, 1)
    p.set_hrir_grid(thin["azi"], thin["zen"])
    p.set_hrirs(thin["hL"], thin["hR"])
    if kind == "from_atf":
        p.set_atfs(atf, aazi, azen)
    return p, args


@pytest.mark.parametrize("kind", ["emagls_real", "emagls_complex", "ema_ch_complex", "magls_real", "from_atf"])
def test_epilogue_of_a_design(kind, thin, grids):
    """The plan's own spectra W and delays through the debug entry with the arguments the design passes: the same filters, bit for bit, as
    get_filters() -- and those within the bound of the longdouble epilogue of that W.  The plan's twiddle table is the debug entry's."""
    p, (conj_mode, dc_rule, shift_mode) = design_plan(kind, thin, grids)
    try:
        p.execute()
        p.synchronize()
        i = p.info()
        nfft, P, Cn, length = i.nfft, i.num_pos_freqs, i.out_cols, i.out_rows
        W = np.ascontiguousarray(p.debug("W", np.complex128)[:2 * P * Cn].reshape(2, P, Cn))
        grpd = p.debug("grpd", np.float64)[:2].copy()
        tw = p.debug("tw", np.complex128)[:nfft].copy()
        wL, wR = p.get_filters()
    finally:
        p.close()
    assert (nfft, length) == (256, 128) and np.array_equal(tw, debug_twiddles(nfft))
    out_cplx = int(i.out_is_complex)
    got = debug_epilogue(W, nfft, length, grpd, conj_mode, dc_rule, shift_mode, out_cplx, 2, 0.15)
    assert np.array_equal(got[0], wL.T) and np.array_equal(got[1], wR.T)
    ref = R.epilogue_ref(W, nfft, length, grpd, conj_mode, dc_rule, shift_mode, out_cplx, 2, 0.15)
    r = max(float(R.ratio(g, v, b).max()) for g, (v, b) in zip(got, ref))
    print(f"epilogue of the {kind} design ({Cn} channels, conj_mode {conj_mode}, dc_rule {dc_rule}, shift_mode {shift_mode}): largest error / bound = {r:.4f}")
    assert r <= 1.0
