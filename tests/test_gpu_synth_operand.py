"""The operand the resident sweeps synthesise (sweep_synth.hip, sweep_reg.hip, synth_ls_kernel) against a longdouble sum, step by
step: the Chebyshev coefficients synth_coeff_kernel writes, the microphone map, and the evaluation synth_group<GS> of
synth_common.hpp, run on its own by the debug entry emagls_debug_synth_operand.  Bounds are the a-priori ones of
tests/synth_reference.py (derived there, checked on these inputs by tests/test_synth_reference_host.py), not distances measured
on the kernels.  Thinned grid (901 directions), 128-tap filters, eMagLS2 plans in the real basis on the em32 layout at radii that
give the simulation orders 5, 19, 20, 22 and TOP_ORDER."""
import ctypes as C

import numpy as np
import pytest

import synth_reference as R

pytestmark = pytest.mark.gpu

# The largest simulation order whose plan still reports a synthesising sweep form turned out to be 85, the largest the library
# takes at all (86 orders, rows of 86: the ring's 96 are not reached); every order from 19 up to it synthesises on this grid
# (test_top_order_is_the_largest_synthesising_one).
TOP_ORDER = 85
# eMagLS2's `order` only sets f_cut = 500 Hz x order.  The synthesising sweep needs every swept bin on the Gram route, which a
# 32-microphone array of 1 cm enters at bin 36 only: that plan is designed with f_cut = 7.5 kHz (k_cut 40)
FCUT_ORDER = {5: 15}
ORDERS = tuple(sorted(R.RADIUS_OF_ORDER)) + (TOP_ORDER,)
EPS = R.EPS64


def radius_of(order):
    return R.RADIUS_OF_ORDER.get(order, (order - 0.5) * R.C_SOUND / (R.FS * np.pi))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def synth_operand(bsc, x, gs):
    """(E + O, E - O) [nbins][nx] of the debug entry"""
    from emagls_amd import _lib as L
    bsc = np.ascontiguousarray(bsc, dtype=np.complex128)
    x = np.ascontiguousarray(x, dtype=np.float64)
    gp = np.full((bsc.shape[0], x.size), np.nan + 0j)
    gm = np.full((bsc.shape[0], x.size), np.nan + 0j)
    L.check(L.load().emagls_debug_synth_operand(ptr(bsc), bsc.shape[0], bsc.shape[1], ptr(x), x.size, gs, ptr(gp), ptr(gm)))
    return gp, gm


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


def make_plan(grids, thin, order):
    from emagls_amd import Plan, _lib as L
    r = radius_of(order)
    assert L.load().emagls_simulation_order(L.KIND_EMAGLS2, 4, R.FS, r) == order
    p = Plan(L.KIND_EMAGLS2, "real", FCUT_ORDER.get(order, 4), R.FS, R.TAPS, thin["hL"].shape[0], thin["hL"].shape[1], r, 32)
    p.set_hrir_grid(thin["azi"], thin["zen"])
    p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
    return p


@pytest.fixture(scope="module")
def designs(grids, thin):
    """order -> the executed plan's modal terms, Chebyshev rows and microphone map, with the longdouble reference of the same b_n
    (computed once, shared by the tests below)"""
    R.require_longdouble()
    out = {}
    for order in ORDERS:
        p = make_plan(grids, thin, order)
        p.set_hrirs(thin["hL"], thin["hR"])
        p.execute()
        p.synchronize()
        i = p.info()
        nOrd, P = order + 1, i.num_pos_freqs
        assert (i.sim_order, P) == (order, R.NBINS) and i.sweep_form in (2, 3), (order, i.sim_order, P, i.sweep_form)
        nord_pad = (nOrd + 1) & ~1
        d = dict(order=order, nOrd=nOrd, nord_pad=nord_pad, P=P, sweep_form=i.sweep_form, sweep_units=i.sweep_units,
                 bn=p.debug("bn", np.complex128, (P, nOrd)).copy(), bsc=p.debug("bsc", np.complex128, (P, nord_pad)).copy(),
                 smap=p.debug("smap", np.int32)[:34].copy())
        p.close()
        d["beta"] = R.beta_of_bn(d["bn"], nyquist_last=True)
        d["bsc_ref"] = R.legendre_to_chebyshev(d["beta"])
        out[order] = d
    return out


def test_top_order_is_the_largest_synthesising_one(grids, thin):
    from emagls_amd import _lib as L
    p = make_plan(grids, thin, TOP_ORDER)
    assert p.info().sweep_form in (2, 3)
    p.close()
    try:
        p = make_plan(grids, thin, TOP_ORDER + 1)
    except L.EmaglsError:
        return   # (no plan at all at that order)
    form = p.info().sweep_form
    p.close()
    assert form not in (2, 3)


@pytest.mark.parametrize("order", ORDERS)
def test_chebyshev_coefficients(designs, order):
    """bsc of synth_coeff_kernel against the longdouble conversion of the same plan's b_n, element by element within bound_bsc;
    the Nyquist row comes from the real part of b_n; the padding column of an odd number of orders is exactly zero."""
    d = designs[order]
    nOrd, P, bsc = d["nOrd"], d["P"], d["bsc"]
    assert np.all(np.isfinite(bsc.view(np.float64)))
    bound = R.bound_bsc(d["beta"])
    err = np.abs(R.to_cld(bsc[:, :nOrd]) - d["bsc_ref"]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"order {order}: bsc error / bound_bsc, largest = {ratio.max():.3f} (bin {np.unravel_index(ratio.argmax(), ratio.shape)[0]})")
    assert np.all(err <= bound)
    # Nyquist: b_n has an imaginary part there and the row does not (the reference above was fed the real part)
    assert np.abs(d["bn"][P - 1].imag).max() > 1e-3 * np.abs(d["bn"][P - 1]).max()
    assert np.all(bsc[P - 1].imag == 0) and np.abs(bsc[P - 2].imag).max() > 0
    if nOrd & 1:
        assert d["nord_pad"] == nOrd + 1 and np.all(bsc[:, nOrd] == 0)
    else:
        assert d["nord_pad"] == nOrd


def test_residues_and_orders_covered():
    nords = [o + 1 for o in ORDERS]
    assert {n % 4 for n in nords} == {0, 1, 2, 3} and min(nords) < 8 and 20 in nords
    assert {((n + 1) & ~1) % 4 for n in nords} == {0, 2}   # both residues of the row length: the re-read last pass


@pytest.mark.parametrize("order", ORDERS)
def test_microphone_map(grids, designs, order):
    """smap: rows 0 .. M - 1 are a permutation of the microphones, pairs first; 2 pairs + singles = microphones; every claimed
    pair is antipodal to the host's tolerance (unit vectors cancel to 8 eps per component); the em32 gives 15 or 16 pairs."""
    d = designs[order]
    smap, M = d["smap"], 32
    assert smap.shape == (34,)
    npr, nsg = int(smap[32]), int(smap[33])
    assert sorted(smap[:M].tolist()) == list(range(M))
    assert 2 * npr + nsg == M and npr + nsg == d["sweep_units"] == 17 and npr in (15, 16)
    az, zn = grids["mic_azi"], grids["mic_zen"]
    u = np.stack([np.sin(zn) * np.cos(az), np.sin(zn) * np.sin(az), np.cos(zn)], axis=1)
    for q in range(npr):
        a, b = smap[2 * q], smap[2 * q + 1]
        assert np.abs(u[a] + u[b]).max() <= 8 * EPS, (q, a, b)
    # and the singles have no partner among themselves
    singles = smap[2 * npr:M]
    for a in singles:
        for b in singles:
            assert a == b or np.abs(u[a] + u[b]).max() > 8 * EPS


@pytest.mark.parametrize("order", ORDERS)
def test_evaluation_against_the_legendre_sum(grids, designs, order):
    """synth_group on the plan's own rows: g_plus / g_minus within bound_g of the longdouble Legendre sums at x and -x (every 4th
    bin and the ends), the three group sizes bitwise equal."""
    d = designs[order]
    bins = R.selected_bins(d["P"])
    x = R.eval_points(grids)
    got = {gs: synth_operand(d["bsc"][bins], x, gs) for gs in (2, 3, 4)}
    for gs in (3, 4):
        assert np.array_equal(got[gs][0], got[2][0]) and np.array_equal(got[gs][1], got[2][1]), gs
    gp, gm = got[3]
    assert np.all(np.isfinite(gp.view(np.float64))) and np.all(np.isfinite(gm.view(np.float64)))
    ref = R.legendre_sum(d["beta"][bins], np.concatenate([x, -x]))
    bound = R.bound_g(d["bsc_ref"][bins])
    gmax = np.abs(ref).astype(np.float64).max(axis=1)
    if order <= 22:
        assert np.all(bound <= 1e-12 * gmax)   # (the condition tests/test_synth_reference_host.py checks on the oracle's b_n)
    ep = np.abs(R.to_cld(gp) - ref[:, :x.size]).astype(np.float64)
    em = np.abs(R.to_cld(gm) - ref[:, x.size:]).astype(np.float64)
    ratio = np.maximum(ep, em) / bound[:, None]
    k, i = np.unravel_index(ratio.argmax(), ratio.shape)
    edge = np.abs(x) >= 1.0 - 2.0 ** -52
    print(f"order {order}: |g - Legendre sum| / bound_g: largest {ratio.max():.4f} (bin {bins[k]}, x = {x[i]!r}), at |x| = 1 and its "
          f"neighbours {ratio[:, edge].max():.4f}; largest error / max|g| = {(np.maximum(ep, em).max(axis=1) / gmax).max():.3e}; "
          f"bound_g / max|g| up to {(bound / gmax).max():.2e}")
    assert np.all(ep <= bound[:, None]) and np.all(em <= bound[:, None])
    # the kernel's own series (its FP64 rows taken as exact) at 11 more bits: the evaluation alone, without the conversion's error
    own = R.chebyshev_sum(d["bsc"][bins], np.concatenate([x, -x]))
    eo = np.maximum(np.abs(R.to_cld(gp) - own[:, :x.size]), np.abs(R.to_cld(gm) - own[:, x.size:])).astype(np.float64)
    print(f"order {order}: |g - longdouble Chebyshev sum of the same rows| / bound_g: largest {(eo / bound[:, None]).max():.4f}")
    assert np.all(eo <= bound[:, None])


def test_cosines_as_the_sweeps_form_them(grids, thin):
    """synth_zen / synth_x2 of synth_common.hpp -- what sweep_synth.hip, sweep_reg.hip and synth_ls_kernel evaluate the series at --
    against the host's cosines in the SH matrices' convention (cos(zen), and the sine from it), zeniths at and a rounding outside
    [0, pi] included, directions and microphones.  Tolerance on 2 cos: 16 eps -- cos(dazi) and the two zenith cosines 2 ulp <= eps
    each against the exact ones, four roundings in the two sines (2 eps), three in the products and the fused sum (1.5 eps), all
    doubled (13 eps) -- plus twice what a zenith cosine that is eps off the host's does through sqrt(1 - c^2), which next to a pole
    is most of it (synth_reference.cosines)."""
    from emagls_amd import _lib as L
    R.require_longdouble()
    edge = np.array([0.0, np.pi, np.nextafter(np.pi, 4.0), np.pi + 1e-7, -1e-7, float(np.float32(np.pi)), 0.5 * np.pi])
    azi = np.ascontiguousarray(np.concatenate([thin["azi"], np.linspace(0.3, 5.9, edge.size)]))
    zen = np.ascontiguousarray(np.concatenate([thin["zen"], edge]))
    maz = np.ascontiguousarray(np.concatenate([grids["mic_azi"], [1.0, 2.0, 4.0]]))
    mzn = np.ascontiguousarray(np.concatenate([grids["mic_zen"], [0.0, np.pi + 1e-7, -1e-7]]))
    assert (thin["zen"] > np.pi).sum() >= 1    # the fixtures' own grid holds pi in single precision
    x2 = np.full((azi.size, maz.size), np.nan)
    L.check(L.load().emagls_debug_synth_cosines(ptr(azi), ptr(zen), azi.size, ptr(maz), ptr(mzn), maz.size, ptr(x2)))
    want, allow = R.cosines(azi, zen, maz, mzn, with_allowance=True)
    err = np.abs(x2 - 2.0 * want.astype(R.LD)).astype(np.float64)
    tol = 16 * EPS + 2.0 * allow
    i, j = np.unravel_index((err / tol).argmax(), err.shape)
    print(f"2 cos(direction, microphone), {azi.size} x {maz.size}: largest error {err.max() / EPS:.2f} eps; largest error / tolerance "
          f"{(err / tol).max():.3f} (zenith {zen[i]!r}, microphone zenith {mzn[j]!r}); bitwise equal to the host's: {(x2 == 2.0 * want).mean():.4f}")
    assert np.all(err <= tol) and np.abs(x2).max() <= 2.0
    # (the signed sines would be visibly elsewhere for the zeniths outside, tolerance included)
    signed = np.sin(zen)[:, None] * np.sin(mzn)[None, :] * np.cos(azi[:, None] - maz[None, :]) + np.cos(zen)[:, None] * np.cos(mzn)[None, :]
    outside = (zen > np.pi) | (zen < 0)
    assert (np.abs(2.0 * signed - x2) - tol)[outside].max() > 1e-8


@pytest.fixture(scope="module")
def materialised(grids, thin, designs):
    """Order 19: |G_k - g_k| per bin, microphone and direction, G_k from the materialising pipeline (EMAGLS_SWEEP_SYNTH=0: SH matrices
    times b_n, dspace.hip), g_k synthesised at the host's cosines between all directions and microphones; and the tolerance per bin,
    bound_g + 64 eps max|G_k| (the second term: the SH-product side)."""
    import os
    from emagls_amd import _lib as L
    d = designs[19]
    os.environ["EMAGLS_SWEEP_SYNTH"] = "0"
    L.check(L.load().emagls_cache_clear())
    try:
        p = make_plan(grids, thin, 19)
        p.set_hrirs(thin["hL"], thin["hR"])
        p.set_profiling(1)
        p.execute()
        p.synchronize()
        i = p.info()
        assert i.sweep_form == 1
        D, g0, P = thin["hL"].shape[1], i.g_first, i.num_pos_freqs
        ldD = -(-D // 64) * 64
        G = p.debug("G", np.complex128)[:(P - g0) * 32 * ldD].reshape(P - g0, 32, ldD)[:, :, :D].copy()
        bn0 = p.debug("bn", np.complex128, (P, 20)).copy()
        p.close()
    finally:
        del os.environ["EMAGLS_SWEEP_SYNTH"]
        L.check(L.load().emagls_cache_clear())
    assert np.array_equal(bn0, d["bn"])   # both pipelines start from the same modal terms
    bins = np.array([k for k in R.selected_bins(P) if k >= g0])
    assert bins.size >= 8 and bins[-1] == P - 1
    x = R.cosines(thin["azi"], thin["zen"], grids["mic_azi"], grids["mic_zen"])    # [D][32]
    gp, _ = synth_operand(d["bsc"][bins], x.ravel(), 3)
    gp = gp.reshape(bins.size, D, 32).transpose(0, 2, 1)                               # [bin][microphone][direction] like G
    Gb = G[bins - g0]
    gmax = np.abs(Gb).max(axis=(1, 2))
    assert gmax.min() > 0.1
    return dict(bins=bins, err=np.abs(Gb - gp), gmax=gmax, tol=R.bound_g(d["bsc_ref"][bins]) + 64 * EPS * gmax)


def test_against_the_materialised_operand(thin, materialised):
    """The synthesised operand against the materialised one within bound_g + 64 eps max|G_k|, over all 901 directions -- the one at
    zen = 3.14159274 (pi in single precision, 8.7e-8 beyond the pole) included, where sqrt(1 - cos^2) of the SH matrices stands for
    a sine 1.5 % off: the sweeps form their cosine from the same two numbers (synth_zen), so both mean the same direction.  (With
    sincos in the sweeps that direction was 2.2e-6 max|G| away, signed sine, and 6.8e-9 with |sin|: 45000 times this tolerance.)"""
    m = materialised
    err = m["err"].max(axis=(1, 2))
    k = (err / m["tol"]).argmax()
    pole = np.abs(np.sin(thin["zen"]))
    pole = (pole > 0) & (pole < 1e-3)
    assert pole.sum() == 1
    print(f"order 19: synthesised vs materialised operand, {m['bins'].size} bins x {thin['zen'].size} directions x 32 microphones: largest "
          f"|G - g| / max|G| = {(err / m['gmax']).max():.3e}; largest error / tolerance = {(err / m['tol']).max():.4f} (bin {m['bins'][k]}); "
          f"in the direction next to the pole {(m['err'][:, :, pole].max(axis=(1, 2)) / m['tol']).max():.4f}")
    assert np.all(err <= m["tol"])


@pytest.mark.parametrize("nord_pad", [2, 4, 6, 96])
def test_single_chebyshev_terms(nord_pad):
    """Hand-made rows through the debug entry alone: a single T_m for the first two and the last two terms of a row (a missed first
    pass, an off-by-one in the last pass's re-read), with a real and an imaginary coefficient; the kernel returns T_m(x) and
    (-1)^m T_m(x) within bound_g, which for m <= 3 is replaced by 4 eps."""
    R.require_longdouble()
    ms = sorted({0, 1, nord_pad - 2, nord_pad - 1})
    coef = (1.0 + 0j, -2.0j)
    rows = np.zeros((len(ms) * len(coef), nord_pad), dtype=np.complex128)
    for a, m in enumerate(ms):
        for b, c in enumerate(coef):
            rows[a * len(coef) + b, m] = c
    inner = 1.0 - 2.0 ** -53
    x = np.concatenate([[1.0, -1.0, inner, -inner, 0.0, 0.5, -0.5, np.nextafter(1.0, 2.0)], np.random.default_rng(3).uniform(-1, 1, 300)])
    got = {gs: synth_operand(rows, x, gs) for gs in (2, 3, 4)}
    for gs in (3, 4):
        assert np.array_equal(got[gs][0], got[2][0]) and np.array_equal(got[gs][1], got[2][1]), gs
    gp, gm = got[4]
    for a, m in enumerate(ms):
        t = R.chebyshev_t(m, x)
        for b, c in enumerate(coef):
            r = a * len(coef) + b
            tol = abs(c) * (4 * EPS if m <= 3 else float(R.bound_g(rows[r] / abs(c))[0]))
            ep = np.abs(R.to_cld(gp[r]) - R.to_cld(np.array(c)) * t).astype(np.float64).max()
            em = np.abs(R.to_cld(gm[r]) - R.to_cld(np.array(c)) * ((-1) ** m) * t).astype(np.float64).max()
            print(f"row length {nord_pad}, {c} T_{m}: largest error {max(ep, em):.3e}, tolerance {tol:.3e}")
            assert ep <= tol and em <= tol, (nord_pad, m, c)
            # nothing leaks into the other part
            other = (gp[r].imag, gm[r].imag) if c.imag == 0 else (gp[r].real, gm[r].real)
            assert np.all(other[0] == 0) and np.all(other[1] == 0)
