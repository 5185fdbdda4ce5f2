"""The longdouble reference of the synthesised operand (tests/synth_reference.py) against mpmath at 50 digits, and the inputs of
tests/test_gpu_synth_operand.py against the a-priori bounds: a GPU test that holds the kernel to bound_g says something only where
bound_g is small against the operand itself."""
import numpy as np
import pytest

import synth_reference as R
from oracle import emagls_oracle as O

NORDS = (5, 6, 20, 21, 22, 23, 86)    # numbers of orders (simulation order + 1): 86 is the largest the library takes
KR = (1e-3, 0.03, 0.4, 2.0, 7.5, 19.0, 45.0, 90.0)


@pytest.fixture(scope="module")
def points():
    R.require_longdouble()
    inner = 1.0 - 2.0 ** -53
    return np.concatenate([[1.0, -1.0, inner, -inner, 0.0], np.random.default_rng(7).uniform(-1.0, 1.0, 200)])


def mp_series(mp, bn_row, xs):
    """(Legendre sum, Chebyshev coefficients, Chebyshev sum) of one bin in mpmath: the same formulas, term by term"""
    nOrd = len(bn_row)
    beta = [mp.mpc(float(b.real), float(b.imag)) * (2 * n + 1) / (4 * mp.pi) for n, b in enumerate(bn_row)]
    lam = [mp.mpf(1)]
    for j in range(1, nOrd):
        lam.append(lam[-1] * mp.mpf(2 * j - 1) / (2 * j))
    bsc = [sum(((1 if m == 0 else 2) * lam[(n - m) // 2] * lam[(n + m) // 2] * beta[n] for n in range(m, nOrd, 2)), mp.mpc(0)) for m in range(nOrd)]
    leg, che = [], []
    for xv in xs:
        x = mp.mpf(float(xv))
        p0, p1, t0, t1, gl, gc = mp.mpf(1), x, mp.mpf(1), x, mp.mpc(0), mp.mpc(0)
        for n in range(nOrd):
            gl += beta[n] * p0
            gc += bsc[n] * t0
            p0, p1 = p1, ((2 * n + 3) * x * p1 - (n + 1) * p0) / (n + 2)
            t0, t1 = t1, 2 * x * t1 - t0
        leg.append(gl)
        che.append(gc)
    return beta, bsc, leg, che


def ld_minus_mp(mp, a_ld, b_mp):
    """|a - b| with a in longdouble (split into two doubles, exact) and b in mpmath"""
    def mpf_of(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - R.LD(hi)))
    return float(abs(mp.mpc(mpf_of(a_ld.real), mpf_of(a_ld.imag)) - b_mp))


@pytest.mark.parametrize("nord", NORDS)
def test_longdouble_routines_against_mpmath(points, nord):
    """Legendre sum and Legendre-to-Chebyshev conversion in longdouble agree with 50-digit arithmetic to 1e-17 sum|beta_n|, and in
    50 digits the converted series IS the Legendre series: sum_m bsc_m T_m(x) = sum_n beta_n P_n(x)."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    bn = -O.sphModalCoeffs(nord - 1, np.array(KR))
    beta_ld = R.beta_of_bn(bn)
    g_ld = R.legendre_sum(beta_ld, points)
    bsc_ld = R.legendre_to_chebyshev(beta_ld)
    worst_g = worst_c = worst_id = 0.0
    for k in range(len(KR)):
        beta, bsc, leg, che = mp_series(mp, bn[k], points)
        scale = float(sum(abs(b) for b in beta))
        assert scale > 0
        for i in range(points.size):
            worst_g = max(worst_g, ld_minus_mp(mp, g_ld[k, i], leg[i]) / scale)
            worst_id = max(worst_id, float(abs(che[i] - leg[i])) / scale)
        for m in range(nord):
            worst_c = max(worst_c, ld_minus_mp(mp, bsc_ld[k, m], bsc[m]) / scale)
    print(f"{nord} orders: longdouble vs 50 digits, relative to sum|beta|: Legendre sum {worst_g:.2e}, conversion {worst_c:.2e}; "
          f"Chebyshev series - Legendre series in 50 digits {worst_id:.2e}")
    assert worst_g <= 1e-17 and worst_c <= 1e-17
    assert worst_id <= 1e-40


def test_conversion_matrix_entries():
    """every c_mn of the pattern lies in (0, 2], the rest is zero, and the columns sum to P_n(1) = 1"""
    R.require_longdouble()
    c = R.conversion_matrix(96)
    m, n = np.indices(c.shape)
    pattern = (n >= m) & ((n - m) % 2 == 0)
    assert np.all(c[pattern] > 0) and np.all(c[pattern] <= 2) and np.all(c[~pattern] == 0)
    assert np.abs(c.sum(axis=0) - 1).max() < 1e-17


@pytest.mark.parametrize("order", sorted(R.RADIUS_OF_ORDER))
def test_gpu_test_inputs_are_well_inside_the_bounds(grids, order):
    """The GPU tests' own inputs (the plans' radii, bins and arguments, with b_n from the oracle -- the device's agree with it to
    1e-12, tests/test_gpu_stages.py): at orders up to 22 bound_g <= 1e-12 max|g| in every bin, so an operand within bound_g is an
    operand right to twelve digits of its largest value, not a vacuous statement."""
    R.require_longdouble()
    assert order <= 22
    radius = R.RADIUS_OF_ORDER[order]
    assert O.emagls2_simulation_order(R.FS, radius) == order
    bn = -O.sphModalCoeffs(order, R.plan_kr(radius))
    assert bn.shape == (R.NBINS, order + 1)
    bins = R.selected_bins(R.NBINS)
    beta = R.beta_of_bn(bn, nyquist_last=True)[bins]
    x = R.eval_points(grids)
    assert x.size == 8 + 64 * 32 + 300 and np.abs(x).max() <= np.nextafter(1.0, 2.0)
    g = R.legendre_sum(beta, np.concatenate([x, -x]))
    gmax = np.abs(g).astype(np.float64).max(axis=1)
    bg = R.bound_g(R.legendre_to_chebyshev(beta))
    ratio = bg / gmax
    print(f"order {order} (radius {radius} m): bound_g / max|g| over the bins: {ratio.min():.2e} ... {ratio.max():.2e}")
    assert np.all(ratio <= 1e-12)
    # and the coefficient bound against the coefficients' own scale
    bb = R.bound_bsc(beta)
    assert np.all(bb.sum(axis=1) <= 1e-12 * np.abs(beta).astype(np.float64).sum(axis=1))
