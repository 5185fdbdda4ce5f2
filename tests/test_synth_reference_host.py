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


# ---- the longdouble bin step (synth_reference.sweep_step) and its a-priori bound, on host-made inputs of the GPU tests' geometries

def microphone_map(maz, mzn):
    """smap as synth_pairing (plan_setup.hip) orders the rows: antipodal pairs (unit vectors cancel to 8 eps) first, then the singles"""
    M = len(maz)
    u = np.stack([np.sin(mzn) * np.cos(maz), np.sin(mzn) * np.sin(maz), np.cos(mzn)], axis=1)
    partner = [-1] * M
    for j in range(M):
        if partner[j] >= 0:
            continue
        for k in range(j + 1, M):
            if partner[k] < 0 and np.abs(u[j] + u[k]).max() <= 8 * R.EPS64:
                partner[j], partner[k] = k, j
                break
    smap = np.zeros(34, dtype=np.int32)
    rows = [x for j in range(M) if partner[j] > j for x in (j, partner[j])]
    singles = [j for j in range(M) if partner[j] < 0]
    smap[:M] = rows + singles
    smap[32], smap[33] = len(rows) // 2, len(singles)
    return smap


def ordered_sum(a, axis, order):
    """sum over `axis` in plain FP64, in a fixed order: forward, reversed, or pairwise (neighbours first)"""
    a = np.moveaxis(a, axis, 0)
    if order == "forward":
        return np.cumsum(a, axis=0)[-1]
    if order == "reversed":
        return np.cumsum(a[::-1], axis=0)[-1]
    while a.shape[0] > 1:
        if a.shape[0] & 1:
            a = np.concatenate([a, np.zeros_like(a[:1])], axis=0)
        a = a[0::2] + a[1::2]
    return a[0]


def fp64_step(u_prev, Mt_prev, habs, g, order, nyquist=False):
    """the step in complex128, every sum in the given order"""
    w = ordered_sum(u_prev[:, :, None] * np.conj(Mt_prev)[None, :, :], 1, order)             # [2][M]
    p = ordered_sum(w[:, None, :] * g[None, :, :], 2, order)                                  # [2][D]
    a = np.sqrt(p.real * p.real + p.imag * p.imag)
    t = np.where(a > 0, habs * p / np.where(a > 0, a, 1.0), habs + 0j)
    if nyquist:
        t = t.real + 0j
    return ordered_sum(t[:, :, None] * np.conj(g)[None, :, :], 1, order)                     # [2][M]


STEP_GEOMETRIES = {
    # name: (microphones, directions, radius, simulation order, first swept bin) -- the direction-count edge case of
    # tests/test_gpu_sweep_step.py (12 microphones without a pair, order-5 radius, f_cut 7.5 kHz, one direction more than a workgroup of
    # four waves), a seven-microphone slab case, and the em32 at its own radius on the thin grid (order 19, 15 pairs and 2 singles)
    "12 microphones, 129 directions": (12, 129, R.RADIUS_OF_ORDER[5], 5, 39),
    "7 microphones, 65 directions": (7, 65, 0.042, 19, 5),
    "em32, 901 directions": (32, 901, R.RADIUS_OF_ORDER[19], 19, 10),
}


@pytest.fixture(scope="module")
def step_inputs(grids):
    """name -> the inputs of every selected swept bin, from an FP64 chain over the swept bins: totals of the previous bin, Mt of the
    previous bin (the regularised inverse Gram matrix of its operand, as the oracle clips the singular values at 0.01 of the
    largest), |H|, the longdouble operand with its moduli and operand bound.  Computed once."""
    from emagls_amd import synth
    R.require_longdouble()
    out = {}
    for name, (M, D, radius, order, kfirst) in STEP_GEOMETRIES.items():
        if M == 32:
            sub = slice(0, 2702, 3)
            azi, zen, maz, mzn = grids["azi"][sub], grids["zen"][sub], grids["mic_azi"], grids["mic_zen"]
        else:
            (azi, zen), (maz, mzn) = synth.fibonacci_grid(D), R.jittered_array(M)
        assert azi.size == D and O.emagls2_simulation_order(R.FS, radius) == order
        hL, hR = synth.rigid_sphere_hrirs(azi, zen)
        habs = np.abs(np.stack([np.fft.rfft(hL, 2 * R.TAPS, axis=0), np.fft.rfft(hR, 2 * R.TAPS, axis=0)]))   # [2][P][D]
        H = np.stack([np.fft.rfft(hL, 2 * R.TAPS, axis=0), np.fft.rfft(hR, 2 * R.TAPS, axis=0)])
        smap = microphone_map(maz, mzn)
        assert (int(smap[32]), int(smap[33])) == ((15, 2) if M == 32 else (0, M))
        bn = -O.sphModalCoeffs(order, R.plan_kr(radius))
        nord_pad = (order + 2) & ~1
        bsc = np.zeros((R.NBINS, nord_pad), dtype=np.complex128)     # the kernel's rows: FP64, zero padded
        bsc[:, :order + 1] = R.legendre_to_chebyshev(R.beta_of_bn(bn, nyquist_last=True)).astype(np.complex128)
        P = R.NBINS
        bins = np.array(sorted({k for k in R.selected_bins(P) if k >= kfirst} | {kfirst, P - 1}))
        # the FP64 chain: operand and Mt of every bin from kfirst - 1 on, the totals from the least-squares bin kfirst - 1
        ra, rb = R.unit_rows(int(smap[32]), int(smap[33]))
        xu = R.cosines(azi, zen, maz[smap[ra]], mzn[smap[ra]])     # [D][units]: to the first microphone of every unit

        def g64(k):
            g = np.zeros((D, M), dtype=np.complex128)
            cheb = np.polynomial.chebyshev.chebval
            g[:, ra] = cheb(xu, bsc[k].real) + 1j * cheb(xu, bsc[k].imag)
            gm = cheb(-xu, bsc[k].real) + 1j * cheb(-xu, bsc[k].imag)
            g[:, rb[rb >= 0]] = gm[:, rb >= 0]
            return g

        def mt64(g):
            U, s, _ = np.linalg.svd(g.T, full_matrices=False)
            return np.conj((U / (s * np.maximum(s, 0.01 * s[0]))[None, :]) @ U.conj().T)

        gk = g64(kfirst - 1)
        u = H[:, kfirst - 1, :] @ np.conj(gk)
        prev, Mt = {}, mt64(gk)
        for k in range(kfirst, P):
            prev[k] = (u, Mt)
            gk = g64(k)
            u = fp64_step(u, Mt, habs[:, k, :], gk, "forward", nyquist=(k == P - 1))
            Mt = mt64(gk)
        g, m, dg, units = R.step_operand(bsc[bins], xu, smap)
        out[name] = dict(bins=bins, P=P, units=units, D=D, M=M,
                         steps=[dict(k=int(k), u_prev=prev[k][0], Mt_prev=prev[k][1], habs=habs[:, k, :], g=g[i], m=m[i], dg=dg[i], nyquist=(k == P - 1))
                                for i, k in enumerate(bins)])
    return out


@pytest.mark.parametrize("name", ["12 microphones, 129 directions", "em32, 901 directions"])
def test_step_bound_holds_for_fp64_in_three_summation_orders(step_inputs, name):
    """Validity: the step in plain FP64 NumPy with every sum forward, reversed and pairwise lies within bound_step of the longdouble
    step, element by element, in every selected swept bin (the first and the Nyquist bin included)."""
    d = step_inputs[name]
    worst = {}
    for s in d["steps"]:
        ref = R.sweep_step(s["u_prev"], s["Mt_prev"], s["habs"], s["g"], nyquist=s["nyquist"])
        bound = R.bound_step(s["u_prev"], s["Mt_prev"], s["habs"], s["g"], s["m"], s["dg"], d["units"], nyquist=s["nyquist"], step=ref)
        assert np.all(np.isfinite(bound)) and np.all(bound > 0)
        g64 = s["g"].astype(np.complex128)
        for order in ("forward", "reversed", "pairwise"):
            ratio = R.step_ratio(fp64_step(s["u_prev"], s["Mt_prev"], s["habs"], g64, order, s["nyquist"]), ref[0], bound)
            worst[order] = max(worst.get(order, 0.0), float(ratio.max()))
            assert np.all(ratio <= 1.0), (name, s["k"], order, float(ratio.max()))
    print(f"{name}: FP64 step / bound_step over {len(d['steps'])} bins, largest: " + ", ".join(f"{o} {v:.4f}" for o, v in worst.items()))
    assert min(worst.values()) > 0    # (the three orders do differ from the longdouble step)


@pytest.mark.parametrize("name", ["12 microphones, 129 directions", "7 microphones, 65 directions"])
def test_step_bound_is_sharp_enough_to_reject_injected_errors(step_inputs, name):
    """Sharpness: a u_k in which one direction's t_d is 1e-9 relative off (one ear, a direction in the middle of the grid), a u_k
    in which one unit's contribution of the last direction entered with the wrong sign, and a u_k whose every t_d is 1e-10 relative too
    long (a normalisation p / |p| that far off) each miss the bound in at least 90 % of the selected swept bins.  This is a condition on the inputs: a geometry whose conditioning or direction count makes bound_step too wide
    to see 1e-9 in one of D directions does not belong here (the em32 on 901 directions does not: D gamma_D alone is 2e-10 there)."""
    d = step_inputs[name]
    D, M = d["D"], d["M"]
    dmid, ulast = D // 2, R.unit_rows(*d["units"])[0][-1]
    hit_t = hit_s = hit_n = 0
    least_t = least_s = np.inf
    for s in d["steps"]:
        u, w, p, t = R.sweep_step(s["u_prev"], s["Mt_prev"], s["habs"], s["g"], nyquist=s["nyquist"])
        bound = R.bound_step(s["u_prev"], s["Mt_prev"], s["habs"], s["g"], s["m"], s["dg"], d["units"], nyquist=s["nyquist"], step=(u, w, p, t))
        bad_t = u.copy()
        bad_t[0] += R.LD(1e-9) * t[0, dmid] * np.conj(s["g"][dmid])
        bad_s = u.copy()
        bad_s[:, ulast] -= 2 * t[:, D - 1] * np.conj(s["g"][D - 1, ulast])
        rt, rs = R.step_ratio(bad_t, u, bound).max(), R.step_ratio(bad_s, u, bound).max()
        hit_t += rt > 1.0
        hit_s += rs > 1.0
        hit_n += R.step_ratio(u * (1 + R.LD(1e-10)), u, bound).max() > 1.0
        least_t, least_s = min(least_t, rt), min(least_s, rs)
        assert R.step_ratio(u, u, bound).max() == 0.0
    n = len(d["steps"])
    print(f"{name}: t_d off by 1e-9 rejected in {hit_t} of {n} bins (smallest error / bound {least_t:.2f}); wrong sign of the last direction "
          f"rejected in {hit_s} of {n} (smallest {least_s:.3g}); every t_d 1e-10 too long rejected in {hit_n} of {n}")
    assert n >= 20 and hit_t >= 0.9 * n and hit_s >= 0.9 * n and hit_n >= 0.9 * n


def test_rows_and_mt_references_against_fp64():
    """mt_from and rows_from_totals: FP64 NumPy products lie within their bounds of the longdouble ones, and a single flipped sign in Pm
    does not."""
    R.require_longdouble()
    rng = np.random.default_rng(5)
    C, M = 25, 32
    Mk = rng.standard_normal((C, C)) + 1j * rng.standard_normal((C, C))
    Pm = rng.standard_normal((C, M))
    u = rng.standard_normal((2, M)) + 1j * rng.standard_normal((2, M))
    mt, bmt = R.mt_from(Mk, Pm)
    w, bw = R.rows_from_totals(u, Pm, Mk)
    assert mt.shape == (M, M) and w.shape == (2, C)
    r_mt = R.step_ratio(Pm.T @ (Mk @ Pm), mt, bmt).max()
    r_w = R.step_ratio((u @ Pm.T) @ np.conj(Mk), w, bw).max()
    print(f"FP64 / bound: Pm^T M Pm {r_mt:.4f}, rows from totals {r_w:.4f}")
    assert 0 < r_mt <= 1.0 and 0 < r_w <= 1.0
    Pb = Pm.copy()
    Pb[3, 7] = -Pb[3, 7]
    assert R.step_ratio(Pb.T @ (Mk @ Pb), mt, bmt).max() > 1e6 and R.step_ratio((u @ Pb.T) @ np.conj(Mk), w, bw).max() > 1e6
