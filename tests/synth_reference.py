"""High-precision reference of the sweeps' synthesised operand (sweep_synth.hip, synth_common.hpp), in NumPy longdouble.

The resident sweeps rebuild pwGrid_k inside the launch: synth_coeff_kernel converts the bin's Legendre series
    g_k(x) = sum_n beta_n P_n(x),   beta_n = b_n(k) (2n + 1) / (4 pi)
into a Chebyshev series sum_m bsc[m] T_m(x), and synth_group evaluates that with T_{m+1} = 2x T_m - T_{m-1}.  This module holds
the same two steps in 64-bit-mantissa arithmetic (the FP64 b_n are taken as exact inputs) and two A-PRIORI error bounds for the
FP64 kernels.  The bounds are derived below, not measured; tests/test_synth_reference_host.py checks the routines against mpmath
at 50 digits and the inputs of the GPU tests against the bounds, tests/test_gpu_synth_operand.py holds the kernels to them.

Error bounds (eps = 2^-52, unit roundoff u = eps / 2):

bound_bsc[m] = 4 nOrd eps sum_n c_mn |beta_n|.  The kernel forms beta_n with two roundings and a rounded 4 pi (3 u relative),
    lambda(j) by a running product of j rounded quotients (2 j u), c_mn = (2 - delta_m0) lambda((n-m)/2) lambda((n+m)/2) with one
    more rounding (the two indices add up to n < nOrd: (2 n + 1) u together), and adds at most nOrd / 2 + 1 terms with one fused
    operation each ((nOrd / 2 + 1) u on the sum of the moduli).  Together below (1.5 nOrd + 5) u < nOrd eps for nOrd >= 5
    per real part; 4 nOrd eps leaves room for the second-order terms and for the complex modulus.  Every c_mn is in (0, 2], so
    the bound is a sum of non-negative terms.

bound_g = 4 eps sum_m (m^2 / 2 + m + 2) |bsc_m|  (the same for every |x| <= 1).  The forward recurrence commits one rounding
    per step; the computed T~_m = T_m + d_m with d_m = sum_j U_{m-j}(x) r_j, |r_j| <= u |T~_j| (the local error re-enters the
    same recurrence, whose fundamental solution is U), so |d_m| <= u sum_{j<m} |U_j| <= u m (m + 1) / 2 with |U_j| <= j + 1.
    Each term enters its sum (E or O) by one fused operation, counted with one rounding u |bsc_m| and a margin that grows with m:
    u sum_m (m + 2) |bsc_m|.  Per real part that is u sum_m (m^2 / 2 + 1.5 m + 2) |bsc_m|; the factor 4 eps = 8 u in place of u
    covers real and imaginary part in the modulus and the rounding of E + O / E - O.  (The recurrence part is a worst case.  The
    accumulation part counts the rounding that adds a term, not the up to nord_pad / 2 later roundings of the same sum, each
    u times the partial sum: a worst case would weight bsc_0 by nord_pad / 2 + 1 instead of 2.  The factor 8 absorbs that for
    nord_pad <= 20 whatever the series; for longer rows the bound is a first-order estimate where bsc_0 dominates the series.)
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
EPS64 = float(np.finfo(np.float64).eps)
HAVE_LONGDOUBLE = float(np.finfo(LD).eps) < 1e-18
SKIP_REASON = "numpy longdouble has no 64-bit mantissa on this platform (eps = %.1e)" % float(np.finfo(LD).eps)

C_SOUND = 343.0
FS = 48000.0
TAPS = 128                      # filter length of the GPU tests' plans: nfft 256, 129 bins
NBINS = TAPS + 1
# simulation order -> array radius of the GPU tests' plans (eMagLS2: order = max(4, ceil(fs pi r / c))); nOrd = order + 1 covers
# the residues 2, 0, 1, 3 mod 4 (row lengths nord_pad 6, 20, 22, 24: both residues of the last pass), one order below 8, and 19,
# the em32 at its own radius (config 3)
RADIUS_OF_ORDER = {5: 0.0105, 19: 0.042, 20: 0.045, 22: 0.05}


def require_longdouble():
    import pytest
    if not HAVE_LONGDOUBLE:
        pytest.skip(SKIP_REASON)


def ld_pi():
    return 4 * np.arctan(LD(1))


def to_cld(z):
    """complex128 -> clongdouble without a detour that could round (both parts are exact in the wider type)"""
    z = np.asarray(z)
    out = np.zeros(z.shape, dtype=CLD)
    out.real = np.real(z).astype(LD)
    out.imag = np.imag(z).astype(LD)
    return out


def beta_of_bn(bn, nyquist_last=False):
    """beta[k][n] = b_n(k) (2n + 1) / (4 pi) in longdouble; nyquist_last: the last row from the real part of b_n (the Nyquist bin
    is real, dependencies/getSMAIRMatrix.m:115-117)."""
    b = to_cld(np.atleast_2d(bn))
    if nyquist_last:
        b[-1].imag = 0
    n = np.arange(b.shape[1]).astype(LD)
    return b * ((2 * n + 1) / (4 * ld_pi()))[None, :]


def legendre_sum(beta, x):
    """g[k][i] = sum_n beta[k][n] P_n(x[i]) by (n + 1) P_{n+1} = (2n + 1) x P_n - n P_{n-1}, longdouble"""
    beta = np.atleast_2d(beta)
    x = np.asarray(x, dtype=np.float64).astype(LD)
    nOrd = beta.shape[1]
    g = np.zeros((beta.shape[0], x.size), dtype=CLD)
    p0, p1 = np.ones_like(x), x.copy()
    for n in range(nOrd):
        g += beta[:, n, None] * p0[None, :]
        p0, p1 = p1, ((2 * n + 3) * x * p1 - (n + 1) * p0) / LD(n + 2)
    return g


def chebyshev_sum(bsc, x):
    """sum_m bsc[k][m] T_m(x[i]) with the forward recurrence in longdouble (the kernel's own series at 11 more bits)"""
    bsc = to_cld(np.atleast_2d(bsc))
    x = np.asarray(x, dtype=np.float64).astype(LD)
    g = np.zeros((bsc.shape[0], x.size), dtype=CLD)
    t0, t1 = np.ones_like(x), x.copy()
    for m in range(bsc.shape[1]):
        g += bsc[:, m, None] * t0[None, :]
        t0, t1 = t1, 2 * x * t1 - t0
    return g


def chebyshev_t(m, x):
    x = np.asarray(x, dtype=np.float64).astype(LD)
    t0, t1 = np.ones_like(x), x.copy()
    for _ in range(m):
        t0, t1 = t1, 2 * x * t1 - t0
    return t0


def conversion_matrix(nOrd, dtype=LD):
    """c[m][n] of P_n = sum_m c_mn T_m (the comment above synth_coeff_kernel): c_mn = (2 - delta_m0) lambda((n - m) / 2)
    lambda((n + m) / 2) for n >= m, n - m even, lambda(j) = prod_{i < j} (i + 1/2) / (i + 1); zero elsewhere."""
    lam = np.ones(max(nOrd, 1), dtype=dtype)
    for j in range(1, lam.size):
        lam[j] = lam[j - 1] * (dtype(2 * j - 1) / dtype(2 * j))
    c = np.zeros((nOrd, nOrd), dtype=dtype)
    for m in range(nOrd):
        for n in range(m, nOrd, 2):
            c[m, n] = (1 if m == 0 else 2) * lam[(n - m) // 2] * lam[(n + m) // 2]
    return c


def legendre_to_chebyshev(beta):
    """bsc[k][m] = sum_n c_mn beta[k][n], longdouble"""
    beta = np.atleast_2d(beta)
    c = conversion_matrix(beta.shape[1])
    out = np.zeros(beta.shape, dtype=CLD)
    for m in range(beta.shape[1]):
        out[:, m] = (beta[:, m::2] * c[m, m::2][None, :]).sum(axis=1)
    return out


def bound_bsc(beta):
    """[k][m], float64: 4 nOrd eps sum_n c_mn |beta_n|"""
    beta = np.atleast_2d(beta)
    nOrd = beta.shape[1]
    c = conversion_matrix(nOrd).astype(np.float64)
    return 4.0 * nOrd * EPS64 * (np.abs(beta).astype(np.float64) @ c.T)


def bound_g(bsc):
    """[k], float64: 4 eps sum_m (m^2 / 2 + m + 2) |bsc_m| (holds for every |x| <= 1)"""
    a = np.abs(np.atleast_2d(bsc)).astype(np.float64)
    m = np.arange(a.shape[1], dtype=np.float64)
    return 4.0 * EPS64 * (a @ (0.5 * m * m + m + 2.0))


# ---- the inputs of the GPU tests (tests/test_gpu_synth_operand.py), shared with the host test that checks them against the bounds

def plan_kr(radius, nbins=NBINS, fs=FS):
    """kr of a plan's bins: 2 pi f / c r on f = linspace(0, fs / 2, nbins) (dependencies/getSMAIRMatrix.m:90,107)"""
    return 2.0 * np.pi * (np.arange(nbins) * (fs / 2.0) / (nbins - 1)) / C_SOUND * radius


def selected_bins(nbins):
    """every 4th bin and the two at either end"""
    return np.array(sorted(set(range(0, nbins, 4)) | {0, 1, nbins - 2, nbins - 1}))


def zenith_sin_cos(zen):
    """(sine, cosine) of a zenith as the SH matrices take them (MATLAB's legendre sees only the cosine; sh_basis.hip and synth_zen of
    synth_common.hpp follow it): c = fl(cos zen) and s = sqrt(1 - c^2) >= 0 in the same FP64 steps.  A zenith a rounding beyond pi --
    the HRIR grid of the fixtures has one, pi in single precision -- is the direction mirrored back inside; next to a pole s carries
    the rounding of c, u c / s relative to 1."""
    c = np.cos(np.asarray(zen, dtype=np.float64))
    return np.sqrt(np.maximum(0.0, 1.0 - c * c)), c


def cosines(azi, zen, mic_azi, mic_zen, with_allowance=False):
    """cos of the angle between directions and microphones, [D][M], from zenith_sin_cos: the product and sum in longdouble, rounded
    once.  The difference of the azimuths is formed in FP64 as the kernels form it (an IEEE subtraction: the same value there and
    here).  with_allowance: also what a device cosine of the zeniths that is `eps` (2 ulp) off the host's moves the result by,
    d_s = c d_c / s through the sine (sqrt(2 d_c) where s = 0) and d_c itself: |d_sd| sm + sd |d_sm| + d_c (|cd| + |cm|)."""
    a, ma = np.asarray(azi, dtype=np.float64), np.asarray(mic_azi, dtype=np.float64)
    (sd, cd), (sm, cm) = zenith_sin_cos(zen), zenith_sin_cos(mic_zen)
    dazi = (a[:, None] - ma[None, :]).astype(LD)
    v = sd.astype(LD)[:, None] * sm.astype(LD)[None, :] * np.cos(dazi) + cd.astype(LD)[:, None] * cm.astype(LD)[None, :]
    v = np.clip(v, -1, 1).astype(np.float64)
    if not with_allowance:
        return v
    dc = EPS64
    with np.errstate(divide="ignore", invalid="ignore"):
        dsd = np.where(sd > 0, np.abs(cd) * dc / sd, np.sqrt(2 * dc))
        dsm = np.where(sm > 0, np.abs(cm) * dc / sm, np.sqrt(2 * dc))
    return v, dsd[:, None] * sm[None, :] + sd[:, None] * dsm[None, :] + dc * (np.abs(cd)[:, None] + np.abs(cm)[None, :])


def eval_points(grids, ndirs=64, nrandom=300, seed=20):
    """The arguments of the evaluation test: the end points and their neighbours inside (the kernel's 2 cos can be any of them),
    nextafter(1, 2) one ulp outside, 0, +-0.5, the true cosines between the first `ndirs` directions of the thinned HRIR grid and
    the em32's microphones, and random values."""
    sub = slice(0, 2702, 3)
    azi, zen = grids["azi"][sub][:ndirs], grids["zen"][sub][:ndirs]
    inner = 1.0 - 2.0 ** -53
    special = np.array([1.0, -1.0, inner, -inner, 0.0, 0.5, -0.5, np.nextafter(1.0, 2.0)])
    rnd = np.random.default_rng(seed).uniform(-1.0, 1.0, nrandom)
    return np.concatenate([special, cosines(azi, zen, grids["mic_azi"], grids["mic_zen"]).ravel(), rnd])


# ---- one bin step of the resident sweeps (sweep_synth.hip, sweep_reg.hip) in longdouble, with an a-priori bound for the FP64 kernels
#
# The chain of a design runs in the microphone domain, rows in the order of `smap` (npr antipodal pairs in rows 2u, 2u + 1, then nsg
# single microphones).  With the totals u(k-1) [ear][row] the chain stored, Mt(k-1) = Pm^T M(k-1) Pm, |H(k)| and the operand
# g_k[d][row] one bin is
#     w' = u(k-1) conj(Mt(k-1)),    p_d = sum_j w'_j g_k[d][j],    t_d = |H_d| p_d / |p_d|,    u(k)_j = sum_d t_d conj(g_k[d][j])
# (the first swept bin takes w' = Winit as it stands; the Nyquist bin keeps the real part of t; p_d = 0 gives t_d = |H_d|:
# unit_phase of persist_common.hpp).  A unit's operand is E + O (first row) and E - O (second row of a pair) with E, O the even and odd
# part of the series at the FIRST microphone's cosine: the second row is g(-x) at that same x.
#
# bound_step, per element of u(k), on |kernel - longdouble step| (moduli of complex numbers).  eps = 2^-52; gamma_n = n eps / (1 - n eps).
# A sum of n complex products, in any order, with or without fused operations, has 2 n real products per component: each component is
# within gamma^u_{2n} = gamma_n (u = eps / 2) times the sum of the moduli, the modulus within sqrt(2) gamma_n <= gamma_{2n+2}.
#   operand   dg = bound_g of the bin: the series is evaluated at the kernel's own arguments (the GPU test reads 2 cos(direction,
#             microphone) as the sweeps form it, synth_x2, and holds it to `cosines` within the tolerance of the operand test), so what
#             is left is the evaluation.  bound_g covers E and O together (its recurrence part is per term, its factor 8 the roundings
#             of E +- O), so |dE| + |dO| <= dg as well.
#   w'        dw'_j = gamma_{2M+2} sum_i |u_i| |Mt_ij|   (M products; zero for the first swept bin).
#   p_d       the register form multiplies E and O apart, with the weights w'_A + w'_B and w'_A - w'_B of a pair (both w' for a single
#             microphone): 2 units products, each weight one rounding more, and the moduli that enter are
#                 A_d = sum_units (|w'_A| + |w'_B|) (|E_d| + |O_d|)   >=   sum_j |w'_j| |g_dj|   (what the slab form sums),
#             so  dp_d = gamma_{4 units + 2} A_d + sum_units (|w'_A| + |w'_B|) dg + sum_units (dw'_A + dw'_B) (|E_d| + |O_d|).
#             (gamma_{2M+2} sum_j |w'_j| |g_dj| would hold for the slab form alone: with E and O apart a pair whose g(x) is small against
#             E and O has a larger rounding error than that, and an array without pairs has 2 M products.)
#   phase     two unit vectors whose directions p, p + dp differ by r = dp / |p| < 1 are 2 sin(asin(r) / 2) apart at most (= r to first
#             order), any two by 2:  dphi_d = that, and dt_d = |H_d| (dphi_d + 4 eps): |p|^2 two roundings (one after the square root),
#             the reciprocal square root 2 u (fast_rsqrt), the products with |H| and with p one each: 5 u < 4 eps.  A direction with a
#             tiny |p_d| widens the bound through its own dphi_d; none is left out.
#   sum       du_j = gamma_{D+c} sum_d |H_d| m_dj + sum_d dt_d m_dj + sum_d |H_d| dg,   m_dj = |E_d| + |O_d| of row j's unit (>= |g_dj|;
#             the register form sums t conj(E) and t conj(O) and adds or subtracts them at the end), c = ceil((sqrt(2) - 1) D) + 4:
#             D products and one more addition per component (gamma_{D+1}), sqrt(2) for the modulus.
# Second-order terms (a gamma times a gamma) are left to the margins above (eps where u would do for the roundings of single values).

def gamma(n):
    return n * EPS64 / (1.0 - n * EPS64)


def f64(a):
    return np.asarray(a).astype(np.float64)


def unit_rows(npr, nsg):
    """(first row, second row or -1) of every unit in the chain's row order"""
    a = np.array([2 * u for u in range(npr)] + [2 * npr + s for s in range(nsg)], dtype=int)
    b = np.array([2 * u + 1 for u in range(npr)] + [-1] * nsg, dtype=int)
    return a, b


def step_operand(bsc, x, smap):
    """The operand of the bins `bsc` holds rows of, in the chain's row order: g [k][D][M] (clongdouble), m [k][D][M] = |E| + |O| of the
    row's unit, dg [k][D][M] the operand term of bound_step, and (npr, nsg).  The series is the kernel's own (its FP64 rows taken as
    exact, chebyshev_sum); x [D][units]: the cosine between direction and FIRST microphone of every unit (smap[unit_rows(...)[0]])."""
    smap = np.asarray(smap)
    npr, nsg = int(smap[32]), int(smap[33])
    M = 2 * npr + nsg
    ra, rb = unit_rows(npr, nsg)
    x = np.asarray(x, dtype=np.float64)
    D, U = x.shape
    assert U == ra.size
    bsc = np.atleast_2d(bsc)
    gp = chebyshev_sum(bsc, x.ravel()).reshape(-1, D, U)
    gm = chebyshev_sum(bsc, -x.ravel()).reshape(-1, D, U)
    mu = (np.abs(gp + gm) / 2 + np.abs(gp - gm) / 2).astype(np.float64)
    g = np.zeros((bsc.shape[0], D, M), dtype=CLD)
    m = np.zeros((bsc.shape[0], D, M))
    g[:, :, ra] = gp
    m[:, :, ra] = mu
    pr = rb >= 0
    g[:, :, rb[pr]] = gm[:, :, pr]
    m[:, :, rb[pr]] = mu[:, :, pr]
    dg = np.broadcast_to(bound_g(bsc)[:, None, None], m.shape)
    return g, m, dg, (npr, nsg)


def sweep_step(u_prev, Mt_prev, habs_k, g_k, nyquist=False, w_start=None):
    """One bin in clongdouble: u_prev [2][M], Mt_prev [M][M], habs_k [2][D], g_k [D][M] -> (u_k [2][M], w' [2][M], p [2][D], t [2][D]).
    w_start: the first swept bin, whose w' is the start value as it stands (u_prev and Mt_prev are not read)."""
    g = g_k if g_k.dtype == CLD else to_cld(g_k)
    w = to_cld(w_start) if w_start is not None else to_cld(u_prev) @ np.conj(to_cld(Mt_prev))
    p = w @ g.T
    a = np.abs(p)
    h = np.asarray(habs_k, dtype=np.float64).astype(LD)
    t = np.zeros(p.shape, dtype=CLD)
    nz = a > 0
    t[nz] = h[nz] * p[nz] / a[nz]
    t[~nz] = h[~nz]
    if nyquist:
        t.imag = 0
    return t @ np.conj(g), w, p, t


def bound_step(u_prev, Mt_prev, habs_k, g_k, m_k, dg_k, units, nyquist=False, w_start=None, step=None):
    """[2][M], float64: the a-priori bound derived above on |FP64 kernel - sweep_step| per element of u_k.  m_k, dg_k [D][M] and units =
    (npr, nsg) from step_operand; step: the tuple sweep_step returned for the same arguments (computed when omitted)."""
    if step is None:
        step = sweep_step(u_prev, Mt_prev, habs_k, g_k, nyquist, w_start)
    _, w, p, _ = step
    D, M = m_k.shape
    ra, rb = unit_rows(*units)
    nun = ra.size
    h = np.asarray(habs_k, dtype=np.float64)
    aw = f64(np.abs(w))
    dw = np.zeros_like(aw) if w_start is not None else gamma(2 * M + 2) * (np.abs(np.asarray(u_prev)).astype(np.float64) @ np.abs(np.asarray(Mt_prev)).astype(np.float64))
    pr = rb >= 0
    ws, dws = aw[:, ra].copy(), dw[:, ra].copy()
    ws[:, pr] += aw[:, rb[pr]]
    dws[:, pr] += dw[:, rb[pr]]
    mu, dgu = m_k[:, ra], dg_k[:, ra]                                           # [D][units]
    dp = gamma(4 * nun + 2) * (ws @ mu.T) + ws @ dgu.T + dws @ mu.T              # [2][D]
    ap = f64(np.abs(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ap > 0, dp / ap, np.inf)
    dphi = np.where(r < 1.0, 2.0 * np.sin(0.5 * np.arcsin(np.minimum(r, 1.0))), 2.0)
    dt = h * (dphi + 4 * EPS64)
    c = int(np.ceil((np.sqrt(2.0) - 1.0) * D)) + 4
    return gamma(D + c) * (h @ m_k) + dt @ m_k + h @ dg_k


def step_ratio(u_got, u_ref, bound):
    """|u_got - u_ref| / bound, element by element (inf where a zero bound is missed)"""
    err = f64(np.abs(to_cld(u_got) - u_ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))


def mt_from(Mk, Pm):
    """Pm^T M Pm in clongdouble (synth_mt_kernel: M Pm first) and its bound gamma_{2C+2} (|Pm|^T |M Pm| + |Pm|^T |M| |Pm|): two sums of C
    products of a complex and a real factor each, the first one's error carried through the second.  Mk [C][C], Pm [C][M] real."""
    C = Mk.shape[0]
    P = np.asarray(Pm, dtype=np.float64).astype(LD)
    tmp = to_cld(Mk) @ P
    aP = np.abs(np.asarray(Pm, dtype=np.float64))
    gm = gamma(2 * C + 2)
    return P.T @ tmp, gm * (aP.T @ f64(np.abs(tmp)) + aP.T @ (np.abs(np.asarray(Mk)).astype(np.float64) @ aP))


def rows_from_totals(u_k, Pm, Mk):
    """W(k,:) = (u_k Pm^T) conj(M_k) in clongdouble (synth_rows_kernel) and its bound gamma_{2C+2} |u Pm^T| |M| + gamma_{2M+2} (|u| |Pm|^T) |M|.
    u_k [2][M], Pm [C][M] real, Mk [C][C]."""
    C, M = np.asarray(Pm).shape
    P = np.asarray(Pm, dtype=np.float64).astype(LD)
    v = to_cld(u_k) @ P.T
    aM = np.abs(np.asarray(Mk)).astype(np.float64)
    dv = gamma(2 * M + 2) * (np.abs(np.asarray(u_k)).astype(np.float64) @ np.abs(np.asarray(Pm, dtype=np.float64)).T)
    return v @ np.conj(to_cld(Mk)), gamma(2 * C + 2) * (f64(np.abs(v)) @ aM) + dv @ aM


def jittered_array(n, seed=None):
    """An array of n microphones without an antipodal pair: a jittered spherical Fibonacci lattice (well conditioned; the arrays of
    tests/test_gpu_sweep_reg_mfma.py)"""
    i = np.arange(n) + 0.5
    zen = np.arccos(1 - 2 * i / n)
    azi = np.mod(np.pi * (1 + 5 ** 0.5) * i, 2 * np.pi)
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    azi = azi + 0.05 * rng.standard_normal(n)
    zen = np.clip(zen + 0.05 * rng.standard_normal(n), 0.05, np.pi - 0.05)
    return azi, zen
