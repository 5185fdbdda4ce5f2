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
