"""The operand chain of the two equatorial-array designs (csrc/array_model.hpp, csrc/emash.hip, csrc/dspace.hip) against a truth that shares
nothing with the library or the CPU oracle.  CPU only; tests/test_ema_reference_host.py proves this module, tests/test_gpu_ema_operands.py holds
the kernels to it.

    mic_azi --CH, pinv--> Zlo --x Y_mic--> Ech --diag(Nnm)--> E0 --\
    (azi_d, pi/2) --SH--> Ycm, Yc ---------------------------------qt--> QT0 --x Rot_d--> QT --sum_n b_n(k)--> G_k
    (azi_d, zen_d) --rot_points--> fit points --SH--> Arot --pinv(B) A_d--> Rot_d --/
    EMAinCH: E = Zlo Y_mic, SH of the grid itself, no Nnm, no Rot.

The SHs of a direction within sqrt(u) of a pole are the one place where the library and the oracle, which both restate MATLAB's
legendre(n, cos(zen)) and so take sin = sqrt(1 - cos^2), differ from the SHs of the angle by more than rounding (4.4e-9 at zen = 1e-9, order 7).
The truth here stays the SHs of the angle; sh_cos_allowance derives what an evaluation through the cosine may differ by, and the EMAinCH
cases, whose grids hold zen = 0, pi and 1e-9, grant it entry by entry on top of the level.  EMAinSH never evaluates an SH there.

Truth.  mpmath at DPS digits for the special functions and the small dense algebra: the SH and CH bases from the derivative form of the Legendre
polynomials (sin from sin, not from sqrt(1 - cos^2)), b_n of the rigid sphere from Bessel functions, pinv of the M x (2N + 1) CH matrix, Nnm in
closed form, and the EXACT rotation Rot_d -- the SH representation of the right-hand rotation by alpha = pi/2 - zen_d about (sin azi, -cos azi, 0),
R = Rz(azi) Ry(-alpha) Rz(-azi), from Wigner's small d by the factorial sum, D^l_{m'm} = e^{-i m' azi} d^l_{m'm}(-alpha) e^{i m azi}, with
Rot[(l, m)][(l, m')] = D^l_{m'm} in the complex basis and U D U^H in the real one (Y_real = U Y_complex).  No fit.  alpha is the DOUBLE
fl(pi/2 - zen_d), as the kernel forms it.  np.longdouble for everything large: the SH matrices (normalised three-term recurrence), the sums.
Conventions: DESIGN.md and oracle.emagls_oracle -- ACN, Condon-Shortley phase in the complex basis and cancelled in the real one, c = 343 m/s,
row convention c' = c Rot with Y_i(R^-1 x) = sum_j Rot_ij Y_j(x).

Bounds of the steps that are sums (u = 2^-53, gamma_n and the component-wise measure of complex results: tests/gram_reference.py), each on the
DEVICE output of the step before it; "terms" entry by entry:

    Ech     M + 1        small_gemm_kernel: complex arithmetic in either basis, one chain over the M microphones, product and sum unfused
    E0      4            the constant 1 / sqrt 2, Nnm = Ypts[c][c] / chval, Nnm Ech: no sum, a handful of roundings
    Rot     npts         one chain over the fit points: Rot_d[i][j] = sum_p Z[j][p] A[i][d npts + p]
    QT0     2 n + 2      two chains over the 2 n + 1 columns of order n and their sum
    QT      2 l + 1      one chain over the rows of the order-l block of Rot_d, on QT0 carried with its own bound
    G       nOrd + 1     two chains over the orders (the zero padding of the table adds nothing) and their sum; complex b_n times real or
                         complex order terms

Levels of the steps that are not sums -- SH entries, b_n, kr, the rotated fit points through acos / atan2, both pseudo-inverses, and the fit as
a whole against the exact Rot_d: not fixed in advance but MEASURED, as the error of the double-precision oracle (or of a NumPy restatement of the
kernel's formulas) against this truth on the inputs of the cases below, by measure_levels() (python tests/ema_reference.py prints them; the host
test asserts that a fresh measurement lies within a factor 4 of the constants LEVEL_*).  A kernel passes within MARGIN = 8 x level, the margin of the Gram
route's direct inverse.  Measures: SH and Rot entries absolute (entries are O(1)); b_n relative to the largest |b_n| of its bin (what G_k sees)
and entry by entry; fit points by the chord between unit vectors (no pole singularity of the measure itself); pseudo-inverses relative to their
largest entry.
"""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import mpmath as mp
import numpy as np

import gram_reference as G
from synth_reference import HAVE_LONGDOUBLE, require_longdouble  # noqa: F401

LD, CLD = np.longdouble, np.clongdouble
DPS = 50
MARGIN = 8.0
C_SOUND = 343
FS = 16000.0
LENGTH = 4                      # the shortest filter length tried, and the plans accept it (4, 8, 16, 32, 64 tried in turn): nfft = 8, P = 5 bins
LENGTH_LONG = 128               # P = 129: launch_dspace_g splits 64 bins and more into 8 chunks
PI_HALF = 1.5707963267948966    # the double the kernels compare zen with

# measured by measure_levels() on the cases below (python tests/ema_reference.py), rounded up to two digits; profiles/r26_ema_operands.md
# LEVEL_SH[order]: oracle.getSH at every point a case evaluates SHs of that order at, largest absolute error of an entry
LEVEL_SH = {1: 1.5e-15, 2: 7.5e-16, 4: 2.4e-15, 5: 3.3e-15, 7: 1.1e-14, 9: 2.3e-15}
LEVEL_SH_POLE = 4.4e-9     # oracle.getSH within 1e-3 rad of a pole (EMAinCH grids: zen = 1e-9): NOT a level -- the discrepancy of sin = sqrt(1 - cos^2), see sh_cos_allowance
LEVEL_CH = 4.6e-15          # oracle.getCH: largest absolute error of an entry (ch_basis_kernel is held to 8 x this through a MagLS-2D plan's Ycm)
LEVEL_BN_BIN = 4.6e-15      # -oracle.sphModalCoeffs: |error| / largest |b_n| of the bin
LEVEL_BN_ENTRY = 7.8e-15    # ... / |b_n| of the entry itself
LEVEL_KR = 2.4e-16          # 2 pi f / c r in double, relative
LEVEL_POINTS = 1.8e-14      # NumPy restatement of rot_points_kernel: chord between the unit vector of (azr, znr) and the exactly rotated point
LEVEL_PINV_CH = 5.0e-15     # numpy.linalg.pinv(oracle.getCH): relative to the largest entry of the pseudo-inverse
LEVEL_PINV_B = 5.8e-15      # numpy.linalg.pinv of the fit set's SH matrix, relative to its largest entry
LEVEL_ROT = 8.5e-15         # oracle.shRotationForElevation against the exact Rot_d: largest absolute error of an entry


def mpf(v):
    return mp.mpf(float(v))


def to_ld(v):
    """mp number -> (c)longdouble through two doubles (exact to 106 bits)"""
    if isinstance(v, mp.mpc):
        return CLD(to_ld(v.real)) + CLD(1j) * CLD(to_ld(v.imag))
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def mat_to_ld(rows, cplx):
    out = np.zeros((len(rows), len(rows[0])), dtype=CLD if cplx else LD)
    for i, r in enumerate(rows):
        for j, v in enumerate(r):
            out[i, j] = to_ld(v) if cplx else to_ld(mp.re(v))
    return out


def acn(n, m):
    return n * n + n + m


def ch_index(m):
    """column of a circular harmonic in [C_0, C_-1, C_1, ..., C_-N, C_N]"""
    return 0 if m == 0 else 2 * abs(m) - (1 if m < 0 else 0)


# ------------------------------------------------------------------------------------------------ bases
@lru_cache(maxsize=None)
def _dleg_coeffs(n, m):
    """d^m P_n / dx^m as {power: Fraction}"""
    out = {}
    for k in range(n // 2 + 1):
        p = n - 2 * k
        if p < m:
            continue
        c = Fraction((-1) ** k * math.comb(n, k) * math.comb(2 * n - 2 * k, n), 2 ** n)
        out[p - m] = c * math.perm(p, m)
    return out


def plm_mp(n, m, x, s):
    """P_n^m with the Condon-Shortley phase: (-1)^m s^m d^m P_n / dx^m, s = sin(zen), x = cos(zen)"""
    acc = mp.mpf(0)
    for p, c in _dleg_coeffs(n, m).items():
        acc += mp.mpf(c.numerator) / c.denominator * x ** p
    return (-1) ** m * s ** m * acc


def sh_norm_mp(n, m):
    return mp.sqrt(mp.mpf(2 * n + 1) / (4 * mp.pi) * mp.factorial(n - m) / mp.factorial(n + m))


def sh_mp(N, azi, zen, cplx):
    """one direction, mp numbers in; [(N + 1)^2] mp values"""
    x, s = mp.cos(zen), mp.sin(zen)
    out = [mp.mpf(0)] * (N + 1) ** 2
    for n in range(N + 1):
        for m in range(n + 1):
            P = sh_norm_mp(n, m) * plm_mp(n, m, x, s)
            if cplx:
                y = P * mp.expj(m * azi)
                out[acn(n, m)] = y
                if m:
                    out[acn(n, -m)] = (-1) ** m * mp.conj(y)
            else:
                base = (-1) ** m * P
                if m == 0:
                    out[acn(n, 0)] = base
                else:
                    out[acn(n, m)] = base * mp.sqrt(2) * mp.cos(m * azi)
                    out[acn(n, -m)] = base * mp.sqrt(2) * mp.sin(m * azi)
    return out


def sh_ld(N, azi, zen, cplx):
    """[npts][(N + 1)^2] in (c)longdouble at double angles: normalised upward recurrence in n for every m"""
    az, zn = np.asarray(azi, dtype=np.float64).astype(LD), np.asarray(zen, dtype=np.float64).astype(LD)
    return sh_from_xs(N, az, np.cos(zn), np.sin(zn), cplx)


def sh_from_xs(N, az, x, s, cplx):
    """the same from x = cos(zen) and s = sin(zen) given separately (longdouble arrays): the SHs depend on s through the factor s^|m| alone"""
    out = np.zeros((az.size, (N + 1) ** 2), dtype=CLD if cplx else LD)
    pmm = np.full(az.shape, 1 / np.sqrt(16 * np.arctan(LD(1))), dtype=LD)     # sqrt(1 / (4 pi))
    r2 = np.sqrt(LD(2))
    for m in range(N + 1):
        if m:
            pmm = np.sqrt(LD(2 * m + 1) / LD(2 * m)) * s * pmm
        p2, p1 = None, pmm
        for n in range(m, N + 1):
            if n == m:
                p = pmm
            elif n == m + 1:
                p = np.sqrt(LD(2 * m + 3)) * x * pmm
            else:
                a = np.sqrt(LD(4 * n * n - 1) / LD(n * n - m * m))
                b = np.sqrt(LD((n - 1) ** 2 - m * m) / LD(4 * (n - 1) ** 2 - 1))
                p = a * (x * p1 - b * p2)
            p2, p1 = p1, p
            if cplx:
                e = np.cos(m * az) + CLD(1j) * np.sin(m * az)
                out[:, acn(n, m)] = (-1) ** m * p * e
                if m:
                    out[:, acn(n, -m)] = p * np.conj(e)
            elif m == 0:
                out[:, acn(n, 0)] = p
            else:
                out[:, acn(n, m)] = r2 * p * np.cos(m * az)
                out[:, acn(n, -m)] = r2 * p * np.sin(m * az)
    return out


def sh_cos_allowance(N, azi, zen, cplx):
    """What an evaluation that sees the zenith through x = cos(zen) alone may differ by from the SHs of the angle: [npts][(N + 1)^2] float64.
    MATLAB's legendre(n, cos(zen)), which the reference calls and sh_basis.hip and the oracle restate, takes sin = sqrt(1 - x^2).  With
    x^ = fl(cos zen) within 2 ulp of cos zen (|x^ - x| <= 2 u) the sine it forms, s^ = sqrt(1 - x^^2), obeys s^^2 - s^2 = (x - x^)(x + x^), so
    |s^^2 - s^2| <= 4 u and |s^ - s| <= min(4 u / s, 2 sqrt u): rounding level away from the poles, up to 3e-8 within sqrt u of one.  An SH
    depends on s through s^|m| alone and s^|m| is monotone, so the entry moves by at most the larger of |Y(x, s + ds) - Y(x, s)| and
    |Y(x, max(s - ds, 0)) - Y(x, s)|, evaluated here.  (The rounding of s^ itself and of x are part of the measured level.)"""
    az, zn = np.asarray(azi, dtype=np.float64).astype(LD), np.asarray(zen, dtype=np.float64).astype(LD)
    x, sn = np.cos(zn), np.abs(np.sin(zn))
    with np.errstate(divide="ignore"):
        ds = np.minimum(4 * LD(G.U) / sn, 2 * np.sqrt(LD(G.U)))
    Y0 = sh_from_xs(N, az, x, sn, cplx)
    up, dn = sh_from_xs(N, az, x, sn + ds, cplx), sh_from_xs(N, az, x, np.maximum(sn - ds, 0), cplx)
    return np.maximum(np.abs(up - Y0), np.abs(dn - Y0)).astype(np.float64)


def ch_mp(N, azi, cplx):
    """one azimuth (mp); [2 N + 1]"""
    out = [mp.mpf(1)]
    for m in range(1, N + 1):
        if cplx:
            out += [mp.expj(-m * azi), mp.expj(m * azi)]
        else:
            out += [mp.sqrt(2) * mp.sin(m * azi), mp.sqrt(2) * mp.cos(m * azi)]
    return out


def pinv_mp(A):
    """pinv of a full-column-rank mp.matrix: (A^H A)^-1 A^H"""
    AH = A.H
    return mp.inverse(AH * A) * AH


def pinv_ch_ld(N, mic_azi, cplx):
    """pinv(CH(mic_azi)) [2 N + 1][M] in (c)longdouble, mp inside"""
    with mp.workdps(DPS):
        A = mp.matrix([ch_mp(N, mpf(a), cplx) for a in mic_azi])
        Z = pinv_mp(A)
        return mat_to_ld([[Z[i, j] for j in range(Z.cols)] for i in range(Z.rows)], cplx)


def nnm_ld(N, cplx):
    """Nnm[c]: the normalised Legendre value at the equator in closed form, P_n^m(0) = (-1)^((n + m) / 2) (n + m - 1)!! / (n - m)!! for even
    n + m (Condon-Shortley inside), so that E0 = diag(Nnm) Ech[ch(c)]"""
    out = np.zeros((N + 1) ** 2, dtype=LD)
    with mp.workdps(DPS):
        for n in range(N + 1):
            for m in range(-n, n + 1):
                am = abs(m)
                if (n + am) % 2:
                    continue
                P = (-1) ** ((n + am) // 2) * mp.fac2(n + am - 1) / mp.fac2(n - am)
                v = sh_norm_mp(n, am) * P                      # complex basis, m >= 0
                if not cplx or m < 0:
                    v = (-1) ** am * v                         # real: Condon-Shortley cancelled; complex m < 0: (-1)^m conj
                out[acn(n, m)] = to_ld(v)
    return out


# ------------------------------------------------------------------------------------------------ b_n
def _sph_mp(n, x):
    f = mp.sqrt(mp.pi / (2 * x))
    return f * mp.besselj(n + mp.mpf(1) / 2, x), f * mp.bessely(n + mp.mpf(1) / 2, x)


def bn_ld(nOrd, kr, n_valid=None):
    """the library's b_n: -4 pi i^n (j_n - j_n' / h_n^(2)' h_n^(2)) for the rigid sphere, [len(kr)][nOrd] clongdouble; zeros above n_valid;
    kr = 0: [-4 pi, 0, ...]"""
    n_valid = nOrd - 1 if n_valid is None else n_valid
    out = np.zeros((len(kr), nOrd), dtype=CLD)
    with mp.workdps(DPS):
        for k, v in enumerate(kr):
            if v == 0:
                out[k, 0] = to_ld(-4 * mp.pi)
                continue
            x = mpf(v)
            jy = [_sph_mp(n, x) for n in range(nOrd + 1)]
            for n in range(min(nOrd, n_valid + 1)):
                j, y = jy[n]
                # f_n' = n / x f_n - f_{n+1}
                dj, dy = n / x * j - jy[n + 1][0], n / x * y - jy[n + 1][1]
                h, dh = mp.mpc(j, -y), mp.mpc(dj, -dy)
                out[k, n] = to_ld(-4 * mp.pi * mp.mpc(0, 1) ** n * (j - dj / dh * h))
    return out


def kr_ld(fs, P, radius):
    f = np.arange(P).astype(LD) * (LD(fs) / 2 / LD(P - 1))
    return 2 * (4 * np.arctan(LD(1))) * f / LD(C_SOUND) * LD(radius)


# ------------------------------------------------------------------------------------------------ the exact rotation
@lru_cache(maxsize=None)
def _wigner_table(l):
    """per (m', m): the square of the prefactor and the terms (sign / denominators, power of cos, power of sin)"""
    f = math.factorial
    tab = {}
    for mp_ in range(-l, l + 1):
        for m in range(-l, l + 1):
            pre = f(l + mp_) * f(l - mp_) * f(l + m) * f(l - m)
            terms = []
            for s in range(max(0, m - mp_), min(l + m, l - mp_) + 1):
                den = f(l + m - s) * f(s) * f(mp_ - m + s) * f(l - mp_ - s)
                terms.append((Fraction((-1) ** (mp_ - m + s), den), 2 * l + m - mp_ - 2 * s, mp_ - m + 2 * s))
            tab[(mp_, m)] = (pre, terms)
    return tab


def wigner_d_mp(l, beta):
    """d^l_{m'm}(beta) as [m' + l][m + l]  (<l m'| e^{-i beta J_y} |l m>)"""
    c, s = mp.cos(beta / 2), mp.sin(beta / 2)
    cp, sp = [c ** k for k in range(2 * l + 1)], [s ** k for k in range(2 * l + 1)]
    out = [[None] * (2 * l + 1) for _ in range(2 * l + 1)]
    for (mp_, m), (pre, terms) in _wigner_table(l).items():
        acc = mp.mpf(0)
        for coef, pc, ps in terms:
            acc += mp.mpf(coef.numerator) / coef.denominator * cp[pc] * sp[ps]
        out[mp_ + l][m + l] = mp.sqrt(pre) * acc
    return out


@lru_cache(maxsize=None)
def _real_from_complex(l):
    """U with Y_real = U Y_complex on order l, rows and columns m = -l .. l"""
    U = mp.zeros(2 * l + 1)
    r = 1 / mp.sqrt(2)
    U[l, l] = 1
    for m in range(1, l + 1):
        U[l + m, l + m], U[l + m, l - m] = (-1) ** m * r, r
        U[l - m, l + m], U[l - m, l - m] = (-1) ** m * r / mp.mpc(0, 1), -r / mp.mpc(0, 1)
    return U


def rot_block_mp(l, azi, alpha, cplx):
    """order-l block of Rot for the elevation alpha at the azimuth azi (mp numbers): mp.matrix, rows i = (l, m), columns j = (l, m')"""
    d = wigner_d_mp(l, -alpha)
    B = mp.zeros(2 * l + 1)
    for m in range(-l, l + 1):
        for m2 in range(-l, l + 1):
            B[m + l, m2 + l] = mp.expj(-m2 * azi) * d[m2 + l][m + l] * mp.expj(m * azi)
    if cplx:
        return B
    U = _real_from_complex(l)
    return U * B * U.H


def rot_ld(azi_d, zen_d, N, cplx):
    """exact Rot_d [C][C] in (c)longdouble for the DOUBLE direction (azi_d, zen_d); alpha = fl(pi/2 - zen_d)"""
    C = (N + 1) ** 2
    out = np.zeros((C, C), dtype=CLD if cplx else LD)
    alpha = float(np.float64(PI_HALF) - np.float64(zen_d))
    if alpha == 0.0:
        out[np.arange(C), np.arange(C)] = 1
        return out
    with mp.workdps(DPS):
        for l in range(N + 1):
            B = rot_block_mp(l, mpf(azi_d), mpf(alpha), cplx)
            out[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = mat_to_ld([[B[i, j] for j in range(B.cols)] for i in range(B.rows)], cplx)
    return out


def rot_all_ld(azi, zen, N, cplx):
    return np.stack([rot_ld(a, z, N, cplx) for a, z in zip(azi, zen)])


# ------------------------------------------------------------------------------------------------ fit points
def ema_sh_npts(C):
    return 4 * C + 8


def fib_points(npts):
    i = np.arange(npts) + 0.5
    return np.mod(np.pi * (1 + 5 ** 0.5) * i, 2 * np.pi), np.arccos(1 - 2 * i / npts)


def unit_ld(azi, zen):
    a, z = np.asarray(azi).astype(LD), np.asarray(zen).astype(LD)
    return np.stack([np.sin(z) * np.cos(a), np.sin(z) * np.sin(a), np.cos(z)], axis=-1)


def rotated_points_ld(azi_p, zen_p, azi_d, zen_d):
    """R_d^-1 x_p exactly, [D][npts][3] longdouble unit vectors, x_p from the double angles (azi_p, zen_p), alpha_d = fl(pi/2 - zen_d)"""
    x = unit_ld(azi_p, zen_p)[None]                                              # [1][npts][3]
    alpha = (np.float64(PI_HALF) - np.asarray(zen_d, dtype=np.float64)).astype(LD)[:, None, None]
    ad = np.asarray(azi_d, dtype=np.float64).astype(LD)
    ax = np.stack([np.sin(ad), -np.cos(ad), np.zeros_like(ad)], axis=-1)[:, None, :]   # [D][1][3]
    cr = np.cross(ax, x)
    dt = np.sum(ax * x, axis=-1, keepdims=True)
    return x * np.cos(alpha) - cr * np.sin(alpha) + ax * dt * (1 - np.cos(alpha))


def rot_points_np(azi_d, zen_d, npts):
    """rot_points_kernel restated in NumPy doubles: (azr, znr) [D + 1][npts], the unrotated set last"""
    a, z = fib_points(npts)
    x = np.stack([np.sin(z) * np.cos(a), np.sin(z) * np.sin(a), np.cos(z)], axis=-1)[None]
    alpha = (np.pi / 2 - np.asarray(zen_d, dtype=np.float64))[:, None, None]
    ad = np.asarray(azi_d, dtype=np.float64)
    ax = np.stack([np.sin(ad), -np.cos(ad), np.zeros_like(ad)], axis=-1)[:, None, :]
    xr = x * np.cos(alpha) - np.cross(ax, x) * np.sin(alpha) + ax * np.sum(ax * x, axis=-1, keepdims=True) * (1 - np.cos(alpha))
    xr = np.concatenate([xr, x], axis=0)
    return np.arctan2(xr[..., 1], xr[..., 0]), np.arccos(np.clip(xr[..., 2], -1, 1))


def points_error(azr, znr, azi_d, zen_d):
    """chord between the unit vectors of (azr, znr) [D + 1][npts] and the exact rotation of the set's own unrotated points (row D)"""
    truth = rotated_points_ld(azr[-1], znr[-1], azi_d, zen_d)
    return np.sqrt(np.sum((unit_ld(azr[:-1], znr[:-1]) - truth) ** 2, axis=-1)).astype(np.float64)


def pole_distance(znr):
    z = np.asarray(znr, dtype=np.float64)
    return float(np.minimum(z, np.pi - z).min())


def pinv_full_rank_ld(B):
    """pinv of a well-conditioned full-column-rank [rows][cols] matrix in (c)longdouble: (B^H B)^-1 B^H, the inverse by two Newton steps
    from the double one (cond(B^H B) ~ 1.1 for the fit set: converged to longdouble rounding)"""
    BH = np.conj(B.T)
    A = BH @ B
    X = np.linalg.inv(A.astype(np.complex128 if np.iscomplexobj(A) else np.float64)).astype(A.dtype)
    I2 = 2 * np.eye(A.shape[0], dtype=A.dtype)
    for _ in range(3):
        X = X @ (I2 - A @ X)
    return X @ BH


# ------------------------------------------------------------------------------------------------ steps on device outputs
def wide(a, cplx):
    return np.asarray(a).astype(CLD if cplx else LD)


def step_ech(Z, Ymic, cplx):
    """Ech[c][s] = sum_m Z[c][m] Ymic[m][s]; Z complex [nOut][M] (real basis: its real part is what counts, the kernel multiplies in complex
    arithmetic all the same), Ymic [M][S]"""
    Zw, Yw = np.asarray(Z).astype(CLD), np.asarray(Ymic).astype(CLD)
    ref = Zw @ Yw
    bound = G.g_terms(Z.shape[1] + 1, True) * (np.abs(Zw).astype(LD) @ np.abs(Yw).astype(LD)).astype(np.float64)
    return (ref if cplx else ref.real), bound


def channel_nm(c):
    n = int(math.isqrt(c))
    return n, c - n * n - n


def step_e0(Ypts_diag, Ech, C, cplx):
    """E0[c][s] = (Ypts[c][c] / chval) Ech[ch(c)][s], chval = sqrt 2 for the real basis' m != 0"""
    nn = wide(Ypts_diag, cplx).copy()
    rows = np.zeros(C, dtype=int)
    for c in range(C):
        n, m = channel_nm(c)
        rows[c] = ch_index(m)
        if not cplx and m != 0:
            nn[c] = nn[c] / np.sqrt(LD(2))
    E = wide(Ech, cplx)[rows]
    ref = nn[:, None] * E
    return ref, G.g_terms(4, cplx) * np.abs(ref).astype(np.float64)


def step_rot(Zb, A_d, cplx, blocks=None):
    """Rot_d[i][j] = sum_p Z[j][p] A_d[i][p] for a batch of directions: Zb [C][npts] complex, A_d [D][C][npts].  blocks = N: the diagonal
    order blocks only, as the blockwise kernel of orders 5..7 writes them -- zero, and a zero bound, everywhere else"""
    Zw = wide(Zb if cplx else np.asarray(Zb).real, cplx)
    Aw = wide(A_d, cplx)
    aZ, aA = np.abs(Zw).astype(LD), np.abs(Aw).astype(LD)
    g = G.g_terms(Zw.shape[1], cplx)
    if blocks is None:
        return Aw @ Zw.T, g * (aA @ aZ.T).astype(np.float64)
    D, C = Aw.shape[0], Aw.shape[1]
    ref, bound = np.zeros((D, C, C), dtype=Aw.dtype), np.zeros((D, C, C))
    for l in range(blocks + 1):
        sl = slice(l * l, (l + 1) ** 2)
        ref[:, sl, sl] = Aw[:, sl, :] @ Zw[sl].T
        bound[:, sl, sl] = g * (aA[:, sl, :] @ aZ[sl].T).astype(np.float64)
    return ref, bound


def nnm_azimuths(C, cplx):
    """one azimuth per SH channel at which its circular harmonic is 1 (or sqrt 2): where the library reads Nnm off its own basis"""
    return np.array([np.pi / (2.0 * -channel_nm(c)[1]) if (not cplx and channel_nm(c)[1] < 0) else 0.0 for c in range(C)])


def step_qt0(Yc, E, nOrd, cplx, dY=0.0, dE=None):
    """QT0[n][c][d] = sum_{s in order n} Yc[d][s] E[c][s]; Yc [D][S], E [C][S].  dY (a scalar or [D][S]), dE [C][S]: what the inputs carry (composed)"""
    Yw, Ew = wide(Yc, cplx), wide(E, cplx)
    D, C = Yw.shape[0], Ew.shape[0]
    ref = np.zeros((nOrd, C, D), dtype=Yw.dtype)
    bound = np.zeros((nOrd, C, D))
    aY, aE = np.abs(Yw).astype(LD), np.abs(Ew).astype(LD)
    for n in range(nOrd):
        sl = slice(n * n, (n + 1) ** 2)
        ref[n] = Ew[:, sl] @ Yw[:, sl].T
        b = G.g_terms(2 * n + 2, cplx) * (aE[:, sl] @ aY[:, sl].T)
        if dE is not None:
            dYa = np.broadcast_to(np.asarray(dY, dtype=np.float64), aY.shape).astype(LD)                  # a level, or entry by entry [D][S]
            b = b + (aE[:, sl] + np.asarray(dE)[:, sl]) @ dYa[:, sl].T + np.asarray(dE)[:, sl].astype(LD) @ aY[:, sl].T
        bound[n] = b.astype(np.float64)
    return ref, bound


def step_rotate(QT0, dQT0, Rot, N, cplx, dRot=0.0):
    """QT[n][c0 + j][d] = sum_i QT0[n][c0 + i][d] Rot[d][c0 + i][c0 + j] per order l >= 1 (order 0 is left alone); QT0 in the wide type with
    its bound dQT0, Rot [D][C][C]"""
    Rw = wide(Rot, cplx)
    ref, bound = QT0.copy(), dQT0.copy()
    aQ, aR = np.abs(QT0).astype(LD), np.abs(Rw).astype(LD)
    for l in range(1, N + 1):
        sl = slice(l * l, (l + 1) ** 2)
        ref[:, sl, :] = np.einsum("nid,dij->njd", QT0[:, sl, :], Rw[:, sl, sl])
        b = np.einsum("nid,dij->njd", dQT0[:, sl, :].astype(LD), aR[:, sl, sl]) + G.g_terms(2 * l + 1, cplx) * np.einsum("nid,dij->njd", aQ[:, sl, :], aR[:, sl, sl])
        if dRot:
            b = b + dRot * (aQ[:, sl, :] + dQT0[:, sl, :]).sum(axis=1, keepdims=True)
        bound[:, sl, :] = b.astype(np.float64)
    return ref, bound


def coef_b(bn, kb, P):
    """the Nyquist bin P - 1 takes real(b_n), the rule tests/test_gpu_stages.py's Xk restates"""
    b = np.asarray(bn[kb]).astype(CLD)
    return b.real.astype(CLD) if kb == P - 1 else b


def step_g(QT, bn, bins, P, cplx, dQT=None, dbn=None):
    """G_k[c][d] = sum_n b_n(k) QT[n][c][d] for the listed bins; QT in any type, [nOrd][C][D]"""
    Qw = np.asarray(QT).astype(CLD)
    aQ = np.abs(Qw).astype(LD)
    nOrd = Qw.shape[0]
    ref, bound = {}, {}
    for kb in bins:
        b = coef_b(bn, kb, P)
        ab = np.abs(b).astype(LD)
        ref[kb] = np.tensordot(b, Qw, axes=(0, 0))
        bd = G.g_terms(nOrd + 1, cplx) * np.tensordot(ab, aQ, axes=(0, 0))
        if dQT is not None:
            bd = bd + np.tensordot(ab, np.asarray(dQT).astype(LD), axes=(0, 0)) + np.tensordot(np.asarray(dbn[kb]).astype(LD), aQ + np.asarray(dQT), axes=(0, 0))
        bound[kb] = bd.astype(np.float64)
    return ref, bound


# ------------------------------------------------------------------------------------------------ cases
def sim_order(N, fs, radius):
    return max(N, int(math.ceil(fs * math.pi * radius / C_SOUND)))


def mic_set(kind, M):
    a = np.linspace(0.0, 2 * np.pi, M, endpoint=False)
    if kind == "uniform":
        return a
    if kind == "offset":
        return a + 0.1
    return a + 0.15 * np.sin(1.0 + 2.3 * np.arange(M))        # jittered: a non-unitary CH matrix


def directions(D):
    """a Fibonacci grid with the edge directions written in: zen = pi/2 exactly and its two neighbouring doubles, 0, pi, 1e-9; azimuths 0, 7, -4"""
    i = np.arange(D) + 0.5
    zen, azi = np.arccos(1 - 2 * i / D), np.mod(np.pi * (1 + 5 ** 0.5) * i, 2 * np.pi)
    zen[:6] = [PI_HALF, np.nextafter(PI_HALF, 4.0), np.nextafter(PI_HALF, 0.0), 0.0, np.pi, 1e-9]
    azi[:6] = [0.0, 7.0, -4.0, 0.0, 7.0, -4.0]
    zen[6], azi[7], azi[8] = PI_HALF, 7.0, -4.0              # (one more horizontal direction at an ordinary azimuth; the edge azimuths at ordinary elevations)
    return azi, zen


# name: design, N, basis, D, microphones, radius  (fs = 16 kHz: simulation order 7 at 4.2 cm, 9 at 6 cm)
CASES = {
    "sh1":  dict(kind="sh", N=1, cplx=False, D=65, mics=("offset", 16), radius=0.042),
    "sh2":  dict(kind="sh", N=2, cplx=False, D=200, mics=("jitter", 7), radius=0.06),
    "sh4r": dict(kind="sh", N=4, cplx=False, D=127, mics=("uniform", 9), radius=0.06, length=LENGTH_LONG),
    "sh4c": dict(kind="sh", N=4, cplx=True, D=129, mics=("offset", 16), radius=0.042),
    "sh5":  dict(kind="sh", N=5, cplx=False, D=65, mics=("uniform", 11), radius=0.042),
    "sh7r": dict(kind="sh", N=7, cplx=False, D=65, mics=("jitter", 17), radius=0.042),
    "sh7c": dict(kind="sh", N=7, cplx=True, D=65, mics=("offset", 16), radius=0.042),
    "ch4r": dict(kind="ch", N=4, cplx=False, D=129, mics=("offset", 16), radius=0.042),
    "ch4c": dict(kind="ch", N=4, cplx=True, D=65, mics=("jitter", 11), radius=0.042),
}


def case(name):
    c = dict(CASES[name])
    c["name"] = name
    c["azi"], c["zen"] = directions(c["D"])
    c["mic_azi"] = mic_set(*c["mics"])
    c["M"] = c["mic_azi"].size
    c["simOrder"] = sim_order(c["N"], FS, c["radius"])
    c["nOrd"], c["S"] = c["simOrder"] + 1, (c["simOrder"] + 1) ** 2
    c["C"] = (c["N"] + 1) ** 2 if c["kind"] == "sh" else 2 * c["N"] + 1
    c.setdefault("length", LENGTH)
    c["nfft"] = 2 * c["length"]
    c["P"] = c["nfft"] // 2 + 1
    c["k_cut"] = int(math.ceil(max(1000.0, 500.0 * c["N"]) / (FS / c["nfft"])))
    c["npts"] = ema_sh_npts(c["C"])
    assert c["D"] >= c["S"]
    return c


def check_bins(c, g0):
    """bin 1, the bins around k_cut, P / 2 and P - 1 -- those of them the plan materialises (from g0 on)"""
    kc0, P = c["k_cut"] - 1, c["P"]
    return sorted({k for k in (1, kc0 - 1, kc0, kc0 + 1, P // 2, P - 1) if max(g0, 1) <= k < P})


# ------------------------------------------------------------------------------------------------ the truth of the whole chain, composed bound
def truth(c, bins):
    """every operand from the case's inputs alone, with the bound a chain of correct steps may reach (levels x MARGIN through the
    sums, plus the sums' own bounds; the products of two input errors are kept: where the truth is
    an exact zero -- Nnm for odd n + m, the alias-free columns of a uniform array -- they are all there is)"""
    N, cplx, M, S, nOrd, C, P = c["N"], c["cplx"], c["M"], c["S"], c["nOrd"], c["C"], c["P"]
    dSH, dSHlo = MARGIN * LEVEL_SH[c["simOrder"]], MARGIN * LEVEL_SH[N]
    eq = np.full(M, PI_HALF)
    Ymic = sh_ld(c["simOrder"], c["mic_azi"], eq, cplx)                        # [M][S]
    Z = pinv_ch_ld(N, c["mic_azi"], cplx)                                      # [2N+1][M]
    aZ, aYm = np.abs(Z).astype(LD), np.abs(Ymic).astype(LD)
    Ech = Z @ Ymic
    dZ = MARGIN * LEVEL_PINV_CH * float(aZ.max())
    dEch = (dZ * aYm.sum(axis=0)[None, :] + dSH * aZ.sum(axis=1)[:, None] + G.g_terms(M + 1, True) * (aZ @ aYm)).astype(np.float64)
    bn = bn_ld(nOrd, kr_ld(FS, P, c["radius"]).astype(np.float64))
    dbn = MARGIN * LEVEL_BN_BIN * np.abs(bn).max(axis=1, keepdims=True).astype(np.float64) * np.ones((1, nOrd))
    if c["kind"] == "ch":
        # EMAinCH: E = pinv(CH) Y_mic, the SHs of the grid itself (zeniths at the poles included: the allowance of an evaluation
        # through cos(zen) alone, sh_cos_allowance, entry by entry on top of the level), no Nnm, no Rot
        Y = sh_ld(c["simOrder"], c["azi"], c["zen"], cplx)
        dY = dSH + sh_cos_allowance(c["simOrder"], c["azi"], c["zen"], cplx)
        QT, dQT = step_qt0(np.conj(Y), Ech, nOrd, cplx, dY=dY, dE=dEch)
        Gk, dG = step_g(QT, bn, bins, P, cplx, dQT=dQT, dbn=dbn)
        return dict(Ymic=Ymic, Z=Z, E=Ech, dE=dEch, Y=Y, dY=dY, QT=QT, dQT=dQT, bn=bn, G=Gk, dG=dG)
    nnm = nnm_ld(N, cplx)
    rows = np.array([ch_index(channel_nm(ch)[1]) for ch in range(C)])
    E0 = nnm[:, None] * Ech[rows]
    dE0 = (dSHlo * (np.abs(Ech[rows]) + dEch[rows]) + np.abs(nnm)[:, None] * dEch[rows] + G.g_terms(4, cplx) * np.abs(E0)).astype(np.float64)
    Rot = rot_all_ld(c["azi"], c["zen"], N, cplx)
    dRot = MARGIN * LEVEL_ROT
    Yhor = sh_ld(c["simOrder"], c["azi"], np.full(c["D"], PI_HALF), cplx)
    QT0, dQT0 = step_qt0(np.conj(Yhor), E0, nOrd, cplx, dY=dSH, dE=dE0)
    QT, dQT = step_rotate(QT0, dQT0, Rot, N, cplx, dRot=dRot)
    Gk, dG = step_g(QT, bn, bins, P, cplx, dQT=dQT, dbn=dbn)
    return dict(Ymic=Ymic, Z=Z, Ech=Ech, E0=E0, dE0=dE0, Rot=Rot, dRot=dRot, Yhor=Yhor, QT=QT, dQT=dQT, bn=bn, G=Gk, dG=dG)


# ------------------------------------------------------------------------------------------------ levels
def measure_levels(names=None, rot_dirs=12):
    """the double-precision oracle (oracle.emagls_oracle) and the NumPy restatements above against the truth, on the inputs of the cases:
    {level name: largest value over the cases}.  rot_dirs: directions per case the fit as a whole is measured on (the edge ones come first)"""
    from oracle import emagls_oracle as O
    out = dict(SH={}, SH_POLE=0.0, CH=0.0, BN_BIN=0.0, BN_ENTRY=0.0, KR=0.0, POINTS=0.0, PINV_CH=0.0, PINV_B=0.0, ROT=0.0)

    def up(k, v, order=None):
        if order is None:
            out[k] = max(out[k], float(v))
        else:
            out[k][order] = max(out[k].get(order, 0.0), float(v))

    for name in (names or CASES):
        c = case(name)
        N, cplx, basis = c["N"], c["cplx"], "complex" if c["cplx"] else "real"
        eq = np.full(c["M"], PI_HALF)
        up("SH", G.err(O.getSH(c["simOrder"], np.column_stack([c["mic_azi"], eq]), basis), sh_ld(c["simOrder"], c["mic_azi"], eq, cplx)).max(), c["simOrder"])
        zen_y = np.full(c["D"], PI_HALF) if c["kind"] == "sh" else c["zen"]
        eY = G.err(O.getSH(c["simOrder"], np.column_stack([c["azi"], zen_y]), basis), sh_ld(c["simOrder"], c["azi"], zen_y, cplx))
        near = np.minimum(zen_y, np.pi - zen_y) < 1e-3          # EMAinCH: the grid's own zeniths, 0, pi and 1e-9 among them
        up("SH", eY[~near].max(), c["simOrder"])
        if near.any():
            # the oracle sees the zenith through cos alone, like MATLAB's legendre: its distance to the SHs of the angle there is no
            # rounding level but the discrepancy sh_cos_allowance bounds -- recorded, and held within that bound
            up("SH_POLE", eY[near].max())
            assert np.all(eY[near] <= MARGIN * LEVEL_SH[c["simOrder"]] + sh_cos_allowance(c["simOrder"], c["azi"], zen_y, cplx)[near])
        kr = kr_ld(FS, c["P"], c["radius"])
        f = np.linspace(0, FS / 2, c["P"])
        kr_d = 2 * np.pi * f / O.C_SOUND * c["radius"]
        up("KR", np.abs((kr_d[1:].astype(LD) - kr[1:]) / kr[1:]).max())
        b_o, b_t = -O.sphModalCoeffs(c["simOrder"], kr_d), bn_ld(c["nOrd"], kr_d)
        e = np.abs(b_o.astype(CLD) - b_t).astype(np.float64)
        ab = np.abs(b_t).astype(np.float64)
        up("BN_BIN", (e / ab.max(axis=1, keepdims=True)).max())
        up("BN_ENTRY", (e[1:] / ab[1:]).max())                       # (bin 0 is the exact row [-4 pi, 0, ...])
        with mp.workdps(DPS):
            up("CH", G.err(O.getCH(N, c["mic_azi"], basis), mat_to_ld([ch_mp(N, mpf(a), cplx) for a in c["mic_azi"]], cplx)).max())
        Zt = pinv_ch_ld(N, c["mic_azi"], cplx)
        Zo = np.linalg.pinv(O.getCH(N, c["mic_azi"], basis))
        up("PINV_CH", G.err(Zo, Zt).max() / float(np.abs(Zt).max()))
        if c["kind"] != "sh":
            continue
        azr, znr = rot_points_np(c["azi"], c["zen"], c["npts"])
        up("POINTS", points_error(azr, znr, c["azi"], c["zen"]).max())
        up("SH", G.err(O.getSH(N, np.column_stack([azr.ravel(), znr.ravel()]), basis), sh_ld(N, azr.ravel(), znr.ravel(), cplx)).max(), N)
        B = O.getSH(N, np.column_stack([azr[-1], znr[-1]]), basis)
        Bt = pinv_full_rank_ld(wide(B, cplx))
        up("PINV_B", G.err(np.linalg.pinv(B), Bt).max() / float(np.abs(Bt).max()))
        for d in range(min(rot_dirs, c["D"])):
            if c["zen"][d] == PI_HALF:
                continue
            up("ROT", G.err(O.shRotationForElevation(c["azi"][d], c["zen"][d], N, basis), rot_ld(c["azi"][d], c["zen"][d], N, cplx)).max())
    return out


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    for k, v in measure_levels().items():
        print("LEVEL_%-9s %s" % (k, "%.3g" % v if not isinstance(v, dict) else {o: float("%.3g" % e) for o, e in sorted(v.items())}))
