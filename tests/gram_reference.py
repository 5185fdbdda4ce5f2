"""The Gram route (csrc/gram_chol.hip: launch_gram; csrc/gramroute.hip: launch_gram_kmat, launch_gram_gemm, launch_gram_solve; csrc/emash.hip:
launch_gram_from_g) step by step against longdouble sums and, for the direct inverse, a multiprecision truth.  CPU only; the GPU test
(tests/test_gpu_gram_route.py) runs the launchers through the debug entries of csrc/gram_debug.hip and holds them to what is derived here.

    conj(Y) --gram--> Gy --F, K and its fold--> Kmat --GEMM with Cf--> Apk --solve--> M_k = A_k^-1 (route 2) | A_k for the Jacobi kernel (route 1)
                                                   G_k --gram_from_g--^

Inputs come bit for bit from the integer generator of factor_reference.py (ints): values n 2^-26 with |n| <= 2^26, so that products do round
in FP64 and are exact in longdouble.  Every step is referenced in (c)longdouble on the DEVICE output of the step before it, so its bound is
a pure summation bound; `composed` adds one bound from Gy, E and b_n straight to Apk.

Bounds.  u = 2^-53, gamma_n = n u / (1 - n u).  A sum of n real products, in any order, fused or not (one rounding per product and per
addition at most, a term passes through n of them at most), lies within gamma_n sum |a| |b| of the exact value.  A complex sum of n
products has 2 n real products per component and |a_r| |b_r| + |a_i| |b_i| <= |a| |b|, so EACH COMPONENT lies within gamma_{2n} sum |a| |b|:
complex results are measured component by component (err()), never by modulus.  n, the "terms" of a step, entry by entry:

    Gy          D + ks       D products (the MFMA chain of a K slice, then the ks partials of the reduce kernel; ks = gram_ksplit, also
                             granted to the LDS kernel, which has no split); the zero rows up to gram_dpad add nothing
    F           2 n' + 1     F[n'][c][s] = sum over the 2 n' + 1 columns j of order n' of Gy(s, j) E[c][j], one chain
    K, folded   2 n + 3      K[c][c'] = sum over the 2 n + 1 rows s of order n of conj(E[c][s]) F[n'][c'][s] in two chains (+ 1 for their sum),
                             + 1 for K[a][b] +- conj(K[b][a]); the factor 1/2 of a diagonal pair is exact.  Per packed entry the bound is
                             gamma (sum |E_a| |F_b| + sum |E_b| |F_a|), halved on diagonal pairs
    Cf          3            |b_n|^2 = x^2 + y^2 unfused: three roundings; Re, Im of conj(b_n) b_n': two fused steps.  gamma_3 |b_n| |b_n'|
    GEMM        round_up(nOrd^2, 4)   real, one MFMA chain over every row of Kmat and Cf, pad rows (exact zeros) included
    gram_from_g D + 2        complex, one chain over the D directions (the zeros that fill the last tile of 64 add nothing); + 2 for the
                             rounding of the exact result it is held against (exact_gram of factor_reference.py, rounded once)

Every bound is multiplied by 1 + 2^-10 for what the longdouble reference itself rounds (2^-64 per term against 2^-53).  `composed` carries
the bound of each step through the next (|E| dF into K, dCf |K| + |Cf| dK into the product); products of two gammas are left out, they are
2^-40 of the terms kept.

Layouts -- each lives in one function here: pack_herm / unpack_herm (a Hermitian C x C matrix as C^2 reals: P[c C + c'] = Re X[c][c'] for
c <= c', Im X[c'][c] for c > c'), kmat_row (row n for n = n', rows nOrd + 2 q and + 1 for the q-th pair n < n' in lexicographic order), and
coef_b (the Nyquist bin P - 1 takes real(b_n)).

The direct inverse.  Truth: mpmath at 60 digits on the FP64 matrix as given, tests/golden/gram_solve_truth.npz (written by
tests/golden/make_gram_truth.py): per bin the eigenvalues of A, M = V diag(s_reg / s) V^H (= A^-1 wherever cond_2(A) <= 1 / reg_c^2, in
particular on every bin the certificate can pass; what the Jacobi kernel must return elsewhere) and the errors numpy.linalg.inv and
numpy.linalg.eigh make on the same bin.  A kernel result passes within MARGIN = 8 x level, level = max(the largest LAPACK error over the
bins of the same class and size, C u cond_2(A)): the forward error a backward-stable method may make, and the floor that takes the 40-fold
lottery out of a single bin's LAPACK error.  The measure of route 2 is the relative Frobenius error of M, that of the chain
(launch_factor_jacobi_gram on the rejected bins) the largest element error relative to the largest element, as test_gpu_factor_chain.py
has it.  The matrices: A = V diag(lambda) V^H with V two integer Householder reflectors and lambda falling linearly from 1 to
(s_min / s_max)^2, all in exact integers over one denominator, rounded once.
"""
from __future__ import annotations

import math
import os
from fractions import Fraction

import numpy as np

import factor_reference as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "gram_solve_truth.npz")
U = 2.0 ** -53
LD, CLD = np.longdouble, np.clongdouble
SLACK = 1.0 + 2.0 ** -10
REG_C = 0.01
MARGIN = 8.0
DPS = 60
SENTINEL_BITS = 0x7ff8dead0000beef     # EMAGLS_DEBUG_SENTINEL_BITS


def gamma(n):
    return n * U / (1.0 - n * U)


def g_terms(n, cplx):
    """the factor of a step with n terms: gamma_n (real arithmetic) or gamma_2n per component (complex)"""
    return gamma(2 * n if cplx else n) * SLACK


def err(a, ref):
    """|a - ref| element by element, float64; complex: the larger of the two components' errors"""
    d = np.asarray(a).astype(CLD if np.iscomplexobj(a) or np.iscomplexobj(ref) else LD) - ref
    if np.iscomplexobj(d):
        return np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
    return np.abs(d).astype(np.float64)


def worst(e, bound):
    """largest error / bound; an error where the bound is zero counts as infinite"""
    e, bound = np.asarray(e, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if not np.all(np.isfinite(e)):
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, e / bound, np.where(e > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def round_up(v, m):
    return (v + m - 1) // m * m


def wide(cplx):
    return CLD if cplx else LD


def f64(a):
    return np.asarray(a).astype(np.float64)


# ------------------------------------------------------------------------------------------------ inputs
def rand_real(seed, shape, bits=26):
    n = int(np.prod(shape))
    return (R.ints(seed, n, -(1 << bits), 1 << bits).astype(np.float64) / float(1 << bits)).reshape(shape)


def rand(seed, shape, cplx, bits=26):
    if not cplx:
        return rand_real(seed, shape, bits)
    v = rand_real(seed, (2,) + tuple(shape), bits)
    return v[0] + 1j * v[1]


def sentinel_filled(shape, dtype=np.float64):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint64)[...] = np.uint64(SENTINEL_BITS)
    return a


def is_sentinel(a):
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(SENTINEL_BITS)


# ------------------------------------------------------------------------------------------------ launch_gram
GRAM_CASES = {1: dict(cplx=False, S=81, D=37, Sh=49), 2: dict(cplx=False, S=400, D=901, Sh=256), 3: dict(cplx=True, S=400, D=901, Sh=400),
              4: dict(cplx=False, S=1024, D=300, Sh=64), 5: dict(cplx=False, S=1000, D=300, Sh=64)}


def gram_ksplit(D, S):
    """the K split launch_gram takes (gram_chol.hip)"""
    nbt = (S + 63) // 64
    nt = nbt * (nbt + 1) // 2
    ks = 32
    while ks > 1 and (D // ks < 32 or nt * ks > 1024 + nt):
        ks >>= 1
    return ks


def gram_kernel(case, lanes=1):
    """which kernel launch_gram reaches, from its dispatch conditions"""
    S, nbt = case["S"], (case["S"] + 63) // 64
    if not case["cplx"] and nbt * (nbt + 1) // 2 * lanes >= 128 and round_up(S, 64) >= 64 * nbt:
        return "gram_lds_kernel, %d tiles, no split" % (nbt * (nbt + 1) // 2)
    return "gram_mfma_kernel + gram_reduce_kernel, %d tiles x %d splits" % (nbt * (nbt + 1) // 2, gram_ksplit(case["D"], S))


def gram_input(k):
    """Yc [D][ld], ld = round_up(S, 64); the columns from S on are NaN: no element of G may depend on them"""
    c = GRAM_CASES[k]
    ld = round_up(c["S"], 64)
    Y = np.full((c["D"], ld), np.nan, dtype=np.complex128 if c["cplx"] else np.float64)
    Y[:, :c["S"]] = rand(7100 + k, (c["D"], c["S"]), c["cplx"])
    return Y


def ref_gram(Yc, S, cplx, dt=None):
    """G = Yc^H Yc [S][S] and its bound"""
    D = Yc.shape[0]
    Y = Yc[:, :S].astype(dt or wide(cplx))
    a = np.abs(Yc[:, :S])
    return Y.conj().T @ Y, g_terms(D + gram_ksplit(D, S), cplx) * (a.T @ a)


# ------------------------------------------------------------------------------------------------ the layouts
def pack_herm(X):
    """Hermitian [..][C][C] -> [..][C^2] reals: P[c C + c'] = Re X[c][c'] for c <= c', Im X[c'][c] for c > c'"""
    C = X.shape[-1]
    up = np.triu(np.ones((C, C), dtype=bool))
    return np.where(up, X.real, np.swapaxes(X.imag, -1, -2)).reshape(X.shape[:-2] + (C * C,))


def unpack_herm(P, C, conj_lower=True):
    """the inverse of pack_herm, as gram_solve_kernel reads it: the upper element as stored, the lower one its conjugate (the sign of a
    zero or a NaN included), the diagonal with imaginary part +0.  conj_lower = False is a planted defect."""
    P = np.asarray(P)
    P = P[..., :C * C].reshape(P.shape[:-1] + (C, C))
    i, k = np.indices((C, C))
    a, b = np.minimum(i, k), np.maximum(i, k)
    im = np.where(a < b, P[..., b, a], 0.0)
    out = np.empty(P.shape, dtype=np.complex128)
    out.real = P[..., a, b]
    out.imag = np.where(i <= k, im, np.negative(im) if conj_lower else im)
    return out


def pair_index(n, n2, nOrd):
    """q of the pair n < n2 in lexicographic order"""
    return n * nOrd - n * (n + 1) // 2 + (n2 - n - 1)


def kmat_row(n, n2, nOrd, defect=None):
    """first row of the pair n <= n2 in Kmat and Cf"""
    if n == n2:
        return n
    q = pair_index(n, n2, nOrd)
    if defect == "q_off_by_one":
        q = (q + 1) % (nOrd * (nOrd - 1) // 2)
    if defect == "rows_transposed":                          # the pairs counted column after column
        q = n2 * (n2 - 1) // 2 + n
    return nOrd + 2 * q


def coef_b(bn, kb, P, defect=None):
    b = np.asarray(bn)[kb]
    return b.real + 0j if kb == P - 1 and defect != "nyquist_imag" else b


def block(n):
    return n * n, (n + 1) * (n + 1)


def all_pairs(nOrd):
    return [(n, n2) for n in range(nOrd) for n2 in range(n, nOrd)]


# ------------------------------------------------------------------------------------------------ the steps of the assembly
def gy_block(Gy, n, n2, dt, defect=None):
    """rows of order n, columns of order n2 >= n, from the upper triangle alone"""
    (sb, se), (jb, je) = block(n), block(n2)
    B = np.asarray(Gy[sb:se, jb:je]).astype(dt)
    if n == n2:
        low = np.triu(B, 1).T
        B = np.triu(B) + (low if defect == "gy_lower_unconjugated" else np.conj(low))
    return B


def f_block(Gy, E, n, n2, cplx, dt=None, defect=None):
    """F[n2][:, rows of order n] for n <= n2, [C][2 n + 1], and its bound"""
    dt = dt or wide(cplx)
    jb, je = block(n2)
    G = gy_block(Gy, n, n2, dt, defect)
    Eb = np.asarray(E[:, jb:je])
    return (G @ Eb.astype(dt).T).T, g_terms(2 * n2 + 1, cplx) * (f64(np.abs(G)) @ np.abs(Eb).T).T


def step_f(Gy, E, C, nOrd, cplx, dt=None, defect=None, pairs=None):
    """F [nOrd][C][S] (NaN where the kernel writes nothing or `pairs` asks for nothing) and its bound"""
    dt = dt or wide(cplx)
    S = nOrd * nOrd
    F = np.full((nOrd, C, S), np.nan, dtype=dt)
    B = np.zeros((nOrd, C, S))
    for n, n2 in (pairs or all_pairs(nOrd)):
        sb, se = block(n)
        F[n2][:, sb:se], B[n2][:, sb:se] = f_block(Gy, E, n, n2, cplx, dt, defect)
    return F, B


def step_kmat(E, F, C, nOrd, cplx, dt=None, defect=None, pairs=None, dF=None):
    """Kmat [round_up(nOrd^2, 4)][C^2] from E and F (rows of other pairs than `pairs`: zero) and its bound; dF: a bound on F to carry"""
    dt = dt or wide(cplx)
    Kp = round_up(nOrd * nOrd, 4)
    rt = np.float64 if dt in (np.float64, np.complex128) else LD
    K = np.zeros((Kp, C * C), dtype=rt)
    Bd = np.zeros((Kp, C * C))
    up = np.triu(np.ones((C, C), dtype=bool))
    for n, n2 in (pairs or all_pairs(nOrd)):
        sb, se = block(n)
        Eb, Fb = np.asarray(E[:, sb:se]), np.asarray(F[n2][:, sb:se])
        Kc = np.conj(Eb.astype(dt)) @ Fb.astype(dt).T + 0j
        aK = g_terms(2 * n + 3, cplx) * (np.abs(Eb) @ f64(np.abs(Fb)).T)
        if dF is not None:
            aK = aK + np.abs(Eb) @ dF[n2][:, sb:se].T
        sym = aK + aK.T
        bsym = np.where(up, sym, sym.T).reshape(-1)
        X, Z = Kc + np.conj(Kc.T), 1j * (Kc - np.conj(Kc.T))
        if defect == "z_sign":
            Z = -Z
        r = kmat_row(n, n2, nOrd, defect)
        if n == n2:
            K[r], Bd[r] = pack_herm(X if defect == "no_half" else X / 2), bsym / 2
        else:
            K[r], Bd[r] = pack_herm(X), bsym
            K[r + 1], Bd[r + 1] = pack_herm(Z), bsym
    if defect == "pad_row" and Kp > nOrd * nOrd:
        K[Kp - 1, 0] = 2.0 ** -60
    return K, Bd


def step_cf(bn, nOrd, P, kb0, nbins, dt=None, defect=None):
    """Cf [round_up(nOrd^2, 4)][nbins] and its bound"""
    real_t = np.float64 if dt in (np.float64, np.complex128) else LD
    Kp = round_up(nOrd * nOrd, 4)
    Cf = np.zeros((Kp, nbins), dtype=real_t)
    Bd = np.zeros((Kp, nbins))
    for bi in range(nbins):
        b = coef_b(bn, kb0 + bi, P, defect)
        br, bim, ab = b.real.astype(real_t), b.imag.astype(real_t), np.abs(b)
        for n in range(nOrd):
            Cf[n, bi], Bd[n, bi] = br[n] * br[n] + bim[n] * bim[n], ab[n] * ab[n]
            for m in range(n + 1, nOrd):
                r = kmat_row(n, m, nOrd, "rows_transposed" if defect == "rows_transposed" else None)
                Cf[r, bi] = br[n] * br[m] + bim[n] * bim[m]            # conj(b_n) b_m
                Cf[r + 1, bi] = br[n] * bim[m] - bim[n] * br[m]
                Bd[r, bi] = Bd[r + 1, bi] = ab[n] * ab[m]
    return Cf, Bd * (gamma(3) * SLACK)


def step_gemm(Cf, Kmat, nbins, C, dt=LD, dCf=None, dK=None):
    """Apk [nbins][C^2] = Cf^T Kmat over every row, and its bound"""
    a, k = np.asarray(Cf)[:, :nbins], np.asarray(Kmat)[:, :C * C]
    A = a.astype(dt).T @ k.astype(dt)
    B = g_terms(a.shape[0], False) * (f64(np.abs(a)).T @ f64(np.abs(k)))
    if dCf is not None:
        B = B + dCf.T @ f64(np.abs(k)) + f64(np.abs(a)).T @ dK
    return A, B


def composed(Gy, E, bn, C, nOrd, P, kb0, nbins, cplx, dt=None, defect=None):
    """Apk from Gy, E and b_n straight, every step in `dt` (longdouble by default), with the bounds of the steps carried through"""
    F, dF = step_f(Gy, E, C, nOrd, cplx, dt, defect)
    K, dK = step_kmat(E, F, C, nOrd, cplx, dt, defect, dF=dF)
    Cf, dCf = step_cf(bn, nOrd, P, kb0, nbins, dt, defect)
    real_t = np.float64 if dt in (np.float64, np.complex128) else LD
    A, dA = step_gemm(Cf, K, nbins, C, real_t, dCf, dK)
    return dict(F=F, dF=dF, Kmat=K, dK=dK, Cf=Cf, dCf=dCf, Apk=A, dA=dA)


# the cases of launch_gram_kmat + launch_gram_gemm
ASM_CASES = {"K1": dict(cplx=False, C=25, nOrd=20, P=70, kb0=3, nbins=67), "K2": dict(cplx=True, C=25, nOrd=20, P=70, kb0=3, nbins=67),
             "K3": dict(cplx=False, C=32, nOrd=9, P=10, kb0=1, nbins=9), "K4": dict(cplx=True, C=4, nOrd=5, P=130, kb0=1, nbins=129),
             "K5": dict(cplx=False, C=9, nOrd=31, P=65, kb0=64, nbins=1), "K6": dict(cplx=True, C=32, nOrd=65, P=6, kb0=1, nbins=5)}
K6_PAIRS = [(n, n) for n in range(65)] + [(0, 1), (0, 64), (63, 64), (31, 33)]


def asm_input(name):
    """Gy [S][S] with every strictly lower element NaN (and a real diagonal), E [C][ldE] dense, ldE = round_up(S, 64) with NaN beyond S,
    bn [P][nOrd] complex (n 2^-44) with non-zero imaginary parts"""
    c = ASM_CASES[name]
    S, seed = c["nOrd"] ** 2, 8000 + 10 * int(name[1])
    Gy = rand(seed, (S, S), c["cplx"])
    Gy[np.tril_indices(S, -1)] = np.nan
    if c["cplx"]:
        Gy[np.arange(S), np.arange(S)] = Gy[np.arange(S), np.arange(S)].real
    ldE = round_up(S, 64)
    E = np.full((c["C"], ldE), np.nan, dtype=Gy.dtype)
    E[:, :S] = rand(seed + 1, (c["C"], S), c["cplx"])
    bn = rand(seed + 2, (c["P"], c["nOrd"]), True, bits=44)     # (44 bits: the coefficients round in FP64 too)
    bn.imag[bn.imag == 0] = 2.0 ** -44
    return Gy, E, bn


# ------------------------------------------------------------------------------------------------ launch_gram_from_g
FROM_G_SHAPES = [(1, 1), (9, 63), (25, 64), (32, 65), (32, 901)]
FROM_G = dict(kb0=3, g0=2, nbins=5)


def from_g_input(C, D):
    """G [nbins + kb0 - g0][C][ldD], ldD = round_up(D, 64), the gaps NaN"""
    slots = FROM_G["nbins"] + FROM_G["kb0"] - FROM_G["g0"]
    G = np.full((slots, C, round_up(D, 64)), np.nan + 1j * np.nan)
    G[:, :, :D] = rand(9000 + 100 * C + D, (slots, C, D), True)
    return G


def ref_from_g(G, D):
    """packed A_k = G_k^H G_k for the bins kb0 ... (slots kb0 - g0 ...), rounded once from exact integers, and the bound"""
    C = G.shape[1]
    out = np.zeros((FROM_G["nbins"], C * C))
    Bd = np.zeros_like(out)
    for i in range(FROM_G["nbins"]):
        X = G[i + FROM_G["kb0"] - FROM_G["g0"]][:, :D].T      # D x C
        Ar, Ai, e = R.exact_gram(np.ascontiguousarray(X))
        A = np.array([[complex(R._ratio(int(Ar[a, b]), e), R._ratio(int(Ai[a, b]), e)) for b in range(C)] for a in range(C)])
        out[i] = pack_herm(A)
        a = np.abs(X)
        s = a.T @ a
        Bd[i] = g_terms(D + 2, True) * np.where(np.triu(np.ones((C, C), dtype=bool)), s, s.T).reshape(-1)
    return out, Bd


# ------------------------------------------------------------------------------------------------ launch_gram_solve
SOLVE_C = (1, 2, 4, 9, 16, 25, 31, 32)
SOLVE_KB0 = 2
# eleven bins (not a multiple of the four per workgroup); the NaN bin shares its workgroup with bins 0, 2 and 3, which take route 2
SOLVE_BINS = [("r", Fraction(1)), ("nan", Fraction(10)), ("r", Fraction(10)), ("r", Fraction(50)), ("r", Fraction(101)), ("r", Fraction(300)),
              ("r", Fraction(30000)), ("indef", None), ("zero", None), ("r", Fraction(90)), ("r", Fraction(999, 10))]
SOLVE_NBINS = len(SOLVE_BINS)


def _gauss_matmul(ar, ai, br, bi):
    return ar @ br - ai @ bi, ar @ bi + ai @ br


def exact_hermitian(C, lam_num, den, seed):
    """V diag(lam_num / den) V^H, V = H2 H1 with H = I - 2 v v^H / v^H v of small integer vectors v: the C x C complex matrix rounded once
    from exact integers over one denominator"""
    wr, wi, N = np.eye(C, dtype=object), np.zeros((C, C), dtype=object), 1
    for t in range(2):
        vr, vi = R.int_vector(seed + 11 + t, C)
        vr, vi = vr.astype(np.int64).astype(object), vi.astype(np.int64).astype(object)
        nv = int(np.sum(vr * vr + vi * vi))
        hr = np.eye(C, dtype=object) * nv - 2 * (np.outer(vr, vr) + np.outer(vi, vi))      # N I - 2 v v^H
        hi = -2 * (np.outer(vi, vr) - np.outer(vr, vi))
        wr, wi = _gauss_matmul(hr, hi, wr, wi)
        N *= nv
    lam = np.array([int(x) for x in lam_num], dtype=object)
    ar, ai = _gauss_matmul(wr * lam[None, :], wi * lam[None, :], wr.T, -wi.T)             # W diag(lam) W^H
    D = den * N * N
    A = np.zeros((C, C), dtype=np.complex128)
    for a in range(C):
        for b in range(C):
            A[a, b] = complex(float(Fraction(int(ar[a, b]), D)), float(Fraction(int(ai[a, b]), D)))
    return A


def solve_matrix(C, b):
    """the matrix of bin b and its exact eigenvalues before the one rounding"""
    kind, ratio = SOLVE_BINS[b]
    if kind == "zero":
        return np.zeros((C, C), dtype=np.complex128), [Fraction(0)] * C
    r2 = Fraction(-4) if kind == "indef" else ratio * ratio           # lambda falls linearly from 1 to 1 / r2
    a, bb = r2.numerator, r2.denominator
    den = a * max(C - 1, 1)
    num = [a * max(C - 1, 1) - (a - bb) * (i if C > 1 else 1) for i in range(C)]
    A = exact_hermitian(C, num, den, 31000 + 100 * C + b)
    if kind == "nan":
        A[C // 2, C // 2] = np.nan
    return A, [Fraction(n, den) for n in num]


def solve_input(C, scale=0):
    """A [11][C][C] and the packed rows [11][ldA], ldA = round_up(C^2, 64), the padding NaN; scale: A 2^scale (exact)"""
    A = np.stack([solve_matrix(C, b)[0] for b in range(SOLVE_NBINS)]) * 2.0 ** scale
    Apk = np.full((SOLVE_NBINS, round_up(C * C, 64)), np.nan)
    Apk[:, :C * C] = pack_herm(A)
    return A, Apk


def solve_class(b):
    """bins of one class share a level"""
    return str(SOLVE_BINS[b][1]) if SOLVE_BINS[b][0] == "r" else SOLVE_BINS[b][0]


_truth = None


def load_solve_truth():
    """{(C, bin): entries}: lam [2][C], M [2][C][C] (hi + lo), lapack_inv, lapack_eigh, sum"""
    global _truth
    if _truth is None:
        z = np.load(FIXTURE)
        out = {}
        for key in z.files:
            name, k = key.split("/")
            Cn, b = (int(x) for x in name[1:].split("_"))
            out.setdefault((Cn, b), {})[k] = z[key]
        for tr in out.values():
            tr["M"] = R.unpack_upper(tr.pop("Mu"))
        _truth = out
    return _truth


def mp_truth(A):
    """eigenvalues (ascending) and M = V diag(s_reg / s) V^H of the FP64 Hermitian matrix A at DPS digits, as hi + lo stacks"""
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    C = A.shape[0]
    Ar, e1 = R._to_int(A.real.copy())
    Ai, e2 = R._to_int(A.imag.copy())
    e = max(e1, e2)
    Am = R._mp_matrix(mp, Ar * (1 << (e - e1)), Ai * (1 << (e - e2)), e)
    s, _, M = R._mp_m_of_a(mp, Am, 0, REG_C, 0.0)
    return {"lam": R._hilo(mp, [x * x for x in s], (C,), False), "M": R._hilo(mp, [M[i, j] for i in range(C) for j in range(C)], (C, C), True)}, (mp, Am, M)


def truth_facts(C, b, tr=None):
    """what the checks need of a positive definite bin: s_max, s_min, cond_2(A), ||A||_F^2 ||M||_F^2 in longdouble, the predicted route"""
    tr = tr or load_solve_truth()[(C, b)]
    A = solve_matrix(C, b)[0]
    lam = tr["lam"][0].astype(LD) + tr["lam"][1]
    fa = np.sum(np.abs(A.astype(CLD)) ** 2)
    Mt = tr["M"][0].astype(CLD) + tr["M"][1]
    fm = np.sum(np.abs(Mt) ** 2)
    cond = float(lam.max() / lam.min())
    clipped = cond > 1.0 / REG_C ** 2            # (M of the fixture is A^-1 only where nothing is clipped; elsewhere ||A^-1||_F >= cond / ||A||_F)
    prod = float(fa * fm) if not clipped else math.inf
    thr2 = 1.0 / REG_C ** 4
    return dict(smax=float(np.sqrt(lam.max())), smin=float(np.sqrt(lam.min())), cond=cond, prod=prod, rel=prod / thr2 - 1.0,
                route=2 if prod <= thr2 else 1)


def predicted_routes(C):
    return [truth_facts(C, b)["route"] if SOLVE_BINS[b][0] == "r" else 1 for b in range(SOLVE_NBINS)]


def level(C, b, which):
    """max(the largest LAPACK error over the bins of the class at this size, C u cond_2(A))"""
    T = load_solve_truth()
    same = [x for x in range(SOLVE_NBINS) if SOLVE_BINS[x][0] == "r" and solve_class(x) == solve_class(b)]
    return max(max(float(T[(C, x)][which][0]) for x in same), C * U * truth_facts(C, b)["cond"])


def inv_error(M, tr):
    """relative Frobenius error of M against the truth"""
    d = (M - tr["M"][0]).astype(CLD) - tr["M"][1]
    return float(np.sqrt(np.sum(np.abs(d) ** 2)) / np.sqrt(np.sum(np.abs(tr["M"][0].astype(CLD)) ** 2)))


def chain_error(M, tr):
    """largest element error relative to the largest element (gram_measures of factor_reference.py)"""
    return float(np.max(np.abs((M - tr["M"][0]) - tr["M"][1])) / np.max(np.abs(tr["M"][0])))


def gauss_jordan(Apk, C, kb0, reg_c=REG_C, defect=None):
    """gram_solve_kernel in plain FP64 NumPy (Gauss-Jordan without pivoting on the unpacked matrix, the Frobenius certificate, the bounds in
    sv, the hand-over), writing into sentinel-filled arrays of the debug entry's shapes.  defect: a planted one."""
    nb = Apk.shape[0]
    P = kb0 + nb
    Mw, R2w = sentinel_filled((P, C, C), np.complex128), sentinel_filled((P, C, C), np.complex128)
    sv = sentinel_filled((P, C))
    route, sweeps = np.full(P, -1, dtype=np.int32), np.full(P, -1, dtype=np.int32)
    for i in range(nb):
        kb = kb0 + i
        A = unpack_herm(Apk[i], C, conj_lower=defect != "no_conj_lower")
        X = A.copy()
        fa, bad = float(np.sum(np.abs(A) ** 2)), False
        with np.errstate(all="ignore"):
            for j in range(C):
                p = X[j, j].real
                bad = bad or not p > 0.0
                ip = 1.0 / (p if p > 0.0 else 1.0)
                if defect == "pivot_single":
                    ip = float(np.float32(ip))
                X[j, j] = 1.0
                X[j, :] = X[j, :] * ip
                for r in range(C):
                    if r != j:
                        f = X[r, j]
                        X[r, j] = 0.0
                        X[r, :] = X[r, :] - f * X[j, :]
            fm = float(np.sum(np.abs(X) ** 2))
            measure = fa * fm
            if defect == "two_norm" and np.all(np.isfinite(A)) and np.all(np.isfinite(X)):
                measure = (np.linalg.norm(A, 2) * np.linalg.norm(X, 2)) ** 2
            direct = (not bad) and fa > 0.0 and measure <= 1.0 / reg_c ** 4
        if direct:
            Mw[kb - 1] = X
            hi, lo = math.sqrt(math.sqrt(fa)), 1.0 / math.sqrt(math.sqrt(fm))
            sv[kb, :] = hi if defect == "sv_swapped" else lo
            sv[kb, 0] = lo if defect == "sv_swapped" else hi
            route[kb], sweeps[kb] = 2, 0
        else:
            R2w[kb - 1] = A
            route[kb] = 1
    return dict(Mw=Mw, R2w=R2w, sv=sv, route=route, sweeps=sweeps)


def check_solve(C, Apk, out, kb0=SOLVE_KB0, scale=0, report=None):
    """every assertion on the outputs of launch_gram_solve for the bins of solve_input(C, scale); returns the list of what fails.
    report: a list that receives (C, bin, class, route, error, level, ratio) of the route-2 bins."""
    T = load_solve_truth()
    fails = []
    routes = predicted_routes(C)
    Mw, R2w, sv, route, sweeps = (out[k] for k in ("Mw", "R2w", "sv", "route", "sweeps"))
    unpacked = unpack_herm(Apk, C)
    sc = 2.0 ** scale
    for b in range(SOLVE_NBINS):
        kb = kb0 + b
        if route[kb] != routes[b]:
            fails.append("C %d bin %d: route %d, predicted %d" % (C, b, route[kb], routes[b]))
            continue
        if routes[b] == 2:
            tr, f = T[(C, b)], truth_facts(C, b)
            M = Mw[kb - 1] * sc                       # (exact: a power of two)
            e, lv = inv_error(M, tr), level(C, b, "lapack_inv")
            if report is not None:
                report.append((C, b, solve_class(b), 2, e, lv, e / lv))
            if not e <= MARGIN * lv:
                fails.append("C %d bin %d: |M - A^-1|_F / |A^-1|_F = %.3g > 8 x %.3g" % (C, b, e, lv))
            if not np.max(np.abs(M - M.conj().T)) <= 4 * U * np.linalg.norm(M):
                fails.append("C %d bin %d: M is not Hermitian to 4 u |M|" % (C, b))
            s = sv[kb] / math.sqrt(sc)
            if not s[0] >= f["smax"] * (1 - 1e-12):
                fails.append("C %d bin %d: sv[0] = %.17g below s_max = %.17g" % (C, b, s[0], f["smax"]))
            if C > 1 and not (np.all(s[1:] <= f["smin"] * (1 + 1e-12)) and np.all(s[1:] == s[1])):
                fails.append("C %d bin %d: sv[1:] above s_min = %.17g or not all equal" % (C, b, f["smin"]))
            if sweeps[kb] != 0:
                fails.append("C %d bin %d: sweeps %d" % (C, b, sweeps[kb]))
            if not f["cond"] <= 1.0 / REG_C ** 2:
                fails.append("C %d bin %d: passed with cond_2(A) = %.6g" % (C, b, f["cond"]))
            if not np.all(is_sentinel(R2w[kb - 1])):
                fails.append("C %d bin %d: R2w written on route 2" % (C, b))
        else:
            if not np.array_equal(np.ascontiguousarray(R2w[kb - 1]).view(np.uint64), np.ascontiguousarray(unpacked[b]).view(np.uint64)):
                fails.append("C %d bin %d: R2w is not the unpacked input bit for bit" % (C, b))
            if not (np.all(is_sentinel(Mw[kb - 1])) and np.all(is_sentinel(sv[kb])) and sweeps[kb] == -1):
                fails.append("C %d bin %d: Mw, sv or sweeps written on route 1" % (C, b))
    # nothing outside the bins: the slots before kb0 and the last slot of Mw / R2w
    if not (np.all(is_sentinel(Mw[:kb0 - 1])) and np.all(is_sentinel(R2w[:kb0 - 1])) and np.all(is_sentinel(Mw[-1])) and np.all(is_sentinel(R2w[-1]))
            and np.all(is_sentinel(sv[:kb0])) and np.all(route[:kb0] == -1) and np.all(sweeps[:kb0] == -1)):
        fails.append("C %d: written outside the bins" % C)
    return fails
