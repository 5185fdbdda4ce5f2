"""The per-bin factor chain (csrc/factor.hip, launch_wa_factor and launch_wa_factor_tiled of csrc/wide_array.hip) against a multiprecision truth: the test matrices,
the truth, the four measures and the stand-ins the host test runs through them.  CPU only.

Inputs are not stored anywhere: they are rebuilt bit for bit from the integer generator below.  Every floating-point step of a
construction is a single IEEE operation on whole arrays (+, -, *, / on float64, real and imaginary parts kept apart, sums taken in a
written-out order), so the result does not depend on a BLAS, on a library's random stream or on fused multiply-adds; the fixture stores a
checksum of every input and load_truth() compares it.  The finished FP64 matrix is then taken as given: the truth (mpmath, 100 digits) is
the exact result for exactly these doubles.

With X (S x C) the matrix of a bin, X = U S V^H:   A = X^H X = V S^2 V^H (mp.eighe),  s = sqrt(lambda),
    mode 0:  s_reg = 1 / max(s, reg_c s_max)          mode 1:  s_reg = 1 / s above tol = tol_dim eps(s_max), 0 below (MATLAB pinv)
    M = V diag(s_reg / s) V^H,   Zc = X M = U diag(s_reg) V^H  (the kernels return Z = conj(Zc)),   P = X^H Zc = A M
and for two rows Hq[e] of small integers  W[e] = sum_s Hq[e][s] Z[s][:]  -- a contraction over every row of Z.
The fixture (tests/golden/factor_truth.npz, written by tests/golden/make_factor_truth.py) keeps per case s, s_reg, P, W and Z at no more
than 16 listed rows as hi + lo doubles, and the errors FP64 LAPACK makes on the same case through the same formulas.

Path 1 also has the shapes of 9 ... 32 columns at which FromAtf's dense route calls launch_wa_factor (NARROW1); path 2 is launch_wa_factor_tiled
(TILED2: shape, classes, leaf bound), whose cutting rule tiling() restates and whose chain tiled_route() runs in NumPy, with the index errors
a kernel could make as injectable faults.  Class K6 exists for it: a column exactly zero on the first leaf, another on the last.

Measures of a result (sv, Z, W) -- the first three do not depend on the conditioning of X:
    A   max |sort(sv) - sort(s)| / s_max
    B   max |svd(Z) - sort(s_reg)| / max(s_reg): Z has the singular values s_reg exactly when U and V are orthonormal
    C   max |X^H conj(Z) - P|   (P has the eigenvalues s s_reg <= 1)
    D   max |W - W_truth| / max |W_truth|  and  max |Z[rows] - Z_truth[rows]| / max |Z|
"""
from __future__ import annotations

import hashlib
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "factor_truth.npz")   # path 0; the wide path and the Gram form have files of their own (size)
FIXTURES = (FIXTURE, os.path.join(HERE, "golden", "factor_truth_wide.npz"), os.path.join(HERE, "golden", "factor_truth_gram.npz"),
            os.path.join(HERE, "golden", "factor_truth_tiled.npz"))
EPS = 2.0 ** -52
REG_C = 0.01
MARGIN = 8.0          # a result passes within MARGIN x max(LAPACK's error on the case, C eps)
DPS = 100


# ------------------------------------------------------------------------------------------------ integers
def ints(seed, n, lo, hi):
    """n integers in [lo, hi] from a counter-based 64-bit mix (splitmix64 finaliser) of seed and index."""
    with np.errstate(over="ignore"):
        z = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)) % np.uint64(hi - lo + 1)).astype(np.int64) + lo


def int_vector(seed, n, amp=7):
    """complex vector of n small integers (as two float64 arrays), never zero"""
    v = ints(seed, 2 * n, -amp, amp).astype(np.float64)
    vr, vi = v[:n].copy(), v[n:].copy()
    vr[0] += amp + 1.0
    return vr, vi


# ------------------------------------------------------------------------------------------------ reflectors, one IEEE operation at a time
def _reflect_left(xr, xi, vr, vi):
    """X <- (I - 2 v v^H / v^H v) X;  v^H X summed row after row"""
    beta = 2.0 / float(np.sum(vr.astype(np.int64) ** 2 + vi.astype(np.int64) ** 2))
    wr = np.zeros(xr.shape[1])
    wi = np.zeros(xr.shape[1])
    for s in range(xr.shape[0]):   # w += conj(v_s) X[s]
        wr = wr + (vr[s] * xr[s] + vi[s] * xi[s])
        wi = wi + (vr[s] * xi[s] - vi[s] * xr[s])
    br, bi = (beta * vr)[:, None], (beta * vi)[:, None]
    return xr - (br * wr[None, :] - bi * wi[None, :]), xi - (br * wi[None, :] + bi * wr[None, :])


def _reflect_right(xr, xi, vr, vi):
    """X <- X (I - 2 v v^H / v^H v);  X v summed column after column"""
    beta = 2.0 / float(np.sum(vr.astype(np.int64) ** 2 + vi.astype(np.int64) ** 2))
    tr = np.zeros(xr.shape[0])
    ti = np.zeros(xr.shape[0])
    for c in range(xr.shape[1]):   # t += X[:, c] v_c
        tr = tr + (xr[:, c] * vr[c] - xi[:, c] * vi[c])
        ti = ti + (xr[:, c] * vi[c] + xi[:, c] * vr[c])
    br, bi = (beta * vr)[None, :], (-beta * vi)[None, :]   # beta conj(v)
    return xr - (tr[:, None] * br - ti[:, None] * bi), xi - (tr[:, None] * bi + ti[:, None] * br)


def spectrum_matrix(S, C, s, seed):
    """S x C matrix with (nearly) the singular values s: two integer reflectors on either side of diag(s), rounded as they come"""
    xr = np.zeros((S, C))
    xi = np.zeros((S, C))
    xr[np.arange(C), np.arange(C)] = s
    for t in range(2):
        xr, xi = _reflect_left(xr, xi, *int_vector(seed + 11 + t, S))
        xr, xi = _reflect_right(xr, xi, *int_vector(seed + 23 + t, C))
    return xr + 1j * xi


def integer_matrix(S, C, seed, amp=8):
    g = ints(seed, 2 * S * C, -amp, amp).astype(np.float64)
    return g[:S * C].reshape(S, C) + 1j * g[S * C:].reshape(S, C)


# ------------------------------------------------------------------------------------------------ the classes
def spectrum(cls, C):
    k = np.arange(C)
    if cls == "K1":     # 1 ... 1/30, linear: nothing clipped
        d = 30.0 * max(C - 1, 1)
        return (d - 29.0 * k) / d
    if cls == "K2":     # pairs (L, L (1 - 2^-12)) on levels 2^0 ... 2^-21 (six decades): clustered, several below 0.01 s_max
        m = (C + 1) // 2
        lev = (21 * (k // 2)) // max(m - 1, 1)
        return np.ldexp(1.0, -lev) * np.where(k % 2 == 1, 1.0 - 2.0 ** -12, 1.0)
    if cls == "K4":     # 1 ... 2^-13, full rank, cond 8192 ~ 1e4
        return np.ldexp(1.0, -((13 * k + (C - 1) // 2) // max(C - 1, 1)))
    raise ValueError(cls)


def class_matrix(cls, S, C, seed, leaf_rows=0):
    if cls in ("K1", "K2", "K4"):
        return spectrum_matrix(S, C, spectrum(cls, C), seed)
    if cls == "K3":     # rows n^2 ... (n+1)^2 - 1 scaled 10^(-2.6 n) (to the nearest power of two), the largest first: B_k at low k r
        n = np.array([math.isqrt(s) for s in range(S)])
        return integer_matrix(S, C, seed) * np.ldexp(1.0, -np.round(2.6 * n * math.log2(10.0)).astype(int))[:, None]
    if cls == "K5":     # two exactly equal columns
        assert C >= 2 and S >= 16 * C
        x = integer_matrix(S, C, seed)
        x[:, C - 1] = x[:, 0]
        return x
    if cls == "K6":     # block-deficient: a column exactly zero on the first leaf, another on the last; the whole matrix has full rank
        leaves, leaf_h, _ = tiling(S, C, leaf_rows)
        assert leaves >= 2
        x = integer_matrix(S, C, seed)
        x[:leaf_h, C // 2] = 0.0
        if C > 1:
            x[(leaves - 1) * leaf_h:, 0] = 0.0
        return x
    raise ValueError(cls)


# ------------------------------------------------------------------------------------------------ the tiled form (path 2)
LEAF_ROWS = 3072       # the library's bound of a leaf's height


def tiling(S, C, leaf_rows=0):
    """(leaves, leaf_h, ldT) of launch_wa_factor_tiled, restated: leaves = ceil(S / bound), the bound rounded down to a multiple of 64;
    leaf_h = ceil(S / leaves) rounded up to a multiple of 64, the last leaf takes the rest; ldT = leaves C rounded up to a multiple of 64"""
    bound = (leaf_rows if leaf_rows else LEAF_ROWS) // 64 * 64
    leaves = -(-S // bound)
    leaf_h = 64 * -(-(-(-S // leaves)) // 64)
    assert S - (leaves - 1) * leaf_h >= C, "a leaf with fewer rows than columns"
    return leaves, leaf_h, 64 * -(-leaves * C // 64)


MODE = {"K1": 0, "K2": 0, "K3": 0, "K4": 1, "K5": 1, "K6": 0}

# path 0: the smallest and the largest shape of every instance dispatch() has; path 1: the forms of launch_wa_factor
SHAPES0 = [(1, 1), (2, 2), (31, 25), (32, 32), (33, 32), (128, 31), (129, 8), (256, 25), (257, 2), (416, 32), (417, 25), (512, 7), (513, 32), (768, 25),
           (769, 8), (1536, 5), (1537, 8), (2752, 1), (2753, 3), (4096, 8)]
EXTRA0 = [("K3", 33, 32), ("K3", 513, 32), ("K4", 31, 25), ("K4", 1537, 8), ("K5", 129, 8), ("K5", 4096, 8)]
SHAPES1 = [(64, 64), (65, 33), (448, 64), (449, 40), (3072, 33), (3073, 34), (4096, 33)]
EXTRA1 = [("K3", 449, 40)]
# 9 ... 32 columns (FromAtf's dense route calls launch_wa_factor there): the ends of the reg-7, the tall and the pair form, partial grids
NARROW1 = [(9, 9), (448, 32), (449, 9), (3072, 17), (3073, 9), (4096, 32)]
# path 2 = launch_wa_factor_tiled: (S, C, classes, leaf bound; 0 = the library's)
TILED2 = [(4097, 1, ("K1", "K2"), 0), (4097, 9, ("K1", "K2", "K6"), 0), (4097, 31, ("K1", "K2"), 0), (4160, 32, ("K1", "K2"), 0),
          (6145, 8, ("K1", "K2", "K6"), 0), (16384, 32, ("K2",), 0),
          (1025, 32, ("K1", "K2", "K6"), 1024), (2049, 5, ("K1", "K2"), 1024), (3073, 9, ("K1", "K2"), 1024), (16384, 32, ("K2",), 1024),
          (6209, 9, ("K1", "K2"), 4096)]


def instance(path, S, C):
    """(lanes per column, rows per lane) of the kernel instance the shape selects: where the row boundaries of a lane group lie"""
    if path == 1:
        return 64, (S + 63) // 64
    if C * 32 <= 1024:
        for r in (1, 4, 8, 13, 16, 24):
            if S <= 32 * r:
                return 32, r
    for r in (24, 43, 64):
        if S <= 64 * r:
            return 64, r
    raise ValueError((S, C))


def _case(path, cls, S, C, leaf_rows=0):
    name = "p%d_%s_%dx%d" % (path, cls, S, C) + ("_h%d" % leaf_rows if leaf_rows else "")
    seed = 1000 * S + 10 * C + int(cls[1]) + 500000 * path + 7 * leaf_rows
    return dict(name=name, path=path, cls=cls, S=S, C=C, mode=MODE[cls], reg_c=REG_C, tol_dim=float(max(S, C)), seed=seed,
                ldS=64 * ((S + 63) // 64), leaf_rows=leaf_rows)


CASES = [_case(0, cls, S, C) for (S, C) in SHAPES0 for cls in ("K1", "K2")] + [_case(0, *e) for e in EXTRA0] + \
        [_case(1, cls, S, C) for (S, C) in SHAPES1 for cls in ("K1", "K2")] + [_case(1, *e) for e in EXTRA1] + \
        [_case(1, cls, S, C) for (S, C) in NARROW1 for cls in ("K1", "K2")] + \
        [_case(2, cls, S, C, h) for (S, C, classes, h) in TILED2 for cls in classes]
CASE = {c["name"]: c for c in CASES}


def build_input(case):
    """X (S x C complex128) and Hq (2 x S, small complex integers)"""
    S, C = case["S"], case["C"]
    X = class_matrix(case["cls"], S, C, case["seed"], case.get("leaf_rows", 0))
    h = ints(case["seed"] + 77, 4 * S, -4, 4).astype(np.float64)
    Hq = (h[:2 * S] + 1j * h[2 * S:]).reshape(2, S)
    return np.ascontiguousarray(X), Hq


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], dtype=np.uint64)[0]


def listed_rows(case):
    """at most 16 rows: the first two, the last two, the rows on either side of the lane-group boundaries NCH i (evenly thinned to six)"""
    S = case["S"]
    if case["path"] == 2:
        return _listed_rows_tiled(case)
    nch, rpt = instance(case["path"], S, case["C"])
    bnd = [nch * i for i in range(1, rpt) if nch * i < S]
    if len(bnd) > 6:
        bnd = [bnd[(len(bnd) - 1) * t // 5] for t in range(6)]
    rows = {0, 1, S - 2, S - 1}
    for b in bnd:
        rows |= {b - 1, b}
    return np.array(sorted(r for r in rows if 0 <= r < S), dtype=np.int64)


def _listed_rows_tiled(case):
    """path 2: the first two and the last two rows, the rows on either side of every leaf boundary (evenly thinned to four: 16 rows in all)
    and of the 64-row group boundaries nearest the middle of the first and of the last leaf"""
    S = case["S"]
    leaves, leaf_h, _ = tiling(S, case["C"], case["leaf_rows"])
    bnd = [leaf_h * i for i in range(1, leaves)]
    if len(bnd) > 4:
        bnd = [bnd[(len(bnd) - 1) * t // 3] for t in range(4)]
    r0 = (leaves - 1) * leaf_h
    bnd += [64 * ((leaf_h // 2 + 32) // 64), r0 + 64 * (((S - r0) // 2 + 32) // 64)]
    rows = {0, 1, S - 2, S - 1}
    for b in bnd:
        if 0 < b < S:
            rows |= {b - 1, b}
    rows = np.array(sorted(r for r in rows if 0 <= r < S), dtype=np.int64)
    assert len(rows) <= 16
    return rows


# ------------------------------------------------------------------------------------------------ regularisation rules (FP64 and mp share them)
def pinv_tol(smax, tol_dim):
    """tol_dim eps(s_max), eps(x) = 2^(e - 53) for x = m 2^e, m in [0.5, 1)"""
    return tol_dim * math.ldexp(1.0, math.frexp(float(smax))[1] - 53) if smax > 0 else 0.0


def s_reg_fp64(s, mode, reg_c, tol_dim, tol_size=None):
    s = np.asarray(s, dtype=np.float64)
    smax = s.max()
    if mode == 0:
        return 1.0 / np.maximum(s, reg_c * smax)
    tol = pinv_tol(smax, tol_dim if tol_size is None else tol_size)
    return np.where(s > tol, 1.0 / np.where(s > tol, s, 1.0), 0.0)


# ------------------------------------------------------------------------------------------------ the truth (mpmath)
def _to_int(a):
    """float64 array -> (object array of Python integers n, e) with a = n 2^-e exactly"""
    m, ex = np.frexp(a)
    nz = a != 0
    e = int(53 - ex[nz].min()) if nz.any() else 0
    out = np.empty(a.shape, dtype=object)
    flat, mi, ei = out.reshape(-1), np.ldexp(m, 53).astype(np.int64).reshape(-1), ex.reshape(-1)
    for i in range(flat.size):
        flat[i] = int(mi[i]) << int(ei[i] - 53 + e) if mi[i] else 0
    return out, e


def exact_gram(X):
    """A = X^H X in exact integer arithmetic: (Ar, Ai, e) with A = (Ar + i Ai) 2^-e"""
    xr, e1 = _to_int(X.real.copy())
    xi, e2 = _to_int(X.imag.copy())
    e = max(e1, e2)
    xr, xi = xr * (1 << (e - e1)), xi * (1 << (e - e2))
    return xr.T @ xr + xi.T @ xi, xr.T @ xi - xi.T @ xr, 2 * e


def _mp_matrix(mp, Ar, Ai, e):
    n, m = Ar.shape
    out = mp.matrix(n, m)
    sc = mp.ldexp(mp.mpf(1), -e)
    for i in range(n):
        for j in range(m):
            out[i, j] = mp.mpc(mp.mpf(int(Ar[i, j])) * sc, mp.mpf(int(Ai[i, j])) * sc)
    return out


def _split(v):
    """mp number or list -> (hi, lo) float64"""
    hi = float(v)
    return hi, float(v - hi)


def _hilo(mp, vals, shape, cplx):
    n = int(np.prod(shape))
    hi = np.zeros(n, dtype=np.complex128 if cplx else np.float64)
    lo = np.zeros_like(hi)
    for i, v in enumerate(vals):
        if cplx:
            a, b = _split(mp.re(v)), _split(mp.im(v))
            hi[i], lo[i] = complex(a[0], b[0]), complex(a[1], b[1])
        else:
            hi[i], lo[i] = _split(v)
    return np.stack([hi.reshape(shape), lo.reshape(shape)])


def _mp_m_of_a(mp, A, mode, reg_c, tol_dim):
    """s, s_reg (ascending in s) and M = V diag(s_reg / s) V^H of the Hermitian mp matrix A"""
    C = A.rows
    lam, V = mp.eighe(A)
    lmax = max(lam[i] for i in range(C))
    s = [mp.sqrt(lam[i]) if lam[i] > lmax * mp.mpf(10) ** -60 else mp.mpf(0) for i in range(C)]   # (below 1e-60: exactly rank deficient)
    smax = max(s)
    if mode == 0:
        sr = [1 / max(x, mp.mpf(reg_c) * smax) for x in s]
    else:
        tol = mp.mpf(pinv_tol(float(smax), tol_dim))
        sr = [1 / x if x > tol else mp.mpf(0) for x in s]
    g = [sr[i] / s[i] if s[i] > 0 else mp.mpf(0) for i in range(C)]
    M = mp.matrix(C, C)
    for a in range(C):
        for b in range(a, C):
            acc = mp.mpc(0)
            for i in range(C):
                acc += V[a, i] * g[i] * mp.conj(V[b, i])
            M[a, b] = acc
            M[b, a] = mp.conj(acc)
    return s, sr, M


def truth(case):
    """the fixture's entries of one case (hi + lo float64 stacks), computed at DPS digits"""
    X, Hq = build_input(case)
    return truth_of(X, Hq, case["mode"], case["reg_c"], case["tol_dim"], listed_rows(case))


def truth_of(X, Hq, mode, reg_c, tol_dim, rows):
    """the same for any FP64 matrix X (S x C), rows Hq (2 x S, integers) and list of rows of Z"""
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    S, C = X.shape
    A = _mp_matrix(mp, *exact_gram(X))
    s, sr, M = _mp_m_of_a(mp, A, mode, reg_c, tol_dim)
    P = A * M
    out = {"s": _hilo(mp, s, (C,), False), "s_reg": _hilo(mp, sr, (C,), False), "P": _hilo(mp, [P[i, j] for i in range(C) for j in range(C)], (C, C), True)}
    # W[e] = sum_s Hq[e][s] Z[s][:] = conj( (conj(Hq[e]) X) M ): the row conj(Hq[e]) X exactly, then C^2 mp products
    xr, e1 = _to_int(X.real.copy())
    xi, e2 = _to_int(X.imag.copy())
    W = []
    for e in range(2):
        hr, hi = Hq[e].real.astype(np.int64).astype(object), (-Hq[e].imag).astype(np.int64).astype(object)   # conj(Hq)
        tr = (hr @ xr) * (1 << e2) - (hi @ xi) * (1 << e1)
        ti = (hr @ xi) * (1 << e1) + (hi @ xr) * (1 << e2)
        t = _mp_matrix(mp, tr.reshape(1, C), ti.reshape(1, C), e1 + e2)
        w = t * M
        W += [mp.conj(w[0, c]) for c in range(C)]
    out["W"] = _hilo(mp, W, (2, C), True)
    rows = np.asarray(rows, dtype=np.int64)
    Z = []
    for r in rows:
        xrow = mp.matrix(1, C)
        for c in range(C):
            xrow[0, c] = mp.mpc(float(X[r, c].real), float(X[r, c].imag))
        z = xrow * M
        Z += [mp.conj(z[0, c]) for c in range(C)]
    out["Z"] = _hilo(mp, Z, (len(rows), C), True)
    out["rows"] = rows
    out["sum"] = np.array([checksum(X, Hq)], dtype=np.uint64)
    return out


# ------------------------------------------------------------------------------------------------ measures
def hl(a):
    """hi + lo stack -> the pair; a difference is taken as (x - hi) - lo"""
    return a[0], a[1]


def measures(tr, X, sv, Z, W):
    """A, B, C, DW, DZ of a result (sv [C], Z [S][C] = the kernels' Z, W [2][C]) against the truth entries tr of the case"""
    s_hi, s_lo = hl(tr["s"])
    r_hi, r_lo = hl(tr["s_reg"])
    smax = s_hi.max()
    order = np.argsort(s_hi)
    mA = np.max(np.abs((np.sort(sv) - s_hi[order]) - s_lo[order])) / smax
    zs = np.linalg.svd(Z, compute_uv=False)
    order = np.argsort(r_hi)
    mB = np.max(np.abs((np.sort(zs) - r_hi[order]) - r_lo[order])) / r_hi.max()
    P_hi, P_lo = hl(tr["P"])
    mC = np.max(np.abs((_dd_gemm_hc(X, np.conj(Z)) - P_hi) - P_lo))
    W_hi, W_lo = hl(tr["W"])
    mDW = np.max(np.abs((W - W_hi) - W_lo)) / np.max(np.abs(W_hi))
    Z_hi, Z_lo = hl(tr["Z"])
    mDZ = np.max(np.abs((Z[tr["rows"]] - Z_hi) - Z_lo)) / float(np.asarray(tr["zmax"]).reshape(-1)[0])
    return {"A": float(mA), "B": float(mB), "C": float(mC), "DW": float(mDW), "DZ": float(mDZ)}


def _dd_gemm_hc(X, Y):
    """X^H Y in longdouble accumulation (the measure must not add a C-sized rounding of its own to a C eps bound)"""
    if np.finfo(np.longdouble).eps >= EPS:   # no wider type on this platform: FP64
        return X.conj().T @ Y
    cld = np.clongdouble
    acc = np.zeros((X.shape[1], Y.shape[1]), dtype=cld)
    for r0 in range(0, X.shape[0], 512):
        acc += X[r0:r0 + 512].conj().T.astype(cld) @ Y[r0:r0 + 512].astype(cld)
    return acc.astype(np.complex128)


def bound(lapack_err, C):
    return MARGIN * max(float(lapack_err), C * EPS)


ASSERTED = {"K1": ("A", "B", "C", "DW", "DZ"), "K2": ("A", "B", "C", "DW", "DZ"), "K3": ("A", "B", "C"), "K4": ("A", "B", "C", "DW", "DZ"),
            "K5": ("A", "B", "C", "DW", "DZ"), "K6": ("A", "B", "C", "DW", "DZ")}   # (K3: LAPACK's own forward error is 1e-4 at cond 1e13 -- D is printed next to it, not asserted)


# ------------------------------------------------------------------------------------------------ stand-ins for the kernel (FP64)
def from_svd(U, s, Vh, X, Hq, mode, reg_c, tol_dim, tol_size=None, clip=None):
    sr = s_reg_fp64(s, mode, reg_c if clip is None else clip, tol_dim, tol_size)
    Z = np.conj(U) @ (sr[:, None] * np.conj(Vh))      # conj(U) diag(s_reg) V^T
    return s, Z, Hq @ Z


def lapack_route(X, Hq, mode, reg_c, tol_dim, **kw):
    U, s, Vh = np.linalg.svd(X, full_matrices=False)
    return from_svd(U, s, Vh, X, Hq, mode, reg_c, tol_dim, **kw)


def jacobi_route(X, Hq, mode, reg_c, tol_dim, order="cyclic", unrotate=None, **kw):
    """Householder QR, then one-sided (Hestenes) Jacobi on R^H -- the chain of factor.hip in plain NumPy.  order: 'cyclic' (row by row) or
    'reverse'.  unrotate = t (an injected error): the state one rotation before convergence -- the columns of the largest and the smallest
    singular value are turned back so that |gamma| / sqrt(alpha beta) = t between them, as if that last rotation had been left out."""
    Q, R = np.linalg.qr(X)
    J, s, Vn = _jacobi_of_r(R, mode, reg_c, order, unrotate)
    # R^H = Xrot J^H  ->  R = J Xrot^H = J diag(s) (Xrot / s)^H:  X = (Q J) diag(s) (Xrot / s)^H
    return from_svd(Q @ J, s, Vn.conj().T, X, Hq, mode, reg_c, tol_dim, **kw)


def _jacobi_of_r(R, mode, reg_c, order="cyclic", unrotate=None):
    """the Jacobi step of jacobi_route on a C x C triangle: J, s, Vn with R = J diag(s) Vn^H"""
    C = R.shape[1]
    G = R.conj().T.copy()          # R^H = G: G J = Xrot with orthogonal columns; R = J Sigma (Xrot / Sigma)^H
    J = np.eye(C, dtype=np.complex128)
    pairs = [(p, q) for p in range(C - 1) for q in range(p + 1, C)]
    if order == "reverse":
        pairs = pairs[::-1]

    def rotate(p, q, cs, sn, ph):
        for Mx in (G, J):
            xp, xq = Mx[:, p].copy(), Mx[:, q].copy()
            Mx[:, p] = cs * xp - sn * np.conj(ph) * xq
            Mx[:, q] = sn * ph * xp + cs * xq

    for sweep in range(40):
        big = 0.0
        for p, q in pairs:
            al, be = np.vdot(G[:, p], G[:, p]).real, np.vdot(G[:, q], G[:, q]).real
            ga = np.vdot(G[:, p], G[:, q])
            if abs(ga) <= EPS * math.sqrt(al * be) or ga == 0:
                continue
            big = max(big, abs(ga) / math.sqrt(al * be))
            zeta = (be - al) / (2.0 * abs(ga))
            t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            cs = 1.0 / math.sqrt(1.0 + t * t)
            rotate(p, q, cs, cs * t, ga / abs(ga))
        if big < 1e-8:
            break
    s = np.sqrt(np.sum(np.abs(G) ** 2, axis=0))
    if unrotate is not None and C >= 2:
        nzs = np.where(s > 1e-10 * s.max(), s, np.inf)   # (not a column of the null space: its weight is zero)
        p, q = int(np.argmax(s)), int(np.argmin(nzs))
        clipped = np.flatnonzero((s > 0) & (s < reg_c * s.max())) if mode == 0 else np.array([], dtype=int)
        if clipped.size >= 2 and s[clipped].max() > s[clipped].min():   # two clipped ones: equal weights, the defect shows to first order
            p, q = int(clipped[np.argmax(s[clipped])]), int(clipped[np.argmin(s[clipped])])
        th = unrotate * s[p] * s[q] / (s[p] ** 2 - s[q] ** 2)    # gamma = (beta - alpha) sin cos
        rotate(p, q, math.cos(th), math.sin(th), 1.0)
        s = np.sqrt(np.sum(np.abs(G) ** 2, axis=0))
    return J, s, G / np.where(s > 0, s, 1.0)[None, :]


# ------------------------------------------------------------------------------------------------ the tiled chain (path 2) in NumPy
def householder_qr(X):
    """V (the reflectors, column j zero above row j), tau, R (C x C) with (I - tau_0 v_0 v_0^H) ... X = [R; 0], as the wide forms do it:
    alpha = -x_0 / |x_0| |x|, v = x - alpha e_0, tau = 2 / |v|^2 -- and tau = 0, the step left out, on a column that is zero from j down"""
    A = X.astype(np.complex128).copy()
    S, C = A.shape
    V = np.zeros_like(A)
    tau = np.zeros(C)
    for j in range(min(S, C)):
        x = A[j:, j].copy()
        nx, ax = math.sqrt(float(np.sum(x.real ** 2 + x.imag ** 2))), abs(x[0])
        alpha = -x[0] / ax * nx if ax > 0 else -nx
        nv2 = 2.0 * nx * (nx + ax)
        tau[j] = 2.0 / nv2 if nv2 > 0 else 0.0
        x[0] -= alpha
        V[j:, j] = x
        A[j:, j] = 0.0
        A[j, j] = alpha
        if j + 1 < C:
            A[j:, j + 1:] -= tau[j] * np.outer(x, x.conj() @ A[j:, j + 1:])
    R = np.zeros((C, C), dtype=np.complex128)
    R[:min(S, C)] = np.triu(A[:C])[:min(S, C)]
    return V, tau, R


def apply_q(V, tau, T):
    """Q [T; 0] for the reflectors of householder_qr (S x C) and a C x C block T: the back-transform"""
    S, C = V.shape
    Y = np.zeros((S, T.shape[1]), dtype=np.complex128)
    Y[:min(S, C)] = T[:min(S, C)]
    for j in range(C - 1, -1, -1):
        Y -= tau[j] * np.outer(V[:, j], V[:, j].conj() @ Y)
    return Y


FAULTS = ("swap_T", "short_last", "stale_tau", "drop_row")


def tiled_route(X, Hq, mode, reg_c, tol_dim, leaf_rows=0, fault=None, ldS=None):
    """launch_wa_factor_tiled in plain NumPy: Householder QR of every leaf, the triangles one below the other, QR of that stack,
    jacobi_route's Jacobi and clipping on the stack's R, and the two-level back-transform (the stack's, which leaves a C x C block T_i per
    leaf, then every leaf's own with its T_i).  fault (an injected error, what a wrong index in the kernels would do):
      'swap_T'      leaves 0 and 1 use each other's T_i
      'short_last'  the last leaf is treated as leaf_h rows.  The rows beyond S are zeros -- up to ldS; the ones beyond ldS are, in the
                    [C][ldS] storage of the kernels, the first rows of the NEXT column (zeros behind the last one), and they are what the
                    error shows by: leaf_h rows of which all beyond S are zeros give the same R and the same rows of Z, bit for bit
      'stale_tau'   the last leaf's back-transform reads leaf 0's tau
      'drop_row'    the last row of the last leaf is left out of its QR (its row of Z stays zero)"""
    assert fault is None or fault in FAULTS
    S, C = X.shape
    leaves, leaf_h, _ = tiling(S, C, leaf_rows)
    ldS = 64 * ((S + 63) // 64) if ldS is None else ldS
    blocks = []
    for i in range(leaves):
        r0 = i * leaf_h
        Xi = X[r0:min(r0 + leaf_h, S)]
        if i == leaves - 1 and fault == "drop_row":
            Xi = Xi[:-1]
        if i == leaves - 1 and fault == "short_last":
            flat = np.zeros((C + 1) * ldS, dtype=np.complex128)       # the storage [C][ldS], one more column of zeros behind it
            flat[:C * ldS].reshape(C, ldS)[:, :S] = X.T
            Xi = np.stack([flat[c * ldS + r0:c * ldS + r0 + leaf_h] for c in range(C)], axis=1)
        blocks.append((r0, Xi.shape[0]) + householder_qr(Xi))
    Vs, taus, Rs = householder_qr(np.concatenate([b[4] for b in blocks], axis=0))
    J, s, Vn = _jacobi_of_r(Rs, mode, reg_c)
    sr = s_reg_fp64(s, mode, reg_c, tol_dim)
    T = apply_q(Vs, taus, (J * sr[None, :]) @ Vn.conj().T)     # [T_0; T_1; ...] = Q_stack J diag(s_reg) Vn^H
    Ti = [T[i * C:(i + 1) * C] for i in range(leaves)]
    if fault == "swap_T":
        Ti[0], Ti[1] = Ti[1], Ti[0]
    Zc = np.zeros((S, C), dtype=np.complex128)
    for i, (r0, h, V, tau, _) in enumerate(blocks):
        if i == leaves - 1 and fault == "stale_tau":
            tau = blocks[0][3]
        n = min(h, S - r0)
        Zc[r0:r0 + n] = apply_q(V, tau, Ti[i])[:n]
    Z = np.conj(Zc)
    return s, Z, Hq @ Z


# ------------------------------------------------------------------------------------------------ the Gram form
GRAM_C = (7, 25, 32)
GRAM_BINS = 11
GRAM_SKIP = 5          # route 2
GRAM_JUMP = 6          # the chain restarts from other vectors here
GRAM_HIGH = 8          # the bin whose smallest singular value is lowered: cond just above cond_limit
GRAM_CASES = [dict(name="g_%s_%d" % (cls, C), cls=cls, C=C, seed=900000 + 100 * C + int(cls[1])) for C in GRAM_C for cls in ("K1", "K2")]
GRAM_CASE = {c["name"]: c for c in GRAM_CASES}


def gram_chain(case):
    """A [11][C][C]: A_k = X_k^H X_k formed exactly and rounded once; X_k has the class spectrum (drifting by 2^-10 per bin) between integer
    reflectors that turn slowly with k, other ones from bin GRAM_JUMP on; at bin GRAM_HIGH the smallest singular value is 7/8 of its place"""
    C, cls, seed = case["C"], case["cls"], case["seed"]
    S = C + 3
    out = np.zeros((GRAM_BINS, C, C), dtype=np.complex128)
    base = spectrum(cls, C)
    for k in range(GRAM_BINS):
        s = base * (1.0 + k * 2.0 ** -10 * (np.arange(C) % 3))
        if k == GRAM_HIGH:
            s[np.argmin(s)] *= 0.875
        sd = seed + (5000 if k >= GRAM_JUMP else 0)
        xr = np.zeros((S, C))
        xi = np.zeros((S, C))
        xr[np.arange(C), np.arange(C)] = s
        for t in range(2):
            lr, li = int_vector(sd + 11 + t, S)
            dr, di = int_vector(sd + 31 + t, S, 3)
            xr, xi = _reflect_left(xr, xi, 64.0 * lr + k * dr, 64.0 * li + k * di)
            rr, ri = int_vector(sd + 23 + t, C)
            dr, di = int_vector(sd + 43 + t, C, 3)
            xr, xi = _reflect_right(xr, xi, 64.0 * rr + k * dr, 64.0 * ri + k * di)
        Ar, Ai, e = exact_gram(xr + 1j * xi)
        for a in range(C):
            for b in range(C):
                out[k, a, b] = complex(_ratio(int(Ar[a, b]), e), _ratio(int(Ai[a, b]), e))
    return out


def _ratio(n, e):
    """n 2^-e rounded to the nearest double (integer division by a power of two is exact in Fraction -> float)"""
    from fractions import Fraction
    return float(Fraction(n, 1 << e))


def gram_truth(case):
    import mpmath
    mp = mpmath.mp
    mp.dps = DPS
    A = gram_chain(case)
    C = case["C"]
    s_all, M_all = [], []
    for k in range(GRAM_BINS):
        Ar, e1 = _to_int(A[k].real.copy())
        Ai, e2 = _to_int(A[k].imag.copy())
        e = max(e1, e2)
        s, _, M = _mp_m_of_a(mp, _mp_matrix(mp, Ar * (1 << (e - e1)), Ai * (1 << (e - e2)), e), 0, REG_C, 0.0)
        s_all += s
        M_all += [M[i, j] for i in range(C) for j in range(C)]
    return {"s": _hilo(mp, s_all, (GRAM_BINS, C), False), "M": _hilo(mp, M_all, (GRAM_BINS, C, C), True),
            "sum": np.array([checksum(A)], dtype=np.uint64)}


def gram_lapack(A, reg_c=REG_C):
    lam, V = np.linalg.eigh(A)
    s = np.sqrt(np.maximum(lam, 0.0))
    g = s_reg_fp64(s, 0, reg_c, 0.0) / np.where(s > 0, s, 1.0)
    return s, (V * g[None, :]) @ V.conj().T


def gram_measures(tr, k, sv, M):
    s_hi, s_lo = tr["s"][0][k], tr["s"][1][k]
    order = np.argsort(s_hi)
    mA = np.max(np.abs((np.sort(sv) - s_hi[order]) - s_lo[order])) / s_hi.max()
    M_hi, M_lo = tr["M"][0][k], tr["M"][1][k]
    mM = np.max(np.abs((M - M_hi) - M_lo)) / np.max(np.abs(M_hi))
    return {"A": float(mA), "M": float(mM)}


# ------------------------------------------------------------------------------------------------ the fixture
_loaded = None


def load_truth():
    """{case name: entries}; every entry of the npz is '<case>/<key>'"""
    global _loaded
    if _loaded is None:
        out = {}
        for fn in FIXTURES:
            z = np.load(fn)
            for key in z.files:
                name, k = key.split("/")
                out.setdefault(name, {})[k] = z[key]
        for tr in out.values():
            for pu, full in (("Pu", "P"), ("Mu", "M")):
                if pu in tr:
                    tr[full] = unpack_upper(tr.pop(pu))
        _loaded = out
    return _loaded


def unpack_upper(u):
    """[...][C (C + 1) / 2] (upper triangle, row after row) -> the Hermitian [...][C][C]"""
    C = int(round((math.sqrt(8 * u.shape[-1] + 1) - 1) / 2))
    iu = np.triu_indices(C)
    full = np.zeros(u.shape[:-1] + (C, C), dtype=u.dtype)
    full[..., iu[1], iu[0]] = np.conj(u)
    full[..., iu[0], iu[1]] = u
    return full


def case_inputs(case):
    """X, Hq of a case, checked against the checksum the truth was computed for"""
    X, Hq = build_input(case)
    want = load_truth()[case["name"]]["sum"][0]
    assert checksum(X, Hq) == want, "the input of %s is not the one the fixture was computed for" % case["name"]
    return X, Hq
