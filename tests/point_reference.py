"""The point-source array responses of DESIGN.md section 14, restated in NumPy for the tests (never the code under test).

    H_q(k, m) = sum_j G_j(k) exp(-2 pi i k (tau_j + tau_0) / nfft) sum_n b'_n(k) F_n(kappa_k rho_j) P_n(u_j . v_m)
    F_n(x) = (-i)^(n+1) x e^(ix) h_n^(2)(x)

point_legendre evaluates the product b'_n F_n DIRECTLY: b_n from the oracle's sphModalCoeffs, h_n^(2) = j_n - i y_n from
scipy.special.  That is valid while neither factor leaves FP64 (it asserts so); bin 0 is the limit kappa -> 0,
b'_n F_n -> -(2n+1)/(n+1) (r/rho)^n.  scaled_numpy is the scaled table and recurrence of section 14 in NumPy, held to the
multiprecision fixture by tests/test_array_point_host.py; it serves as nothing's truth.
"""
import numpy as np
from scipy.special import spherical_jn, spherical_yn

from oracle import emagls_oracle as O
from test_gpu_array_irs import unit  # noqa: E402

C_SOUND = 343.0


def point_factor(n, x):
    """F_n(x) for x > 0, directly."""
    x = np.asarray(x, dtype=np.float64)
    h2 = spherical_jn(n, x) - 1j * spherical_yn(n, x)
    return (-1j) ** (n + 1) * x * np.exp(1j * x) * h2


def direct_product(N, fs, r, nfft, rho):
    """b'_n(k) F_n(kappa_k rho) as [N+1][P] for one distance, the last bin with Re b'_n; bin 0 the closed limit."""
    P = nfft // 2 + 1
    k = np.arange(P)
    kappa = 2 * np.pi * (k * fs / nfft) / C_SOUND
    n = np.arange(N + 1)
    bn = -O.sphModalCoeffs(N, kappa * r).T * ((2 * n + 1) / (4 * np.pi))[:, None]
    bn[:, -1] = bn[:, -1].real
    out = np.zeros((N + 1, P), dtype=complex)
    with np.errstate(all="raise"):
        for nn in n:
            F = point_factor(nn, kappa[1:] * rho)
            assert np.isfinite(F).all() and (np.abs(bn[nn, 1:]) > 1e-280).all(), (nn, rho)     # neither factor has left FP64
            out[nn, 1:] = bn[nn, 1:] * F
    out[:, 0] = -(2 * n + 1) / (n + 1) * (r / rho) ** n
    return out


def point_legendre(fs, r, mics, sources, dists, order, nfft, pre, refl=None, exps=None, att=None, paths=None):
    """[Q x P x M].  sources: list of [J x 4] (azi, zen, delay, gain); dists: list of [J]; the spectral gain as in
    spectral_legendre (direct powers)."""
    N = O.simulation_order(order, fs, r)
    P = nfft // 2 + 1
    k = np.arange(P)
    v = unit(mics)
    out = np.zeros((len(sources), P, mics.shape[0]), dtype=complex)
    for q, s in enumerate(sources):
        for j in range(s.shape[0]):
            bf = direct_product(N, fs, r, nfft, float(dists[q][j]))              # [N+1][P]
            x = unit(s[j:j + 1, :2]) @ v.T                                      # [1 x M]
            p0, p1 = np.ones_like(x), x
            acc = bf[0][:, None] * p0
            for n in range(1, N + 1):
                acc = acc + bf[n][:, None] * p1
                p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
            d = s[j, 2] + pre
            di = np.floor(d)
            turns = ((k * int(di)) % nfft + k * (d - di)) / nfft
            fac = s[j, 3] * np.exp(-2j * np.pi * turns)
            if refl is not None:
                for w in range(refl.shape[0]):
                    fac = fac * refl[w] ** int(exps[q][j, w])
            if att is not None:
                fac = fac * np.exp(-att * paths[q][j])
            out[q] += fac[:, None] * acc
        out[q, -1] = out[q, -1].real
    return out


def dc_closed_form(r, mics, sources, dists, N):
    """[Q x M]: -sum_j g_j sum_n (2n+1)/(n+1) (r/rho_j)^n P_n(u_j . v_m); no Bessel function."""
    v = unit(mics)
    out = np.zeros((len(sources), mics.shape[0]))
    for q, s in enumerate(sources):
        if s.shape[0] == 0:
            continue
        x = unit(s[:, :2]) @ v.T
        t = (r / np.asarray(dists[q]))[:, None]
        p0, p1 = np.ones_like(x), x
        acc = np.ones_like(x)
        for n in range(1, N + 1):
            acc = acc + (2 * n + 1) / (n + 1) * t ** n * p1
            p0, p1 = p1, ((2 * n + 1) * x * p1 - n * p0) / (n + 1)
        out[q] = -(s[:, 3][:, None] * acc).sum(axis=0)
    return out


def scaled_g(N, x):
    """G^_n(x) = F_n(x) (ix)^n / (2n-1)!! for n = 0 .. N by G^_(n+1) = G^_n - x^2 / (4n^2 - 1) G^_(n-1): [N+1] + x.shape."""
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros((N + 1,) + x.shape, dtype=complex)
    g[0] = 1.0
    if N >= 1:
        g[1] = 1.0 + 1j * x
    for n in range(1, N):
        g[n + 1] = g[n] - x * x / (4 * n * n - 1) * g[n - 1]
    return g


def scaled_beta(N, x):
    """b^_n = b'_n (2n-1)!! / (i x)^n at x = kappa r, from G^ alone: [N+1] + x.shape."""
    x = np.asarray(x, dtype=np.float64)
    g = scaled_g(N, x)
    e = np.exp(1j * x)
    b = np.zeros_like(g)
    b[0] = -e / (1.0 + 1j * x)
    for n in range(1, N + 1):
        b[n] = (2 * n + 1) * e / (x * x * g[n - 1] / (2 * n - 1) - (n + 1) * g[n])
    return b


def scaled_numpy(N, fs, r, nfft, rho):
    """b'_n(k) F_n(kappa_k rho) [N+1][P] through the scaled form, the last bin with Re b'_n."""
    P = nfft // 2 + 1
    kappa = 2 * np.pi * (np.arange(P) * fs / nfft) / C_SOUND
    b = scaled_beta(N, kappa * r)
    n = np.arange(N + 1)
    last = (1j ** n) * b[:, -1]
    b[:, -1] = (-1j) ** n * last.real
    return b * scaled_g(N, kappa * rho) * ((r / rho) ** n)[:, None]
