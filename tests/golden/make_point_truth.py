"""Writes tests/golden/point_truth.npz: the multiprecision truth of the point-source array responses at the extreme orders
(tests/test_array_point_host.py, tests/test_gpu_array_point.py).  Run from the repository root:

    python tests/golden/make_point_truth.py        (about four minutes on one core)

The shape: fs 8000, r = 0.042, nfft 1024 (513 bins), the distances RHO = 1.2 r, 3 r, 1 m, 20 m, orders up to 85.  mpmath at 120 digits:

    F_n(x)   = sum_{m <= n} (n+m)! / (m! (n-m)!) (1 / (2ix))^m                      (the finite sum, no recurrence)
    h_n(x)   = i^(n+1) e^(-ix) F_n(x) / x,   h_n' = h_(n-1) - (n+1)/x h_n               (h = h^(2))
    b'_n(x)  = (2n+1) i^(n+1) / (x^2 h_n'(x))       (= -b_n (2n+1)/(4 pi), b_n = 4 pi i^n (j_n - j_n'/h_n' h_n), by the Wronskian)

and a handful of entries are checked against mpmath's own besselj / bessely with a numerical derivative before anything is written.
In the last bin Re b'_n is used; bin 0 is the limit -(2n+1)/(n+1) (r/rho)^n.

    table   [86][NB][4] complex   b'_n(k) F_n(kappa_k rho) at the bins `bins` [NB] (0 .. 16, then every eighth, and the last): a full table
                                  would pass the size limit of a committed file
    mics    [2][2], dirs [4][2]   (azi, zen) of the response case
    resp44, resp85 [4][513][2] complex   sum_{n <= N} b'_n(k) F_n(kappa_k rho_j) P_n(u_j . v_m), N = 44 and 85, per component, ALL bins
"""
import os

import mpmath as mp
import numpy as np

FS, R, NFFT, NMAX = 8000.0, 0.042, 1024, 85
RHO = (1.2 * R, 3 * R, 1.0, 20.0)
MICS = np.array([[0.3, 1.1], [2.9, 2.0]])
DIRS = np.array([[0.0, 1.5], [1.0, 0.4], [-2.0, 2.5], [3.0, 1.2]])
mp.mp.dps = 120


def F_all(nmax, x):
    """F_0 .. F_nmax at x > 0 by the finite sum."""
    z = 1 / (2j * x)
    out = []
    for n in range(nmax + 1):
        s, zm = mp.mpc(0), mp.mpc(1)
        for m in range(n + 1):
            s += mp.factorial(n + m) / (mp.factorial(m) * mp.factorial(n - m)) * zm
            zm *= z
        out.append(s)
    return out


def h2_all(nmax, x):
    F = F_all(nmax, x)
    e = mp.exp(-1j * x)
    return [mp.mpc(0, 1) ** (n + 1) * e * F[n] / x for n in range(nmax + 1)]


def bprime_all(nmax, x, real_part):
    h = h2_all(max(nmax, 1), x)
    out = []
    for n in range(nmax + 1):
        dh = (h[n - 1] if n else -h[1]) - (mp.mpf(n + 1) / x * h[n] if n else 0)       # h_0' = -h_1
        b = (2 * n + 1) * mp.mpc(0, 1) ** (n + 1) / (x * x * dh)
        out.append(mp.mpc(b.real, 0) if real_part else b)
    return out


def spot_check():
    jn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.besselj(n + mp.mpf(1) / 2, x)   # noqa: E731
    yn = lambda n, x: mp.sqrt(mp.pi / (2 * x)) * mp.bessely(n + mp.mpf(1) / 2, x)   # noqa: E731
    h2 = lambda n, x: jn(n, x) - 1j * yn(n, x)                                     # noqa: E731
    for n, x, y in ((0, "0.31", "7.3"), (4, "0.02", "0.05"), (19, "1.7", "0.4"), (85, "3.07", "3.7"), (85, "0.003", "1500")):
        x, y = mp.mpf(x), mp.mpf(y)
        bn = 4 * mp.pi * mp.mpc(0, 1) ** n * (jn(n, x) - mp.diff(lambda t: jn(n, t), x) / mp.diff(lambda t: h2(n, t), x) * h2(n, x))
        want_b = -bn * (2 * n + 1) / (4 * mp.pi)
        want_F = mp.mpc(0, -1) ** (n + 1) * y * mp.exp(1j * y) * h2(n, y)
        got_b, got_F = bprime_all(n, x, False)[n], F_all(n, y)[n]
        assert abs(got_b - want_b) < mp.mpf(10) ** -40 * abs(want_b), (n, x)       # (the numerical derivative limits this one)
        assert abs(got_F - want_F) < mp.mpf(10) ** -80 * abs(want_F), (n, y)


def legendre(nmax, x):
    p = [mp.mpf(1), x]
    for n in range(1, nmax):
        p.append(((2 * n + 1) * x * p[n] - n * p[n - 1]) / (n + 1))
    return p


def unit(d):
    return [mp.sin(d[1]) * mp.cos(d[0]), mp.sin(d[1]) * mp.sin(d[0]), mp.cos(d[1])]


def main():
    spot_check()
    P = NFFT // 2 + 1
    bins = sorted(set(range(17)) | set(range(0, P, 8)) | {P - 1})
    r = mp.mpf(R)
    rho = [mp.mpf(v) for v in RHO]                                                    # (the doubles the tests pass)
    cosang = [[sum(a * b for a, b in zip(unit([mp.mpf(v) for v in d]), unit([mp.mpf(v) for v in m]))) for m in MICS] for d in DIRS]
    pn = [[legendre(NMAX, c) for c in row] for row in cosang]
    table = np.zeros((NMAX + 1, len(bins), 4), dtype=complex)
    resp = {44: np.zeros((4, P, 2), dtype=complex), 85: np.zeros((4, P, 2), dtype=complex)}
    for k in range(P):
        kappa = 2 * mp.pi * (mp.mpf(k) * mp.mpf(FS) / NFFT) / 343
        if k:
            bp = bprime_all(NMAX, kappa * r, k == P - 1)
        for j in range(4):
            if k:
                F = F_all(NMAX, kappa * rho[j])
                prod = [bp[n] * F[n] for n in range(NMAX + 1)]
            else:
                prod = [-mp.mpf(2 * n + 1) / (n + 1) * (r / rho[j]) ** n for n in range(NMAX + 1)]
            if k in bins:
                table[:, bins.index(k), j] = [complex(v) for v in prod]
            for N in resp:
                for m in range(2):
                    resp[N][j, k, m] = complex(sum(prod[n] * pn[j][m][n] for n in range(N + 1)))
        if k % 64 == 0:
            print("bin", k, flush=True)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "point_truth.npz")
    np.savez(out, table=table, bins=np.array(bins), rho=np.array([float(v) for v in rho]), mics=MICS, dirs=DIRS, resp44=resp[44],
             resp85=resp[85], fs=FS, r=R, nfft=NFFT)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
