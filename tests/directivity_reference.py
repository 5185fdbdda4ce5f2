"""The definition of DESIGN.md section 15 (source directivity and orientation of the array room responses) restated in NumPy: the
emission vectors of a shoebox room's components and the directive spectra.  Never the code under test: the basis is
oracle.getSH(Nd, ., 'real'), the undirected responses are the restatements the earlier sections' tests hold the library to
(legendre_spectra, spectral_legendre, point_legendre), and the enumeration is shoebox_numpy's.

The restatements take the real part of the last bin of every source they return, so a component's own last bin is recovered from
two calls: Im z = Re(-i z), and half a sample more of pre-delay multiplies the last bin (k = nfft / 2) by exp(-i pi / 2) = -i.
"""
import numpy as np

from oracle import emagls_oracle as O
from point_reference import point_legendre
from test_gpu_array_irs import legendre_spectra
from test_gpu_array_irs_spectral import spectral_legendre
from test_gpu_array_room_irs import shoebox_numpy


def shoebox_emission_numpy(room, beta, src, pos, fs, max_delay, max_order=None):
    """([J x 4] (azi, zen, delay, gain), [J x 3] emission vectors e_i = -(1 - 2 p_i) v_i / d) in the definition's order: shoebox_numpy's
    meshgrid and keep mask, restated with the parities kept; asserts that the four columns are that function's."""
    comps, _ = shoebox_numpy(room, beta, src, pos, fs, max_delay, max_order)        # (asserts the cut-off margin)
    L, beta, s, a = (np.asarray(v, dtype=np.float64) for v in (room, beta, src, pos))
    box = [int(np.floor(max_delay * 343.0 / fs / (2 * L[i]))) + 1 for i in range(3)]
    if max_order is not None:
        box = [min(b, (max_order + 1) // 2) for b in box]
    ax = [np.arange(-b, b + 1) for b in box]
    nz, ny, nx, pz, py, px = (g.ravel() for g in np.meshgrid(ax[2], ax[1], ax[0], [0, 1], [0, 1], [0, 1], indexing="ij"))
    g, order, v, sign = np.ones(nx.size), np.zeros(nx.size, dtype=np.int64), [], []
    for i, (n, p) in enumerate(((nx, px), (ny, py), (nz, pz))):
        e0, e1 = np.abs(n - p), np.abs(n)
        order += e0 + e1
        g = g * beta[2 * i] ** e0 * beta[2 * i + 1] ** e1
        v.append(((1 - 2 * p) * s[i] + 2 * n * L[i]) - a[i])
        sign.append(1 - 2 * p)
    d = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    tau, g = d / 343.0 * fs, g / d
    keep = (g != 0.0) & (tau <= max_delay)
    if max_order is not None:
        keep &= order <= max_order
    mine = np.column_stack([np.arctan2(v[1], v[0]), np.arccos(v[2] / d), tau, g])[keep]
    assert np.array_equal(mine, comps)
    e = np.column_stack([-sign[i] * v[i] / d for i in range(3)])[keep]
    return comps, e


def directivity_factors(emit, rot, coef):
    """D [J x P] of one source: emit [J x 3], rot [3 x 3] or None, coef [Kd x P] complex."""
    Kd = coef.shape[0]
    Nd = int(round(np.sqrt(Kd))) - 1
    assert (Nd + 1) ** 2 == Kd
    if emit.shape[0] == 0:
        return np.zeros((0, coef.shape[1]), dtype=complex)
    w = emit if rot is None else emit @ np.asarray(rot)                              # rows: (R^T e)^T = e^T R
    dirs = np.column_stack([np.arctan2(w[:, 1], w[:, 0]), np.arccos(np.clip(w[:, 2], -1.0, 1.0))])
    return O.getSH(Nd, dirs, "real") @ coef


def directive_spectra(fs, r, mics, sources, emits, rots, coefs, order, nfft, pre, dists=None, refl=None, exps=None, att=None, paths=None):
    """[Q x P x M]: the undirected restatement of every component on its own, times D_j(k), summed; the last bin is the real part of
    the sum.  sources: list of [J x 4]; emits: list of [J x 3]; rots: list of [3 x 3] (or None: identity for all); coefs: list of
    [Kd x P]; dists (point sources), refl / exps, att / paths as in point_legendre and spectral_legendre."""
    P = nfft // 2 + 1
    out = np.zeros((len(sources), P, mics.shape[0]), dtype=complex)
    for q, s in enumerate(sources):
        J = s.shape[0]
        if J == 0:
            continue
        D = directivity_factors(emits[q], None if rots is None else rots[q], np.asarray(coefs[q], dtype=complex))
        singles = [s[j:j + 1] for j in range(J)]
        one = lambda a: None if a is None else [a[q][j:j + 1] for j in range(J)]   # noqa: E731

        def each(pre_delay):
            if dists is not None:
                return point_legendre(fs, r, mics, singles, one(dists), order, nfft, pre_delay, refl, one(exps), att, one(paths))
            if refl is not None or att is not None:
                return spectral_legendre(fs, r, mics, singles, order, nfft, pre_delay, refl, one(exps), att, one(paths))
            return legendre_spectra(fs, r, mics, singles, order, nfft, pre_delay)

        H = each(pre)                                                                # [J x P x M], last bin real
        H[:, -1] = H[:, -1] + 1j * each(pre + 0.5)[:, -1].real
        out[q] = (H * D[:, :, None]).sum(axis=0)
        out[q, -1] = out[q, -1].real
    return out
