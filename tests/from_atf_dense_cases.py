"""Inputs of the FromAtf dense-route tests at 9..32 microphones (tests/test_gpu_from_atf_dense.py on the GPU,
tests/test_from_atf_dense_inputs.py for the inputs themselves): ATF sets whose matched matrices atfsMatched(k,:,:) exceed the
Gram route's conditioning limit (cond < 3e4) at every bin or at the lowest bins only, while the reference's clipped inverse
(lib/getEMagLsFiltersFromAtf.m:100-120) stays well determined -- ONE isolated small singular value per bin.

One microphone is a near-copy of its neighbour: mic[M-1] = mic[M-2] + a small independent response.  The small singular value of a
bin is then about |difference(k)| sqrt(Dm / 2) and its singular vectors are fixed by the difference itself, far above rounding.
"""
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, LEN, F_TRANS = 48000.0, 256, 2000.0
NATF, ATF_TAPS = 2048, 128
NFFT = 512                      # 2^nextpow2(max(len, taps) ...) of these sizes: 257 bins
P = NFFT // 2 + 1
KCUT0 = int(np.ceil(F_TRANS / (FS / NFFT))) - 1   # first swept bin, 0-based (k_cut - 1): the bins below are least-squares bins


@functools.lru_cache(maxsize=None)
def thin_grid():
    """Every third of the 2702 golden HRIR directions (Dm = 901) with the suite's rigid-sphere HRIRs, as the `thin` fixture of
    tests/test_gpu_from_atf.py."""
    from emagls_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_fixtures.npz"))
    azi, zen = g["grid/hrirGridAziRad"], g["grid/hrirGridZenRad"]
    hL, hR = synth.rigid_sphere_hrirs(azi, zen)
    sub = slice(0, 2702, 3)
    return dict(hL=hL[:, sub], hR=hR[:, sub], azi=azi[sub], zen=zen[sub])


@functools.lru_cache(maxsize=None)
def fib_grid(ndirs=3500):
    """A Fibonacci HRIR grid of more than 3072 directions (the two-waves-per-column kernels) with synth's HRIR generator."""
    from emagls_amd import synth
    azi, zen = synth.fibonacci_grid(ndirs)
    hL, hR = synth.rigid_sphere_hrirs(azi, zen)
    return dict(hL=hL, hR=hR, azi=azi, zen=zen)


# The base set.  With noise = 0 the arc of a rigid sphere is rank deficient in FP64 at the low bins from about a dozen microphones on
# (singular values fall like (kr)^n / (2n-1)!!): the reference then inverts rounding noise and differs from itself between the two
# LAPACK drivers.  The widths where that happens keep glasses_atfs' own measurement floor; the near-copy sits on top of it.
BASE_NOISE = {9: 0.0, 16: 1e-4, 32: 1e-4}
# the near-copy's difference (white, so no bin holds an exact duplicate): small enough that EVERY bin exceeds the limit tenfold -- also
# the highest bins, where the responses roll off and a noise floor carries the matrix
COPY_EPS = {9: 1e-6, 16: 1e-9, 32: 1e-9}


@functools.lru_cache(maxsize=None)
def base_atfs(nmics):
    from emagls_amd import synth
    return synth.glasses_atfs(natf=NATF, nmics=nmics, taps=ATF_TAPS, noise=BASE_NOISE[nmics])


def near_copy_atfs(nmics, eps=None):
    """cond(atfsMatched(k,:,:)) far above the limit at every bin."""
    atf, aazi, azen = base_atfs(nmics)
    atf = atf.copy()
    eps = COPY_EPS[nmics] if eps is None else eps
    rng = np.random.default_rng(3)
    atf[:, nmics - 1, :] = atf[:, nmics - 2, :] + eps * rng.standard_normal(atf[:, nmics - 2, :].shape)
    return atf, aazi, azen


# difference filters and scalings of the frequency-shaped near-copy: |1 - e^{-iw}|^order grows with the bin, so only the lowest bins
# exceed the limit.  (order, scale) chosen on the CPU from conds() below so that the last bin above cond = 3e4 lies well inside
# (1, KCUT0) and (KCUT0, P): bin 7 (cond 2e6 at bin 1, 4e3 at bin 19) and about bin 130 (cond 2e5 at bin 22, 25 at the top).
SHAPED = {"below_cut": (2, 1e-3), "above_cut": (1, 4e-6)}


def shaped_copy_atfs(which, nmics=16):
    order, scale = SHAPED[which]
    atf, aazi, azen = base_atfs(nmics)
    atf = atf.copy()
    rng = np.random.default_rng(5)
    d = rng.standard_normal(atf[:, nmics - 2, :].shape)
    d[ATF_TAPS - order:] = 0.0                       # (room for the filter's tail: a truncated difference would leave a white floor)
    for _ in range(order):
        d = np.diff(d, axis=0, prepend=0.0)          # first difference along the taps
    atf[:, nmics - 1, :] = atf[:, nmics - 2, :] + scale * d
    return atf, aazi, azen


def case(name):
    """(hL, hR, hrir grid [D x 2], atf, atf grid [Da x 2]) of a named case."""
    if name.startswith("copy"):                      # copy9 / copy16 / copy32
        g, (atf, aazi, azen) = thin_grid(), near_copy_atfs(int(name[4:]))
    elif name in SHAPED:
        g, (atf, aazi, azen) = thin_grid(), shaped_copy_atfs(name)
    elif name == "tall":                             # 3072 < Dm <= 4096: the ATF grid is the smaller one, Dm = 3500
        g = fib_grid()
        from emagls_amd import synth
        atf, aazi, azen = synth.glasses_atfs(natf=4000, nmics=16, taps=ATF_TAPS, noise=BASE_NOISE[16])
        rng = np.random.default_rng(3)
        atf[:, 15, :] = atf[:, 14, :] + COPY_EPS[16] * rng.standard_normal(atf[:, 14, :].shape)
    else:
        raise KeyError(name)
    return g["hL"], g["hR"], np.column_stack([g["azi"], g["zen"]]), atf, np.column_stack([aazi, azen])


CASES = ("copy9", "copy16", "copy32", "below_cut", "above_cut", "tall")


def conds(name):
    """cond(atfsMatched(k,:,:)) per bin 1 .. P-1 (0-based bins), for choosing the scalings."""
    from oracle import emagls_oracle as O
    hL, hR, hg, atf, ag = case(name)
    smaller, idx, _ = O.matchGrids(hg, ag)
    X = np.fft.rfft(atf, NFFT, axis=0)               # [P x M x Da]
    if smaller:
        X = X[:, :, idx]
    out = np.empty(P - 1)
    for kb in range(1, P):
        s = np.linalg.svd(X[kb], compute_uv=False)
        out[kb - 1] = s[0] / s[-1]
    return out


@functools.lru_cache(maxsize=None)
def oracle_filters(name, driver=None):
    """The oracle's filters of a case; driver 'gesdd' / 'gesvd': with that LAPACK SVD (the switch of tools/fuzz_random.py)."""
    from oracle import emagls_oracle as O
    hL, hR, hg, atf, ag = case(name)
    if driver is None:
        return O.getEMagLsFiltersFromAtf(hL, hR, hg, atf, ag, FS, LEN, F_TRANS)[:2]
    import scipy.linalg as sl
    orig = np.linalg.svd
    np.linalg.svd = lambda a, full_matrices=False: sl.svd(a, full_matrices=full_matrices, lapack_driver=driver)
    try:
        return O.getEMagLsFiltersFromAtf(hL, hR, hg, atf, ag, FS, LEN, F_TRANS)[:2]
    finally:
        np.linalg.svd = orig
