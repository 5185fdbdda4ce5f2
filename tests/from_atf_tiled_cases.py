"""Inputs of the FromAtf dense-route tests above 4096 matched directions (tests/test_gpu_from_atf_tiled.py on the GPU,
tests/test_from_atf_tiled_inputs.py for the inputs themselves): the near-copy ATF sets of tests/from_atf_dense_cases.py -- ONE
isolated small singular value per bin, so the reference's clipped inverse stays well determined far above cond = 3e4 -- on
Fibonacci grids tall enough for the tiled form of the dense route (row blocks of at most 3072 rows + a tree step over their
triangles, wide_array.hip: launch_wa_factor_tiled).  Sizes as there: LEN = 256, 128 ATF taps, 257 bins.

The cutting rule: leaves = ceil(Dm / 3072), leaf height = ceil(Dm / leaves) rounded up to a multiple of 64, the last leaf takes the
rest.  The heights:
  4106  the first refused heights; two leaves (2112 + 1994 rows).  Cut at 4096 the second leaf would have 10 rows, fewer than the
        16 columns.
  4200  two leaves (2112 + 2088) at 8 microphones (the width that used factor.hip's register tiles below 4096) and at the
        narrowest and widest of the 9..32 forms
  6150  this rule's own awkward height: the first heights that need a third leaf (6145 on) also give the shortest last leaf the
        rule produces there, 2112 + 2112 + 1926
  9000  three leaves of 3008 + 3008 + 2984: full-height leaves, the tree stack three triangles tall
"""
import functools

import numpy as np

from from_atf_dense_cases import (ATF_TAPS, BASE_NOISE, COPY_EPS, F_TRANS, FS, KCUT0, LEN, NFFT, P, SHAPED)  # noqa: F401

BASE_NOISE = dict(BASE_NOISE)
COPY_EPS = dict(COPY_EPS)
# 8 microphones: the measurement floor and the difference of 16, so that every bin is above the limit by itself.  (9's values -- no
# floor, 1e-6 -- put the middle of the band below it at both widths, cond 170 at bin 255; those designs are dense at every bin
# because the route starts behind the HIGHEST offending bin and the rolled-off Nyquist bin is one: cond 9e10.)
BASE_NOISE[8], COPY_EPS[8] = BASE_NOISE[16], COPY_EPS[16]

#        name       M   HRIR directions, ATF directions   (the smaller grid is the matched one)
SHAPES = {
    "two16": (16, 4106, 4500),
    "two8": (8, 4500, 4200),
    "two9": (9, 4500, 4200),
    "two32": (32, 4500, 4200),
    "third16": (16, 6500, 6150),
    "three16": (16, 9500, 9000),
    "partly16": (16, 4500, 4200),
}
CASES = tuple(SHAPES)
ALL_DENSE = tuple(n for n in CASES if n != "partly16")


@functools.lru_cache(maxsize=None)
def fib_grid(ndirs):
    from emagls_amd import synth
    azi, zen = synth.fibonacci_grid(ndirs)
    hL, hR = synth.rigid_sphere_hrirs(azi, zen)
    return dict(hL=hL, hR=hR, azi=azi, zen=zen)


@functools.lru_cache(maxsize=None)
def base_atfs(nmics, natf):
    from emagls_amd import synth
    return synth.glasses_atfs(natf=natf, nmics=nmics, taps=ATF_TAPS, noise=BASE_NOISE[nmics])


def near_copy_atfs(nmics, natf):
    """cond(atfsMatched(k,:,:)) far above the limit at every bin (from_atf_dense_cases.near_copy_atfs on another grid)."""
    atf, aazi, azen = base_atfs(nmics, natf)
    atf = atf.copy()
    rng = np.random.default_rng(3)
    atf[:, nmics - 1, :] = atf[:, nmics - 2, :] + COPY_EPS[nmics] * rng.standard_normal(atf[:, nmics - 2, :].shape)
    return atf, aazi, azen


def shaped_copy_atfs(nmics, natf, which="above_cut"):
    """The frequency-shaped near-copy (from_atf_dense_cases.shaped_copy_atfs): only the lowest bins exceed the limit."""
    order, scale = SHAPED[which]
    atf, aazi, azen = base_atfs(nmics, natf)
    atf = atf.copy()
    rng = np.random.default_rng(5)
    d = rng.standard_normal(atf[:, nmics - 2, :].shape)
    d[ATF_TAPS - order:] = 0.0
    for _ in range(order):
        d = np.diff(d, axis=0, prepend=0.0)
    atf[:, nmics - 1, :] = atf[:, nmics - 2, :] + scale * d
    return atf, aazi, azen


def case(name):
    """(hL, hR, hrir grid [D x 2], atf, atf grid [Da x 2]) of a named case."""
    nmics, ndirs, natf = SHAPES[name]
    g = fib_grid(ndirs)
    atf, aazi, azen = shaped_copy_atfs(nmics, natf) if name == "partly16" else near_copy_atfs(nmics, natf)
    return g["hL"], g["hR"], np.column_stack([g["azi"], g["zen"]]), atf, np.column_stack([aazi, azen])


def matched(name):
    nmics, ndirs, natf = SHAPES[name]
    return min(ndirs, natf)


def conds(name):
    """cond(atfsMatched(k,:,:)) per bin 1 .. P-1 (0-based bins)."""
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
