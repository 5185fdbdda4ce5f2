"""A condition on the INPUTS of tests/test_gpu_from_atf_dense.py, not on the library: the reference's result must be defined far
below the suite's tolerance on them.  An ATF set above the Gram route's conditioning limit is one step from a set whose clipped
inverse (lib/getEMagLsFiltersFromAtf.m:100-120) carries 100 / s_max times singular vectors of rounding noise -- there the oracle
differs from itself between LAPACK's two SVD drivers and no implementation can be held to it.  So every case runs through the
oracle with gesdd and with gesvd (the switch of tools/fuzz_random.py); the two must agree to 1e-8 relative, two decades under
TOL = 1e-6.  A case that does not gets another input (tests/from_atf_dense_cases.py), never another bound."""
import numpy as np
import pytest

import from_atf_dense_cases as C

SELF_TOL = 1e-8


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", C.CASES)
def test_oracle_agrees_with_itself_across_svd_drivers(name):
    a, b = C.oracle_filters(name, "gesdd"), C.oracle_filters(name, "gesvd")
    dev = max(rel(a[0], b[0]), rel(a[1], b[1]))
    print(f"{name}: oracle gesdd vs gesvd = {dev:.3e}")
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert dev < SELF_TOL


def test_shaped_cases_cross_the_limit_where_they_should():
    """cond(atfsMatched(k,:,:)) > 3e4 at the lowest bins only: up to a bin below the first swept one / between it and Nyquist, with
    a factor 3 of room on either side for the device's own estimate."""
    for name, lo, hi in (("below_cut", 1, C.KCUT0 - 1), ("above_cut", C.KCUT0, C.P - 2)):
        c = C.conds(name)
        bins = np.arange(1, C.P)
        assert bins[c > 1e5].max() >= lo and bins[c > 1e4].max() <= hi, name
        assert c[0] > 1e5
