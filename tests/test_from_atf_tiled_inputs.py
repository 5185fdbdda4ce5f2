"""A condition on the INPUTS of tests/test_gpu_from_atf_tiled.py, not on the library, as tests/test_from_atf_dense_inputs.py holds
it for the shorter cases: every case runs through the oracle with LAPACK's gesdd and with gesvd, and the two results must agree to
that file's SELF_TOL = 1e-8 relative, two decades under the suite's TOL = 1e-6.  A case that does not gets another input
(tests/from_atf_tiled_cases.py), never another bound."""
import numpy as np
import pytest

import from_atf_tiled_cases as C
from test_from_atf_dense_inputs import SELF_TOL, rel


@pytest.mark.parametrize("name", C.CASES)
def test_oracle_agrees_with_itself_across_svd_drivers(name):
    a, b = C.oracle_filters(name, "gesdd"), C.oracle_filters(name, "gesvd")
    dev = max(rel(a[0], b[0]), rel(a[1], b[1]))
    print(f"{name}: oracle gesdd vs gesvd = {dev:.3e}")
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert dev < SELF_TOL


def test_near_copies_put_the_whole_design_on_the_dense_route():
    """The route starts behind the highest bin above the limit, so the last bin decides: cond(atfsMatched(P-1,:,:)) > 1e5, the Gram
    route's limit of 3e4 with the factor 3 of room for the device's own estimate that the partly dense case keeps."""
    for name in C.ALL_DENSE:
        c = C.conds(name)
        print(f"{name}: cond {c.min():.3e} .. {c.max():.3e}, last bin {c[-1]:.3e}")
        assert c[-1] > 1e5, name


def test_partly_dense_case_crosses_the_limit_inside_the_swept_bins():
    """cond(atfsMatched(k,:,:)) > 3e4 at the lowest bins only, up to a bin between the first swept one and Nyquist, with a factor 3
    of room on either side for the device's own estimate."""
    c = C.conds("partly16")
    bins = np.arange(1, C.P)
    print(f"partly16: last bin above 1e5: {bins[c > 1e5].max()}, above 1e4: {bins[c > 1e4].max()}")
    assert bins[c > 1e5].max() >= C.KCUT0 and bins[c > 1e4].max() <= C.P - 2
    assert c[0] > 1e5
