"""Y_reg_inv_k = Q Z_k of the designs with 33 ... 64 channels (wa_yri_kernel and wa_yri_mfma_kernel of csrc/wide_array.hip, the latter on
v_mfma_f64_16x16x4 with a hand-made row order), run by the debug entry emagls_debug_wa_yri through launch_wa_yri in both forms
(EMAGLS_WA_YRI_MFMA, read per call).

Integer cases: Q and Z of small integers (|values| <= 8), so that every partial sum is an integer below 2^53 and the result is the NumPy
product bit for bit whatever the order of the sum -- a layout test: the row permutation of the matrix-core form, the tail masks in S (chunks
of 32), C (tiles of 8 channels) and D (blocks of 64, tiles of 16), two bins with different Z, paddings of NaN on the input side that must
not be read and the sentinel in the columns D ... ldD-1 of the output.  One rounded case: the rows s of Z scaled by powers of two over 48
bits, against the longdouble product within the a-priori bound of a real dot product of S terms in any order, gamma_(S+1) (|Q| |Z|) per
component (gram_reference.g_terms).
"""
import numpy as np
import pytest

import factor_reference as R
import gram_reference as G

pytestmark = pytest.mark.gpu

FORMS = [("0", "vector"), ("1", "mfma")]


def up64(n):
    return 64 * ((n + 63) // 64)


def checked(rc):
    """a HIP error ends the session: nothing more is started on a device that has faulted"""
    from emagls_amd import _lib as L
    if rc == L.ERR_HIP:
        pytest.exit("HIP error in a debug entry: %s" % L.load().emagls_last_error().decode(), returncode=3)
    L.check(rc)


def run_yri(Q, Z, ldD):
    """Q [D][S] real, Z [bins][C][S] complex -> Yri [bins][C][D] and its padding [bins][C][ldD - D]; the inputs padded with NaN to ldS"""
    from emagls_amd import _lib as L
    D, S = Q.shape
    nb, Cn, _ = Z.shape
    ldS = up64(S)
    Qp = np.full((D, ldS), np.nan)
    Qp[:, :S] = Q
    Zp = np.full((nb, Cn, ldS), np.nan + 1j * np.nan)
    Zp[:, :, :S] = Z
    Y = np.zeros((nb, Cn, ldD), dtype=np.complex128)
    checked(L.load().emagls_debug_wa_yri(Qp.ctypes.data, ldS, Zp.ctypes.data, S, Cn, ldS, D, ldD, nb, Y.ctypes.data))
    return Y[:, :, :D], Y[:, :, D:]


def is_sentinel(a):
    from emagls_amd import _lib as L
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(L.DEBUG_SENTINEL_BITS)


@pytest.mark.parametrize("S", [1, 33, 449])
@pytest.mark.parametrize("flag,form", FORMS, ids=[f[1] for f in FORMS])
def test_integer_product_is_exact(flag, form, S, monkeypatch):
    monkeypatch.setenv("EMAGLS_WA_YRI_MFMA", flag)
    for Cn in (5, 33, 40, 64):
        for D in (1, 63, 65, 130):
            seed = 7000 + 97 * S + 13 * Cn + D
            Q = R.ints(seed, D * S, -8, 8).astype(np.float64).reshape(D, S)
            z = R.ints(seed + 1, 2 * 2 * Cn * S, -8, 8).astype(np.float64).reshape(2, 2, Cn, S)
            Z = z[0] + 1j * z[1]
            want = np.stack([Z[k].real @ Q.T + 1j * (Z[k].imag @ Q.T) for k in range(2)])   # (integers below 2^53: exact in any order)
            got, pad = run_yri(Q, Z, up64(D))
            assert np.array_equal(got, want), (form, S, Cn, D, np.argwhere(got != want)[:4])
            assert np.all(is_sentinel(pad)), (form, S, Cn, D)
    assert not np.array_equal(Z[0], Z[1])


@pytest.mark.parametrize("flag,form", FORMS, ids=[f[1] for f in FORMS])
def test_rounded_product_within_the_dot_product_bound(flag, form, monkeypatch):
    monkeypatch.setenv("EMAGLS_WA_YRI_MFMA", flag)
    S, Cn, D = 449, 64, 130
    Q = R.ints(4711, D * S, -8, 8).astype(np.float64).reshape(D, S) * np.ldexp(1.0, -(np.arange(D) % 5))[:, None]
    z = R.ints(4712, 2 * 2 * Cn * S, -8, 8).astype(np.float64).reshape(2, 2, Cn, S) * np.ldexp(1.0, -3 * (np.arange(S) % 17))   # rows s: 48 bits apart
    Z = z[0] + 1j * z[1]
    got, pad = run_yri(Q, Z, up64(D))
    assert np.all(is_sentinel(pad))
    ld = np.longdouble
    factor = G.g_terms(S + 1, False)
    worst = 0.0
    for k in range(2):
        for part, have in ((Z[k].real, got[k].real), (Z[k].imag, got[k].imag)):
            want = part.astype(ld) @ Q.T.astype(ld)
            bound = factor * (np.abs(part) @ np.abs(Q.T))
            e = np.abs(have.astype(ld) - want).astype(np.float64)
            assert np.all(bound > 0)
            worst = max(worst, float(np.max(e / bound)))
    print("wa_yri %s %dx%dx%d: largest error / bound %.3g" % (form, S, Cn, D, worst))
    assert worst <= 1.0, worst
