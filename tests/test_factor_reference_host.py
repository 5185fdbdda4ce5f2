"""Host checks of the factor-chain reference (tests/factor_reference.py, tests/golden/factor_truth*.npz): the fixture belongs to the inputs
this machine rebuilds, correct factorisations pass its measures with the margin of the GPU test, and the errors a kernel could make do not.
No GPU."""
import numpy as np
import pytest

import factor_reference as R

KEYS = ("A", "B", "C", "DW", "DZ")
SMALL = ((31, 25), (129, 8))          # the shapes of the injected errors: three classes each
SMALL_CASES = [c for c in R.CASES if c["path"] == 0 and (c["S"], c["C"]) in SMALL]


def misses(case, tr, X, sv, Z, W):
    """the asserted measures a result does not meet"""
    m = R.measures(tr, X, sv, Z, W)
    return [k for i, k in enumerate(KEYS) if k in R.ASSERTED[case["cls"]] and not m[k] <= R.bound(float(tr["lapack"][i]), case["C"])]


def test_inputs_rebuild_bit_for_bit():
    """every input the fixture was computed for comes out of the integer generator again, to the bit"""
    truth = R.load_truth()
    for case in R.CASES:
        X, Hq = R.case_inputs(case)     # (asserts the checksum)
        assert X.shape == (case["S"], case["C"]) and np.all(np.isfinite(X.view(np.float64)))
        assert np.array_equal(truth[case["name"]]["rows"], R.listed_rows(case)) and len(truth[case["name"]]["rows"]) <= 16
    for case in R.GRAM_CASES:
        assert R.checksum(R.gram_chain(case)) == truth[case["name"]]["sum"][0]


@pytest.mark.parametrize("name", ["p0_K1_2x2", "p0_K2_2x2"])
def test_fixture_is_current(name):
    """the two cheapest cases recomputed at 100 digits: the stored hi + lo pairs to 1e-30"""
    ld = np.longdouble
    new, old = R.truth(R.CASE[name]), R.load_truth()[name]
    for key in ("s", "s_reg", "P", "W", "Z"):
        a, b = new[key], old[key]
        d = (a[0] - b[0]).astype(np.clongdouble if np.iscomplexobj(a) else ld) + (a[1] - b[1])
        assert np.max(np.abs(d)) <= ld(1e-30) * max(1.0, float(np.max(np.abs(b[0])))), key
    assert new["sum"][0] == old["sum"][0]


def test_lapack_passes_every_case():
    """FP64 LAPACK in the kernel's place meets every bound: it is measured against its own stored error, with the margin"""
    truth = R.load_truth()
    for case in R.CASES:
        X, Hq = R.case_inputs(case)
        sv, Z, W = R.lapack_route(X, Hq, case["mode"], case["reg_c"], case["tol_dim"])
        assert misses(case, truth[case["name"]], X, sv, Z, W) == [], case["name"]
    for case in R.GRAM_CASES:
        tr, A = truth[case["name"]], R.gram_chain(case)
        for k in range(R.GRAM_BINS):
            s, M = R.gram_lapack(A[k])
            m = R.gram_measures(tr, k, s, M)
            assert m["A"] <= R.bound(tr["lapack"][k, 0], case["C"]) and m["M"] <= R.bound(tr["lapack"][k, 1], case["C"]), (case["name"], k)


@pytest.mark.parametrize("order", ["cyclic", "reverse"])
def test_householder_jacobi_passes(order):
    """so does the chain of factor.hip written in plain NumPy (Householder QR, Hestenes-Jacobi on R^H), in two rotation orders: the margin
    of 8 holds between two backward-stable methods, on every case of up to 32 columns"""
    truth = R.load_truth()
    for case in R.CASES:
        if case["path"] != 0:
            continue
        X, Hq = R.case_inputs(case)
        sv, Z, W = R.jacobi_route(X, Hq, case["mode"], case["reg_c"], case["tol_dim"], order=order)
        assert misses(case, truth[case["name"]], X, sv, Z, W) == [], case["name"]


@pytest.mark.parametrize("case", SMALL_CASES, ids=[c["name"] for c in SMALL_CASES])
def test_injected_errors_fail(case):
    """what a subtly wrong kernel would return fails at least one measure, on every case of two small shapes the error can touch: the clip
    constant on the cases with clipped singular values (K2; K1 clips nothing and the modes of K4 / K5 have no clip), the others on all"""
    tr = R.load_truth()[case["name"]]
    X, Hq = R.case_inputs(case)
    args = (X, Hq, case["mode"], case["reg_c"], case["tol_dim"])
    sv, Z, W = R.lapack_route(*args)
    assert misses(case, tr, X, sv, Z, W) == []
    if case["cls"] == "K2":     # 0.0101 s_max instead of 0.01 s_max
        assert misses(case, tr, X, *R.lapack_route(*args, clip=0.0101)) != []
    # one Jacobi rotation of size 1e-9 left out
    assert misses(case, tr, X, *R.jacobi_route(*args)) == []
    assert misses(case, tr, X, *R.jacobi_route(*args, unrotate=1e-9)) != []
    # the last row of Z dropped
    Zd = Z.copy()
    Zd[-1] = 0.0
    assert misses(case, tr, X, sv, Zd, Hq @ Zd) != []
    # one column of Z not conjugated
    Zc = Z.copy()
    Zc[:, case["C"] // 2] = np.conj(Zc[:, case["C"] // 2])
    assert misses(case, tr, X, sv, Zc, Hq @ Zc) != []


@pytest.mark.parametrize("S,Cn", [(129, 8), (257, 2)])     # (many more rows than columns: the two tolerances lie well apart)
def test_injected_pinv_tolerance_fails(S, Cn):
    """reg_mode 1 with min(size) eps(s_max) instead of max(size) eps(s_max).  The classes of the fixture cannot show it -- K4 and K5 keep every
    singular value 100 x above the tolerance or exactly zero, and the rounding residue of K5's null direction lies below both tolerances --,
    so the matrix is built here: integers with the last column = the first + 2^-k x another, its smallest singular value between the two
    tolerances; the truth (which drops it) is computed on the spot."""
    X = R.integer_matrix(S, Cn, 31337 + S)
    other = R.integer_matrix(S, 1, 4242 + S)[:, 0]
    smax = np.linalg.svd(X, compute_uv=False).max()
    lo, hi = R.pinv_tol(smax, float(min(S, Cn))), R.pinv_tol(smax, float(max(S, Cn)))
    k = int(round(-np.log2(np.sqrt(2.0 * lo * hi) / np.linalg.norm(other))))   # (the two nearly equal columns share the perturbation: s_min ~ 2^-k |other| / sqrt 2)
    X[:, Cn - 1] = X[:, 0] + other * 2.0 ** -k
    Hq = R.integer_matrix(2, S, 99, 4)
    s = np.linalg.svd(X, compute_uv=False)
    assert lo * 2 < s.min() < hi / 2 and s[-2] > 100 * hi
    case = dict(name="tol", C=Cn, cls="K5")
    tr = R.truth_of(X, Hq, 1, R.REG_C, float(max(S, Cn)), [0, 1, S - 2, S - 1])
    assert tr["s_reg"][0].min() == 0.0
    sv, Z, W = R.lapack_route(X, Hq, 1, R.REG_C, float(max(S, Cn)))
    tr["zmax"] = np.abs(Z).max()
    m = R.measures(tr, X, sv, Z, W)
    tr["lapack"] = np.array([m[key] for key in KEYS])
    assert max(m[key] for key in ("A", "B", "C")) < 100 * Cn * R.EPS     # the right rule: at rounding level
    assert misses(case, tr, X, *R.lapack_route(X, Hq, 1, R.REG_C, float(max(S, Cn)), tol_size=float(min(S, Cn)))) != []
