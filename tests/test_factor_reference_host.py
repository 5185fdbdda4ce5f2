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


# ------------------------------------------------------------------------------------------------ the narrow and the tiled cases
WIDE_BEFORE = [c["name"] for c in R.CASES if c["path"] == 1 and ((c["S"], c["C"]) in R.SHAPES1 or (c["cls"], c["S"], c["C"]) in R.EXTRA1)]
WIDE_BEFORE_SHA256 = "eb347667a61bca7cffac2193e28d51b927e6f980a96cf767070845325cbb2951"


def test_wide_fixture_kept_its_entries():
    """factor_truth_wide.npz gained the cases of 9 ... 32 columns by a partial run of the generator: the entries of the fifteen cases it held
    before are the bytes they were (key, dtype, shape and data of each, in the order of the keys, under one SHA-256 taken from the file as
    it was)"""
    import hashlib
    z = np.load(R.FIXTURES[1])
    assert len(WIDE_BEFORE) == 15
    h = hashlib.sha256()
    keys = sorted(k for k in z.files if k.split("/")[0] in WIDE_BEFORE)
    assert len(keys) == 9 * 15
    for k in keys:
        h.update(k.encode()); h.update(str(z[k].dtype).encode()); h.update(str(z[k].shape).encode()); h.update(np.ascontiguousarray(z[k]).tobytes())
    assert h.hexdigest() == WIDE_BEFORE_SHA256


def test_tiling_rule():
    """the cutting rule at the heights the issue of the tiled cases names"""
    assert R.tiling(4097, 9) == (2, 2112, 64) and 4097 - 2112 == 1985
    assert R.tiling(6145, 8) == (3, 2112, 64) and 6145 - 2 * 2112 == 1921
    assert R.tiling(6144, 8)[0] == 2 and R.tiling(16384, 32) == (6, 2752, 192)
    assert R.tiling(1025, 32, 1024) == (2, 576, 64) and 1025 - 576 == 449
    assert R.tiling(2049, 5, 1024)[0] == 3 and R.tiling(3073, 9, 1024)[0] == 4 and R.tiling(16384, 32, 1024) == (16, 1024, 512)
    assert R.tiling(6209, 9, 4096) == (2, 3136, 64)
    for c in R.CASES:
        if c["path"] == 2:
            rows, (leaves, leaf_h, _) = R.listed_rows(c), R.tiling(c["S"], c["C"], c["leaf_rows"])
            assert len(rows) <= 16 and {0, 1, c["S"] - 2, c["S"] - 1, leaf_h - 1, leaf_h, (leaves - 1) * leaf_h - 1, (leaves - 1) * leaf_h} <= set(rows.tolist())


def test_block_deficient_class():
    """K6: a leaf's own block has a zero column (a singular R_i, a tau = 0 step) while the matrix has full rank and nothing is clipped"""
    for c in R.CASES:
        if c["cls"] != "K6":
            continue
        X, _ = R.case_inputs(c)
        leaves, leaf_h, _ = R.tiling(c["S"], c["C"], c["leaf_rows"])
        first, last = X[:leaf_h], X[(leaves - 1) * leaf_h:]
        assert np.all(first[:, c["C"] // 2] == 0) and np.all(last[:, 0] == 0)
        _, tau, Ri = R.householder_qr(first)
        assert tau[c["C"] // 2] == 0.0 and Ri[c["C"] // 2, c["C"] // 2] == 0.0
        s = R.load_truth()[c["name"]]["s"][0]
        assert s.min() > R.REG_C * s.max()


TILED_HOST = ["p2_K1_1025x32_h1024", "p2_K2_1025x32_h1024", "p2_K6_1025x32_h1024", "p2_K1_2049x5_h1024", "p2_K2_3073x9_h1024", "p2_K1_4097x9",
              "p2_K2_4097x9", "p2_K6_4097x9", "p2_K2_6145x8", "p2_K6_6145x8", "p2_K2_6209x9_h4096"]


@pytest.mark.parametrize("name", TILED_HOST)
def test_tiled_stand_in_and_its_faults(name):
    """launch_wa_factor_tiled in plain NumPy (leaf QRs, stacked triangles, QR of the stack, Jacobi, two-level back-transform) meets all five
    measures within the bound; with each of the four injected index errors at least one asserted measure is 100 x beyond its bound.
    'short_last' is an error only where leaves x leaf_h passes ldS, so that the over-long last leaf reaches into the next column's storage
    (2049 x 5 and 6209 x 9 end exactly at ldS: there the extra rows are zeros, the result is the right one, and the test says so)"""
    case = R.CASE[name]
    tr = R.load_truth()[name]
    X, Hq = R.case_inputs(case)
    args = (X, Hq, case["mode"], case["reg_c"], case["tol_dim"], case["leaf_rows"])
    assert misses(case, tr, X, *R.tiled_route(*args)) == []
    leaves, leaf_h, _ = R.tiling(case["S"], case["C"], case["leaf_rows"])
    for fault in R.FAULTS:
        sv, Z, W = R.tiled_route(*args, fault=fault)
        if fault == "short_last" and leaves * leaf_h <= case["ldS"]:
            assert misses(case, tr, X, sv, Z, W) == []
            continue
        m = R.measures(tr, X, sv, Z, W)
        worst = max(m[k] / R.bound(float(tr["lapack"][i]), case["C"]) for i, k in enumerate(KEYS) if k in R.ASSERTED[case["cls"]])
        assert worst >= 100.0, (fault, m)
