"""The per-bin factor chain -- launch_factor (csrc/factor.hip: assemble or load, Householder QR, one-sided Jacobi in LDS, back-transform),
launch_wa_factor (csrc/wide_array.hip: 33..64 columns, and 9..32 as FromAtf's dense route calls it), launch_wa_factor_tiled (the same in
row blocks with a tree step, path 2; the leaf bound as a parameter), launch_wa_ls behind both (the least-squares rows W) and
launch_factor_jacobi_gram (the Jacobi kernel on A = B^H B with warm starts) --
run by the debug entries emagls_debug_factor / emagls_debug_factor_gram on the matrices of tests/factor_reference.py and held against the
multiprecision truth of tests/golden/factor_truth*.npz.

Shapes: the smallest and the largest of each of the nine template instances dispatch() picks by row count, and of the four forms of the
wide path; classes K1 ... K5 of factor_reference.py.  Measures A (singular values), B (the singular values of Z against s_reg: the
orthonormality of U), C (X^H conj(Z) against P) do not depend on the conditioning; D (W and listed rows of Z, forward) does.

Tolerances are measured, not chosen: a kernel result passes within 8 x max(e, C eps), e the error FP64 LAPACK makes on the same case through
the same formulas (stored next to the truth).  D is asserted on K1, K2, K4, K5 and printed for K3, where LAPACK's own forward error is 1e-4.
With EMAGLS_FACTOR_CHAIN_REPORT=<file> the module writes every measured value there (profiles/r22_factor_chain.md is such a file; profiles/r30_dense_route.md holds the rows of
the narrow and the tiled cases).
"""
import ctypes as C
import os

import numpy as np
import pytest

import factor_reference as R

pytestmark = pytest.mark.gpu

KEYS = ("A", "B", "C", "DW", "DZ")
REPORT = []     # (case, variant, measure, kernel, lapack, asserted)


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    path = os.environ.get("EMAGLS_FACTOR_CHAIN_REPORT")
    if not path or not REPORT:
        return
    with open(path, "w") as f:
        f.write("| case | run | measure | kernel | LAPACK | kernel / max(LAPACK, C eps) | asserted |\n|---|---|---|---|---|---|---|\n")
        for case, variant, key, err, ref, floor, asserted in REPORT:
            f.write("| %s | %s | %s | %.3g | %.3g | %.3g | %s |\n" % (case, variant, key, err, ref, err / max(ref, floor), "yes" if asserted else "no"))


def ptr(a):
    return a.ctypes.data if a is not None else None


def checked(rc):
    """a HIP error ends the session: nothing more is started on a device that has faulted"""
    from emagls_amd import _lib as L
    if rc == L.ERR_HIP:
        pytest.exit("HIP error in a debug entry: %s" % L.load().emagls_last_error().decode(), returncode=3)
    L.check(rc)


def is_sentinel(a):
    from emagls_amd import _lib as L
    return np.ascontiguousarray(a).view(np.uint64) == np.uint64(L.DEBUG_SENTINEL_BITS)


def pack(Xs, ldS):
    """matrices [S][C] -> the entry's layout [bin][c][ldS], the padding NaN on the input side too (it must not be read)"""
    S, Cn = Xs[0].shape
    out = np.full((len(Xs), Cn, ldS), np.nan + 1j * np.nan)
    for i, X in enumerate(Xs):
        out[i, :, :S] = X.T
    return out


def run_factor(S, Cn, ldS, nbins=1, Xd=None, xd_stride=None, Tn=None, bn=None, kb0=0, P=None, mode=0, reg_c=R.REG_C, tol_dim=0.0, Hq=None,
               ls_end=None, hq_conj=0, phases=3, path=0, leaf_rows=0, expect=0):
    """one call of emagls_debug_factor; returns Z [bin][S][C], the padding [bin][C][ldS - S], sv, sweeps, N, R2, tau, W [2][P][C]"""
    from emagls_amd import _lib as L
    P = nbins if P is None else P
    Z = np.zeros((nbins, Cn, ldS), dtype=np.complex128)
    sv = np.zeros((nbins, Cn))
    sweeps = np.zeros(nbins, dtype=np.int32)
    N = np.zeros((nbins, Cn, Cn), dtype=np.complex128)
    R2 = np.zeros_like(N)
    tau = np.zeros((nbins, Cn))
    W = np.zeros((2, P, Cn), dtype=np.complex128)
    a = L.DebugFactorArgs(S=S, C=Cn, ldS=ldS, nbins=nbins, kb0=kb0, P=P, reg_mode=mode, reg_c=reg_c, tol_dim=tol_dim, phases=phases, path=path,
                          hq_conj=hq_conj, leaf_rows=leaf_rows, Z=ptr(Z), sv=ptr(sv), sweeps=ptr(sweeps), N=ptr(N), R2=ptr(R2), tau=ptr(tau), W=ptr(W))
    keep = []
    if Xd is not None:
        Xd = np.ascontiguousarray(Xd, dtype=np.complex128)
        a.Xd, a.xd_stride = ptr(Xd), (Cn * ldS if xd_stride is None else xd_stride)
    else:
        Tn = np.ascontiguousarray(Tn)
        bn = np.ascontiguousarray(bn, dtype=np.complex128)
        a.Tn, a.tn_cplx, a.bn, a.nOrders = ptr(Tn), int(np.iscomplexobj(Tn)), ptr(bn), bn.shape[1]
    if Hq is not None:
        Hp = np.zeros((2, nbins, ldS), dtype=np.complex128)
        Hp[:, :, :S] = Hq
        keep.append(Hp)
        a.Hq, a.ldHq, a.ls_end = ptr(Hp), ldS, (P if ls_end is None else ls_end)
    rc = L.load().emagls_debug_factor(C.byref(a))
    if expect != 0:
        assert rc == expect, (rc, L.load().emagls_last_error())
        return L.load().emagls_last_error().decode()
    checked(rc)
    return dict(Z=np.transpose(Z[:, :, :S], (0, 2, 1)).copy(), pad=Z[:, :, S:], sv=sv, sweeps=sweeps, N=N, R2=R2, tau=tau, W=W)


def judge(case, tr, X, sv, Z, W, variant, failures):
    """the measures of one bin against the case's bounds; records them, appends what misses to `failures`"""
    m = R.measures(tr, X, sv, Z, W)
    for i, key in enumerate(KEYS):
        ref, floor = float(tr["lapack"][i]), case["C"] * R.EPS
        asserted = key in R.ASSERTED[case["cls"]]
        REPORT.append((case["name"], variant, key, m[key], ref, floor, asserted))
        print("%-18s %-10s %-2s kernel %.3g  LAPACK %.3g  ratio %.3g%s" % (case["name"], variant, key, m[key], ref, m[key] / max(ref, floor),
                                                                          "" if asserted else "  (not asserted)"))
        if asserted and not m[key] <= R.bound(ref, case["C"]):
            failures.append("%s %s %s: %.3g > 8 x max(%.3g, %.3g)" % (case["name"], variant, key, m[key], ref, floor))
    return m


def run_case(case, variant="", **kw):
    tr = R.load_truth()[case["name"]]
    X, Hq = R.case_inputs(case)
    S, Cn, ldS = case["S"], case["C"], case["ldS"]
    wide = case["path"] != 0
    # (the wide paths: W by launch_wa_ls behind the factor, as the designs form it; one more row of W than bins, which nothing may write)
    out = run_factor(S, Cn, ldS, Xd=pack([X], ldS), mode=case["mode"], reg_c=case["reg_c"], tol_dim=case["tol_dim"], path=case["path"],
                     leaf_rows=case.get("leaf_rows", 0), Hq=Hq[:, None, :], P=2 if wide else None, ls_end=1 if wide else None, **kw)
    if wide:
        assert np.all(is_sentinel(out["W"][:, 1])) and not np.any(is_sentinel(out["W"][:, 0])), "W beyond the bins was written, or a row of a bin was not"
    failures = []
    judge(case, tr, X, out["sv"][0], out["Z"][0], out["W"][:, 0, :], variant or "single", failures)
    assert not failures, failures
    assert 1 <= out["sweeps"][0] <= 20, out["sweeps"]
    assert np.all(np.isfinite(out["tau"])) and np.all(np.isfinite(out["N"])) and np.all(np.isfinite(out["R2"]))
    if case["path"] == 0:
        assert np.all(is_sentinel(out["pad"])), "rows S ... ldS-1 of Z were written"
    else:
        assert np.all(out["pad"] == 0), "rows S ... ldS-1 of Z are not the zeros the wide forms write"
    return out


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["path"] == 0])
def test_factor_case(name):
    run_case(R.CASE[name])


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["path"] == 1])
def test_wide_case(name):
    run_case(R.CASE[name])


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["path"] == 2])
def test_tiled_case(name):
    """launch_wa_factor_tiled: the leaves' QR (LEAF = true instances of the tall and, at a leaf bound of 4096, of the pair form), the stacked
    triangles, the tree step through launch_wa_factor at 1 ... 32 columns, the leaves' back-transform with their T_i, launch_wa_ls"""
    run_case(R.CASE[name])


@pytest.mark.parametrize("name,switch", [("p1_K2_449x9", "EMAGLS_WA_TALL"), ("p1_K2_448x32", "EMAGLS_WA_REG")])
def test_narrow_case_plain_forms(name, switch, monkeypatch):
    """449 x 9 without the tall forms (the kernels that walk the columns through L2) and 448 x 32 without the register form (the tall one
    in its place): the same truth, the same bound"""
    monkeypatch.setenv(switch, "0")
    run_case(R.CASE[name], variant=switch[7:].lower() + "=0")


@pytest.mark.parametrize("shape,leaf_rows", [("4097x9", 0), ("1025x32_h1024", 1024)])
def test_tiled_slots(shape, leaf_rows):
    """the K1, K2 and K6 matrices of one shape as the three bins of one launch (tau, R_i and T_i at the slot bin x leaves + leaf): every
    bin's Z, singular values and W are those of its single-bin launch, bit for bit"""
    cases = [R.CASE["p2_%s_%s" % (k, shape)] for k in ("K1", "K2", "K6")]
    Xs, Hs = zip(*[R.case_inputs(c) for c in cases])
    S, Cn, ldS = cases[0]["S"], cases[0]["C"], cases[0]["ldS"]
    out = run_factor(S, Cn, ldS, nbins=3, Xd=pack(Xs, ldS), Hq=np.stack(Hs, axis=1), path=2, leaf_rows=leaf_rows)
    assert np.all(out["pad"] == 0) and np.all((out["sweeps"] >= 1) & (out["sweeps"] <= 20))
    for i in range(3):
        one = run_factor(S, Cn, ldS, Xd=pack(Xs[i:i + 1], ldS), Hq=Hs[i][:, None, :], path=2, leaf_rows=leaf_rows)
        assert np.all(np.isfinite(one["Z"])) and np.all(np.isfinite(one["W"]))
        assert np.array_equal(out["Z"][i], one["Z"][0]) and np.array_equal(out["sv"][i], one["sv"][0]), i
        assert np.array_equal(out["W"][:, i], one["W"][:, 0]), i


def test_tiled_equal_bits():
    """no atomics, every sum in a fixed order: a second run gives the same bits"""
    case = R.CASE["p2_K2_6145x8"]
    X, Hq = R.case_inputs(case)
    a, b = [run_factor(case["S"], case["C"], case["ldS"], Xd=pack([X], case["ldS"]), Hq=Hq[:, None, :], path=2) for _ in range(2)]
    assert np.all(np.isfinite(a["Z"]))
    for key in ("Z", "sv", "W", "N", "R2", "tau", "sweeps"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES if c["path"] == 1 and (c["S"], c["C"]) in ((448, 64), (449, 40))])
def test_wide_case_plain_forms(name, monkeypatch):
    """the same with the register and the LDS-reflector forms switched off: the kernels that walk the columns through L2"""
    monkeypatch.setenv("EMAGLS_WA_REG", "0")
    monkeypatch.setenv("EMAGLS_WA_TALL", "0")
    run_case(R.CASE[name], variant="plain")


def test_several_bins_in_one_launch():
    """three distinct matrices of one shape as the bins of one launch, each against its own truth; then one matrix read by three bins
    (xd_stride = 0): every bin is the single launch's result, bit for bit"""
    cases = [R.CASE["p0_%s_33x32" % k] for k in ("K1", "K2", "K3")]
    Xs, Hs = zip(*[R.case_inputs(c) for c in cases])
    S, Cn, ldS = 33, 32, cases[0]["ldS"]
    out = run_factor(S, Cn, ldS, nbins=3, Xd=pack(Xs, ldS), Hq=np.stack(Hs, axis=1))
    failures = []
    for i, c in enumerate(cases):
        judge(c, R.load_truth()[c["name"]], Xs[i], out["sv"][i], out["Z"][i], out["W"][:, i, :], "bin %d of 3" % i, failures)
    assert not failures, failures
    assert np.all(is_sentinel(out["pad"])) and np.all((out["sweeps"] >= 1) & (out["sweeps"] <= 20))
    one = run_factor(S, Cn, ldS, Xd=pack(Xs[1:2], ldS), Hq=Hs[1][:, None, :])
    same = run_factor(S, Cn, ldS, nbins=3, Xd=pack(Xs[1:2], ldS), xd_stride=0, Hq=np.stack([Hs[1]] * 3, axis=1))
    for i in range(3):
        assert np.array_equal(same["Z"][i], one["Z"][0]) and np.array_equal(same["sv"][i], one["sv"][0])
        assert np.array_equal(same["W"][:, i], one["W"][:, 0])


# one shape per back-transform form: staged (RPT <= 8), global with the reflector in registers (RPT <= 16), global re-reading it (RPT > 16)
@pytest.mark.parametrize("name", ["p0_K2_31x25", "p0_K2_256x25", "p0_K2_417x25", "p0_K2_769x8", "p0_K2_4096x8"])
def test_phases_split_equals_joined(name):
    case = R.CASE[name]
    X, Hq = R.case_inputs(case)
    kw = dict(Xd=pack([X], case["ldS"]), Hq=Hq[:, None, :])
    joined = run_factor(case["S"], case["C"], case["ldS"], phases=3, **kw)
    split = run_factor(case["S"], case["C"], case["ldS"], phases=12, **kw)
    for key in ("Z", "sv", "W", "N", "R2", "tau", "sweeps"):
        assert np.array_equal(joined[key], split[key]), key
    assert np.all(is_sentinel(split["pad"]))


@pytest.mark.parametrize("name", ["p0_K1_129x8", "p0_K2_129x8", "p0_K1_769x8", "p0_K2_4096x8"])
def test_hq_conj_forms(name):
    """W from Hq (hq_conj = 0) and from conj(Hq) flagged as such (hq_conj = 1): the same rows, both against the truth"""
    case = R.CASE[name]
    tr = R.load_truth()[name]
    X, Hq = R.case_inputs(case)
    failures = []
    for flag, H in ((0, Hq), (1, np.conj(Hq))):
        out = run_factor(case["S"], case["C"], case["ldS"], Xd=pack([X], case["ldS"]), Hq=H[:, None, :], hq_conj=flag)
        judge(case, tr, X, out["sv"][0], out["Z"][0], out["W"][:, 0, :], "hq_conj=%d" % flag, failures)
    assert not failures, failures


def test_ls_end_limits_the_rows():
    """W is formed for the bins below ls_end only: the others keep the sentinel"""
    case = R.CASE["p0_K1_129x8"]
    X, Hq = R.case_inputs(case)
    out = run_factor(case["S"], case["C"], case["ldS"], nbins=3, Xd=pack([X], case["ldS"]), xd_stride=0, Hq=np.stack([Hq] * 3, axis=1), ls_end=2)
    assert not np.any(is_sentinel(out["W"][:, :2])) and np.all(is_sentinel(out["W"][:, 2]))


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_assembled_input(cplx):
    """B_k = sum_n b_n(k) T_n assembled by the kernel: T_n of small integers and b_n of small dyadic numbers, so that every B_k is exact in
    FP64 whatever the order of the sum; every entry the start-order rule must skip ((n+1)^2 <= s) is NaN; bins 2, 3 and 4 of P = 5, the
    last one the Nyquist bin (real part of b_n).  The truth of each B_k is computed here (36 x 7: 0.1 s per bin)."""
    nO, Cn, P, kb0, nb = 6, 7, 5, 2, 3
    S, ldS = nO * nO, 64
    t = R.ints(4242 + cplx, 2 * nO * Cn * S, -8, 8).astype(np.float64).reshape(2, nO, Cn, S)
    T = t[0] + 1j * t[1] if cplx else t[0]
    b = R.ints(77, 2 * P * nO, -16, 16).astype(np.float64).reshape(2, P, nO) / 8.0
    bn = b[0] + 1j * b[1]
    bn[:, 0] += 4.0
    Tn = np.full((nO, Cn, ldS), np.nan, dtype=T.dtype)
    s = np.arange(S)
    for n in range(nO):
        live = (n + 1) ** 2 > s
        Tn[n][:, :S][:, live] = T[n][:, live]
    Hq = R.ints(99, 4 * S, -4, 4).astype(np.float64)
    Hq = (Hq[:2 * S] + 1j * Hq[2 * S:]).reshape(2, S)
    out = run_factor(S, Cn, ldS, nbins=nb, Tn=Tn, bn=bn, kb0=kb0, P=P, Hq=np.stack([Hq] * nb, axis=1))
    rows = np.array([0, 1, 3, 4, 8, 9, 24, 25, 31, 32, 34, 35])
    failures = []
    for i in range(nb):
        kb = kb0 + i
        coef = bn[kb].real if kb == P - 1 else bn[kb]
        X = np.zeros((S, Cn), dtype=np.complex128)
        for n in range(nO):
            X += coef[n] * np.where(((n + 1) ** 2 > s)[:, None], T[n].T, 0.0)   # (exact: small integers times eighths)
        tr = R.truth_of(X, Hq, 0, R.REG_C, 0.0, rows)
        sv, Z, W = R.lapack_route(X, Hq, 0, R.REG_C, 0.0)
        tr["zmax"] = np.abs(Z).max()
        lm = R.measures(tr, X, sv, Z, W)
        tr["lapack"] = np.array([lm[k] for k in KEYS])
        case = dict(name="assembled_%s_36x7" % ("complex" if cplx else "real"), C=Cn, cls="K1")
        judge(case, tr, X, out["sv"][i], out["Z"][i], out["W"][:, kb, :], "bin %d of P=%d" % (kb, P), failures)
    assert not failures, failures
    assert np.all(is_sentinel(out["pad"])) and np.all(is_sentinel(out["W"][:, :kb0]))


def test_refusals():
    """what the launchers refuse, by their own messages"""
    from emagls_amd import _lib as L
    one = lambda S, Cn: np.ones((1, Cn, 64 * ((S + 63) // 64)), dtype=np.complex128)   # noqa: E731
    msg = run_factor(769, 9, 832, Xd=one(769, 9), expect=L.ERR_UNSUPPORTED)
    assert "problem shape (rows x channels) not supported" in msg
    msg = run_factor(3, 5, 64, Xd=one(3, 5), expect=L.ERR_UNSUPPORTED)
    assert "fewer rows than channels" in msg
    msg = run_factor(40, 33, 64, Xd=one(40, 33), expect=L.ERR_UNSUPPORTED)
    assert "more than 32 output channels" in msg
    msg = run_factor(30, 33, 64, Xd=one(30, 33), path=1, expect=L.ERR_UNSUPPORTED)
    assert "rank-deficient array model" in msg
    msg = run_factor(40, 33, 64, Xd=one(40, 33), path=2, expect=L.ERR_ARG)
    assert "the tiled path takes" in msg
    msg = run_factor(64, 4, 16448, Xd=np.ones((1, 4, 64), dtype=np.complex128), path=2, expect=L.ERR_ARG)   # (refused before anything is read)
    assert "the tiled path takes" in msg
    msg = run_factor(16, 4, 64, Tn=np.zeros((97, 4, 64)), bn=np.zeros((1, 97), dtype=np.complex128), expect=L.ERR_UNSUPPORTED)
    assert "simulation order above 95" in msg


# ------------------------------------------------------------------------------------------------ the Gram form
def run_gram(A, route, jrun, cond_limit):
    from emagls_amd import _lib as L
    nb, Cn = A.shape[0], A.shape[1]
    A = np.ascontiguousarray(A, dtype=np.complex128)
    route = np.ascontiguousarray(route, dtype=np.int32)
    M = np.zeros_like(A)
    sv = np.zeros((nb, Cn))
    sweeps = np.zeros(nb, dtype=np.int32)
    status = np.zeros(4, dtype=np.int32)
    checked(L.load().emagls_debug_factor_gram(ptr(A), nb, Cn, ptr(route), jrun, R.REG_C, cond_limit, ptr(M), ptr(sv), ptr(sweeps), ptr(status)))
    return M, sv, sweeps, status


@pytest.mark.parametrize("name", [c["name"] for c in R.GRAM_CASES])
def test_gram_chain(name):
    """eleven slowly varying A_k with one abrupt change, bin 5 skipped (route 2), runs of 1, 2 and 3 bins per workgroup (warm starts; 11 is a
    multiple of neither), one bin's conditioning just above cond_limit: M and the singular values of every bin against the truth, the
    skipped bin untouched, the status words, and the run lengths against each other"""
    case = R.GRAM_CASE[name]
    tr = R.load_truth()[name]
    A = R.gram_chain(case)
    assert R.checksum(A) == tr["sum"][0]
    route = np.ones(R.GRAM_BINS, dtype=np.int32)
    route[R.GRAM_SKIP] = 2
    Cn, floor = case["C"], case["C"] * R.EPS
    # LAPACK's error on the case is the largest over the bins the kernel factors.  Both measures of this form depend on the conditioning
    # (eigenvalues of A = B^H B: an absolute error of eps |A| is 1e-10 s_max on the smallest singular value of K2), all bins of a chain share
    # one spectrum, and what eigh realises of that level on a single bin is a draw: 2.9e-12 ... 1.2e-10 over the bins of g_K2_7, where the
    # kernel's 4.7e-11 on bin 2 is 16 x that bin's draw and 0.4 x the chain's.
    used = [k for k in range(R.GRAM_BINS) if k != R.GRAM_SKIP]
    ref_case = tr["lapack"][used].max(axis=0)
    results, failures = {}, []
    for jrun in (1, 2, 3):
        M, sv, sweeps, status = run_gram(A, route, jrun, float(tr["cond_limit"][0]))
        results[jrun] = M
        assert np.all(is_sentinel(M[R.GRAM_SKIP])) and sweeps[R.GRAM_SKIP] == -1
        assert status[2] == 1 and status[3] == R.GRAM_HIGH, status
        for k in range(R.GRAM_BINS):
            if k == R.GRAM_SKIP:
                continue
            assert 1 <= sweeps[k] <= 20, (k, sweeps)
            m = R.gram_measures(tr, k, sv[k], M[k])
            for i, key in enumerate(("A", "M")):
                ref = float(ref_case[i])
                REPORT.append((name, "jrun=%d bin %d" % (jrun, k), key, m[key], ref, floor, True))
                print("%-10s jrun %d bin %2d %s kernel %.3g  LAPACK (eigh) %.3g  ratio %.3g  sweeps %d" % (name, jrun, k, key, m[key], ref, m[key] / max(ref, floor), sweeps[k]))
                if not m[key] <= R.bound(ref, Cn):
                    failures.append("%s jrun %d bin %d %s: %.3g > 8 x max(%.3g, %.3g)" % (name, jrun, k, key, m[key], ref, floor))
    assert not failures, failures
    # the run lengths agree within the same bound (each is within it of the truth), and are not the same computation
    for k in range(R.GRAM_BINS):
        if k == R.GRAM_SKIP:
            continue
        scale = np.max(np.abs(tr["M"][0][k]))
        for j in (2, 3):
            d = np.max(np.abs(results[j][k] - results[1][k])) / scale
            assert d <= R.bound(float(ref_case[1]), Cn), (k, j, d)
    assert any(not np.array_equal(results[j], results[1]) for j in (2, 3))
