"""Host checks of the Gram-route reference (tests/gram_reference.py, tests/golden/gram_solve_truth.npz): the longdouble steps agree with exact
arithmetic on small cases written from the definition, a plain FP64 NumPy emulation of every step lies inside every bound, and what a subtly
wrong kernel would return lies outside.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import factor_reference as R
import gram_reference as G

F64 = {False: np.float64, True: np.complex128}


def frac(x):
    return Fraction(float(x))


def cfrac(z):
    return (frac(np.real(z)), frac(np.imag(z)))


def cmul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def cconj(a):
    return (a[0], -a[1])


# ------------------------------------------------------------------------------------------------ layouts
def test_layouts():
    X = G.rand(1, (2, 7, 7), True)
    X = X + np.conj(np.swapaxes(X, -1, -2))
    P = G.pack_herm(X)
    assert P.shape == (2, 49) and P.dtype == np.float64
    assert P[0][2 * 7 + 5] == X[0, 2, 5].real and P[0][5 * 7 + 2] == X[0, 2, 5].imag and P[0][3 * 7 + 3] == X[0, 3, 3].real
    assert np.array_equal(G.unpack_herm(P, 7), X)
    for nOrd in (1, 2, 5, 20):
        rows = []
        for n, n2 in G.all_pairs(nOrd):
            r = G.kmat_row(n, n2, nOrd)
            rows += [r] if n == n2 else [r, r + 1]
        assert sorted(rows) == list(range(nOrd * nOrd))
    assert [G.kmat_row(0, 1, 4), G.kmat_row(0, 3, 4), G.kmat_row(1, 2, 4), G.kmat_row(2, 3, 4)] == [4, 8, 10, 14]
    bn = np.array([[1 + 2j, 3 - 1j], [2 + 1j, -1 + 4j]])
    assert np.array_equal(G.coef_b(bn, 1, 2), [2, -1]) and np.array_equal(G.coef_b(bn, 0, 2), bn[0]) and np.array_equal(G.coef_b(bn, 1, 3), bn[1])


# ------------------------------------------------------------------------------------------------ the reference against exact arithmetic
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_composed_reference_is_the_definition(cplx):
    """A_k[c][c'] = sum_{s,j} conj(E[c][s] b_n(s)) Gy(s, j) b_n(j) E[c'][j] in exact rationals, bins 1 and 2 = Nyquist: the longdouble chain
    with its layouts, unpacked, is that matrix to 2^-58 of sum |terms|"""
    C, nOrd, P = 3, 3, 3
    S = nOrd * nOrd
    Gy = G.rand(11 + cplx, (S, S), cplx)
    if cplx:
        Gy[np.arange(S), np.arange(S)] = Gy[np.arange(S), np.arange(S)].real
    full = np.triu(Gy) + np.conj(np.triu(Gy, 1)).T
    Gy[np.tril_indices(S, -1)] = np.nan
    E = G.rand(13 + cplx, (C, S), cplx)
    bn = G.rand(17, (P, nOrd), True)
    out = G.composed(Gy, E, bn, C, nOrd, P, 1, 2, cplx)
    A = G.unpack_herm(G.f64(out["Apk"]), C)
    order = [int(np.sqrt(s)) for s in range(S)]
    for bi, kb in enumerate((1, 2)):
        b = bn[kb].real + 0j if kb == P - 1 else bn[kb]
        for c in range(C):
            for c2 in range(C):
                acc, mag = (Fraction(0), Fraction(0)), 0.0
                for s in range(S):
                    left = cconj(cmul(cfrac(E[c, s]), cfrac(b[order[s]])))
                    for j in range(S):
                        t = cmul(cmul(left, cfrac(full[s, j])), cmul(cfrac(b[order[j]]), cfrac(E[c2, j])))
                        acc = (acc[0] + t[0], acc[1] + t[1])
                        mag += abs(E[c, s] * b[order[s]] * full[s, j] * b[order[j]] * E[c2, j])
                got = A[bi, c, c2]
                assert abs(Fraction(got.real) - acc[0]) <= Fraction(mag * 2.0 ** -50) and abs(Fraction(got.imag) - acc[1]) <= Fraction(mag * 2.0 ** -50), (kb, c, c2)
                d = out["Apk"][bi][c * C + c2] - (G.LD(float(acc[0])) + G.LD(float(acc[0] - Fraction(float(acc[0])))))
                if c <= c2:
                    assert abs(d) <= mag * 2.0 ** -58, (kb, c, c2, float(d))
    assert np.all(G.f64(out["dA"]) > 0)


def test_gram_references_against_exact_integers():
    """ref_gram in longdouble is the exact Gram matrix (exact_gram, rounded once) to 2^-62 of sum |a| |b|; ref_from_g is that by construction"""
    for cplx in (False, True):
        Y = G.rand(23 + cplx, (37, 9), cplx) + 0j
        Gr, Bd = G.ref_gram(Y if cplx else Y.real, 9, cplx)
        Ar, Ai, e = R.exact_gram(np.ascontiguousarray(Y))
        for a in range(9):
            for b in range(9):
                want = complex(R._ratio(int(Ar[a, b]), e), R._ratio(int(Ai[a, b]), e))
                assert abs(complex(Gr[a, b]) - want) <= 2.0 ** -51 * abs(want) + 2.0 ** -62 * Bd[a, b] / G.gamma(1), (cplx, a, b)
    Gm = G.from_g_input(9, 63)
    ref, Bd = G.ref_from_g(Gm, 63)
    A = G.unpack_herm(ref, 9)
    X = Gm[1, :, :63].T
    assert np.abs(A[0] - X.conj().T @ X).max() < 1e-13 * np.abs(A[0]).max() and np.all(Bd > 0)


# ------------------------------------------------------------------------------------------------ the FP64 emulation inside every bound
@pytest.mark.parametrize("k", [1, 3, 5])
def test_fp64_gram_inside_bound(k):
    c = G.GRAM_CASES[k]
    Y = G.gram_input(k)
    ref, Bd = G.ref_gram(Y, c["S"], c["cplx"])
    got = Y[:, :c["S"]].conj().T @ Y[:, :c["S"]]
    w = G.worst(G.err(got, ref), Bd)
    print("gram case %d (%s): FP64 NumPy error / bound %.3g" % (k, G.gram_kernel(c), w))
    assert w <= 1.0
    assert G.worst(G.err(got * (1 + 2.0 ** -40), ref), Bd) > 1.0     # (a relative error of 1e-12 is outside)


def emulate_steps(name, defect=None, pairs=None, case=None, inputs=None):
    """every step in plain FP64 on the FP64 output of the step before it, against the longdouble step on the same input; returns the largest
    error / bound per step.  A defect is planted into the FP64 side only."""
    c = case or G.ASM_CASES[name]
    Gy, E, bn = inputs or G.asm_input(name)
    C, nOrd, P, kb0, nb, cplx = c["C"], c["nOrd"], c["P"], c["kb0"], c["nbins"], c["cplx"]
    S = nOrd * nOrd
    dt = F64[cplx]
    F, _ = G.step_f(Gy, E[:, :S], C, nOrd, cplx, dt, defect, pairs)
    Fr, dF = G.step_f(Gy, E[:, :S], C, nOrd, cplx, pairs=pairs)
    written = ~np.isnan(G.f64(np.abs(Fr)))
    assert np.array_equal(written, ~np.isnan(np.abs(F)))
    out = {"F": G.worst(G.err(F[written], Fr[written]), dF[written])}
    Fg, _ = G.step_f(Gy, E[:, :S], C, nOrd, cplx, dt, None, pairs)        # (the next step starts from a sound F)
    K, _ = G.step_kmat(E[:, :S], Fg, C, nOrd, cplx, dt, defect, pairs)
    Kr, dK = G.step_kmat(E[:, :S], Fg, C, nOrd, cplx, pairs=pairs)
    out["Kmat"] = G.worst(G.err(K, Kr), dK)
    Cf, _ = G.step_cf(bn, nOrd, P, kb0, nb, np.float64, defect)
    Cfr, dCf = G.step_cf(bn, nOrd, P, kb0, nb)
    out["Cf"] = G.worst(G.err(Cf, Cfr), dCf)
    Kg, _ = G.step_kmat(E[:, :S], Fg, C, nOrd, cplx, dt, None, pairs)
    Cg, _ = G.step_cf(bn, nOrd, P, kb0, nb, np.float64)
    A, _ = G.step_gemm(Cg, Kg, nb, C, np.float64)
    Ar, dA = G.step_gemm(Cg, Kg, nb, C)
    out["GEMM"] = G.worst(G.err(A, Ar), dA)
    return out


@pytest.mark.parametrize("name", ["K1", "K2", "K3", "K4", "K5"])
def test_fp64_assembly_inside_every_bound(name):
    w = emulate_steps(name)
    print(name, " ".join("%s %.3g" % kv for kv in w.items()))
    assert all(v <= 1.0 for v in w.values()), w
    c = G.ASM_CASES[name]
    assert c["kb0"] <= c["P"] - 1 < c["kb0"] + c["nbins"]        # the Nyquist bin is inside the range


def test_fp64_k6_on_the_listed_pairs():
    """K6 (S = 4225) is referenced on the listed pairs only; its inputs here are cut to what those pairs read"""
    c = G.ASM_CASES["K6"]
    assert 16 * c["C"] * 2 * c["nOrd"] > 64 * 1024 >= 16 * c["C"] * 2 * (c["nOrd"] - 1)     # the first shape above 64 KiB of dynamic LDS
    assert len(G.K6_PAIRS) == 69 and all(n <= n2 < 65 for n, n2 in G.K6_PAIRS)
    # the same channel count and arithmetic at a small order, on a list of pairs of the same kinds
    small = dict(cplx=True, C=32, nOrd=5, P=6, kb0=1, nbins=5)
    Gy = G.rand(8060, (25, 25), True)
    Gy[np.tril_indices(25, -1)] = np.nan
    w = emulate_steps("K6", pairs=[(0, 0), (1, 1), (0, 1), (2, 3), (4, 4), (1, 4)], case=small,
                      inputs=(Gy, G.rand(8061, (32, 25), True), G.rand(8062, (6, 5), True)))
    assert all(v <= 1.0 for v in w.values()), w


def test_fp64_composed_inside_bound():
    for name in ("K2", "K3"):
        c = G.ASM_CASES[name]
        Gy, E, bn = G.asm_input(name)
        S = c["nOrd"] ** 2
        args = (Gy, E[:, :S], bn, c["C"], c["nOrd"], c["P"], c["kb0"], c["nbins"], c["cplx"])
        ref = G.composed(*args)
        got = G.composed(*args, dt=F64[c["cplx"]])
        w = G.worst(G.err(got["Apk"], ref["Apk"]), ref["dA"])
        print("%s composed: FP64 error / bound %.3g" % (name, w))
        assert w <= 1.0
        assert G.worst(G.err(got["Apk"] + 1e-9 * np.abs(got["Apk"]).max(), ref["Apk"]), ref["dA"]) > 1.0   # an error of 1e-9 in A_k is outside


def test_fp64_from_g_inside_bound():
    for C, D in G.FROM_G_SHAPES[:4]:
        Gm = G.from_g_input(C, D)
        ref, Bd = G.ref_from_g(Gm, D)
        X = np.swapaxes(Gm[1:, :, :D], 1, 2)
        got = G.pack_herm(np.conj(np.swapaxes(X, 1, 2)) @ X)
        assert G.worst(G.err(got, ref), Bd) <= 1.0, (C, D)
        assert np.all(np.isnan(Gm[:, :, D:]))


# ------------------------------------------------------------------------------------------------ planted defects
ASSEMBLY_DEFECTS = [("q_off_by_one", "K2", "Kmat"), ("rows_transposed", "K2", "Kmat"), ("rows_transposed", "K2", "Cf"), ("no_half", "K1", "Kmat"),
                    ("z_sign", "K2", "Kmat"), ("nyquist_imag", "K1", "Cf"), ("gy_lower_unconjugated", "K2", "F"), ("pad_row", "K3", "Kmat")]


@pytest.mark.parametrize("defect,name,step", ASSEMBLY_DEFECTS)
def test_planted_assembly_defect_is_outside(defect, name, step):
    """defects 1-4, 6-8 of the list: each leaves the step it belongs to outside its bound, and only a defect does"""
    clean, bad = emulate_steps(name), emulate_steps(name, defect)
    assert all(v <= 1.0 for v in clean.values())
    assert bad[step] > 1.0, (defect, bad)


def test_pad_row_reaches_the_product():
    """the zero rows of Kmat are part of the GEMM: a NaN there is a NaN in every A_k"""
    c = G.ASM_CASES["K3"]
    Gy, E, bn = G.asm_input("K3")
    out = G.composed(Gy, E[:, :81], bn, c["C"], c["nOrd"], c["P"], c["kb0"], c["nbins"], False, dt=np.float64)
    K = out["Kmat"].copy()
    assert K.shape[0] == 84 and np.all(K[81:] == 0)
    K[81:] = np.nan
    assert np.all(np.isnan(G.step_gemm(out["Cf"], K, c["nbins"], c["C"], np.float64)[0]))


# ------------------------------------------------------------------------------------------------ the direct inverse
def test_solve_fixture_is_current():
    T = G.load_solve_truth()
    for C in G.SOLVE_C:
        A, Apk = G.solve_input(C)
        assert Apk.shape == (11, G.round_up(C * C, 64)) and np.all(np.isnan(Apk[:, C * C:]))
        for b in range(G.SOLVE_NBINS):
            kind = G.SOLVE_BINS[b][0]
            if kind == "r":
                assert R.checksum(A[b]) == T[(C, b)]["sum"][0], (C, b)
                assert np.array_equal(A[b], A[b].conj().T)
            elif kind == "indef":
                assert np.linalg.eigvalsh(A[b]).min() < -0.2
            elif kind == "zero":
                assert not A[b].any()
            else:
                assert np.isnan(A[b]).sum() == 1 and np.isnan(A[b, C // 2, C // 2])
    # a small one recomputed: the stored hi + lo pairs to 1e-30, and M A = I in exact rationals to 1e-28
    tr = G.mp_truth(G.solve_matrix(4, 3)[0])[0]
    old = T[(4, 3)]
    for key in ("lam", "M"):
        d = (tr[key][0] - old[key][0]).astype(G.CLD) + (tr[key][1] - old[key][1])
        assert np.max(np.abs(d)) <= 1e-30 * np.max(np.abs(old[key][0])), key
    A = G.solve_matrix(4, 3)[0]
    for i in range(4):
        for j in range(4):
            acc = (Fraction(0), Fraction(0))
            for k in range(4):
                m = (frac(old["M"][0][i, k].real) + frac(old["M"][1][i, k].real), frac(old["M"][0][i, k].imag) + frac(old["M"][1][i, k].imag))
                t = cmul(m, cfrac(A[k, j]))
                acc = (acc[0] + t[0], acc[1] + t[1])
            assert abs(acc[0] - (1 if i == j else 0)) < Fraction(1, 10 ** 25) and abs(acc[1]) < Fraction(1, 10 ** 25)


def test_no_bin_near_the_threshold():
    """(||A||_F ||A^-1||_F)^2 against 1 / reg_c^4 in longdouble from the truth: no positive definite bin within 1e-6 relative, none left out;
    both sides of the threshold occur, and bins the certificate rejects although cond_2(A) <= 1e4"""
    seen = set()
    for C in G.SOLVE_C:
        for b in range(G.SOLVE_NBINS):
            if G.SOLVE_BINS[b][0] != "r":
                continue
            f = G.truth_facts(C, b)
            assert abs(f["rel"]) > 1e-6, (C, b, f)
            assert f["route"] == 1 or f["cond"] <= 1e4
            seen.add((f["route"], f["cond"] <= 1e4))
    assert seen == {(2, True), (1, True), (1, False)}
    assert G.predicted_routes(2) == [2, 1, 2, 2, 1, 1, 1, 1, 1, 2, 2] and G.predicted_routes(32)[9:] == [1, 1]


@pytest.mark.parametrize("C", G.SOLVE_C)
def test_fp64_gauss_jordan_passes(C):
    report = []
    for scale in (0, 100, -100):
        A, Apk = G.solve_input(C, scale)
        out = G.gauss_jordan(Apk, C, G.SOLVE_KB0)
        assert G.check_solve(C, Apk, out, scale=scale, report=report if scale == 0 else None) == []
    print("C %d: largest error / level %.3g" % (C, max(r[-1] for r in report)))


@pytest.mark.parametrize("defect", ["no_conj_lower", "pivot_single", "two_norm", "sv_swapped"])
def test_planted_solve_defect_fails(defect):
    """defects 5, 9, 10, 11 of the list"""
    C = 9
    A, Apk = G.solve_input(C)
    assert G.check_solve(C, Apk, G.gauss_jordan(Apk, C, G.SOLVE_KB0)) == []
    fails = G.check_solve(C, Apk, G.gauss_jordan(Apk, C, G.SOLVE_KB0, defect=defect))
    assert fails, defect
    if defect == "two_norm":
        assert any("bin 9: route 2, predicted 1" in f for f in fails), fails
