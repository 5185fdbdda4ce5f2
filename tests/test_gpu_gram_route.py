"""The Gram route from conj(Y) to the direct inverse -- launch_gram (csrc/gram_chol.hip), launch_gram_kmat and launch_gram_gemm, launch_gram_solve
(csrc/gramroute.hip), launch_gram_from_g (csrc/emash.hip) -- run by the debug entries of csrc/gram_debug.hip on the inputs of
tests/gram_reference.py and held, step by step, to the a-priori bounds derived there: every step against a longdouble sum on the device
output of the step before it, the assembled A_k once more against the composed bound, the direct inverse against the multiprecision truth
of tests/golden/gram_solve_truth.npz within 8 x its level, and the bins it rejects through the Jacobi kernel as test_gpu_factor_chain.py
holds them.  Every case prints its largest error / bound; with EMAGLS_GRAM_ROUTE_REPORT=<file> the module writes them there
(profiles/r24_gram_route.md is such a file).  What a kernel must leave alone keeps the sentinel.
"""
import os

import numpy as np
import pytest

import factor_reference as R
import gram_reference as G

pytestmark = pytest.mark.gpu

REPORT = []     # (group, case, what, value)


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    path = os.environ.get("EMAGLS_GRAM_ROUTE_REPORT")
    if not path or not REPORT:
        return
    with open(path, "w") as f:
        f.write("| group | case | measure | value |\n|---|---|---|---|\n")
        for row in REPORT:
            f.write("| %s | %s | %s | %s |\n" % row)


def note(group, case, what, value):
    text = value if isinstance(value, str) else "%.3g" % value
    REPORT.append((group, case, what, text))
    print("%-10s %-14s %-34s %s" % (group, case, what, text))


def ptr(a):
    return a.ctypes.data if a is not None else None


def checked(rc):
    """A launch the runtime refuses (reported by the launch itself) fails the test; any other HIP error ends the session: nothing more is
    started on a device that has faulted."""
    from emagls_amd import _lib as L
    if rc == L.ERR_HIP:
        msg = L.load().emagls_last_error().decode()
        if "in kernel launch" not in msg:
            pytest.exit("HIP error in a debug entry: %s" % msg, returncode=3)
    L.check(rc)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_sentinel_is_the_library_s():
    from emagls_amd import _lib as L
    assert G.SENTINEL_BITS == L.DEBUG_SENTINEL_BITS


# ------------------------------------------------------------------------------------------------ launch_gram
@pytest.mark.parametrize("k", sorted(G.GRAM_CASES))
def test_gram(k):
    from emagls_amd import _lib as L
    c = G.GRAM_CASES[k]
    S, D, Sh, cplx = c["S"], c["D"], c["Sh"], c["cplx"]
    Y = G.gram_input(k)
    Gd, Rd = np.zeros((S, S), dtype=Y.dtype), np.zeros((Sh, Sh), dtype=Y.dtype)
    checked(L.load().emagls_debug_gram(ptr(Y), D, S, Y.shape[1], int(cplx), Sh, ptr(Gd), ptr(Rd)))
    ref, Bd = G.ref_gram(Y, S, cplx)
    iu = np.triu_indices(S)
    w = G.worst(G.err(Gd[iu], ref[iu]), Bd[iu])
    note("gram", "case %d" % k, "kernel", G.gram_kernel(c))
    note("gram", "case %d" % k, "largest error / bound", w)
    assert w <= 1.0
    assert same_bits(Rd, Gd[:Sh, :Sh]), "R is not the leading block of G bit for bit"
    blk = np.arange(S) >> 6
    assert np.all(Gd[blk[:, None] > blk[None, :]] == 0), "below the block triangle: not the zeros the kernels write"
    assert not np.any(G.is_sentinel(Gd)) and not np.any(G.is_sentinel(Rd))


# ------------------------------------------------------------------------------------------------ launch_gram_kmat + launch_gram_gemm
def run_assemble(c, Gy, E, bn, Kmat_in=None, want_F=True):
    from emagls_amd import _lib as L
    C, nOrd, P, kb0, nb, cplx = c["C"], c["nOrd"], c["P"], c["kb0"], c["nbins"], c["cplx"]
    Kp, ldK, ldC = G.round_up(nOrd * nOrd, 4), G.round_up(C * C, 64), G.round_up(P, 64)
    ldE = E.shape[1] if E is not None else 0
    F = np.zeros((nOrd, C, ldE), dtype=E.dtype) if (want_F and E is not None) else None
    Kmat, Cf, Apk = np.zeros((Kp, ldK)), np.zeros((Kp, ldC)), np.zeros((nb, ldK))
    bn = np.ascontiguousarray(bn, dtype=np.complex128)
    checked(L.load().emagls_debug_gram_assemble(ptr(Gy), ptr(E), ldE, ptr(bn), C, nOrd, P, kb0, nb, int(cplx), ptr(Kmat_in), ptr(F), ptr(Kmat), ptr(Cf), ptr(Apk)))
    return dict(F=F, Kmat=Kmat, Cf=Cf, Apk=Apk)


def check_assembled(name, c, E, bn, out, pairs=None):
    """Kmat from the device F, Cf from b_n, Apk from the device Kmat and Cf: each against its longdouble step; the paddings"""
    C, nOrd, P, kb0, nb, cplx = c["C"], c["nOrd"], c["P"], c["kb0"], c["nbins"], c["cplx"]
    S, C2, Kp = nOrd * nOrd, C * C, G.round_up(nOrd * nOrd, 4)
    F = out["F"][:, :, :S]
    Kr, dK = G.step_kmat(E[:, :S], F, C, nOrd, cplx, pairs=pairs)
    rows = np.arange(Kp) if pairs is None else np.array(sorted({G.kmat_row(n, n2, nOrd) + t for n, n2 in pairs for t in ((0,) if n == n2 else (0, 1))}))
    wK = G.worst(G.err(out["Kmat"][rows, :C2], Kr[rows]), dK[rows])
    note("assemble", name, "K and its fold, error / bound", wK)
    assert wK <= 1.0
    assert np.all(out["Kmat"][S:] == 0) and np.all(out["Kmat"][:, C2:] == 0), "the padding of Kmat is not zero"
    Cr, dC = G.step_cf(bn, nOrd, P, kb0, nb)
    wC = G.worst(G.err(out["Cf"][:, :nb], Cr), dC)
    note("assemble", name, "Cf, error / bound", wC)
    assert wC <= 1.0
    assert np.all(out["Cf"][S:] == 0) and np.all(out["Cf"][:, nb:] == 0), "the padding of Cf is not zero"
    Ar, dA = G.step_gemm(out["Cf"], out["Kmat"], nb, C)
    wA = G.worst(G.err(out["Apk"][:, :C2], Ar), dA)
    note("assemble", name, "GEMM, error / bound", wA)
    assert wA <= 1.0
    assert np.all(np.isfinite(out["Apk"][:, :C2])) and np.all(G.is_sentinel(out["Apk"][:, C2:])), "Apk: not finite, or its padding was written"
    note("assemble", name, "checksum of Apk", "%016x" % R.checksum(out["Apk"][:, :C2]))


@pytest.mark.parametrize("name", ["K1", "K2", "K3", "K4", "K5"])
def test_assemble(name):
    c = G.ASM_CASES[name]
    C, nOrd, cplx = c["C"], c["nOrd"], c["cplx"]
    S = nOrd * nOrd
    Gy, E, bn = G.asm_input(name)
    out = run_assemble(c, Gy, E, bn)
    Fr, dF = G.step_f(Gy, E[:, :S], C, nOrd, cplx)
    written = ~np.isnan(G.f64(np.abs(Fr)))
    F = out["F"][:, :, :S]
    wF = G.worst(G.err(F[written], Fr[written]), dF[written])
    note("assemble", name, "F, error / bound", wF)
    assert wF <= 1.0
    assert np.all(G.is_sentinel(F[~written])) and np.all(G.is_sentinel(out["F"][:, :, S:])), "F written outside s < (n + 1)^2"
    check_assembled(name, c, E, bn, out)
    ref = G.composed(Gy, E[:, :S], bn, C, nOrd, c["P"], c["kb0"], c["nbins"], cplx)
    wE = G.worst(G.err(out["Apk"][:, :C * C], ref["Apk"]), ref["dA"])
    note("assemble", name, "end to end, error / composed bound", wE)
    assert wE <= 1.0


def test_assemble_above_64_kib_of_lds():
    """K6: complex, C = 32, nOrd = 65 -- gy_times_e_kernel asks for 66560 bytes of dynamic LDS.  F and Kmat on the listed pairs, Cf and
    the product in full from the device Kmat."""
    c = G.ASM_CASES["K6"]
    C, nOrd = c["C"], c["nOrd"]
    S = nOrd * nOrd
    Gy, E, bn = G.asm_input("K6")
    note("assemble", "K6", "dynamic LDS of gy_times_e_kernel", "%d bytes" % (16 * C * 2 * nOrd))
    out = run_assemble(c, Gy, E, bn)
    F = out["F"][:, :, :S]
    wF = 0.0
    for n, n2 in G.K6_PAIRS:
        sb, se = G.block(n)
        Fr, dF = G.f_block(Gy, E[:, :S], n, n2, True)
        wF = max(wF, G.worst(G.err(F[n2][:, sb:se], Fr), dF))
    note("assemble", "K6", "F on the listed pairs, error / bound", wF)
    assert wF <= 1.0
    live = np.arange(S)[None, :] < ((np.arange(nOrd) + 1) ** 2)[:, None]           # [n][s]: what gy_times_e_kernel writes
    Ft = F.transpose(0, 2, 1)
    assert np.all(G.is_sentinel(Ft[~live])) and not np.any(G.is_sentinel(Ft[live])), "F written outside s < (n + 1)^2, or not inside"
    check_assembled("K6", c, E, bn, out, pairs=G.K6_PAIRS)
    assert np.all(np.isfinite(out["Kmat"]))


def test_gemm_reads_the_pad_rows_of_kmat():
    """the GEMM-only mode on a Kmat whose pad rows (81 ... 83 at nOrd = 9) are NaN: every A_k is NaN.  The zero fill of those rows is a
    contract of the plan's allocation, not an accident; with zeros there the same call returns the product."""
    c = G.ASM_CASES["K3"]
    C, nOrd = c["C"], c["nOrd"]
    Gy, E, bn = G.asm_input("K3")
    K = G.f64(G.composed(Gy, E[:, :81], bn, C, nOrd, c["P"], c["kb0"], c["nbins"], False)["Kmat"])
    Kin = np.zeros((84, G.round_up(C * C, 64)))
    Kin[:, :C * C] = K
    good = run_assemble(c, None, None, bn, Kmat_in=Kin)
    Ar, dA = G.step_gemm(good["Cf"], Kin, c["nbins"], C)
    assert G.worst(G.err(good["Apk"][:, :C * C], Ar), dA) <= 1.0 and same_bits(good["Kmat"], Kin)
    Kin[81:] = np.nan
    bad = run_assemble(c, None, None, bn, Kmat_in=Kin)
    assert np.all(np.isnan(bad["Apk"][:, :C * C])) and not np.any(G.is_sentinel(bad["Apk"][:, :C * C]))


def test_plan_apk_from_its_own_gy(grids, hrirs):
    """a real-basis eMagLS plan with an odd number of orders (radius 4 cm: simulation order 18, nOrd = 19, 361 -> 364 rows of K), thinned
    grid, 128 taps: Apk of the plan rebuilt from the plan's own Gy, E and b_n within the composed bound -- the plan's allocation of Kmat
    and Cf (zero padding) is part of what is checked"""
    from emagls_amd import Plan, _lib as L
    sub = slice(0, 2702, 3)
    hL, hR = np.ascontiguousarray(hrirs[0][:, sub]), np.ascontiguousarray(hrirs[1][:, sub])
    p = Plan(L.KIND_EMAGLS, "real", 4, 48000.0, 128, hL.shape[0], hL.shape[1], 0.04, 32)
    try:
        p.set_hrir_grid(grids["azi"][sub], grids["zen"][sub])
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
        p.set_hrirs(hL, hR)
        p.set_profiling(1)
        p.execute()
        p.synchronize()
        i = p.info()
        S, C, P, nOrd = i.num_sh_sim, i.num_channels, i.num_pos_freqs, i.sim_order + 1
        assert (i.sim_order, S, C, P) == (18, 361, 25, 129) and 1 <= i.gram_from < P
        ldS, ldK = G.round_up(S, 64), G.round_up(C * C, 64)
        Gy = p.debug("Gy", np.float64, (S, S))
        E = p.debug("E", np.float64, (C, ldS))[:, :S]
        bn = p.debug("bn", np.complex128, (P, nOrd))
        Apk = p.debug("Apk", np.float64).reshape(P, ldK)
        Kmat = p.debug("Kmat", np.float64).reshape(-1, ldK)
        gf, nb = i.gram_from, P - i.gram_from
    finally:
        p.close()
    assert Kmat.shape[0] == 364 and np.all(Kmat[361:] == 0)
    ref = G.composed(Gy, E, bn, C, nOrd, P, gf, nb, False)
    w = G.worst(G.err(Apk[:nb, :C * C], ref["Apk"]), ref["dA"])
    note("plan", "real, nOrd 19", "Apk, error / composed bound", w)
    assert w <= 1.0


# ------------------------------------------------------------------------------------------------ launch_gram_from_g
@pytest.mark.parametrize("C,D", G.FROM_G_SHAPES)
def test_gram_from_g(C, D):
    from emagls_amd import _lib as L
    Gm = G.from_g_input(C, D)
    ldK = G.round_up(C * C, 64)
    Apk = np.zeros((G.FROM_G["nbins"], ldK))
    checked(L.load().emagls_debug_gram_from_g(ptr(Gm), D, C, Gm.shape[2], G.FROM_G["kb0"], G.FROM_G["g0"], G.FROM_G["nbins"], ptr(Apk)))
    ref, Bd = G.ref_from_g(Gm, D)
    w = G.worst(G.err(Apk[:, :C * C], ref), Bd)
    note("from_g", "C %d D %d" % (C, D), "largest error / bound", w)
    assert w <= 1.0
    assert np.all(G.is_sentinel(Apk[:, C * C:]))


# ------------------------------------------------------------------------------------------------ launch_gram_solve
def run_solve(Apk, C, kb0=G.SOLVE_KB0):
    from emagls_amd import _lib as L
    nb = Apk.shape[0]
    P = kb0 + nb
    Mw, R2w = np.zeros((P, C, C), dtype=np.complex128), np.zeros((P, C, C), dtype=np.complex128)
    sv, route, sweeps = np.zeros((P, C)), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    Apk = np.ascontiguousarray(Apk)
    checked(L.load().emagls_debug_gram_solve(ptr(Apk), Apk.shape[1], C, kb0, nb, G.REG_C, ptr(Mw), ptr(R2w), ptr(sv), ptr(route), ptr(sweeps)))
    return dict(Mw=Mw, R2w=R2w, sv=sv, route=route, sweeps=sweeps)


@pytest.mark.parametrize("C", G.SOLVE_C)
def test_gram_solve(C):
    from emagls_amd import _lib as L
    A, Apk = G.solve_input(C)
    out = run_solve(Apk, C)
    report = []
    fails = G.check_solve(C, Apk, out, report=report)
    for (_, b, cls, _, e, lv, ratio) in report:
        note("solve", "C %d bin %d" % (C, b), "s_max / s_min %s: error %.3g, level %.3g, ratio" % (cls, e, lv), ratio)
    note("solve", "C %d" % C, "routes", " ".join(str(r) for r in out["route"][G.SOLVE_KB0:]))
    assert not fails, fails
    # the NaN bin (1) shares its workgroup with bins 0, 2 and 3: with a finite matrix in its place they come out the same, bit for bit
    finite = Apk.copy()
    finite[1] = Apk[2]
    outf = run_solve(finite, C)
    assert outf["route"][G.SOLVE_KB0 + 1] == out["route"][G.SOLVE_KB0 + 2] and out["route"][G.SOLVE_KB0 + 1] == 1
    for b in (0, 2, 3):
        kb = G.SOLVE_KB0 + b
        assert outf["route"][kb] == out["route"][kb] and outf["sweeps"][kb] == out["sweeps"][kb], b
        assert same_bits(outf["Mw"][kb - 1], out["Mw"][kb - 1]) and same_bits(outf["R2w"][kb - 1], out["R2w"][kb - 1]) and same_bits(outf["sv"][kb], out["sv"][kb]), b
    # A 2^+-100: the same routes, M 2^-+100 bit for bit
    for scale in (100, -100):
        _, Apks = G.solve_input(C, scale)
        outs = run_solve(Apks, C)
        assert np.array_equal(outs["route"], out["route"]) and np.array_equal(outs["sweeps"], out["sweeps"]), scale
        direct = np.flatnonzero(out["route"] == 2)
        assert same_bits(outs["Mw"][direct - 1].view(np.float64) * 2.0 ** scale, out["Mw"][direct - 1]), scale    # (scaled as reals: the sign of a zero stays)
        assert G.check_solve(C, Apks, outs, scale=scale) == []
    # the chain: the positive definite bins the certificate rejected go on to the Jacobi kernel in its Gram form
    T = G.load_solve_truth()
    chain = [b for b in range(G.SOLVE_NBINS) if G.SOLVE_BINS[b][0] == "r" and out["route"][G.SOLVE_KB0 + b] == 1]
    if not chain:
        return
    Ain = np.zeros((G.SOLVE_NBINS, C, C), dtype=np.complex128)
    rt = np.full(G.SOLVE_NBINS, 2, dtype=np.int32)
    for b in chain:
        Ain[b], rt[b] = out["R2w"][G.SOLVE_KB0 + b - 1], 1
    M, sv = np.zeros_like(Ain), np.zeros((G.SOLVE_NBINS, C))
    sweeps, status = np.zeros(G.SOLVE_NBINS, dtype=np.int32), np.zeros(4, dtype=np.int32)
    checked(L.load().emagls_debug_factor_gram(ptr(Ain), G.SOLVE_NBINS, C, ptr(rt), 1, G.REG_C, 1e300, ptr(M), ptr(sv), ptr(sweeps), ptr(status)))
    fails = []
    for b in range(G.SOLVE_NBINS):
        if b not in chain:
            assert np.all(G.is_sentinel(M[b])) and sweeps[b] == -1
            continue
        e, lv = G.chain_error(M[b], T[(C, b)]), G.level(C, b, "lapack_eigh")
        note("chain", "C %d bin %d" % (C, b), "s_max / s_min %s: error %.3g, level %.3g, ratio" % (G.solve_class(b), e, lv), e / lv)
        if not (e <= G.MARGIN * lv and 1 <= sweeps[b] <= 20):
            fails.append("C %d bin %d: %.3g > 8 x %.3g, or %d sweeps" % (C, b, e, lv, sweeps[b]))
    assert not fails, fails
