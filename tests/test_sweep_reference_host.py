"""The longdouble steps of tests/sweep_reference.py against mpmath at 50 digits, and the host-made inputs of every case of
tests/test_gpu_sweep_operand_step.py against the a-priori bounds: an FP64 NumPy step stays within them, and the phase term -- loose
only where |p| is near its own rounding error -- stays tight: max dp / |p| < 2^-30 over all bins, ears and directions of a case."""
import numpy as np
import pytest

import sweep_reference as S
import synth_reference as R


def mp_of(mp, z):
    z = complex(z)
    return mp.mpc(z.real, z.imag)


def ld_minus_mp(mp, a_ld, b_mp):
    def mpf_of(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - R.LD(hi)))
    return float(abs(mp.mpc(mpf_of(a_ld.real), mpf_of(a_ld.imag)) - b_mp))


def mp_phase(mp, p, h, nyq):
    t = mp.mpf(h) * p / abs(p) if p != 0 else mp.mpc(h)
    return mp.mpc(t.real, 0) if nyq else t


@pytest.fixture(scope="module")
def small():
    R.require_longdouble()
    rng = np.random.default_rng(5)
    C, D = 5, 7
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    w = cn(2, C)
    X = cn(C, D)
    X[:, 3] = 0.0                       # p == 0 in one direction: t = |H|
    return dict(C=C, D=D, w=w, X=X, Xr=rng.standard_normal((C, D)), Z=cn(C, D), M=cn(C, C), habs=np.abs(rng.standard_normal((2, D))) + 0.1,
                Hc=cn(3, D))


@pytest.mark.parametrize("nyq", [False, True])
def test_steps_against_mpmath(small, nyq):
    """operand_step (complex and real operands), half_step (with M and with the accurate slab) and ls_rows agree with 50-digit
    arithmetic to 64 longdouble roundings of the sums of moduli."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    s = small
    C, D = s["C"], s["D"]
    tol = 64 * float(np.finfo(R.LD).eps)

    def mp_step(X, Z, M=None):
        out = []
        for e in range(2):
            p = [sum((mp_of(mp, s["w"][e, c]) * mp_of(mp, X[c, d]) for c in range(C)), mp.mpc(0)) for d in range(D)]
            t = [mp_phase(mp, p[d], float(s["habs"][e, d]), nyq) for d in range(D)]
            v = [sum((t[d] * mp_of(mp, Z[c, d]) for d in range(D)), mp.mpc(0)) for c in range(C)]
            if M is not None:
                v = [sum((v[j] * mp_of(mp, np.conj(M[j, c])) for j in range(C)), mp.mpc(0)) for c in range(C)]
            out.append(v)
        return out

    def worst(got, want, scale):
        return max(ld_minus_mp(mp, got[e, c], want[e][c]) for e in range(2) for c in range(C)) / scale

    scale = float(np.abs(s["habs"]).sum() * max(np.abs(s["Z"]).max(), np.abs(s["X"]).max()) * max(1.0, np.abs(s["M"]).sum()))
    for X in (s["X"], s["Xr"]):
        got, p, t = S.operand_step(s["w"], s["habs"], X, s["Z"], nyq)
        assert worst(got, mp_step(X, s["Z"]), scale) <= tol
        assert not nyq or np.all(t.imag == 0)
    got, p, t = S.operand_step(s["w"], s["habs"], s["X"], s["Z"], nyq)
    assert p[0, 3] == 0 and t[0, 3] == R.LD(s["habs"][0, 3])
    got, _, _, v = S.half_step(s["w"], s["habs"], s["X"], s["M"], None, nyq)
    assert worst(got, mp_step(s["X"], np.conj(s["X"]), s["M"]), scale) <= tol and v is not None
    got, _, _, v = S.half_step(s["w"], s["habs"], s["X"], None, s["Z"], nyq)
    assert worst(got, mp_step(s["X"], s["Z"]), scale) <= tol and v is None
    if not nyq:
        rows = S.ls_rows(s["Hc"], s["Z"])
        for r in range(3):
            for c in range(C):
                want = sum((mp_of(mp, s["Hc"][r, d]) * mp_of(mp, s["Z"][c, d]) for d in range(D)), mp.mpc(0))
                assert ld_minus_mp(mp, rows[r, c], want) <= tol * scale


def test_fp64_steps_are_the_same_algebra(small):
    """step64 is the longdouble step rounded: they agree to a few FP64 roundings of the sums of moduli"""
    s = small
    for nyq in (False, True):
        a = S.operand_step64(s["w"], s["habs"], s["X"], s["Z"], nyq)
        b = S.operand_step(s["w"], s["habs"], s["X"], s["Z"], nyq)[0]
        assert S.row_errors(a, b).max() <= 64 * R.EPS64 * np.abs(a).max()
        a = S.half_step64(s["w"], s["habs"], s["X"], s["M"], None, nyq)
        b = S.half_step(s["w"], s["habs"], s["X"], s["M"], None, nyq)[0]
        assert S.row_errors(a, b).max() <= 64 * R.EPS64 * max(np.abs(a).max(), 1.0) * s["C"]


def test_cases_reach_their_branches():
    """the shapes of the case table against the kernels' constants: staged partial sums, slabs per workgroup, lane tails, slab heights"""
    c = S.CASE
    assert [S.wide_nwg(c[f"wide-real-{D}"]["D"]) for D in (3072, 3073, 3135, 3137)] == [48, 49, 49, 50]      # NG = 24: 2 x 24 staged
    assert [S.wide_nwg(c[f"wide-complex-{D}"]["D"]) for D in (1536, 1537, 1599)] == [24, 25, 25]             # NG = 12
    assert [S.wide_nwg(D) % 2 for D in (191, 193, 255, 257)] == [1, 0, 0, 1] and [D % 64 for D in (191, 193, 255, 257)] == [63, 1, 63, 1]
    assert [S.dense_nwg(D, 25)[0] for D in (63, 65, 255, 257, 511, 513)] == [1, 2, 4, 5, 8, 9]
    assert S.dense_nwg(5184, 25) == (81, 1) and S.dense_nwg(5185, 25) == (41, 2) and S.dense_nwg(5249, 25) == (42, 2)
    assert [S.persist_dpw(D) for D in (2048, 2049, 3072)] == [64, 96, 96] and -(-3072 // 96) == 32 and -(-2048 // 64) == 32
    for k in c.values():
        n = S.length_of(k)
        P, kcut0, k0 = S.bins_of(n, S.cut_of(k["kind"], k["order"], 2000.0))
        assert P - k0 >= 8 and (k["kind"] != "magls" or kcut0 >= 2), k["name"]
    assert len({k["name"] for k in S.CASES}) == len(S.CASES)


@pytest.mark.parametrize("name", [k["name"] for k in S.CASES])
def test_host_inputs_within_the_bounds(name):
    """On host-made operands of the case's shape an FP64 NumPy step stays within the a-priori bound in every element of every swept
    bin, and dp / |p| stays below 2^-30."""
    R.require_longdouble()
    c = S.CASE[name]
    worst = r_max = 0.0
    nbins = flagged = 0
    for item in S.host_chain(c):
        if item[0] == "operand":
            _, w, habs, X, Z, nyq = item
            step = S.operand_step(w, habs, X, Z, nyq)
            bound, r = S.bound_operand(w, habs, X, Z, step[1])
            w64 = S.operand_step64(w, habs, X, Z, nyq)
        else:
            _, w, habs, G, M, yri, nyq = item
            step = S.half_step(w, habs, G, M, yri, nyq)
            bound, r = S.bound_half(w, habs, G, M, step[1], step[3], yri)
            w64 = S.half_step64(w, habs, G, M, yri, nyq)
            flagged += yri is not None
        assert np.all(bound > 0)
        worst = max(worst, float(S.step_ratio(w64, step[0], bound).max()))
        assert nyq or np.abs(w64.imag).max() > 0          # (a chain that stayed real would not exercise the Nyquist rule)
        r_max = max(r_max, float(r.max()))
        nbins += 1
    print(f"{name}: {nbins} swept bins ({flagged} on the accurate slab), FP64 step error / bound {worst:.3e}, max dp / |p| {r_max:.3e}")
    assert nbins >= 8
    assert worst <= 1.0
    assert r_max < S.R_LIMIT
    if c["note"] == "cond_ok":
        assert flagged >= 1
