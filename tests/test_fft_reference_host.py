"""The longdouble reference of the HRIR prologue, the ATF spectra and the filter epilogue (tests/fft_reference.py) on the host:
against mpmath at 50 digits on small shapes; the float64 oracle against the a-priori bounds on every shape of the GPU test list (the
bounds are attainable); float64 implementations with ONE planted defect against the same bounds (the bounds are not vacuous); and
the share of group-delay bins the bound leaves out next to the 10 eps branch."""
import numpy as np
import pytest

import fft_reference as R
from oracle import emagls_oracle as O

LD = R.LD


@pytest.fixture(scope="module")
def mp():
    R.require_longdouble()
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    return mpmath.mp


def mpf_of(mp, v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def ld_minus_mp(mp, a, b):
    """|a - b| with a in (c)longdouble (split into doubles, exact) and b in mpmath"""
    a = np.asarray(a).reshape(())[()]
    return float(abs(mp.mpc(mpf_of(mp, a.real), mpf_of(mp, a.imag)) - b))


# ---- against mpmath ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nfft", [6, 8, 64, 74, 600])
def test_circle_against_mpmath(mp, nfft):
    """every root of unity of the table within one longdouble eps"""
    c = R.circle(nfft)
    worst = max(ld_minus_mp(mp, c[j], mp.exp(2j * mp.pi * j / nfft)) for j in range(nfft))
    print(f"nfft {nfft}: table vs 50 digits = {worst / R.EPS_LD:.2f} eps_ld")
    assert worst <= R.EPS_LD
    tw, tb = R.twiddle_ref(nfft)
    assert np.array_equal(tw, np.conj(c)) and tb[0] == 0 and tb[nfft // 2] == 0 and tb.max() <= R.tw_max(nfft)


def mp_epilogue(mp, W, nfft, length, grpd, conj_mode, dc_rule, shift_mode, fade_rel, e, c):
    """channel c of ear e in mpmath: the formulas of fft.hip's header comment, term by term"""
    P, C = W.shape[1], W.shape[2]
    w = lambda k, ch: mp.mpc(float(W[e, k, ch].real), float(W[e, k, ch].imag))   # noqa: E731
    if conj_mode == 1:
        n = int(np.floor(np.sqrt(c)))
        m = c - n * n - n
        part, sg = n * n + n - m, (-1) ** m
    elif conj_mode == 2:
        order = [0] + [s * q for q in range(1, C // 2 + 1) for s in (-1, 1)]      # [0, -1, +1, -2, +2, ...]
        part, sg = order.index(-order[c]), 1
    else:
        part, sg = c, 1
    delay = mp.mpf(nfft // 2) if e == 0 else mp.mpf(R.right_delay(nfft, grpd))
    full = []
    for k in range(nfft):
        kb = k if k < P else nfft - k
        v = w(kb, c) if k < P else sg * mp.conj(w(kb, part))
        if k == 0 and dc_rule:
            v = mp.mpc(w(1, c).real, 0)
        if shift_mode == 0:
            E = mp.exp(-2j * mp.pi * mp.mpf(kb) / nfft * delay)
            if kb == P - 1:
                E = mp.mpc(E.real, 0)
            if k >= P:
                E = mp.conj(E)
            v = v * E
        full.append(v)
    nf = R.fade_len(fade_rel, length)
    out = []
    for tt in range(length):
        t = nfft // 2 - length // 2 + tt
        if shift_mode == 1:
            t = (t - nfft // 2) % nfft
        x = sum((full[k] * mp.exp(2j * mp.pi * ((k * t) % nfft) / nfft) for k in range(nfft)), mp.mpc(0)) / nfft
        win = mp.mpf(1)
        if tt < nf or tt >= length - nf:
            i = tt if tt < nf else length - 1 - tt
            win = (1 - mp.cos(2 * mp.pi * i / (2 * nf - 1))) / 2
        out.append(x * win)
    return out


MP_EPILOGUE = [dict(nfft=8, len=8, C=4, conj_mode=1, dc_rule=1, shift_mode=0, fade_rel=0.15, grpd=(3.25, -1.5)),
               dict(nfft=16, len=6, C=5, conj_mode=2, dc_rule=0, shift_mode=0, fade_rel=0.5, grpd=(-700.125, 900.75)),
               dict(nfft=64, len=30, C=3, conj_mode=0, dc_rule=1, shift_mode=1, fade_rel=0.15, grpd=(0.0, 0.0)),
               dict(nfft=6, len=6, C=9, conj_mode=1, dc_rule=1, shift_mode=0, fade_rel=0.05, grpd=(3.25, -1.5)),
               dict(nfft=74, len=36, C=3, conj_mode=2, dc_rule=1, shift_mode=0, fade_rel=0.15, grpd=(3.25, -1.5)),
               dict(nfft=600, len=6, C=1, conj_mode=0, dc_rule=1, shift_mode=0, fade_rel=0.0, grpd=(-700.125, 900.75))]


@pytest.mark.parametrize("case", MP_EPILOGUE, ids=lambda c: "nfft%d" % c["nfft"])
def test_epilogue_ref_against_mpmath(mp, case):
    """epilogue_ref within (nfft + 16) longdouble eps of sum_k |W_k| / nfft: the rounding of a longdouble sum of nfft terms"""
    c = dict(case, n_ears=2, seed=77 + case["nfft"])
    W = R.epilogue_input(c)
    ref = R.epilogue_ref(W, c["nfft"], c["len"], c["grpd"], c["conj_mode"], c["dc_rule"], c["shift_mode"], 1, 2, c["fade_rel"])
    worst = 0.0
    for e in range(2):
        for ch in sorted({0, c["C"] // 2, c["C"] - 1}):
            want = mp_epilogue(mp, W, c["nfft"], c["len"], c["grpd"], c["conj_mode"], c["dc_rule"], c["shift_mode"], c["fade_rel"], e, ch)
            scale = 2.0 * np.abs(W[e]).sum(axis=0).max() / c["nfft"]
            worst = max(worst, max(ld_minus_mp(mp, ref[e][0][ch, t], want[t]) for t in range(c["len"])) / scale)
    print(f"epilogue nfft {c['nfft']}: longdouble vs 50 digits = {worst / R.EPS_LD:.2f} eps_ld of 2 sum|W| / nfft")
    assert worst <= (c["nfft"] + 16) * R.EPS_LD


@pytest.mark.parametrize("nfft,L,mode,g", [(8, 3, 0, (1.25, -0.5)), (64, 17, 0, (3.7, 70.2)), (64, 17, 1, (2.5, -3.49)), (6, 5, 1, (0.5, -0.5)),
                                           (600, 9, 0, (-2.25, 1.5)), (600, 9, 1, (601.5, -0.5))])
def test_spectra_and_group_delay_ref_against_mpmath(mp, nfft, L, mode, g):
    """hrir_spectra_ref, grpdelay_ref and real_spectra_ref within (L + 16) longdouble eps of their sums of moduli"""
    case = dict(nfft=nfft, L=L, D=2, D_src=3, mode=mode, didx=True, seed=5 + nfft + mode)
    hL, hR, didx = R.hrir_input(case)
    P = nfft // 2 + 1
    Hc, _, Ha, _ = R.hrir_spectra_ref(hL, hR, nfft, mode, g, didx)
    tol = (L + 16) * R.EPS_LD
    worst = 0.0
    for e, h in enumerate((hL, hR)):
        s = R.round_half_away(g[e])
        for d in range(2):
            row = h[didx[d]]
            for kb in range(P):
                if mode == 0:
                    v = sum((mp.mpf(float(row[n])) * mp.exp(-2j * mp.pi * ((kb * n) % nfft) / nfft) for n in range(L)), mp.mpc(0))
                    E = mp.exp(2j * mp.pi * mp.mpf(kb) / nfft * mp.mpf(float(g[e])))
                    v *= mp.mpc(E.real, 0) if kb == P - 1 else E
                else:   # out[n] = h[(n + s) mod nfft], zero beyond the L taps
                    v = sum((mp.mpf(float(row[(n + s) % nfft])) * mp.exp(-2j * mp.pi * ((kb * n) % nfft) / nfft)
                             for n in range(nfft) if (n + s) % nfft < L), mp.mpc(0))
                scale = np.abs(row).sum()
                worst = max(worst, ld_minus_mp(mp, Hc[e, kb, d], v) / scale, abs(float(mpf_of(mp, Ha[e, kb, d]) - abs(v))) / scale)
    assert worst <= tol, worst / R.EPS_LD
    # the group delay of the direction sum, bin by bin, and the ATF spectra of the same rows
    gd = R.grpdelay_ref(hL, hR, nfft)
    X, _ = R.real_spectra_ref(hL, nfft)
    for e, h in enumerate((hL, hR)):
        b = [sum(mp.mpf(float(v)) for v in h[:, n]) for n in range(L)]
        for kb in range(P):
            z = [mp.exp(-2j * mp.pi * ((kb * n) % nfft) / nfft) for n in range(L)]
            den, num = sum((b[n] * z[n] for n in range(L)), mp.mpc(0)), sum((n * b[n] * z[n] for n in range(L)), mp.mpc(0))
            assert not gd[e]["excluded"][kb]
            want = (num / den).real
            cond = float(sum(n * abs(b[n]) for n in range(L)) / abs(den) + abs(num) * sum(abs(v) for v in b) / abs(den) ** 2)
            assert abs(float(mpf_of(mp, gd[e]["gd"][kb]) - want)) <= tol * max(cond, 1.0)
    for d in range(hL.shape[0]):
        for kb in range(P):
            v = sum((mp.mpf(float(hL[d, n])) * mp.exp(-2j * mp.pi * ((kb * n) % nfft) / nfft) for n in range(L)), mp.mpc(0))
            assert ld_minus_mp(mp, X[kb, d], v) <= tol * np.abs(hL[d]).sum()


# ---- float64 implementations: the oracle's steps, and the same with one defect planted -----------------------------------------

def epilogue_f64(W, c, defect=None, direct=False):
    """The epilogue in float64 as the oracle does it (O._finish: mirror, ifft, delay phase or rotation, cut, O.hann), for every setting
    of the debug entry.  direct: the inverse transform as a sum over a float64 table (what the 'twiddle' defect perturbs).  Returns the
    ears' [C][len] arrays."""
    nfft, length, P, C = c["nfft"], c["len"], c["nfft"] // 2 + 1, c["C"]
    part, sgn = R.mirror_partner(C, c["conj_mode"])
    if defect == "sign":           # (-1)^m dropped for one m: the first channel with an odd m
        sgn = sgn.copy()
        sgn[np.flatnonzero(sgn < 0)[0]] = 1.0
    n_shift = nfft // 2
    t0 = n_shift - (length // 2 + (1 if defect == "t0" else 0))
    rows = t0 + np.arange(length)
    if c["shift_mode"] == 1:
        rows = (rows - n_shift) % nfft
    nf = R.fade_len(c["fade_rel"], length)
    h = O.hann(2 * nf) if nf > 0 else np.zeros(0)
    if defect == "window":         # the window index off by one
        h = 0.5 * (1 - np.cos(2 * np.pi * (np.arange(2 * nf) + 1) / (2 * nf - 1)))
    win = np.concatenate([h[:nf], np.ones(length - 2 * nf), h[:nf][::-1]])
    out = []
    for e in range(c["n_ears"]):
        We = np.array(W[e], dtype=np.complex128)
        if c["dc_rule"] and defect != "dc":
            We[0] = We[1].real
        full = np.vstack([We, np.conj(We[P - 2:0:-1][:, part]) * sgn[None, :]])
        if c["shift_mode"] == 0:
            g = c["grpd"][::-1] if defect == "swap" else c["grpd"]
            delay = float(n_shift) if e == 0 else R.right_delay(nfft, g)
            E = np.exp(-1j * 2 * np.pi * (np.arange(P) / nfft) * delay)
            if defect != "nyquist":
                E[-1] = E[-1].real
            Em = E[P - 2:0:-1] if defect == "mirror" else np.conj(E[P - 2:0:-1])
            full = full * np.concatenate([E, Em])[:, None]
        if direct:
            tab = np.exp(2j * np.pi * np.arange(nfft) / nfft)
            if defect == "twiddle":    # the entry bin 1 meets at the middle kept sample
                tab[rows[length // 2] % nfft] += 1e-12
            x = tab[(rows[:, None] * np.arange(nfft)[None, :]) % nfft] @ full / nfft
        else:
            x = np.fft.ifft(full, axis=0)[rows % nfft]
        x = x * win[:, None]
        out.append(np.ascontiguousarray((x if c["out_cplx"] else x.real).T))
    return out


def worst_ratio(got, ref):
    return max(float(R.ratio(g, r[0], r[1]).max()) for g, r in zip(got, ref))


@pytest.fixture(scope="module")
def epilogue_refs():
    R.require_longdouble()
    cache = {}

    def get(c):
        key = R.case_id(c) + str(c["seed"])
        if key not in cache:
            W = R.epilogue_input(c)
            cache[key] = (W, R.epilogue_ref(W, c["nfft"], c["len"], c["grpd"], c["conj_mode"], c["dc_rule"], c["shift_mode"], c["out_cplx"],
                                            c["n_ears"], c["fade_rel"]))
        return cache[key]
    return get


def test_epilogue_case_list_is_a_covering_design():
    """every value of every parameter occurs with both classes of nfft, and every nfft of either class occurs"""
    cases = R.epilogue_cases()
    assert 55 <= len(cases) <= 65 and len({R.case_id(c) for c in cases}) == len(cases)
    assert {(c["nfft"], c["len_kind"]) for c in cases} == {(n, k) for n in R.EPI_POW2 + R.EPI_DFT for k in range(5)}
    for nfft in (1024, 2048, 4096):    # the radial-filter use: one ear, fade 0.05, the whole transform kept
        assert any(c["nfft"] == nfft and c["len"] == nfft and (c["n_ears"], c["fade_rel"], c["dc_rule"], c["conj_mode"]) == (1, 0.05, 0, 0) for c in cases)
    assert sum(1 for c in cases if c["len"] == 2 and R.fade_len(c["fade_rel"], 2) == 1) <= 4      # (hann(2) = [0, 0]: such a case checks zeros only)
    for cls, nffts in (("pow2", R.EPI_POW2), ("dft", R.EPI_DFT)):
        cs = [c for c in cases if c["cls"] == cls]
        assert {c["nfft"] for c in cs} == set(nffts)
        assert {(c["conj_mode"], c["C"]) for c in cs} == set(R.EPI_MIRROR)
        assert {c["len_kind"] for c in cs} == set(range(5))
        assert {(c["n_ears"], c["fade_rel"]) for c in cs} == set(R.EPI_EARS_FADE)
        assert {c["grpd"] for c in cs} == set(R.EPI_GRPD)
        for key in ("dc_rule", "shift_mode", "out_cplx"):
            assert {c[key] for c in cs} == {0, 1}, (cls, key)
    for c in cases:
        assert c["len"] % 2 == 0 and 2 <= c["len"] <= c["nfft"]


@pytest.mark.parametrize("case", R.epilogue_cases(), ids=R.case_id)
def test_float64_epilogue_lies_within_the_bound(epilogue_refs, case):
    """The bound is attainable: the oracle's float64 route is inside it on every case of the GPU list -- O._finish itself where its
    fixed settings (two ears, fade 0.15) are the case's, the same steps with the case's settings elsewhere."""
    W, ref = epilogue_refs(case)
    got = epilogue_f64(W, case)
    c = case
    if c["n_ears"] == 2 and c["fade_rel"] == 0.15:
        Wd = W.copy()
        if c["dc_rule"]:
            Wd[:, 0] = Wd[:, 1].real
        conj_fn = {0: None, 1: O.getShFreqDomainConjugate, 2: O.getChFreqDomainConjugate}[c["conj_mode"]]
        n_shift = c["nfft"] // 2
        fin = O._finish(Wd[0], Wd[1], c["nfft"] // 2 + 1, c["nfft"], c["len"], c["conj_mode"] == 0, n_shift,
                        n_shift if c["shift_mode"] else R.right_delay(c["nfft"], c["grpd"]), integer_shift=bool(c["shift_mode"]), conj_fn=conj_fn)
        got = [np.ascontiguousarray((w if c["out_cplx"] else w.real).T) for w in fin]
    r = worst_ratio(got, ref)
    print(f"{R.case_id(case)}: float64 oracle error / bound = {r:.3f}")
    assert r <= 1.0


EPILOGUE_DEFECTS = ("window", "nyquist", "mirror", "sign", "dc", "swap", "twiddle", "t0")


def defect_applies(defect, c):
    """where a defect changes the result at all: the mode it lives in is the case's.  The perturbed table entry (1e-12) is visible where
    the bound is below it: up to nfft 16 -- at nfft 64 the phase term of the bound alone, 3 u pi (nfft / 2)^2 / 2 per unit spectrum,
    reaches 1e-12."""
    nf = R.fade_len(c["fade_rel"], c["len"])
    if c["len"] == 2 and nf == 1:      # hann(2) = [0, 0]: the window leaves nothing of either sample
        return False
    frac = c["n_ears"] == 2 and c["shift_mode"] == 0 and c["grpd"] != (0.0, 0.0)
    return {"window": nf >= 2, "nyquist": frac, "mirror": frac and c["nfft"] > 4, "sign": c["conj_mode"] == 1 and c["C"] >= 4,
            "dc": c["dc_rule"] == 1, "swap": frac, "twiddle": c["nfft"] <= 16, "t0": True}[defect]


@pytest.mark.parametrize("defect", EPILOGUE_DEFECTS)
def test_planted_epilogue_defect_exceeds_the_bound(epilogue_refs, defect):
    """The bound is not vacuous: a float64 epilogue with ONE defect is outside it on every case of the GPU list (up to nfft 600, where
    the float64 table form is quick) in which the defect's mode occurs.  ('t0': the entry takes an even len, whose half needs no
    rounding; the defect is planted as the next integer, len / 2 + 1.)"""
    cases = [c for c in R.epilogue_cases() if c["nfft"] <= 600 and defect_applies(defect, c)]
    assert len(cases) >= 3, defect
    for c in cases:
        W, ref = epilogue_refs(c)
        clean = worst_ratio(epilogue_f64(W, c, None, direct=True), ref)
        bad = worst_ratio(epilogue_f64(W, c, defect, direct=True), ref)
        print(f"{defect} at {R.case_id(c)}: error / bound = {bad:.3g} (without the defect {clean:.3g})")
        assert clean <= 1.0 and bad > 1.0, (defect, R.case_id(c))


# ---- prologue -----------------------------------------------------------------------------------------------------------------------

def spectra_f64(hL, hR, nfft, mode, g, didx, D, defect=None):
    """The prologue's spectra in float64 (np.fft): [2][P][D] complex"""
    sel = np.arange(D) if didx is None else didx
    P = nfft // 2 + 1
    out = np.zeros((2, P, len(sel)), dtype=np.complex128)
    for e, h in enumerate((hL, hR)):
        x = np.zeros((nfft, len(sel)))
        L = h.shape[1]
        if mode == 0:
            x[:L] = h[sel].T
            X = np.fft.fft(x, axis=0)[:P]
            E = np.exp(1j * 2 * np.pi * (np.arange(P) / nfft) * g[e])
            E[-1] = E[-1].real
            X = X * E[:, None]
        else:
            s = int(np.round(g[e])) if defect == "half_even" else R.round_half_away(g[e])
            if defect == "circular":    # the shift taken inside the L taps instead of inside nfft
                x[:L] = np.roll(h[sel].T, -s, axis=0)
            else:
                x[:L] = h[sel].T
                x = np.roll(x, -s, axis=0)
            X = np.fft.fft(x, axis=0)[:P]
        out[e] = X
    return out[::-1].copy() if defect == "ears" else out


def spectra_delays(case, hL, hR):
    """the delays of a case: placed, or the float64 oracle's medians of the direction sums (an input of the phase: the reference is
    evaluated at the delays the implementation under test used)"""
    if case["grpd"] is not None:
        return case["grpd"]
    P = case["nfft"] // 2 + 1
    return tuple(float(np.median(O.grpdelay_fir(h.sum(axis=0), P))) for h in (hL, hR))


@pytest.mark.parametrize("case", R.spectra_cases(), ids=R.case_id)
def test_float64_spectra_lie_within_the_bound(case):
    R.require_longdouble()
    hL, hR, didx = R.hrir_input(case)
    nfft, P = case["nfft"], case["nfft"] // 2 + 1
    g = spectra_delays(case, hL, hR)
    if case["mode"] == 0 and case["grpd"] is None and didx is None and case["D"] == case["D_src"]:
        HL, HR, gL, gR = O._hrir_prologue(hL.T, hR.T, nfft, P)       # the oracle's own prologue where the case is one it can run
        g, got = (gL, gR), np.stack([HL[:P], HR[:P]])
    else:
        got = spectra_f64(hL, hR, nfft, case["mode"], g, didx, case["D"])
    Hc, bc, Ha, ba = R.hrir_spectra_ref(hL, hR, nfft, case["mode"], g, didx, case["D"])
    rc, ra = float(R.ratio(got, Hc, bc).max()), float(R.ratio(np.abs(got), Ha, ba).max())
    print(f"{R.case_id(case)}: float64 error / bound = {rc:.3f} (complex), {ra:.3f} (|H|)")
    assert rc <= 1.0 and ra <= 1.0
    if case["zero_ear"] is not None:
        assert np.all(Ha[case["zero_ear"]] == 0)


@pytest.mark.parametrize("defect", ["half_even", "circular", "ears"])
def test_planted_prologue_defect_exceeds_the_bound(defect):
    """half_even: visible where a delay is a half with an even floor (0.5, -0.5, 2.5); circular: where a shift moves taps across the end
    of the L recorded ones; ears: everywhere."""
    R.require_longdouble()
    cases = [c for c in R.spectra_cases() if c["nfft"] <= 1024 and c["zero_ear"] is None and
             (defect == "ears" and c["L"] > 1 or c["mode"] == 1 and c["grpd"] in ((0.5, -0.5), (2.5, -3.49)))]
    assert len(cases) >= 6
    for c in cases:
        hL, hR, didx = R.hrir_input(c)
        g = spectra_delays(c, hL, hR)
        Hc, bc, _, _ = R.hrir_spectra_ref(hL, hR, c["nfft"], c["mode"], g, didx, c["D"])
        clean = float(R.ratio(spectra_f64(hL, hR, c["nfft"], c["mode"], g, didx, c["D"]), Hc, bc).max())
        bad = float(R.ratio(spectra_f64(hL, hR, c["nfft"], c["mode"], g, didx, c["D"], defect), Hc, bc).max())
        assert clean <= 1.0 and bad > 1.0, (defect, R.case_id(c), clean, bad)


@pytest.mark.parametrize("case", R.grpdelay_cases(), ids=R.case_id)
def test_float64_group_delay_lies_within_the_bound_and_exclusions_are_rare(case):
    """O.grpdelay_fir bin by bin and its median inside the bounds; at most 2 of P bins are left out next to the 10 eps branch, and none at
    all except for the input built to hit it."""
    R.require_longdouble()
    hL, hR = R.grpdelay_input(case)
    P = case["nfft"] // 2 + 1
    for h, ref in zip((hL, hR), R.grpdelay_ref(hL, hR, case["nfft"])):
        nex = int(ref["excluded"].sum())
        assert nex <= 2 and (nex == 0 or case["kind"] == "twotap"), nex
        if case["kind"] == "twotap":
            assert nex == 1 and ref["excluded"][case["nfft"] // 4] and ref["gd"][case["nfft"] // 4] == 0
        got = O.grpdelay_fir(h.sum(axis=0), P)
        keep = ~ref["excluded"]
        r = float(R.ratio(got[keep], ref["gd"][keep], ref["bound"][keep]).max())
        rm = abs(float(LD(float(np.median(got))) - ref["delay"])) / ref["delay_bound"] if ref["delay_bound"] > 0 else 0.0
        print(f"{R.case_id(case)}: float64 group delay error / bound = {r:.3f} per bin, {rm:.3f} median; delay bound {ref['delay_bound']:.2e}")
        assert r <= 1.0 and rm <= 1.0 and ref["delay_bound"] < 1e-4
        if case["kind"] == "impulse":
            assert float(np.abs(ref["gd"] - ref["gd"][0]).max()) < 1e-16 and round(float(ref["delay"])) in (7 % case["L"], 11 % case["L"])


@pytest.mark.parametrize("case", R.real_cases(), ids=R.case_id)
def test_float64_atf_spectra_lie_within_the_bound(case):
    R.require_longdouble()
    x, colidx, _ = R.real_input(case)
    X, b = R.real_spectra_ref(x, case["nfft"], case["ncols"], colidx)
    sel = np.arange(case["ncols"]) if colidx is None else colidx
    got = np.fft.rfft(x[sel], case["nfft"], axis=1).T
    r = float(R.ratio(got, X, b).max())
    assert r <= 1.0, r


def test_twiddle_bound_holds_for_the_kernels_formula_in_float64():
    """the table's formula evaluated in float64 on the host is inside tw_bound at every nfft of the GPU lists -- and outside a flat 2 u at
    the end of a long circle, which is why the bound grows with the argument"""
    R.require_longdouble()
    worst_u = 0.0
    for nfft in sorted(set(R.EPI_POW2 + R.EPI_DFT + (1024, 2048, 600, 6))):
        j = np.arange(nfft)
        a = -2.0 * np.pi * j / nfft
        got = np.cos(a) + 1j * np.sin(a)
        ref, tb = R.twiddle_ref(nfft)
        err = R.f64(np.abs(R.to_cld(got) - ref))
        ok = tb > 0
        assert np.all(err[ok] <= tb[ok])
        worst_u = max(worst_u, float(err.max()) / R.U)
    print(f"float64 table: largest error {worst_u:.2f} u")
    assert worst_u > 2.0
