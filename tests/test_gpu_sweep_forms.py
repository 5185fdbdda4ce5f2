"""GPU parity through the C ABI against the CPU oracle, tolerance 1e-6 relative complex error (BASELINE.json north_star), with the
reference's own assertAllClose metrics (verifyEMagLs.m:370-395): the forms of the sequential MagLS sweep (lib/getEMagLsFilters.m:95-103): launch per bin, persistent on materialised operands, synthesising (slab / register-resident), both placements.
(Split out of tests/test_gpu_parity.py in round 6 so that `-x` loses less.)"""
import os

import numpy as np
import pytest

from oracle import emagls_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-6


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def report(name, w, o):
    nd, db, adb = O.assert_all_close_metrics(w, o)
    print(f"{name}: norm_diff={nd:.3e} max_dB={db:.3e} max|dB|={adb:.3e}")
    return nd


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


def test_register_resident_sweep_spread_over_all_xcds(grids, thin, monkeypatch):
    """A launch of the register-resident sweep keeps every design inside one XCD (the granules of the per-bin exchange stay in its L2)
    or deals a design's workgroups round over all eight (EMAGLS_REG_SPREAD; the default takes it when it needs fewer waves per
    workgroup: 20 designs of config 3 run 220 workgroups of 8 waves instead of 27 per XCD of 10, 4.2 against 5.3 ms).  The partial
    sums are added in workgroup order either way: bitwise the same filters, on a batch of 10 designs, both layouts forced."""
    import ctypes
    from emagls_amd import Batch, Plan, _lib as L, synth
    lib = L.load()
    res = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("EMAGLS_REG_SPREAD", mode)
        plans = []
        for j in range(10):
            azi = np.mod(thin["azi"] + 0.17 * j, 2 * np.pi)
            hL, hR = synth.rigid_sphere_hrirs(azi, thin["zen"], seed=31 + j)
            p = Plan(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, hL.shape[0], hL.shape[1], 0.042, 32)
            p.set_hrir_grid(azi, thin["zen"])
            p.set_mic_grid(np.mod(grids["mic_azi"] + 0.1 * j, 2 * np.pi), grids["mic_zen"])
            p.set_hrirs(hL, hR)
            plans.append(p)
        prev = ctypes.c_int(0)
        L.check(lib.emagls_set_batch_max(16, ctypes.byref(prev)))
        try:
            b = Batch(plans)
        finally:
            L.check(lib.emagls_set_batch_max(prev.value, None))
        b.execute()
        res[mode] = b.get_filters()
        assert plans[0].info().sweep_form == 3
        if mode == "1":   # one design against the oracle
            azi = np.mod(thin["azi"] + 0.17 * 9, 2 * np.pi)
            hL, hR = synth.rigid_sphere_hrirs(azi, thin["zen"], seed=31 + 9)
            oL, oR = O.getEMagLsFilters(hL, hR, azi, thin["zen"], 0.042, np.mod(grids["mic_azi"] + 0.9, 2 * np.pi), grids["mic_zen"], 4, 48000.0, 128, "complex")
            assert rel(res[mode][9][0], oL) < TOL and rel(res[mode][9][1], oR) < TOL
        b.close()
        for p in plans:
            p.close()
    for (aL, aR), (cL, cR) in zip(res["0"], res["1"]):
        assert np.array_equal(aL, cL) and np.array_equal(aR, cR)


@pytest.mark.parametrize("mode", ["launch_per_bin", "persistent_write_through", "synthesising", "synthesising_registers"])
def test_sweep_variants_agree(grids, thin, monkeypatch, mode):
    """The phase sweep on materialised operands has three forms: the persistent launch with XCD-local granule stores (default
    when all workgroups of a design share an XCD), the same with write-through stores (any placement), and one launch per
    bin (shapes the persistent kernel does not cover).  They sum the per-workgroup partials in different fixed
    orders, so they agree to rounding; each is bitwise reproducible.  The synthesising sweep (sweep_synth.hip) evaluates
    pwGrid from the angles between directions and microphones instead of the SH matrices: the same operand to 1.9e-14 of its largest
    value (measured, tests/test_gpu_synth_operand.py), the same filters to what the bins' conditioning makes of that (measured 1e-8; the tolerance of the design
    path is 1e-6)."""
    from emagls_amd import Plan, _lib as L
    monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "0")

    def run():
        p = Plan(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, thin["hL"].shape[0], thin["hL"].shape[1], 0.042, 32)
        p.set_hrir_grid(thin["azi"], thin["zen"])
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
        p.set_hrirs(thin["hL"], thin["hR"])
        outs = []
        for _ in range(3):  # eager, captured, replayed
            p.execute()
            outs.append(p.get_filters())
        launches = p.info().num_sweep_launches
        p.close()
        for wL, wR in outs[1:]:
            assert np.array_equal(wL, outs[0][0]) and np.array_equal(wR, outs[0][1])
        return outs[0], launches

    (dL, dR), n_default = run()
    assert n_default == 1  # the persistent kernel is the default
    if mode == "launch_per_bin":
        monkeypatch.setenv("EMAGLS_SWEEP_PERSIST", "0")
    elif mode == "synthesising":         # sweep_synth.hip: the form of launches of up to 8 designs
        monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "1")
    elif mode == "synthesising_registers":   # sweep_reg.hip (the form of larger launches) for this single design
        monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "1")
        monkeypatch.setenv("EMAGLS_SWEEP_REG", "2")
    else:
        monkeypatch.setenv("EMAGLS_PERSIST_GLOBAL", "1")
    (vL, vR), n_variant = run()
    assert (n_variant > 1) == (mode == "launch_per_bin")
    print(f"sweep variant {mode} vs default: rel = {max(rel(vL, dL), rel(vR, dR)):.3e}")
    # (the synthesising forms are bounded at about 10x their measured distance from the materialised operands -- 5e-9
    # ... 6e-8 over the suite, DESIGN.md section 3 -- not at the oracle tolerance)
    tol = 5e-7 if mode.startswith("synthesising") else 1e-12
    assert rel(vL, dL) < tol and rel(vR, dR) < tol
    if mode.startswith("synthesising"):
        assert rel(vL, dL) > 0   # (it did take the other kernel)


@pytest.mark.parametrize("nmics,paired", [(32, "em32"), (32, "none"), (20, "some"), (12, "none"), (7, "none")])
def test_synthesising_sweep_on_other_arrays(grids, thin, monkeypatch, nmics, paired):
    """sweep_synth.hip evaluates pwGrid from the angles between HRIR directions and microphones; antipodal microphone pairs share
    one polynomial evaluation (g(-x) from the even and odd parts of g(x)).  Arrays with every, some and no antipodal pair, 7 to 32
    microphones (8-, 16- and 32-row slabs): against the oracle, against the materialised operands (EMAGLS_SWEEP_SYNTH=0) and
    with the pairing switched off (EMAGLS_SYNTH_PAIRS is a "process" switch -- DESIGN.md section 8 gives every switch's read time --,
    so that comparison runs in the default process only through the plan's unit count)."""
    import emagls_amd as E
    from emagls_amd import Plan, _lib as L
    rng = np.random.default_rng(1000 + nmics)
    if paired == "em32":
        maz, mzn = grids["mic_azi"], grids["mic_zen"]
    else:
        # a spread-out array (a jittered spherical Fibonacci lattice: a random placement is so ill-conditioned that the oracle
        # itself moves by more than the tolerance with the rounding of its SVD)
        from emagls_amd import synth
        nbase = nmics - 6 if paired == "some" else nmics
        maz, mzn = synth.fibonacci_grid(nbase)
        maz = maz + 0.05 * rng.standard_normal(nbase)
        mzn = np.clip(mzn + 0.05 * rng.standard_normal(nbase), 0.05, np.pi - 0.05)
        if paired == "some":   # six microphones of the upper half get exact antipodes at the end of the list
            up = np.argsort(mzn)[:6]
            maz = np.concatenate([maz, maz[up] + np.pi])
            mzn = np.concatenate([mzn, np.pi - mzn[up]])
    N = 2 if nmics < 16 else (3 if nmics < 25 else 4)   # (orders whose Gram route starts below k_cut: every swept bin qualifies)
    hL, hR, azi, zen = thin["hL"], thin["hR"], thin["azi"], thin["zen"]
    p = Plan(L.KIND_EMAGLS2, "real", N, 48000.0, 128, hL.shape[0], hL.shape[1], 0.042, nmics)
    p.set_hrir_grid(azi, zen)
    p.set_mic_grid(maz, mzn)
    i = p.info()
    want_units = {"em32": 17, "none": nmics, "some": nmics - 6}[paired]
    assert i.sweep_form == 2 and i.sweep_units == want_units, (i.sweep_form, i.sweep_units)
    p.close()
    for fn, extra in (("getEMagLs2Filters", ()), ("getEMagLsFilters", ())):
        if fn == "getEMagLsFilters" and nmics < (N + 1) ** 2:
            continue
        args = (hL, hR, azi, zen, 0.042, maz, mzn, N, 48000.0, 128, "real")
        w = getattr(E, fn)(*args)
        o = getattr(O, fn)(*args)
        e_o = max(rel(w[0], o[0]), rel(w[1], o[1]))
        monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "0")
        L.check(L.load().emagls_cache_clear())   # (the one-shot plan cache holds the synthesising plan of this shape)
        m = getattr(E, fn)(*args)
        monkeypatch.delenv("EMAGLS_SWEEP_SYNTH")
        L.check(L.load().emagls_cache_clear())
        e_m = max(rel(w[0], m[0]), rel(w[1], m[1]))
        print(f"synthesising sweep, {fn}, {nmics} microphones ({paired} pairs, {want_units} units): rel vs oracle = {e_o:.3e}, vs materialised operands = {e_m:.3e}")
        # (explicit margins instead of the oracle tolerance: 10x the largest distances measured over the suite)
        assert e_o < 2e-7 and 0 < e_m < 2e-7
        if want_units <= 18:   # the register-resident form (sweep_reg.hip: the form of launches of more than 8 designs) on the same design
            monkeypatch.setenv("EMAGLS_SWEEP_REG", "2")
            L.check(L.load().emagls_cache_clear())
            r = getattr(E, fn)(*args)
            monkeypatch.delenv("EMAGLS_SWEEP_REG")
            L.check(L.load().emagls_cache_clear())
            e_r, e_rs = max(rel(r[0], o[0]), rel(r[1], o[1])), max(rel(r[0], w[0]), rel(r[1], w[1]))
            print(f"    register-resident form: rel vs oracle = {e_r:.3e}, vs the slab form = {e_rs:.3e}")
            assert e_r < 2e-7 and e_rs < 1e-9
