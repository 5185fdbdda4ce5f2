"""getEMagLsFiltersFromAtf on ATF sets above the Gram route's conditioning limit (cond < 3e4) with MORE than 4096 matched directions:
the dense route's tiled form -- the rows of every dense bin in blocks of at most 3072, each block factored by one workgroup, a tree
step over the blocks' triangles, Jacobi on the result and a two-level back-transform (wide_array.hip: launch_wa_factor_tiled),
lib/getEMagLsFiltersFromAtf.m:100-120.  These designs used to end with "the dense route holds at most 4096 matched directions".
Against the CPU oracle at the suite's TOL with the reference's own assertAllClose metrics; the inputs are those of
tests/from_atf_tiled_cases.py (tests/test_from_atf_tiled_inputs.py holds them to the reference's own floor)."""
import numpy as np
import pytest

from oracle import emagls_oracle as O
import from_atf_tiled_cases as C

pytestmark = pytest.mark.gpu
TOL = 1e-6


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def report(name, w, o):
    nd, db, adb = O.assert_all_close_metrics(w, o)
    print(f"{name}: norm_diff={nd:.3e} max_dB={db:.3e} max|dB|={adb:.3e}")
    return nd


def _plan(name):
    from emagls_amd import Plan, _lib as L
    hL, hR, hg, atf, ag = C.case(name)
    p = Plan(L.KIND_FROM_ATF, "real", 0, C.FS, C.LEN, hL.shape[0], hL.shape[1], nmics=atf.shape[1], f_trans=C.F_TRANS,
             atf_taps=atf.shape[0], natf=atf.shape[2])
    p.set_hrir_grid(hg[:, 0], hg[:, 1])
    p.set_hrirs(hL, hR)
    p.set_atfs(atf, ag[:, 0], ag[:, 1])
    return p


def _run(name):
    p = _plan(name)
    try:
        p.execute()
        wL, wR = p.get_filters()
        i = p.info()
    finally:
        p.close()
    oL, oR = C.oracle_filters(name)
    return wL, wR, oL, oR, i


@pytest.mark.parametrize("name", C.ALL_DENSE)
def test_near_copy_at_every_bin(name):
    """Two and three row blocks, 8 / 9 / 16 / 32 microphones; 4106: cut at 4096 the second block would be shorter than it is wide;
    6150: the first heights with a third block, and the shortest last block of this cutting rule there."""
    nmics = C.SHAPES[name][0]
    wL, wR, oL, oR, i = _run(name)
    assert wL.shape == (C.LEN, nmics)
    eL, eR = report(f"FromAtf tiled dense route, {name}: {nmics} mics x {C.matched(name)} directions L", wL, oL), report("R", wR, oR)
    assert i.gram_from == 0
    assert eL < TOL and eR < TOL


def test_lowest_bins_only():
    """The near-copy's difference is high-passed: only the lowest bins exceed the limit.  Both routes in one design, the boundary
    inside the swept bins."""
    wL, wR, oL, oR, i = _run("partly16")
    eL, eR = report(f"FromAtf tiled, partly dense (gram_from {i.gram_from}) L", wL, oL), report("R", wR, oR)
    kcut0 = i.k_cut - 1
    assert kcut0 == C.KCUT0 and i.num_pos_freqs == C.P
    assert kcut0 < i.gram_from < C.P
    assert eL < TOL and eR < TOL


def test_executing_the_plan_again_gives_equal_bits():
    """The first execute meets the flag and re-runs; the cached plan keeps the moved route.  No atomics, fixed orders: equal bits."""
    p = _plan("two16")
    try:
        outs = []
        for _ in range(3):
            p.execute()
            outs.append(p.get_filters())
        i = p.info()
    finally:
        p.close()
    assert i.gram_from == 0
    for wL, wR in outs[1:]:
        assert np.array_equal(wL, outs[0][0]) and np.array_equal(wR, outs[0][1])
    oL, oR = C.oracle_filters("two16")
    assert report("FromAtf tiled, third execute L", outs[2][0], oL) < TOL and report("R", outs[2][1], oR) < TOL


def test_hrir_sets_in_one_call():
    """fromAtfHrirSets with two HRIR sets on two16: the subjects run plan by plan when bins are dense, and each equals its single
    call (the comparison of test_from_atf_subjects_in_one_call)."""
    import emagls_amd as E
    hL0, hR0, hg, atf, ag = C.case("two16")
    rng = np.random.default_rng(61)
    hL = np.stack([hL0 * (1 + 0.04 * j) + 1e-3 * rng.standard_normal(hL0.shape) for j in range(2)], axis=2)
    hR = np.stack([hR0 * (1 - 0.03 * j) for j in range(2)], axis=2)
    wL, wR, dev = E.fromAtfHrirSets(hL, hR, hg, atf, ag, C.FS, C.LEN, C.F_TRANS)
    assert wL.shape == (C.LEN, 16, 2)
    worst = 0.0
    for j in range(2):
        sL, sR = E.getEMagLsFiltersFromAtf(hL[:, :, j], hR[:, :, j], hg, atf, ag, C.FS, C.LEN, C.F_TRANS, verbose=False)
        worst = max(worst, rel(wL[:, :, j], sL), rel(wR[:, :, j], sR))
    print(f"2 FromAtf subjects on a tiled dense ATF set in one call: worst rel vs single calls = {worst:.3e}")
    assert worst < 1e-11
    assert rel(wL[:, :, 0], wL[:, :, 1]) > 1e-3
