"""The register-resident sweep (sweep_reg.hip) sums its per-bin partials on the matrix pipe: a quad of lanes holds two directions,
each lane a quarter of their units, and v_mfma_f64_4x4x4_4b contracts over the directions.  Every workgroup size (4 ... 12 waves,
EMAGLS_REG_WAVES) and arrays of 7, 12, 14, 17 (the em32) and 18 units -- the unit slots of the quad layout filled in every way the
kernel allows -- against the slab form (EMAGLS_SWEEP_REG=0) and the oracle, on the thin 901-direction grid."""
import numpy as np
import pytest

from oracle import emagls_oracle as O

pytestmark = pytest.mark.gpu
WAVES = (4, 6, 8, 10, 12)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


@pytest.mark.parametrize("nunits", [7, 12, 14, 17, 18])
def test_register_resident_sweep_every_workgroup_size(grids, thin, monkeypatch, nunits):
    import emagls_amd as E
    from emagls_amd import Plan, _lib as L, synth
    if nunits == 17:   # the em32: 15 antipodal pairs and 2 single capsules
        maz, mzn = grids["mic_azi"], grids["mic_zen"]
    else:              # no antipodal pair: one unit per microphone (a jittered Fibonacci lattice, well conditioned)
        rng = np.random.default_rng(2000 + nunits)
        maz, mzn = synth.fibonacci_grid(nunits)
        maz = maz + 0.05 * rng.standard_normal(nunits)
        mzn = np.clip(mzn + 0.05 * rng.standard_normal(nunits), 0.05, np.pi - 0.05)
    nmics = len(maz)
    N = 2 if nmics < 16 else (3 if nmics < 25 else 4)
    hL, hR, azi, zen = thin["hL"], thin["hR"], thin["azi"], thin["zen"]
    p = Plan(L.KIND_EMAGLS2, "real", N, 48000.0, 128, hL.shape[0], hL.shape[1], 0.042, nmics)
    p.set_hrir_grid(azi, zen)
    p.set_mic_grid(maz, mzn)
    assert p.info().sweep_units == nunits
    p.close()
    args = (hL, hR, azi, zen, 0.042, maz, mzn, N, 48000.0, 128, "real")
    o = O.getEMagLs2Filters(*args)
    monkeypatch.setenv("EMAGLS_SWEEP_REG", "0")
    L.check(L.load().emagls_cache_clear())
    s = E.getEMagLs2Filters(*args)
    monkeypatch.setenv("EMAGLS_SWEEP_REG", "2")
    for nw in WAVES:
        monkeypatch.setenv("EMAGLS_REG_WAVES", str(nw))
        L.check(L.load().emagls_cache_clear())
        r = E.getEMagLs2Filters(*args)
        e_o, e_s = max(rel(r[0], o[0]), rel(r[1], o[1])), max(rel(r[0], s[0]), rel(r[1], s[1]))
        print(f"{nunits} units, {nw} waves per workgroup: rel vs oracle = {e_o:.3e}, vs the slab form = {e_s:.3e}")
        assert e_o < 2e-7 and 0 < e_s < 1e-9
    monkeypatch.delenv("EMAGLS_REG_WAVES")
    monkeypatch.delenv("EMAGLS_SWEEP_REG")
    L.check(L.load().emagls_cache_clear())
