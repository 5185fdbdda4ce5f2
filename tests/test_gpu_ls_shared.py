"""Sharing batches take their least-squares rows from one kept regularised inverse per bin (ls_shared.hip, batch_run.hip:
geo_yls_stage, geo_ls_shared_rows).  EMAGLS_GEO_LS_SHARED=0 selects the stages that carry every HRIR set through
the factors, which is what these tests compare against.  The shapes are those of test_gpu_geometry_kept.py: em32 at order 4 on the
complex basis, every third of the 2702 directions (901: not a multiple of any tile), 128 taps.  Bounds: 1e-9 between the two forms
(TOL_UNSHARED of test_gpu_geometry_kept.py), 1e-6 against the oracle (the project's bound for a design), 1e-8 of the largest entry for
an operand Y_reg_inv_k (the bound test_gpu_stages.py::test_stage_factor_and_sweep holds conj(Q) Z_k and conj(G_k) conj(M_k) to)."""
import numpy as np
import pytest

from oracle import emagls_oracle as O

pytestmark = pytest.mark.gpu

TOL_UNSHARED, TOL_ORACLE, TOL_OPERAND = 1e-9, 1e-6, 1e-8
C = 25


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def worst(res, ref):
    return max(rel(res[0], ref[0]), rel(res[1], ref[1]))


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


@pytest.fixture(scope="module")
def sets(thin):
    rng = np.random.default_rng(77)
    return [(thin["hL"] * (1.0 + 0.03 * j) + 1e-3 * rng.standard_normal(thin["hL"].shape),
             thin["hR"] * (1.0 - 0.02 * j) + 1e-3 * rng.standard_normal(thin["hR"].shape)) for j in range(8)]


class Shared:
    """A geometry-sharing batch of the HRIR sets `which` on one radius, executed `runs` times."""

    def __init__(self, thin, grids, sets, which, radius=None, runs=2, kind=None):
        from emagls_amd import Batch, Plan, _lib as L
        self.plans = []
        for j in which:
            hL, hR = sets[j]
            p = Plan(L.KIND_EMAGLS if kind is None else kind, "complex", 4, 48000.0, 128, hL.shape[0], hL.shape[1], grids["mic_radius"] if radius is None else radius, 32)
            p.set_hrir_grid(thin["azi"], thin["zen"])
            p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
            p.set_hrirs(hL, hR)
            self.plans.append(p)
        self.b = Batch(self.plans)
        self.b.share_geometry(True)
        self.outs = []
        for _ in range(runs):
            self.run()

    def run(self):
        self.b.execute()
        assert self.b.shares_geometry()
        self.outs.append(self.b.get_filters())
        return self.outs[-1]

    def info(self):
        return self.plans[0].info()

    def ls_rows(self, j):
        """W of plan j, [ear][bin][channel], the least-squares bins 1 .. k_cut-2"""
        i = self.info()
        return self.plans[j].debug("W", np.complex128)[:2 * i.num_pos_freqs * C].reshape(2, i.num_pos_freqs, C)[:, 1:i.k_cut - 1]

    def keeps_operand(self):
        try:
            self.plans[0].debug("Yls", np.complex128)
            return True
        except Exception:
            return False

    def close(self):
        self.b.close()
        for p in self.plans:
            p.close()


def both_forms(monkeypatch, thin, grids, sets, which, **kw):
    forms = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("EMAGLS_GEO_LS_SHARED", sw)
        forms[sw] = Shared(thin, grids, sets, which, **kw)
    monkeypatch.delenv("EMAGLS_GEO_LS_SHARED")
    return forms["1"], forms["0"]


def compare_forms(new, old, label):
    """filters to 1e-9, every least-squares bin's rows to 1e-9 of the bin's largest entry; the cold and the warm execute of each"""
    assert new.keeps_operand() and not old.keeps_operand()
    w_f = max(worst(a, c) for run_n, run_o in zip(new.outs, old.outs) for a, c in zip(run_n, run_o))
    w_r = 0.0
    for j in range(len(new.plans)):
        Wn, Wo = new.ls_rows(j), old.ls_rows(j)
        w_r = max(w_r, float((np.abs(Wn - Wo).max(axis=2) / np.abs(Wo).max(axis=2)).max()))
    i = new.info()
    print(f"{label}: hh_end {i.hh_end}, gram_from {i.gram_from}, k_cut {i.k_cut}; kept operand vs through the factors: filters {w_f:.3e}, "
          f"least-squares rows per bin {w_r:.3e}")
    assert w_f <= TOL_UNSHARED and w_r <= TOL_UNSHARED


def oracle_filters(thin, grids, hL, hR, radius=None, collect=None):
    return O.getEMagLsFilters(hL, hR, thin["azi"], thin["zen"], grids["mic_radius"] if radius is None else radius, grids["mic_azi"],
                              grids["mic_zen"], 4, 48000.0, 128, "complex", collect=collect)


@pytest.fixture(scope="module")
def oracle05(thin, grids, sets):
    """The oracle's filters of the sets 0 and 5, computed once."""
    return {j: oracle_filters(thin, grids, *sets[j]) for j in (0, 5)}


def test_both_forms_agree_and_stay_on_the_oracle(monkeypatch, thin, grids, sets, oracle05):
    """The same 6-plan sharing batch with the switch at 1 and at 0, a cold and a warm execute each: filters and least-squares rows agree
    to 1e-9; against the oracle on plans 0 and 5 the kept-operand form stays under 1e-6 and within a factor 2 of the other form."""
    new, old = both_forms(monkeypatch, thin, grids, sets, range(6))
    compare_forms(new, old, "em32, 6 plans")
    ref = oracle05
    d_new = max(worst(new.outs[-1][j], ref[j]) for j in (0, 5))
    d_old = max(worst(old.outs[-1][j], ref[j]) for j in (0, 5))
    print(f"against the oracle, plans 0 and 5: kept operand {d_new:.3e}, through the factors {d_old:.3e}")
    assert d_new < TOL_ORACLE and d_new <= 2.0 * d_old
    new.close()
    old.close()


def test_the_kept_operand_is_the_regularised_inverse(thin, grids, sets):
    """Yls_k of the first and the last bin of the Householder route and of the Gram route against the oracle's Y_reg_inv_k, relative
    to its largest entry.  A complex-basis design runs on the real SH channels until its epilogue (EMAGLS_REAL_INTERNAL, the default),
    so the operand is the real-basis one: the oracle is asked for the same geometry on the real basis."""
    yri = {}
    O.getEMagLsFilters(*sets[0], thin["azi"], thin["zen"], grids["mic_radius"], grids["mic_azi"], grids["mic_zen"], 4, 48000.0, 128, "real",
                       collect=lambda k, pw, sv, y: yri.setdefault(k - 1, y))
    s = Shared(thin, grids, sets, range(2), runs=1)
    i = s.info()
    D = thin["azi"].size
    ldD = -(-D // 64) * 64
    ls_end = i.k_cut - 1
    Yls = s.plans[0].debug("Yls", np.complex128)[:(ls_end - 1) * C * ldD].reshape(ls_end - 1, C, ldD)[:, :, :D]
    assert np.array_equal(Yls, s.plans[1].debug("Yls", np.complex128)[:(ls_end - 1) * C * ldD].reshape(ls_end - 1, C, ldD)[:, :, :D])
    assert 1 < i.hh_end < ls_end, "the em32 at 4.2 cm has least-squares bins on both routes"
    for kb, route in ((min(i.hh_end, ls_end) - 1, "Householder"), (ls_end - 1, "Gram"), (1, "Householder"), (i.gram_from, "Gram")):
        e = rel(Yls[kb - 1].T, yri[kb])
        print(f"Yls of bin {kb} ({route} route) vs the oracle's Y_reg_inv: {e:.3e} of its largest entry")
        assert e < TOL_OPERAND, (kb, e)
    s.close()


def test_bits_do_not_depend_on_lanes_neighbours_or_form_of_the_run(monkeypatch, thin, grids, sets):
    """HRIR set 4 as the last plan of a 3-plan batch in stream mode (EMAGLS_BATCH_LANES=0: every launch serves ONE lane -- a batch
    of one plan does not share a geometry), of a 3-lane and of an 8-lane batch (lane 2, lane 2, lane 7): the same bits.  They stay when
    another lane's HRIRs are replaced, and cold and warm executes return the same bits for every plan."""
    monkeypatch.setenv("EMAGLS_BATCH_LANES", "0")
    one = Shared(thin, grids, sets, (0, 1, 4))
    monkeypatch.delenv("EMAGLS_BATCH_LANES")
    assert not one.b.lane_mode()
    three = Shared(thin, grids, sets, (0, 1, 4))
    eight = Shared(thin, grids, sets, (0, 1, 2, 3, 5, 6, 7, 4))
    assert three.b.lane_mode() and eight.b.lane_mode()
    for s in (one, three, eight):
        assert s.keeps_operand() and s.b.geometry_runs() == (1, 1)
        assert all(same(a, c) for a, c in zip(s.outs[0], s.outs[1])), "cold and warm executes differ"
    assert np.array_equal(one.ls_rows(2), three.ls_rows(2)) and np.array_equal(three.ls_rows(2), eight.ls_rows(7))
    assert same(one.outs[1][2], three.outs[1][2]), "one lane per launch against three"
    assert same(three.outs[1][2], eight.outs[1][7]), "three lanes against eight"
    hL, hR = sets[3]
    eight.plans[1].set_hrirs(hL * 1.1, hR * 0.9)
    after = eight.run()
    assert eight.b.geometry_runs() == (1, 2)
    assert not same(after[1], eight.outs[1][1])
    for j in range(8):
        if j != 1:
            assert same(after[j], eight.outs[1][j]), f"plan {j} changed although its HRIRs did not"
    for s in (one, three, eight):
        s.close()


# radii of the range test (em32 microphone grid, k_cut = 11: least-squares bins 1 .. 9)
R_NO_GRAM, R_FEW_HH = 0.005, 0.1


def test_route_ranges(monkeypatch, thin, grids, sets):
    """5 mm: no least-squares bin is on the Gram route (gram_from = 44; the design is not a synthesising one and has flagged swept bins
    on the Householder route, whose Z rows plan 0 solves in place next to the ones the kept operand copies).  10 cm: the Householder
    route keeps bins 1 and 2 only (hh_end = 3).  The other extreme -- NO least-squares bin on the Householder route -- is out of
    reach of this geometry: bin 1 (187.5 Hz) stays on it up to the largest supported radius (19.3 cm at 48 kHz, simulation order 85;
    measured: hh_end = 2 at 15 cm and at 19 cm, simulation orders 66 and 84), so hh_end >= 2 at every radius; 10 cm keeps the plans
    small.  Both forms on three plans each, ranges read from the plan info."""
    for radius, want in ((R_NO_GRAM, "no Gram"), (R_FEW_HH, "few Householder")):
        new, old = both_forms(monkeypatch, thin, grids, sets, range(3), radius=radius)
        i = new.info()
        ls_end = i.k_cut - 1
        if want == "no Gram":
            assert i.gram_from == 0 or i.gram_from >= ls_end, (radius, i.gram_from, i.hh_end, ls_end)
        else:
            assert i.hh_end <= 3 and 0 < i.gram_from < ls_end, (radius, i.gram_from, i.hh_end, ls_end)
        compare_forms(new, old, f"radius {radius} m ({want}-route least-squares bins)")
        new.close()
        old.close()


def test_a_design_on_materialised_operands_keeps_the_old_stages(monkeypatch, thin, grids, sets, oracle05):
    """EMAGLS_SWEEP_SYNTH=0: the Gram-route least-squares bins read the materialised G_k, for which the kept operand has no route.  The
    sharing batch keeps no Yls and runs the stages through the factors whatever the switch says: the same bits with the switch at 1
    and at 0, cold and warm, and plan 0 within 1e-6 of the oracle."""
    monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "0")
    a, b = both_forms(monkeypatch, thin, grids, sets, range(3))
    monkeypatch.delenv("EMAGLS_SWEEP_SYNTH")
    assert not a.keeps_operand() and not b.keeps_operand()
    assert a.b.geometry_runs() == (1, 1)
    for j in range(3):
        assert same(a.outs[1][j], b.outs[1][j]) and same(a.outs[0][j], a.outs[1][j])
    w = worst(a.outs[1][0], oracle05[0])
    print(f"materialised operands, sharing batch on the stages through the factors vs the oracle: {w:.3e}")
    assert w < TOL_ORACLE
    # (raw-microphone designs keep the stages through the factors as well: batch_geo_ls_shared_wanted)
    from emagls_amd import _lib as L
    raw = Shared(thin, grids, sets, range(2), runs=1, kind=L.KIND_EMAGLS2)
    assert not raw.keeps_operand()
    for s in (a, b, raw):
        s.close()
