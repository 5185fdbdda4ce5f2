"""One bin step of the resident sweeps (sweep_reg.hip, sweep_synth.hip) against a longdouble step on the same inputs, bin by bin.

A plan executed with set_profiling(1) keeps the chain's stored totals u(k) (`Usw`), Mt = Pm^T M Pm, M, Pm, |H|, the Chebyshev rows and
the row order of the microphones.  For every selected swept bin (every 4th, the ends, the first and the last swept bin) the kernel's
u(k) is held to synth_reference.sweep_step of u(k-1), Mt(k-1), |H(k)| and the longdouble operand, element by element, within the a-priori
bound_step (derived in tests/synth_reference.py, checked on host-made inputs by tests/test_synth_reference_host.py); Mt to mt_from, the
chain's start value and the swept rows of W to rows_from_totals.  The kernels' forms, workgroup sizes, unit-slot fillings, slab heights
and the direction counts at which their tails change are the cases.  eMagLS2 plans in the real basis, 128 taps, unless said otherwise."""
import ctypes as C

import numpy as np
import pytest

import synth_reference as R

pytestmark = pytest.mark.gpu

WAVES = (4, 6, 8, 10, 12)
TOP_ORDER = 85            # (tests/test_gpu_synth_operand.py: the largest simulation order the library takes)
FCUT_ORDER = 15           # order-5 radius: f_cut = 7.5 kHz, so that every swept bin is on the Gram route (as the operand test does)
# The smallest direction count the order-5 plan of 12 microphones accepts: the orthonormal route of its low bins (bins below 10) takes
# all six orders there, S_h = 36 columns of the grid's SH matrix, and plan_routes refuses D < S_h (found by creating the plan at every
# count from 10 on: 10 and 11 are fewer directions than microphones, 12 ... 35 fewer than S_h, 36 runs)
SMALLEST_D = 36


def radius_of(order):
    return R.RADIUS_OF_ORDER.get(order, (order - 0.5) * R.C_SOUND / (R.FS * np.pi))


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


@pytest.fixture(scope="module")
def scenes(grids, thin):
    """direction count -> (azi, zen, hL, hR): the thin HRIR grid for 901, a Fibonacci lattice with rigid-sphere HRIRs otherwise; and
    unit count -> microphone grid (17: the em32, else a jittered lattice without an antipodal pair).  Made once."""
    from emagls_amd import synth
    R.require_longdouble()
    dirs, mics = {}, {}

    def directions(D):
        if D not in dirs:
            if D == 901:
                dirs[D] = (thin["azi"], thin["zen"], thin["hL"], thin["hR"])
            else:
                azi, zen = synth.fibonacci_grid(D)
                dirs[D] = (azi, zen) + tuple(synth.rigid_sphere_hrirs(azi, zen, seed=77 + D))
        return dirs[D]

    def microphones(nunits):
        if nunits not in mics:
            mics[nunits] = (grids["mic_azi"], grids["mic_zen"]) if nunits == 17 else R.jittered_array(nunits)
        return mics[nunits]
    return directions, microphones


def device_cosines(azi, zen, maz, mzn):
    """2 cos(direction, microphone) [D][M] as the sweeps form it (synth_zen / synth_x2 of synth_common.hpp, run by the debug entry)"""
    from emagls_amd import _lib as L
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (azi, zen, maz, mzn)]
    x2 = np.full((a[0].size, a[2].size), np.nan)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    L.check(L.load().emagls_debug_synth_cosines(ptr(a[0]), ptr(a[1]), a[0].size, ptr(a[2]), ptr(a[3]), a[2].size, ptr(x2)))
    return x2


@pytest.fixture(scope="module")
def operands():
    """(geometry key) -> the longdouble operand of its selected bins (synth_reference.step_operand), computed once per geometry and
    shared by the forms and workgroup sizes that run on it: the Chebyshev rows must be the same bits in every run.  The arguments are
    the sweeps' own 2 cos(direction, first microphone of the unit), so that the step is checked on the same inputs; they are held here
    to synth_reference.cosines of the plan's grids within the tolerance of tests/test_gpu_synth_operand.py (16 eps + twice the
    allowance on 2 cos)."""
    cache = {}

    def get(key, d):
        if key not in cache:
            first = d["smap"][R.unit_rows(int(d["smap"][32]), int(d["smap"][33]))[0]]
            x2 = device_cosines(d["azi"], d["zen"], d["maz"][first], d["mzn"][first])
            want, allow = R.cosines(d["azi"], d["zen"], d["maz"][first], d["mzn"][first], with_allowance=True)
            assert np.all(np.abs(x2 - 2.0 * want.astype(R.LD)).astype(np.float64) <= 16 * R.EPS64 + 2.0 * allow) and np.abs(x2).max() <= 2.0
            g, m, dg, units = R.step_operand(d["bsc"][d["bins"]], 0.5 * x2, d["smap"])
            cache[key] = dict(bsc=d["bsc"].copy(), smap=d["smap"].copy(), bins=d["bins"].copy(), g=g, m=m, dg=dg, units=units)
        o = cache[key]
        assert np.array_equal(o["bsc"], d["bsc"]) and np.array_equal(o["smap"], d["smap"]) and np.array_equal(o["bins"], d["bins"]), key
        return o
    return get


def make_plan(kind, N, radius, scene, mics, basis="real"):
    from emagls_amd import Plan
    azi, zen, hL, hR = scene
    p = Plan(kind, basis, N, R.FS, R.TAPS, hL.shape[0], hL.shape[1], radius, len(mics[0]))
    p.set_hrir_grid(azi, zen)
    p.set_mic_grid(*mics)
    p.set_hrirs(hL, hR)
    return p


def read_design(p, scene, mics, bins=None):
    """The buffers of an executed plan, in the layouts of plan_setup.hip / plan_run.hip: Usw [chunk][ear][bin][32] (the chain's totals in
    chunk 0, rows in smap order), Mt and Mw with bin kb at slot kb - 1 (M x M and C x C, row-major), Pm [32][32] (C x M used), Habs
    [ear][bin - kcut0][ldD], W [ear][bin][C], Winit [ear][32]."""
    i = p.info()
    P, D, M, Cn = i.num_pos_freqs, scene[0].size, len(mics[0]), i.num_channels
    kcut0 = min(i.k_cut - 1, P)
    kfirst = max(kcut0, 1)
    assert P == R.NBINS and kfirst < P - 1 and 0 < i.gram_from <= kfirst
    nord_pad = (i.sim_order + 2) & ~1
    na = max(P - kcut0, 1)
    habs = p.debug("Habs", np.float64)
    assert habs.size % (2 * na) == 0
    ldD = habs.size // (2 * na)
    assert D <= ldD < D + 64
    usw = p.debug("Usw", np.complex128)
    assert usw.size % (2 * P * 32) == 0
    sel = R.selected_bins(P) if bins is None else np.asarray(bins)
    d = dict(P=P, D=D, M=M, C=Cn, kfirst=kfirst, sweep_form=i.sweep_form, sweep_units=i.sweep_units, sim_order=i.sim_order,
             bins=np.array(sorted({int(k) for k in sel if k >= kfirst} | {kfirst, P - 1})),
             azi=scene[0], zen=scene[1], maz=np.asarray(mics[0]), mzn=np.asarray(mics[1]),
             Usw=usw.reshape(-1, 2, P, 32)[0][:, :, :M].copy(), Mt=p.debug("Mt", np.complex128)[:P * M * M].reshape(P, M, M).copy(),
             Mw=p.debug("Mw", np.complex128)[:P * Cn * Cn].reshape(P, Cn, Cn).copy(), Pm=p.debug("Pm", np.float64).reshape(32, 32)[:Cn, :M].copy(),
             Habs=habs.reshape(2, na, ldD)[:, kfirst - kcut0:, :D].copy(), bsc=p.debug("bsc", np.complex128)[:P * nord_pad].reshape(P, nord_pad).copy(),
             smap=p.debug("smap", np.int32)[:34].copy(), W=p.debug("W", np.complex128)[:2 * P * Cn].reshape(2, P, Cn).copy(),
             Winit=p.debug("Winit", np.complex128).reshape(2, 32)[:, :M].copy())
    assert sorted(d["smap"][:M].tolist()) == list(range(M)) and 2 * int(d["smap"][32]) + int(d["smap"][33]) == M
    return d


def run_design(kind, N, radius, scene, mics, bins=None):
    p = make_plan(kind, N, radius, scene, mics)
    p.set_profiling(1)
    p.execute()
    p.synchronize()
    d = read_design(p, scene, mics, bins)
    p.close()
    return d


def check_steps(label, d, o):
    """u(k) of every selected swept bin against the longdouble step within bound_step; returns the largest error / bound"""
    kfirst, P = d["kfirst"], d["P"]
    assert np.all(np.isfinite(d["Usw"][:, kfirst:].view(np.float64)))
    worst, where, missed, rel, seen = 0.0, None, [], [], 0
    for i, k in enumerate(d["bins"]):
        habs, nyq = d["Habs"][:, k - kfirst], bool(k == P - 1)
        u_prev, mt_prev, w0 = (None, None, d["Winit"]) if k == kfirst else (d["Usw"][:, k - 1], d["Mt"][k - 2], None)
        step = R.sweep_step(u_prev, mt_prev, habs, o["g"][i], nyquist=nyq, w_start=w0)
        bound = R.bound_step(u_prev, mt_prev, habs, o["g"][i], o["m"][i], o["dg"][i], o["units"], nyquist=nyq, w_start=w0, step=step)
        ratio = R.step_ratio(d["Usw"][:, k], step[0], bound)
        assert np.abs(step[0]).min() > 0
        rel.append(np.median(bound / np.abs(step[0]).astype(np.float64)))
        seen += bool(np.any(1e-10 * np.abs(step[0]).astype(np.float64) > bound))    # would a p / |p| that is 1e-10 off miss the bound here?
        e, j = np.unravel_index(ratio.argmax(), ratio.shape)
        if ratio.max() >= worst:
            worst, where = float(ratio.max()), (int(k), int(e), int(j))
        if not np.all(ratio <= 1.0):
            missed.append((int(k), int(e), int(j), float(ratio.max())))
    print(f"{label}: form {d['sweep_form']}, {d['sweep_units']} units, {d['D']} directions, {len(d['bins'])} bins: |u(k) - longdouble step| / bound_step, "
          f"largest {worst:.3e} (bin, ear, row {where}); bound_step / |u(k)|, median per bin: {min(rel):.1e} ... {max(rel):.1e} "
          f"(a normalisation 1e-10 off would miss the bound in {seen} of {len(rel)} bins)")
    assert not missed, (label, "form", d["sweep_form"], "(bin, ear, row, error / bound):", missed)
    return worst


def check_around(label, d):
    """Mt against Pm^T M Pm, the chain's start value against W(kfirst - 1,:) Pm, the swept rows of W against (u Pm^T) conj(M)"""
    kfirst, P, M, Cn = d["kfirst"], d["P"], d["M"], d["C"]
    r_mt = r_w = 0.0
    for k in sorted({int(k) for k in d["bins"]} | {int(k) - 1 for k in d["bins"] if k > kfirst}):
        ref, bound = R.mt_from(d["Mw"][k - 1], d["Pm"])
        r_mt = max(r_mt, float(R.step_ratio(d["Mt"][k - 1], ref, bound).max()))
    for k in d["bins"]:
        ref, bound = R.rows_from_totals(d["Usw"][:, k], d["Pm"], d["Mw"][k - 1])
        r_w = max(r_w, float(R.step_ratio(d["W"][:, k], ref, bound).max()))
    Pm = d["Pm"].astype(R.LD)
    ref = R.to_cld(d["W"][:, kfirst - 1]) @ Pm
    bound = R.gamma(2 * Cn + 2) * (np.abs(d["W"][:, kfirst - 1]) @ np.abs(d["Pm"]))
    r_i = float(R.step_ratio(d["Winit"], ref, bound).max())
    print(f"{label}: Mt / bound {r_mt:.3e}, start value / bound {r_i:.3e}, rows of W / bound {r_w:.3e}")
    assert r_mt <= 1.0 and r_i <= 1.0 and r_w <= 1.0, (label, r_mt, r_i, r_w)
    assert np.abs(d["Winit"]).max() > 0 and np.abs(d["W"][:, kfirst:]).min() > 0


def clear_cache():
    from emagls_amd import _lib as L
    L.check(L.load().emagls_cache_clear())


REG_CASES = sorted({(u, nw) for u in (17, 18) for nw in WAVES} | {(u, 4) for u in (7, 12, 14, 17, 18)})


@pytest.mark.parametrize("nunits,nw", REG_CASES)
def test_register_resident_step_workgroup_sizes_and_unit_slots(scenes, operands, monkeypatch, nunits, nw):
    """sweep_reg_kernel on 901 directions: every workgroup size (4 ... 12 waves) on the em32 (17 units: 15 pairs, 2 singles) and on 18
    single microphones (slot 8 of the quad layout full), and the unit-slot fillings 7, 12, 14, 17, 18 at four waves."""
    from emagls_amd import _lib as L
    directions, microphones = scenes
    mics = microphones(nunits)
    N = 2 if len(mics[0]) < 16 else (3 if len(mics[0]) < 25 else 4)
    monkeypatch.setenv("EMAGLS_SWEEP_REG", "2")
    monkeypatch.setenv("EMAGLS_REG_WAVES", str(nw))
    clear_cache()
    try:
        d = run_design(L.KIND_EMAGLS2, N, 0.042, directions(901), mics)
    finally:
        monkeypatch.delenv("EMAGLS_REG_WAVES")
        monkeypatch.delenv("EMAGLS_SWEEP_REG")
        clear_cache()
    assert d["sweep_form"] == 3 and d["sweep_units"] == nunits
    label = f"register form, {nunits} units, {nw} waves"
    check_steps(label, d, operands(("r042", nunits, 901), d))
    if nw == 4:
        check_around(label, d)


def edge_counts(nw):
    return (SMALLEST_D, 32 * nw - 1, 32 * nw, 32 * nw + 1, 32 * nw + 33, 32 * nw + 53)


@pytest.mark.parametrize("nw,D", [(nw, D) for nw in (4, 8) for D in edge_counts(nw)])
def test_register_resident_step_direction_count_edges(scenes, operands, monkeypatch, nw, D):
    """sweep_reg_kernel at the direction counts where its tails change, 12 microphones without a pair at the order-5 radius (36
    simulated channels), four and eight waves: the smallest count the plan accepts (36: the orthonormal route of the low bins factors
    S_h = 36 columns of the grid's SH matrix, and 35 directions are refused), a workgroup less one, full, plus one, a second workgroup
    whose second wave holds one direction (32 nw + 33), and 32 nw + 53: the second wave full in its first half, five of the sixteen
    quads' second directions present -- the last quad in use half filled."""
    from emagls_amd import _lib as L
    directions, microphones = scenes
    mics = microphones(12)
    monkeypatch.setenv("EMAGLS_SWEEP_REG", "2")
    monkeypatch.setenv("EMAGLS_REG_WAVES", str(nw))
    clear_cache()
    try:
        d = run_design(L.KIND_EMAGLS2, FCUT_ORDER, radius_of(5), directions(D), mics)
    finally:
        monkeypatch.delenv("EMAGLS_REG_WAVES")
        monkeypatch.delenv("EMAGLS_SWEEP_REG")
        clear_cache()
    assert d["sweep_form"] == 3 and d["sweep_units"] == 12 and d["sim_order"] == 5
    label = f"register form, {D} directions, {nw} waves"
    check_steps(label, d, operands(("order5", 12, D), d))
    check_around(label, d)


def test_smallest_direction_count_is_the_smallest(scenes):
    from emagls_amd import _lib as L
    directions, microphones = scenes
    with pytest.raises(L.EmaglsError):
        p = make_plan(L.KIND_EMAGLS2, FCUT_ORDER, radius_of(5), directions(SMALLEST_D - 1), microphones(12))
        try:
            p.execute()
            p.synchronize()
        finally:
            p.close()


# directions per workgroup of sweep_synth_kernel (persist_sweep_dpw of sweep_persist.hip): 64 up to 2048 directions, 96 above
SLAB_COUNTS = (64, 65, 901)


@pytest.mark.parametrize("nmics,D", [(m, D) for m in (7, 12, 32) for D in SLAB_COUNTS] + [(12, 2049)])
def test_slab_step(scenes, operands, monkeypatch, nmics, D):
    """sweep_synth_kernel (EMAGLS_SWEEP_REG=0) with 8-, 16- and 32-row slabs (7, 12 and 32 microphones) on one tile of 64 directions,
    one direction more, and 901; and the 96-direction tile of grids above 2048 directions at its smallest count, 2049 = 21 x 96 + 33.
    At 64 and 65 directions the arrays of 12 and 32 microphones stand at the order-5 radius, where the orthonormal route of the low
    bins needs 36 directions (at 4.2 cm it needs more than 65), with f_cut at 7.5 kHz as in the direction-count cases."""
    from emagls_amd import _lib as L
    directions, microphones = scenes
    mics = microphones(17 if nmics == 32 else nmics)
    small = D < 100 and nmics > 7
    N, radius = (FCUT_ORDER, radius_of(5)) if small else (2 if nmics < 16 else 4, 0.042)
    monkeypatch.setenv("EMAGLS_SWEEP_REG", "0")
    clear_cache()
    try:
        d = run_design(L.KIND_EMAGLS2, N, radius, directions(D), mics)
    finally:
        monkeypatch.delenv("EMAGLS_SWEEP_REG")
        clear_cache()
    assert d["sweep_form"] == 2 and d["M"] == nmics
    label = f"slab form, {nmics} microphones, {D} directions"
    check_steps(label, d, operands(("order5" if small else "r042", d["sweep_units"], D), d))
    check_around(label, d)


@pytest.mark.parametrize("reg", ["0", "2"])
def test_sh_domain_design_step(scenes, operands, monkeypatch, reg):
    """eMagLS, order 4, em32, real basis: Pm = pinv(Y_lo) is a full 25 x 32 matrix, so Mt = Pm^T M Pm and the rows (u Pm^T) conj(M) of
    synth_mt_kernel / synth_rows_kernel do arithmetic (for raw microphones Pm is a permutation); both forms on 901 directions."""
    from emagls_amd import _lib as L
    directions, microphones = scenes
    monkeypatch.setenv("EMAGLS_SWEEP_REG", reg)
    clear_cache()
    try:
        d = run_design(L.KIND_EMAGLS, 4, 0.042, directions(901), microphones(17))
    finally:
        monkeypatch.delenv("EMAGLS_SWEEP_REG")
        clear_cache()
    assert d["sweep_form"] == (3 if reg == "2" else 2) and d["C"] == 25 and d["M"] == 32
    assert np.count_nonzero(d["Pm"]) > 25 * 16
    label = f"SH-domain design, form {d['sweep_form']}"
    check_steps(label, d, operands(("r042-sh", 17, 901), d))
    check_around(label, d)


def test_top_order_step(scenes, operands):
    """simulation order 85 (rows of 86 terms), the em32 on 901 directions, in the form the plan reports: three bins"""
    from emagls_amd import _lib as L
    directions, microphones = scenes
    r = radius_of(TOP_ORDER)
    assert L.load().emagls_simulation_order(L.KIND_EMAGLS2, 4, R.FS, r) == TOP_ORDER
    probe = make_plan(L.KIND_EMAGLS2, 4, r, directions(901), microphones(17))
    i = probe.info()
    kfirst = max(min(i.k_cut - 1, i.num_pos_freqs), 1)
    probe.close()
    d = run_design(L.KIND_EMAGLS2, 4, r, directions(901), microphones(17), bins=[kfirst, 64, R.NBINS - 1])
    assert d["sweep_form"] in (2, 3) and d["sim_order"] == TOP_ORDER and len(d["bins"]) == 3
    label = f"order {TOP_ORDER}"
    check_steps(label, d, operands(("top", 17, 901), d))
    check_around(label, d)


@pytest.fixture(scope="module")
def batch_geometries(grids, thin):
    """ten designs on 901 directions as tests/test_gpu_sweep_forms.py makes them: grid and array turned, HRIRs of their own"""
    from emagls_amd import synth
    geo = []
    for j in range(10):
        azi = np.mod(thin["azi"] + 0.17 * j, 2 * np.pi)
        hL, hR = synth.rigid_sphere_hrirs(azi, thin["zen"], seed=31 + j)
        geo.append(((azi, thin["zen"], hL, hR), (np.mod(grids["mic_azi"] + 0.1 * j, 2 * np.pi), grids["mic_zen"])))
    return geo


@pytest.mark.parametrize("spread", ["0", "1"])
def test_step_in_a_launch_of_many_designs(batch_geometries, operands, monkeypatch, spread):
    """A batch of 10 designs (two per XCD slot; EMAGLS_REG_SPREAD 0: every design inside one XCD, 1: dealt over all eight) runs the
    register-resident form in one launch; the step check on the buffers of designs 0, 8 and 9."""
    from emagls_amd import Batch, _lib as L
    lib = L.load()
    monkeypatch.setenv("EMAGLS_REG_SPREAD", spread)
    geo = batch_geometries
    plans = [make_plan(L.KIND_EMAGLS2, 4, 0.042, scene, mics) for scene, mics in geo]
    prev = C.c_int(0)
    L.check(lib.emagls_set_batch_max(16, C.byref(prev)))
    try:
        b = Batch(plans)
    finally:
        L.check(lib.emagls_set_batch_max(prev.value, None))
    try:
        b.execute()
        b.synchronize()
        assert plans[0].info().sweep_form == 3
        for j in (0, 8, 9):
            d = read_design(plans[j], *geo[j])
            check_steps(f"batch of 10, spread {spread}, design {j}", d, operands(("batch", j), d))
    finally:
        b.close()
        for p in plans:
            p.close()
