"""Job lists share one geometry's stages without being asked and keep them between runs (include/emagls.h: emagls_jobs_run,
emagls_batch_geometry_runs).  The shapes are those of the sharing tests of test_gpu_batches.py: the thinned
grid (901 of the 2702 directions), 128 taps, em32 at order 4 on the complex basis; 20 designs with their own HRIR sets, so that the
chunk is on the register-resident sweep.  Bounds: 1e-9 shared against unshared and 2e-7 against single designs, as
test_gpu_batches.py sets them for the same shapes."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 20
TOL_SINGLE, TOL_UNSHARED = 2e-7, 1e-9


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


def hrir_sets(thin, n, seed):
    rng = np.random.default_rng(seed)
    return [(thin["hL"] * (1.0 + 0.03 * j) + 1e-3 * rng.standard_normal(thin["hL"].shape),
             thin["hR"] * (1.0 - 0.02 * j) + 1e-3 * rng.standard_normal(thin["hR"].shape)) for j in range(n)]


def single(thin, grids, hL, hR, mic_azi=None, radius=None):
    import emagls_amd as E
    return E.getEMagLsFilters(hL, hR, thin["azi"], thin["zen"], grids["mic_radius"] if radius is None else radius,
                              grids["mic_azi"] if mic_azi is None else mic_azi, grids["mic_zen"], 4, 48000.0, 128, "complex")


@pytest.fixture(scope="module")
def sets(thin):
    return hrir_sets(thin, N, 77)


@pytest.fixture(scope="module")
def singles(thin, grids, sets):
    """Designs 0, 7 and 19 as single calls: computed once, read by every test that needs them."""
    return {j: single(thin, grids, *sets[j]) for j in (0, 7, 19)}


def job_list(thin, grids, sets, repeat=1, **kw):
    from emagls_amd import _lib as L
    from emagls_amd.jobs import JobList
    jl = JobList()
    for _ in range(repeat):
        for hL, hR in sets:
            jl.add(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, hL, hR, thin["azi"], thin["zen"], mic_radius=kw.get("radius", grids["mic_radius"]),
                   mic_azi=grids["mic_azi"], mic_zen=grids["mic_zen"], out_shape=(128, 25, True))
    return jl


def snapshot(jl):
    return [(a.copy(), b.copy()) for a, b in jl.results()]


def clear():
    from emagls_amd import _lib as L
    L.check(L.load().emagls_cache_clear())


def test_a_job_list_shares_its_geometry_without_being_asked(thin, grids, sets, singles):
    """JobList.run() with default arguments, four times (eager, capture, replay, replay): no chunk runs as independent designs, the
    first run is the cold form and the others the warm one, every run returns the bits of the first; against the same list run as
    independent designs 1e-9, against single designs 2e-7."""
    from emagls_amd.jobs import JobList
    clear()
    jl = job_list(thin, grids, sets)
    outs = []
    for _ in range(4):
        jl.run()
        outs.append(snapshot(jl))
    ind, cold, warm = JobList.geometry_runs()
    print(f"four default runs of a 20-design list: {ind} independent, {cold} cold, {warm} warm chunk executes")
    assert ind == 0 and cold >= 1 and warm >= 2
    for it in (1, 2, 3):
        assert all(same(a, c) for a, c in zip(outs[0], outs[it])), f"run {it} differs from the first"
    jl.run(share_geometry=False)
    indep = snapshot(jl)
    assert JobList.geometry_runs()[0] == 1
    w_i = max(worst(a, c) for a, c in zip(outs[0], indep))
    w_s = max(worst(outs[0][j], w) for j, w in singles.items())
    print(f"shared vs the same list as independent designs {w_i:.3e}; vs single designs {w_s:.3e}")
    assert w_i <= TOL_UNSHARED and w_s <= TOL_SINGLE
    clear()


def test_warm_runs_follow_their_hrirs(thin, grids, sets):
    """New HRIR arrays for designs 0, 5 and 19 of a resident, warm chunk: the next run is still a warm one, those three designs equal
    fresh single calls on the new HRIRs, the others keep their bits."""
    from emagls_amd.jobs import JobList
    clear()
    jl = job_list(thin, grids, sets)
    jl.run()
    jl.run()
    before = snapshot(jl)
    counts = JobList.geometry_runs()
    fresh = hrir_sets(thin, 3, 991)
    for (hL, hR), j in zip(fresh, (0, 5, 19)):
        jl.replace(j, hL=hL * 1.1, hR=hR * 0.9)
    jl.run()
    after = snapshot(jl)
    now = JobList.geometry_runs()
    assert now == (counts[0], counts[1], counts[2] + 1), (counts, now)
    w = 0.0
    for (hL, hR), j in zip(fresh, (0, 5, 19)):
        w = max(w, worst(after[j], single(thin, grids, hL * 1.1, hR * 0.9)))
        assert not same(after[j], before[j])
    print(f"three designs of a warm chunk on new HRIRs vs single calls: {w:.3e}")
    assert w <= TOL_SINGLE
    for j in range(N):
        if j not in (0, 5, 19):
            assert same(after[j], before[j]), f"design {j} changed although its HRIRs did not"
    clear()


def test_a_geometry_change_goes_cold_and_is_right(thin, grids, sets):
    """A new microphone grid for every job: the next run is a cold one and designs 0 and 19 match single calls on the new array.  Then
    a different grid for ONE job: the chunk runs as independent designs and that job matches its single call."""
    from emagls_amd.jobs import JobList
    clear()
    jl = job_list(thin, grids, sets)
    jl.run()
    jl.run()
    counts = JobList.geometry_runs()
    assert counts[0] == 0 and counts[2] >= 1
    maz = grids["mic_azi"] + 0.11
    for j in range(N):
        jl.replace(j, mic_azi=maz)
    jl.run()
    res = snapshot(jl)
    now = JobList.geometry_runs()
    assert now == (counts[0], counts[1] + 1, counts[2]), (counts, now)
    w = max(worst(res[j], single(thin, grids, *sets[j], mic_azi=maz)) for j in (0, 19))
    print(f"all jobs on a shifted array (cold run) vs single calls: {w:.3e}")
    assert w <= TOL_SINGLE
    maz2 = grids["mic_azi"] + 0.23
    jl.replace(4, mic_azi=maz2)
    jl.run()
    res2 = snapshot(jl)
    assert JobList.geometry_runs() == (now[0] + 1, now[1], now[2])
    w2 = worst(res2[4], single(thin, grids, *sets[4], mic_azi=maz2))
    print(f"one job on an array of its own (independent run) vs its single call: {w2:.3e}")
    assert w2 <= TOL_SINGLE and worst(res2[0], res[0]) <= TOL_UNSHARED
    clear()


def test_a_mixed_chunk_is_not_shared(thin, grids, sets):
    """Six designs of one padded simulation-order class, one of them on its own radius: one chunk (the shape is the same), run as
    independent designs, equal to the single calls."""
    from emagls_amd import _lib as L
    from emagls_amd.jobs import JobList
    clear()
    jl = JobList()
    radii = [grids["mic_radius"]] * 6
    radii[3] = grids["mic_radius"] + 1e-4
    for (hL, hR), r in zip(sets[:6], radii):
        jl.add(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, hL, hR, thin["azi"], thin["zen"], mic_radius=r, mic_azi=grids["mic_azi"],
               mic_zen=grids["mic_zen"], sim_order_pad=21, out_shape=(128, 25, True))
    assert not jl.would_share_geometry()
    jl.run()
    assert JobList.geometry_runs() == (1, 0, 0)
    res = jl.results()
    w = max(worst(res[j], single(thin, grids, *sets[j], radius=radii[j])) for j in (0, 3, 5))
    print(f"a chunk with one radius of its own, independent designs vs single calls: {w:.3e}")
    assert w <= TOL_SINGLE
    clear()


def test_a_sharing_batch_keeps_its_geometry(thin, grids, sets):
    """Batch level: 6 plans, share_geometry(True), three executes -- one cold and two warm, the three outputs bit-equal for every plan
    (plan 0 included); switching the batch's profiling on between executes 2 and 3 does not make execute 3 a cold one."""
    from emagls_amd import Batch, Plan, _lib as L
    plans = []
    for hL, hR in sets[:6]:
        p = Plan(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, hL.shape[0], hL.shape[1], grids["mic_radius"], 32)
        p.set_hrir_grid(thin["azi"], thin["zen"])
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
        p.set_hrirs(hL, hR)
        plans.append(p)
    b = Batch(plans)
    assert b.geometry_runs() == (0, 0)
    b.share_geometry(True)
    outs = []
    for it in range(3):
        if it == 2:
            b.set_profiling(1)
        b.execute()
        assert b.shares_geometry()
        outs.append(b.get_filters())
    assert b.geometry_runs() == (1, 2)
    for it in (1, 2):
        for j, (a, c) in enumerate(zip(outs[0], outs[it])):
            assert same(a, c), f"execute {it}, plan {j}"
    # a plan run on its own rewrites its copies of the factors: the next execute is a cold one again
    plans[2].execute()
    b.execute()
    b.get_filters()
    assert b.geometry_runs() == (2, 2)
    b.close()
    for p in plans:
        p.close()


def test_lone_chunk_and_four_in_flight_agree(thin, grids, sets):
    """The same 20 designs as a list of ONE chunk (the device to itself) and as four chunks in flight (80 jobs): bit-equal design for
    design in both placements, cold and warm; no run waits for anything (1.5 s, as in test_sweep_gate_counts_launches_until_they_finish)."""
    clear()

    def timed(jl, **kw):
        t0 = time.perf_counter()
        jl.run(**kw)
        dt = time.perf_counter() - t0
        assert dt < 1.5, f"a run took {dt:.2f} s"
        return snapshot(jl)
    lone = job_list(thin, grids, sets)
    four = job_list(thin, grids, sets, repeat=4)
    lone_runs = [timed(lone), timed(lone)]
    four_runs = [timed(four, batch_size=N, in_flight=4), timed(four, batch_size=N, in_flight=4)]
    for r in (0, 1):
        for k in range(4 * N):
            assert same(four_runs[r][k], lone_runs[r][k % N]), f"run {r}, job {k}"
    clear()
