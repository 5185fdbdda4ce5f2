"""Captured graphs of plans and batches over their whole life: captured, replayed, dropped (emagls_plan_set_streams), captured
again, and destroyed with their owner in either order of batch and plans.  A graph that outlived a drop would replay old work or
old addresses; one destroyed twice, or a batch touching a plan that is gone, would bring the process down.  Thinned grid, N = 4,
128 taps, as tests/test_gpu_batches.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def thin(grids, hrirs):
    sub = slice(0, 2702, 3)
    return dict(hL=hrirs[0][:, sub], hR=hrirs[1][:, sub], azi=grids["azi"][sub], zen=grids["zen"][sub])


def make_plan(grids, thin, kind="emagls", radius=0.042, gain=1.0):
    from emagls_amd import Plan, _lib as L
    hL, hR = thin["hL"] * gain, thin["hR"]
    if kind == "ls":
        p = Plan(L.KIND_LS, "real", 4, 48000.0, 128, hL.shape[0], hL.shape[1])
        p.set_hrir_grid(thin["azi"], thin["zen"])
    else:
        p = Plan(L.KIND_EMAGLS, "complex", 4, 48000.0, 128, hL.shape[0], hL.shape[1], radius, 32)
        p.set_hrir_grid(thin["azi"], thin["zen"])
        p.set_mic_grid(grids["mic_azi"], grids["mic_zen"])
    p.set_hrirs(hL, hR)
    return p


# emagls: the stages before the resident sweep are the captured part; ls: the whole design is one graph
@pytest.mark.parametrize("kind", ["emagls", "ls"])
def test_plan_recaptures_after_its_graphs_were_dropped(grids, thin, kind):
    p = make_plan(grids, thin, kind)
    runs = []
    for it in range(3):   # eager, captured, replayed
        p.execute()
        runs.append(p.get_filters())
    p.set_streams(1)      # the same stream count: the graphs are dropped, the next execute is eager again
    for it in range(3):
        p.execute()
        runs.append(p.get_filters())
    p.close()
    for it, (wL, wR) in enumerate(runs):
        assert np.array_equal(wL, runs[0][0]) and np.array_equal(wR, runs[0][1]), it
    assert np.isfinite(runs[0][0]).all() and np.abs(runs[0][0]).max() > 0


# what the batch holds when it goes: "streams": two simulation orders, so only each plan's own graph of the stages before the sweep;
# "lanes": one radius, two HRIR sets -- the lane group's graph and the one of the stages after the sweep; "geo": the same with
# geometry sharing -- the cold form's, the warm form's and the graph of the stages after the sweep
@pytest.mark.parametrize("first", ["batch", "plan"])
@pytest.mark.parametrize("form", ["streams", "lanes", "geo"])
def test_batch_and_plans_destroyed_in_either_order(grids, thin, form, first):
    from emagls_amd import Batch
    jobs = [(0.042, 1.0), (0.040 if form == "streams" else 0.042, 1.1)]
    singles = []
    for r, g in jobs:
        q = make_plan(grids, thin, radius=r, gain=g)
        q.execute()
        singles.append(q.get_filters())
        q.close()
    assert rel(singles[0][0], singles[1][0]) > 1e-3
    plans = [make_plan(grids, thin, radius=r, gain=g) for r, g in jobs]
    b = Batch(plans)
    if form == "geo":
        b.share_geometry(True)

    def run(n):
        for it in range(n):   # after a drop: eager, captured, replayed
            b.execute()
            for (wL, wR), (sL, sR) in zip(b.get_filters(), singles):
                assert rel(wL, sL) < 1e-12 and rel(wR, sR) < 1e-12, it
    run(3)
    assert b.lane_mode() == (form != "streams")
    if form == "geo":
        assert b.shares_geometry() and b.geometry_runs()[1] >= 1
    if form == "lanes":   # live graphs dropped (forked stages run eagerly), then captured again on one stream
        b.set_streams(2)
        run(1)
        b.set_streams(1)
        run(2)
    if first == "batch":  # the batch goes with its graphs alive
        b.close()
    else:                 # a plan goes before its batch: the batch forgets it and is destroyed without touching it
        plans[0].close()
        b.close()
    p = plans[1]          # a surviving plan, on its own again
    for it in range(3):
        p.execute()
        wL, wR = p.get_filters()
        assert rel(wL, singles[1][0]) < 1e-12 and rel(wR, singles[1][1]) < 1e-12, it
    for q in plans:
        q.close()
