"""One bin step of the operand-fed sweeps -- sweep_dense_kernel, sweep_half_kernel (sweep.hip), sweep_wide_kernel,
sweep_wide_loop_kernel (wide.hip), their finalize kernels and sweep_persist_kernel (sweep_persist.hip) -- against a longdouble step on
the same inputs, bin by bin.

An executed plan keeps every row W(k,:) (workgroup 0 publishes row kb - 1 in each launch, finalize writes the last one), |H| and the
operands of its form: Xc / Ypinv (MagLS, launch per bin), Gm / Mw (MagLS, persistent), G / Yri / Mw / cond_ok (array designs), X / Z
(FromAtf).  No stage after the sweep writes to any of them (plan_setup.hip gives every name its own memory; the epilogue reads W) but
one: a complex-basis eMagLS design on the real-arithmetic pipeline turns its rows into the complex basis in place
(launch_sh_rows_to_complex), so the complex-basis array cases run on the complex-arithmetic pipeline (EMAGLS_REAL_INTERNAL=0), whose rows
stay as the sweep wrote them.  For EVERY swept bin, the first one (the start row), the Nyquist bin and finalize's row included, W(k,:) is
held to tests/sweep_reference.py's step from the kernel's own W(k-1,:): element by element within the a-priori bound, and row by row
within 8 x max(e, C eps ||row||), e the error of an FP64 NumPy step on the same inputs; MagLS rows below the cut to ls_rows.  The cases
(sweep_reference.CASES) are the smallest shapes that reach the kernels' branches; tests/test_sweep_reference_host.py holds their shapes
to the kernels' constants and host-made inputs of the same shapes to the bounds.  Filters of the shortest length the plans accept that
leaves eight swept bins and, for MagLS, a complex start row (sweep_reference.shortest_length: 8 to 26 taps)."""
import numpy as np
import pytest

import sweep_reference as S
import synth_reference as R

pytestmark = pytest.mark.gpu


def clear_cache():
    from emagls_amd import _lib as L
    L.check(L.load().emagls_cache_clear())


def make_plan(c):
    from emagls_amd import Plan, _lib as L
    azi, zen, hL, hR = S.scene(c)
    n = S.length_of(c)
    if c["kind"] == "atf":
        atf, aazi, azen = S.atf_set(c)
        p = Plan(L.KIND_FROM_ATF, "real", 0, S.FS, n, n, c["D"], nmics=c["nmics"], f_trans=2000.0, atf_taps=atf.shape[0], natf=atf.shape[2])
        p.set_hrir_grid(azi, zen)
        p.set_hrirs(hL, hR)
        p.set_atfs(atf, aazi, azen)
        return p
    kind = {"magls": L.KIND_MAGLS, "emagls": L.KIND_EMAGLS, "emagls2": L.KIND_EMAGLS2}[c["kind"]]
    p = Plan(kind, c["basis"], c["order"], S.FS, n, n, c["D"], c["radius"], c["nmics"])
    p.set_hrir_grid(azi, zen)
    if c["kind"] != "magls":
        p.set_mic_grid(*S.microphones(c))
    p.set_hrirs(hL, hR)
    return p


def kernel_of(c, form, Cn, D, launches, nswept):
    """the sweep kernel a plan of this kind, form (emagls_plan_info.sweep_form), channel and direction count runs (plan_run.hip)"""
    if form == 1:
        assert launches == 1 and Cn <= 32 and D <= 3072
        return "persist"
    assert form == 0 and launches == nswept, (form, launches, nswept)
    if Cn > 64:
        return "loop"
    if Cn > 32:
        return "wide"
    if c["kind"] == "magls" or (c["kind"] == "atf" and Cn <= 8 and D <= 768):
        return "dense"
    return "half"


def run_case(c, monkeypatch):
    """create, execute, read: the rows, |H| and the operands of every swept bin in the layouts of plan_setup.hip / plan_run.hip"""
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    clear_cache()
    try:
        p = make_plan(c)
        try:
            p.execute()
            p.synchronize()
            i = p.info()
            P, Cn, D = i.num_pos_freqs, i.num_channels, c["D"]
            kcut0 = min(i.k_cut - 1, P)
            k0 = max(kcut0, 1)
            assert (P, kcut0, k0) == S.bins_of(S.length_of(c), S.cut_of(c["kind"], c["order"], 2000.0))
            na, n_c = max(P - kcut0, 1), max(min(kcut0, P), 1)
            habs = p.debug("Habs", np.float64)
            ldD = habs.size // (2 * na)
            assert habs.size == 2 * na * ldD and ldD == -(-D // 64) * 64, (habs.size, na, D)     # the direction count the plan was made for
            assert kernel_of(c, i.sweep_form, Cn, D, i.num_sweep_launches, P - k0) == c["kernel"] and i.sweep_form == c["form"]
            d = dict(P=P, C=Cn, D=D, kcut0=kcut0, k0=k0, Habs=habs.reshape(2, na, ldD)[:, :, :D].copy(),
                     W=p.debug("W", np.complex128)[:2 * P * Cn].reshape(2, P, Cn).copy())
            mat = lambda name, dt, rows: p.debug(name, dt)[:rows * ldD].reshape(rows, ldD)[:, :D].copy()
            half = c["kernel"] in ("half", "persist")
            if half:
                d["M"] = p.debug("Mw", np.complex128)[:P * Cn * Cn].reshape(P, Cn, Cn).copy()          # bin k at slot k - 1
                d["ok"] = p.debug("cond_ok", np.float64)[:P].copy()
            if c["kind"] == "magls":
                dt = np.complex128 if c["basis"] == "complex" else np.float64
                Z = mat("Ypinv", dt, Cn)
                d["Hc"], d["Zfix"] = p.debug("Hc", np.complex128)[:2 * n_c * ldD].reshape(2, n_c, ldD)[:, :kcut0, :D].copy(), Z
                if half:
                    G = mat("Gm", np.complex128, Cn)
                    d["ops"] = lambda k: (G, d["M"][k - 1], None)
                else:
                    X = mat("Xc", dt, Cn)
                    d["ops"] = lambda k: (X, Z)
            elif c["kind"] == "atf":
                X, Z = mat("X", np.complex128, P * Cn).reshape(P, Cn, D), mat("Z", np.complex128, P * Cn).reshape(P, Cn, D)
                d["ops"] = lambda k: (X[k], Z[k])
            elif half:
                g0, hh_end = i.g_first, i.hh_end
                G = mat("G", np.complex128, (P - g0) * Cn).reshape(P - g0, Cn, D)
                Y = mat("Yri", np.complex128, max(hh_end - k0, 1) * Cn).reshape(-1, Cn, D)               # bins k0 .. hh_end - 1
                d["ops"] = lambda k: (G[k - g0], d["M"][k - 1], None if d["ok"][k] != 0 else Y[k - k0])
                assert np.all(d["ok"][hh_end:] == 1)
            else:   # the 33..64-channel array path: G_k and Y_reg_inv_k of the bins 1 .. P - 1
                G, Y = (mat(nm, np.complex128, (P - 1) * Cn).reshape(P - 1, Cn, D) for nm in ("G", "Yri"))
                d["ops"] = lambda k: (G[k - 1], Y[k - 1])
            return d
        finally:
            p.close()
    finally:
        for k in c["env"]:
            monkeypatch.delenv(k)
        clear_cache()


def check_case(c, d):
    P, k0, kcut0 = d["P"], d["k0"], d["kcut0"]
    half = c["kernel"] in ("half", "persist")
    assert np.all(np.isfinite(d["W"].view(np.float64)))
    worst = dict(bound=(0.0, None), sharp=(0.0, None), over_e=(0.0, None))
    r_max, flagged, missed = 0.0, 0, []
    for k in range(k0, P):
        w_prev, habs, nyq = d["W"][:, k - 1], d["Habs"][:, k - kcut0], k == P - 1
        if half:
            G, M, yri = d["ops"](k)
            step = S.half_step(w_prev, habs, G, M, yri, nyq)
            bound, r = S.bound_half(w_prev, habs, G, M, step[1], step[3], yri)
            w64 = S.half_step64(w_prev, habs, G, M, yri, nyq)
            flagged += yri is not None
        else:
            X, Z = d["ops"](k)
            step = S.operand_step(w_prev, habs, X, Z, nyq)
            bound, r = S.bound_operand(w_prev, habs, X, Z, step[1])
            w64 = S.operand_step64(w_prev, habs, X, Z, nyq)
        assert np.abs(step[0]).max() > 0 and (nyq or np.abs(d["W"][:, k].imag).max() > 0)     # (not a chain that stayed real)
        if nyq:
            assert np.all(step[2].imag == 0)
        ratios = S.check_step(d["W"][:, k], step, bound, w64)
        r_max = max(r_max, float(r.max()))
        for key, v in zip(("bound", "sharp", "over_e"), ratios):
            if v >= worst[key][0]:
                worst[key] = (v, k)
        if ratios[0] > 1.0 or ratios[1] > 1.0:
            missed.append((k,) + tuple(float(v) for v in ratios))
    print(f"{c['name']}: {c['kernel']} form, {d['C']} channels, {d['D']} directions, bins {k0} .. {P - 1} ({flagged} on the accurate slab): "
          f"largest |W(k,:) - longdouble step| / bound {worst['bound'][0]:.3e} (bin {worst['bound'][1]}), "
          f"row error / (8 max(e, C eps ||row||)) {worst['sharp'][0]:.3e} (bin {worst['sharp'][1]}), "
          f"row error / e {worst['over_e'][0]:.3e} (bin {worst['over_e'][1]}); max dp / |p| {r_max:.3e}")
    assert not missed, (c["name"], "(bin, error / bound, row error / sharp limit, row error / e):", missed)
    assert r_max < S.R_LIMIT
    if c["note"] == "cond_ok":
        assert flagged >= 1, "no swept bin of this design is flagged ill-conditioned: the accurate slab is not reached"
    if c["kind"] == "magls":    # the start value of the chain: the least-squares rows below the cut
        assert kcut0 >= 1
        for e in range(2):
            ref = S.ls_rows(d["Hc"][e], d["Zfix"])
            ratio = float(S.step_ratio(d["W"][e, :kcut0], ref, S.bound_ls(d["Hc"][e], d["Zfix"])).max())
            w64 = np.asarray(d["Hc"][e]) @ np.asarray(d["Zfix"]).astype(np.complex128).T
            err, e64 = S.row_errors(d["W"][e, :kcut0], ref), S.row_errors(w64, ref)
            sharp = float((err / S.sharp_limit(e64, ref)).max())
            print(f"{c['name']}: least-squares rows 0 .. {kcut0 - 1}, ear {e}: error / bound {ratio:.3e}, row error / (8 max(e, C eps ||row||)) {sharp:.3e}")
            assert ratio <= 1.0 and sharp <= 1.0 and np.abs(ref).max() > 0


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_operand_fed_sweep_step(monkeypatch, name):
    R.require_longdouble()
    c = S.CASE[name]
    check_case(c, run_case(c, monkeypatch))


@pytest.mark.parametrize("key", sorted(S.SMALLEST_D))
def test_smallest_direction_counts_are_the_smallest(monkeypatch, key):
    """one direction fewer than the smallest cases and the plan is refused, at creation or by its conditioning certificate"""
    from emagls_amd import _lib as L
    kind, order = key
    c = dict(next(k for k in S.CASES if k["kind"] == kind and k["order"] == order and k["D"] == S.SMALLEST_D[key] and k["basis"] == "real"))
    c["D"] -= 1
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    with pytest.raises(L.EmaglsError):
        p = make_plan(c)
        try:
            p.execute()
            p.synchronize()
        finally:
            p.close()
