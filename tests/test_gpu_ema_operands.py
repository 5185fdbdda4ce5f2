"""The operand chain of getEMagLsFiltersEMAinSH and getEMagLsFiltersEMAinCH, stage by stage -- ch_basis_kernel and the CH_PINV branch of array_encoder,
ema_sh_e0_kernel, rot_points_kernel, rot_from_points_kernel / rot_blocks_from_points_kernel, qt_rotate_kernel (both rotate_block forms), launch_qt
and launch_dspace_g as these designs call them -- on the cases of tests/ema_reference.py.  Plans run with set_profiling(1) and the named buffers
are read through Plan.debug.  Every step is held to the reference applied to the device output of the step before it, within that step's
a-priori bound or 8 x its measured level; Rot, E0 and G_k (bin 1, the bins around k_cut, P/2, P-1, as far as the plan materialises them) once
more to the multiprecision truth of the whole chain within the composed bound (EMAinCH: Y of the grid and G_k).  QT is rotated in place: it is checked as the composed step
from the device's own Yc, E and Rot.  On the horizon (zen == pi/2 exactly) Rot_d is the identity bit for bit; its two neighbouring doubles take
the fitted path.  Every case prints its largest error / bound; with EMAGLS_EMA_REPORT=<file> the module writes them there
(profiles/r26_ema_operands.md is such a file).

ch_basis_kernel's own output is consumed by the factorisation behind pinv(CH); the kernel is held on its own through a MagLS-2D plan, whose Ycm
is that kernel's output on the same azimuths.  Paddings: the plan allocates E, Ech, Yc, Ycm and QT zero-filled and their kernels write inside
the live shape only, which is asserted; the pad columns of Zlo and Zb belong to the factorisation's workspace and those of G are never
initialised -- no reader goes there, and nothing is specified about them."""
import os

import numpy as np
import pytest

import ema_reference as E
import gram_reference as G

pytestmark = pytest.mark.gpu

REPORT = []     # (case, measure, value)


@pytest.fixture(scope="module", autouse=True)
def report_file():
    yield
    path = os.environ.get("EMAGLS_EMA_REPORT")
    if not path or not REPORT:
        return
    with open(path, "w") as f:
        f.write("| case | measure | value |\n|---|---|---|\n")
        for row in REPORT:
            f.write("| %s | %s | %s |\n" % row)


def note(case, what, value):
    text = value if isinstance(value, str) else "%.3g" % value
    REPORT.append((case, what, text))
    print("%-6s %-58s %s" % (case, what, text))


def held(case, what, ratio, fails):
    """a largest error / bound: printed, recorded, and a failure above 1"""
    note(case, what + ", largest error / bound", ratio)
    if not ratio <= 1.0:
        fails.append("%s: %s %.3g" % (case, what, ratio))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def run_plan(c, monkeypatch):
    """the case's plan, executed twice: its buffers after the second execute, Rot and G after the first"""
    from emagls_amd import Plan, synth, _lib as L
    if c["kind"] == "ch" and not c["cplx"]:
        monkeypatch.setenv("EMAGLS_SWEEP_SYNTH", "0")     # materialised operands: the synthesising sweep forms neither QT nor G
    hL, hR = synth.rigid_sphere_hrirs(c["azi"], c["zen"], fs=E.FS, taps=c["length"], centre_delay=c["length"] / 3.0)
    dt = np.complex128 if c["cplx"] else np.float64
    p = Plan(L.KIND_EMA_SH if c["kind"] == "sh" else L.KIND_EMA_CH, "complex" if c["cplx"] else "real", c["N"], E.FS, c["length"], c["length"], c["D"],
             c["radius"], c["M"])
    try:
        p.set_hrir_grid(c["azi"], c["zen"])
        p.set_mic_grid(c["mic_azi"])
        p.set_hrirs(hL, hR)
        p.set_profiling(1)
        first = {}
        for it in range(2):
            try:
                p.execute()
                p.synchronize()
            except L.EmaglsError as e:
                if e.code == L.ERR_HIP:
                    pytest.exit("HIP error in a plan: %s" % e, returncode=3)     # nothing more is started on a device that has faulted
                raise
            if it == 0:
                first["G"] = p.debug("G", np.complex128)
                if c["kind"] == "sh":
                    first["Rot"] = p.debug("Rot", dt)
        i = p.info()
        out = dict(first=first, info=dict(P=i.num_pos_freqs, k_cut=i.k_cut, sim=i.sim_order, S=i.num_sh_sim, C=i.num_channels, g0=i.g_first, form=i.sweep_form))
        names = [("mic_azi", np.float64), ("Ymic_rm", dt), ("Zlo", np.complex128), ("E", dt), ("kr", np.float64), ("bn", np.complex128), ("Ycm", dt), ("Yc", dt),
                 ("QT", dt), ("G", np.complex128)]
        if c["kind"] == "sh":
            names += [("Ech", dt), ("Ypts", dt), ("rot_azi", np.float64), ("rot_zen", np.float64), ("Arot", dt), ("Zb", np.complex128), ("Rot", dt)]
        for name, t in names:
            out[name] = p.debug(name, t)
        wL, wR = p.get_filters()
        assert np.all(np.isfinite(wL)) and np.all(np.isfinite(wR))
        return out
    finally:
        p.close()


@pytest.mark.parametrize("name", list(E.CASES))
def test_operand_chain(name, monkeypatch):
    E.require_longdouble()
    c = E.case(name)
    N, cplx, M, S, nOrd, C, P, D = c["N"], c["cplx"], c["M"], c["S"], c["nOrd"], c["C"], c["P"], c["D"]
    sh = c["kind"] == "sh"
    b = run_plan(c, monkeypatch)
    info = b["info"]
    assert (info["P"], info["k_cut"], info["sim"], info["S"], info["C"]) == (P, c["k_cut"], c["simOrder"], S, C), info
    assert info["form"] != 2, "the synthesising sweep: no materialised operands to check"
    g0 = info["g0"]
    ldS, ldD, ldM, nCH = G.round_up(S, 64), G.round_up(D, 64), G.round_up(M, 64), 2 * N + 1
    fails = []
    note(name, "design", "%s N %d %s, D %d, %d microphones (%s), simulation order %d, P %d, G from bin %d" %
         ("EMAinSH" if sh else "EMAinCH", N, "complex" if cplx else "real", D, M, c["mics"][0], c["simOrder"], P, g0))

    # ---- array model: Y_mic, pinv(CH), the encoder product
    assert same_bits(b["mic_azi"], c["mic_azi"])
    Ymic = b["Ymic_rm"].reshape(-1, ldS)[:M, :S]
    held(name, "Y_mic against the longdouble SHs (8 x level)", G.err(Ymic, E.sh_ld(c["simOrder"], c["mic_azi"], np.full(M, E.PI_HALF), cplx)).max() / (E.MARGIN * E.LEVEL_SH[c["simOrder"]]), fails)
    Zlo = b["Zlo"].reshape(-1, ldM)[:nCH, :M]
    Zt = E.pinv_ch_ld(N, c["mic_azi"], cplx)
    held(name, "pinv(CH) against the multiprecision one (8 x level)", G.err(Zlo, Zt).max() / float(np.abs(Zt).max()) / (E.MARGIN * E.LEVEL_PINV_CH), fails)
    Ech = (b["Ech"] if sh else b["E"]).reshape(-1, ldS)[:nCH]
    ref, bd = E.step_ech(Zlo, Ymic, cplx)
    held(name, "encoder product pinv(CH) Y_mic", G.worst(G.err(Ech[:, :S], ref), bd), fails)
    assert np.all(Ech[:, S:] == 0), "the padding of the encoder's rows is not zero"

    # ---- kr, b_n
    kr = b["kr"]
    krt = E.kr_ld(E.FS, P, c["radius"])
    assert kr[0] == 0.0
    held(name, "kr (8 x level)", float(np.abs((kr[1:].astype(E.LD) - krt[1:]) / krt[1:]).max()) / (E.MARGIN * E.LEVEL_KR), fails)
    bn = b["bn"].reshape(P, nOrd)
    bt = E.bn_ld(nOrd, kr)
    e, ab = np.abs(bn.astype(E.CLD) - bt).astype(np.float64), np.abs(bt).astype(np.float64)
    held(name, "b_n over the largest of its bin (8 x level)", (e / ab.max(axis=1, keepdims=True)).max() / (E.MARGIN * E.LEVEL_BN_BIN), fails)
    held(name, "b_n entry by entry (8 x level)", (e[1:] / ab[1:]).max() / (E.MARGIN * E.LEVEL_BN_ENTRY), fails)
    assert abs(bn[0, 0] + 4 * np.pi) <= 4e-15 and np.all(bn[0, 1:] == 0), "the kr = 0 row"

    E0 = b["E"].reshape(-1, ldS)[:C]
    if sh:
        # ---- E0 = diag(Nnm) Ech
        Ypts = b["Ypts"].reshape(C, C)
        Yt = E.sh_ld(N, E.nnm_azimuths(C, cplx), np.full(C, E.PI_HALF), cplx)
        held(name, "Ypts against the longdouble SHs (8 x level)", G.err(Ypts, Yt.T).max() / (E.MARGIN * E.LEVEL_SH[N]), fails)
        ref, bd = E.step_e0(np.diagonal(Ypts), Ech[:, :S], C, cplx)
        held(name, "E0 from the device's Ypts and Ech", G.worst(G.err(E0[:, :S], ref), bd), fails)
        assert np.all(E0[:, S:] == 0), "the padding of E0 is not zero"

        # ---- fit points, their SHs, pinv(B), the fit product
        npts = c["npts"]
        ldP = G.round_up(npts, 64)
        azr, znr = (b[k][:(D + 1) * npts].reshape(D + 1, npts) for k in ("rot_azi", "rot_zen"))
        dpole = E.pole_distance(znr)
        note(name, "closest fit point to a pole, rad", dpole)
        assert dpole >= 1e-3
        held(name, "rotated fit points, chord to the exact rotation (8 x level)", E.points_error(azr, znr, c["azi"], c["zen"]).max() / (E.MARGIN * E.LEVEL_POINTS), fails)
        Arot = b["Arot"].reshape(C, -1)[:, :(D + 1) * npts].reshape(C, D + 1, npts).transpose(1, 0, 2)             # [d][C][npts]
        At = E.sh_ld(N, azr.ravel(), znr.ravel(), cplx).reshape(D + 1, npts, C).transpose(0, 2, 1)
        held(name, "SHs of the fit points against longdouble (8 x level)", G.err(Arot, At).max() / (E.MARGIN * E.LEVEL_SH[N]), fails)
        Zb = b["Zb"].reshape(C, ldP)[:, :npts]
        Zbt = E.pinv_full_rank_ld(E.wide(Arot[D].T, cplx))
        held(name, "pinv(B) of the device's own B (8 x level)", G.err(Zb if cplx else Zb.real, Zbt).max() / float(np.abs(Zbt).max()) / (E.MARGIN * E.LEVEL_PINV_B), fails)
        Rot = b["Rot"].reshape(D, C, C)
        hor = c["zen"] == E.PI_HALF
        assert hor.sum() >= 2 and hor[0] and not hor[1] and not hor[2]
        ref, bd = E.step_rot(Zb, Arot[:D], cplx, blocks=N if C > 32 else None)
        held(name, "fit product pinv(B) A_d (%s kernel)" % ("blockwise" if C > 32 else "narrow"), G.worst(G.err(Rot[~hor], ref[~hor]), bd[~hor]), fails)
        for d in np.flatnonzero(hor):
            assert same_bits(Rot[d], np.eye(C, dtype=Rot.dtype)), "zen == pi/2: not the identity bit for bit"
        Tr = E.truth(c, E.check_bins(c, g0))
        blk = np.zeros((C, C), dtype=bool)
        for l in range(N + 1):
            blk[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = True
        if C > 32:
            assert np.all(Rot[:, ~blk] == 0), "orders 5..7: Rot outside its order blocks is not zero"
        eR = G.err(Rot, Tr["Rot"])
        held(name, "Rot against the exact rotation (8 x level)", eR.max() / Tr["dRot"], fails)
        note(name, "Rot at the two neighbours of pi/2: abs(Rot - I), error", "%.3g, %.3g" % (np.abs(Rot[1:3] - np.eye(C)).max(), eR[1:3].max()))
        assert not same_bits(Rot[1], np.eye(C, dtype=Rot.dtype)) and not same_bits(Rot[2], np.eye(C, dtype=Rot.dtype)), "a neighbour of pi/2 skipped the fit"
        held(name, "E0 against the truth of the chain (composed bound)", G.worst(G.err(E0[:, :S], Tr["E0"]), Tr["dE0"]), fails)

    # ---- SHs of the (projected) grid, conj transpose
    Ycm = b["Ycm"].reshape(S, ldD)
    Yc = b["Yc"].reshape(-1, ldS)
    if not sh:
        # the SHs of the grid itself, zen = 0, pi and 1e-9 among them: sh_basis.hip sees the zenith through cos alone, as MATLAB's legendre
        # does (sin = sqrt(1 - cos^2)); what that may cost is derived in sh_cos_allowance and granted entry by entry on top of the level
        Tr = E.truth(c, E.check_bins(c, g0))
        eY = G.err(Ycm[:, :D].T, Tr["Y"])
        held(name, "Y of the grid against longdouble (8 x level + the cos-only allowance)", G.worst(eY, Tr["dY"]), fails)
        near = np.minimum(c["zen"], np.pi - c["zen"]) < 1e-3
        note(name, "Y within 1e-3 rad of a pole: largest distance to the SHs of the angle, allowance there", "%.3g, %.3g" % (eY[near].max(), (Tr["dY"][near]).max()))
        held(name, "Y elsewhere against longdouble (8 x level)", eY[~near].max() / (E.MARGIN * E.LEVEL_SH[c["simOrder"]]), fails)
    if sh:
        held(name, "Y of the projected grid against longdouble (8 x level)", G.err(Ycm[:, :D].T, E.sh_ld(c["simOrder"], c["azi"], np.full(D, E.PI_HALF), cplx)).max() / (E.MARGIN * E.LEVEL_SH[c["simOrder"]]), fails)
    assert same_bits(Yc[:D, :S], np.conj(Ycm[:, :D].T)), "Yc is not conj(Ycm)^T bit for bit"
    assert np.all(Yc[D:] == 0) and np.all(Yc[:, S:] == 0), "the padding of Yc is not zero"
    assert np.all(Ycm[:, D:] == 0), "the padding of Ycm is not zero"

    # ---- order terms (rotated in place: the composed step), G_k
    QT = b["QT"].reshape(nOrd, C, ldD)
    ref, bd = E.step_qt0(Yc[:D, :S], E0[:, :S], nOrd, cplx)
    if sh:
        ref, bd = E.step_rotate(ref, bd, Rot, N, cplx)
    held(name, "order terms from the device's Yc, E%s" % (" and Rot" if sh else ""), G.worst(G.err(QT[:, :, :D], ref), bd), fails)
    assert np.all(QT[:, :, D:] == 0), "the padding of QT is not zero"
    nb = P - g0
    Gd = b["G"][:nb * C * ldD].reshape(nb, C, ldD)
    bins = list(range(g0, P))
    ref, bd = E.step_g(QT[:, :, :D], bn, bins, P, cplx)
    held(name, "G_k from the device's QT and b_n, bins %d..%d" % (g0, P - 1), max(G.worst(G.err(Gd[kb - g0][:, :D], ref[kb]), bd[kb]) for kb in bins), fails)
    for kb in sorted(Tr["G"]):
        held(name, "G_k against the truth of the chain (composed bound), bin %d" % kb, G.worst(G.err(Gd[kb - g0][:, :D], Tr["G"][kb]), Tr["dG"][kb]), fails)

    # ---- a second execute returns the same bits
    assert same_bits(b["first"]["G"][:nb * C * ldD], b["G"][:nb * C * ldD]), "G differs between two executes"
    if sh:
        assert same_bits(b["first"]["Rot"], b["Rot"]), "Rot differs between two executes"
    assert not fails, fails


@pytest.mark.parametrize("name", list(E.CASES))
def test_ch_basis_kernel(name):
    """the circular harmonics of the case's microphone azimuths, order N, the case's basis: Ycm of a MagLS-2D plan on those azimuths is
    ch_basis_kernel's output (doubles in the real basis, complex otherwise) -- against the multiprecision CH within 8 x the oracle's level"""
    import mpmath as mp
    from emagls_amd import Plan, synth, _lib as L
    E.require_longdouble()
    c = E.case(name)
    N, cplx, M, azi = c["N"], c["cplx"], c["M"], c["mic_azi"]
    taps = 16                                                   # (k_cut >= 2 is required of a MagLS design: 500 Hz bins)
    hL, hR = synth.rigid_sphere_hrirs(azi, np.full(M, E.PI_HALF), fs=E.FS, taps=taps, centre_delay=5.0)
    p = Plan(L.KIND_MAGLS_2D, "complex" if cplx else "real", N, E.FS, taps, taps, M, 0.0, 0)
    try:
        p.set_hrir_grid(azi, None)
        p.set_hrirs(hL, hR)
        p.set_profiling(1)
        try:
            p.execute()
            p.synchronize()
        except L.EmaglsError as e:
            if e.code == L.ERR_HIP:
                pytest.exit("HIP error in a plan: %s" % e, returncode=3)
            raise
        Y = p.debug("Ycm", np.complex128 if cplx else np.float64).reshape(2 * N + 1, -1)
    finally:
        p.close()
    with mp.workdps(E.DPS):
        T = E.mat_to_ld([E.ch_mp(N, E.mpf(a), cplx) for a in azi], cplx)            # [M][2N+1]
    fails = []
    held(name, "CH of the microphone azimuths against the multiprecision one (8 x level)", G.err(Y[:, :M], T.T).max() / (E.MARGIN * E.LEVEL_CH), fails)
    assert np.all(Y[:, M:] == 0), "the padding of the CH matrix is not zero"
    assert not fails, fails
