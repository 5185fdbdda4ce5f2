"""tests/ema_reference.py proved on the host before the GPU test leans on it: the exact rotation is a rotation (unitary, the plane-wave identity,
angles add up, the identity on the horizon), the longdouble bases are the multiprecision ones, the truth agrees with the CPU oracle at the
oracle's double-precision level -- printed, and held within the constants LEVEL_* the GPU test allows 8 x of --, the a-priori bounds hold for a
plain NumPy double evaluation of every step on the inputs of the GPU cases, and no point the rotation fit evaluates SHs at lies near a pole."""
import numpy as np
import mpmath as mp
import pytest

import ema_reference as E
import gram_reference as G
from oracle import emagls_oracle as O

LD, CLD = E.LD, E.CLD


@pytest.fixture(autouse=True)
def _ld():
    E.require_longdouble()


def mp_max(M):
    return max(abs(M[i, j]) for i in range(M.rows) for j in range(M.cols))


DIRS = [(0.3, 0.4), (7.0, 1e-9), (-4.0, np.pi), (2.0, 0.0), (1.1, np.nextafter(E.PI_HALF, 4.0)), (5.5, 2.9)]


@pytest.mark.parametrize("cplx", [False, True])
def test_exact_rotation_is_the_rotation(cplx):
    """unitary and, in the real basis, real to 1e-30; Y_i(R^-1 x) = sum_j Rot_ij Y_j(x) at random points to 1e-30, orders up to 7"""
    rng = np.random.default_rng(5)
    with mp.workdps(E.DPS):
        for a, z in DIRS:
            azi, alpha = E.mpf(a), E.mpf(float(np.float64(E.PI_HALF) - np.float64(z)))
            ax = [mp.sin(azi), -mp.cos(azi), mp.mpf(0)]
            pts = [(E.mpf(rng.uniform(0, 2 * np.pi)), E.mpf(rng.uniform(0.05, 3.0))) for _ in range(3)]
            for l in range(8):
                B = E.rot_block_mp(l, azi, alpha, cplx)
                assert mp_max(B * B.H - mp.eye(2 * l + 1)) < mp.mpf("1e-30")
                if not cplx:
                    assert max(abs(mp.im(B[i, j])) for i in range(B.rows) for j in range(B.cols)) < mp.mpf("1e-30")
            for pa, pz in pts:
                x = [mp.sin(pz) * mp.cos(pa), mp.sin(pz) * mp.sin(pa), mp.cos(pz)]
                cr = [ax[1] * x[2] - ax[2] * x[1], ax[2] * x[0] - ax[0] * x[2], ax[0] * x[1] - ax[1] * x[0]]
                dt = ax[0] * x[0] + ax[1] * x[1]
                xr = [x[j] * mp.cos(alpha) - cr[j] * mp.sin(alpha) + ax[j] * dt * (1 - mp.cos(alpha)) for j in range(3)]    # R^-1 x
                Yx = E.sh_mp(7, pa, pz, cplx)
                Yr = E.sh_mp(7, mp.atan2(xr[1], xr[0]), mp.acos(xr[2]), cplx)
                for l in range(8):
                    B = E.rot_block_mp(l, azi, alpha, cplx)
                    lo = l * l
                    for i in range(2 * l + 1):
                        s = sum(B[i, j] * Yx[lo + j] for j in range(2 * l + 1))
                        assert abs(s - Yr[lo + i]) < mp.mpf("1e-30"), (a, z, l, i)


@pytest.mark.parametrize("cplx", [False, True])
def test_elevations_about_one_axis_add_up(cplx):
    with mp.workdps(E.DPS):
        azi, a1, a2 = mp.mpf("0.7"), mp.mpf("0.4"), mp.mpf("-1.3")
        for l in range(1, 8):
            P = E.rot_block_mp(l, azi, a1, cplx) * E.rot_block_mp(l, azi, a2, cplx)
            assert mp_max(P - E.rot_block_mp(l, azi, a1 + a2, cplx)) < mp.mpf("1e-30")


def test_horizon_is_the_identity_exactly():
    for cplx in (False, True):
        R = E.rot_ld(7.0, E.PI_HALF, 7, cplx)
        assert np.array_equal(R, np.eye(64, dtype=R.dtype))
    with mp.workdps(E.DPS):       # (rot_ld returns the identity outright at alpha == 0: the Wigner construction itself at the horizon)
        for cplx in (False, True):
            for l in range(8):
                assert mp_max(E.rot_block_mp(l, mp.mpf(7), mp.mpf(0), cplx) - mp.eye(2 * l + 1)) < mp.mpf("1e-30")
    up = E.rot_ld(7.0, np.nextafter(E.PI_HALF, 4.0), 4, False)
    assert not np.array_equal(up, np.eye(25, dtype=LD)) and np.abs(up - np.eye(25)).max() < 1e-15


@pytest.mark.parametrize("cplx", [False, True])
def test_longdouble_bases_are_the_multiprecision_ones(cplx):
    """order 19, poles and the edge elevations included"""
    azi = np.array([0.0, 7.0, -4.0, 1.0, 2.5, 0.3, 6.0])
    zen = np.array([0.0, np.pi, 1e-9, E.PI_HALF, np.nextafter(E.PI_HALF, 0.0), 0.7, 3.0])
    Y = E.sh_ld(19, azi, zen, cplx)
    with mp.workdps(E.DPS):
        for p in range(azi.size):
            t = E.sh_mp(19, E.mpf(azi[p]), E.mpf(zen[p]), cplx)
            for c in range(400):
                assert abs(E.to_ld(t[c] + mp.mpc(0) if cplx else t[c]) - Y[p, c]) < 2e-17, (p, c)


@pytest.mark.parametrize("cplx", [False, True])
def test_nnm_closed_form(cplx):
    """against the SHs at the equator over the circular harmonics, and against the oracle's expansion matrix"""
    N = 7
    nn = E.nnm_ld(N, cplx)
    basis = "complex" if cplx else "real"
    J = O.getChToShExpansionMatrix(N, basis)
    with mp.workdps(E.DPS):
        phi = mp.mpf("0.37")
        Y, Cc = E.sh_mp(N, phi, mp.pi / 2, cplx), E.ch_mp(N, phi, cplx)
        for c in range((N + 1) ** 2):
            n, m = E.channel_nm(c)
            assert abs(E.to_ld(Y[c] - mp.mpf(0)) - nn[c] * E.to_ld(Cc[E.ch_index(m)])) < 1e-18, c
            assert abs(float(nn[c]) - J[c, E.ch_index(m)]) < 4e-16 and np.count_nonzero(J[c]) <= 1


def test_levels_of_the_oracle():
    """the measurement the GPU test's levels come from: the oracle (and the NumPy restatement of the fit points) against the truth"""
    lv = E.measure_levels()
    flat = {}
    for k, v in lv.items():
        for o, e in (v.items() if isinstance(v, dict) else [(None, v)]):
            flat[k if o is None else "%s[%d]" % (k, o)] = (e, getattr(E, "LEVEL_" + k) if o is None else getattr(E, "LEVEL_" + k)[o])
    for k, (v, const) in flat.items():
        print("oracle level %-9s measured %.3g   constant %.3g" % (k, v, const))
    for k, (v, const) in flat.items():
        # (the constants record one measurement; LAPACK's and libm's last bits may differ between machines: within a factor 4 either way)
        assert const / 4 <= v <= 4 * const, k


@pytest.mark.parametrize("name", [n for n in E.CASES if E.CASES[n]["kind"] == "sh"])
def test_no_fit_point_near_a_pole(name):
    c = E.case(name)
    azr, znr = E.rot_points_np(c["azi"], c["zen"], c["npts"])
    d = E.pole_distance(znr)
    print("%s: closest fit point to a pole %.3g rad" % (name, d))
    assert d >= 1e-3


@pytest.mark.parametrize("name", list(E.CASES))
def test_bounds_hold_for_numpy(name):
    """every step that is a sum, evaluated by NumPy in double on the case's inputs, lies within its a-priori bound of the longdouble step on the
    same inputs; the whole chain in double lies within the composed bound of the truth"""
    c = E.case(name)
    N, cplx, basis, nOrd, P, C = c["N"], c["cplx"], "complex" if c["cplx"] else "real", c["nOrd"], c["P"], c["C"]
    eq = np.full(c["M"], E.PI_HALF)
    Ymic = O.getSH(c["simOrder"], np.column_stack([c["mic_azi"], eq]), basis)
    Z = np.linalg.pinv(O.getCH(N, c["mic_azi"], basis)).astype(np.complex128)
    Ech = (Z @ Ymic) if cplx else (Z.real @ Ymic)
    ref, bd = E.step_ech(Z, Ymic, cplx)
    assert G.worst(G.err(Ech, ref), bd) <= 1.0
    kr = 2 * np.pi * np.linspace(0, E.FS / 2, P) / O.C_SOUND * c["radius"]
    bn = -O.sphModalCoeffs(c["simOrder"], kr)
    bins = E.check_bins(c, 1)
    if c["kind"] == "ch":
        Yc = np.conj(O.getSH(c["simOrder"], np.column_stack([c["azi"], c["zen"]]), basis))
        E0 = Ech
    else:
        Yc = np.conj(O.getSH(c["simOrder"], np.column_stack([c["azi"], np.full(c["D"], E.PI_HALF)]), basis))
        J = O.getChToShExpansionMatrix(N, basis)
        nn = J.sum(axis=1)
        chv = np.array([1.0 if (cplx or E.channel_nm(ch)[1] == 0) else np.sqrt(2.0) for ch in range(C)])
        E0 = J @ Ech
        ref, bd = E.step_e0(nn * chv, Ech, C, cplx)
        assert G.worst(G.err(E0, ref), bd) <= 1.0
    QT0 = np.stack([E0[:, n * n:(n + 1) ** 2] @ Yc[:, n * n:(n + 1) ** 2].T for n in range(nOrd)])
    r0, b0 = E.step_qt0(Yc, E0, nOrd, cplx)
    assert G.worst(G.err(QT0, r0), b0) <= 1.0
    QT = QT0
    if c["kind"] == "sh":
        azr, znr = E.rot_points_np(c["azi"], c["zen"], c["npts"])
        A = O.getSH(N, np.column_stack([azr.ravel(), znr.ravel()]), basis).reshape(c["D"] + 1, c["npts"], C).transpose(0, 2, 1)   # [d][C][npts]
        Zb = np.linalg.pinv(A[-1].T).astype(np.complex128)                                                                        # [C][npts]
        Rot = A[:-1] @ (Zb if cplx else Zb.real).T
        ref, bd = E.step_rot(Zb, A[:-1], cplx)
        assert G.worst(G.err(Rot, ref), bd) <= 1.0
        Rot[c["zen"] == E.PI_HALF] = np.eye(C)
        QT = QT0.copy()
        for l in range(1, N + 1):
            sl = slice(l * l, (l + 1) ** 2)
            QT[:, sl, :] = np.einsum("nid,dij->njd", QT0[:, sl, :], Rot[:, sl, sl])
        ref, bd = E.step_rotate(r0, b0, Rot, N, cplx)
        assert G.worst(G.err(QT, ref), bd) <= 1.0
    Gd = {kb: np.tensordot(np.asarray(E.coef_b(bn, kb, P)).astype(np.complex128), QT, axes=(0, 0)) for kb in bins}
    ref, bd = E.step_g(QT, bn, bins, P, cplx)
    assert max(G.worst(G.err(Gd[kb], ref[kb]), bd[kb]) for kb in bins) <= 1.0
    if c["kind"] == "ch":
        T = E.truth(c, bins)
        wY = G.worst(G.err(np.conj(Yc), T["Y"]), T["dY"])
        wG = max(G.worst(G.err(Gd[kb], T["G"][kb]), T["dG"][kb]) for kb in bins)
        print("%s: NumPy chain against the truth, error / composed bound: Y %.3g, G %.3g" % (name, wY, wG))
        assert max(wY, wG) <= 1.0
    if c["kind"] == "sh":
        T = E.truth(c, bins)
        wE = G.worst(G.err(E0, T["E0"]), T["dE0"])
        wR = G.worst(G.err(Rot, T["Rot"]), np.full(Rot.shape, T["dRot"]))
        wG = max(G.worst(G.err(Gd[kb], T["G"][kb]), T["dG"][kb]) for kb in bins)
        print("%s: NumPy chain against the truth, error / composed bound: E0 %.3g, Rot %.3g, G %.3g" % (name, wE, wR, wG))
        assert max(wE, wR, wG) <= 1.0
