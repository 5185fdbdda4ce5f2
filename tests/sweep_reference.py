"""One bin step of the operand-fed sweeps (sweep.hip, wide.hip, sweep_persist.hip) in NumPy longdouble, with a-priori error bounds
for the FP64 kernels, and the cases of tests/test_gpu_sweep_operand_step.py with host-made inputs of the same shapes.

The five kernel forms that read their operands from memory do one of two pieces of arithmetic per bin k (W(k-1,:) [ear][C], |H_k|
[ear][D], operands [C][D] as the plans store them; lib/getEMagLsFilters.m:95-103):

  operand_step (sweep_dense_kernel, sweep_wide_kernel, sweep_wide_loop_kernel and their finalize kernels)
      p = W(k-1,:) X_k,    t_d = |H_d| p_d / |p_d|  (|H_d| where p_d = 0; the real part alone at the Nyquist bin),    W(k,:) = t Z_k^T
  half_step (sweep_half_kernel + sweep_half_finalize_kernel, sweep_persist_kernel), with Y_reg_inv_k = conj(G_k) conj(M_k)
      p = W(k-1,:) G_k,    t as above,    v = t conj(G_k)^T,    W(k,:) = v conj(M_k);    a bin with cond_ok == 0:  W(k,:) = t Yri_k^T
  ls_rows (ls_apply_kernel):  W(k,:) = Hc(k,:) Zfix^T for the bins below the cut, the start value of every MagLS chain.

All three are evaluated in clongdouble; the kernel's FP64 operands and its own previous row are taken as exact inputs.

Error bounds, per element of W(k,:), on |FP64 kernel - longdouble step| (moduli of complex numbers).  eps = 2^-52, u = eps / 2,
gamma_n = n eps / (1 - n eps) as in tests/synth_reference.py, whose bound_step these follow term by term.  Nothing below is measured.

  p       a sum of C complex products has 2 C real products per component, each entering with one fused operation; in any order, as
          one chain or as the two to four partial chains the kernels add up at the end (a term of a partial chain passes fewer
          roundings than in one chain), a component is within gamma^u_{2C} = gamma_C times its sum of moduli:
              dp_d = gamma_{C+2} A_d,    A_d = sum_c |W(k-1,c)| |X_cd|,
          the two further units for the additions of the partial chains and the lane reductions being counted as whole terms.  (Per
          component this is a worst case.  For the modulus of the error the worst case is sqrt(2) gamma_C -- every factor with equal
          real and imaginary parts and all 4 C roundings aligned; gamma_{C+2} is first order in that corner, as bound_g is for long
          rows.  It enters only through the phase term, r below, which the conditioning condition keeps under 2^-30.)
          A real operand (MagLS in the real basis) has half the products: the same bound holds with room.
  phase   two unit vectors whose directions p, p + dp differ by r = dp / |p| < 1 are 2 sin(asin(r) / 2) apart at most (= r to first
          order), any two by 2:   dphi_d = that, and dt_d = |H_d| (dphi_d + 4 eps): |p|^2 two roundings, the reciprocal square root
          2 u (fast_rsqrt; wide.hip divides by the rounded square root: 2 u as well), the products with |H| and with p one each:
          5 u < 4 eps.  A direction with a tiny |p_d| widens the bound through its own dphi_d; none is left out.  The Nyquist rule drops
          the imaginary part of both t and its reference: |Re t - Re t'| <= |t - t'|.
  sum     W(k,c) = sum_d t_d Z_cd:  D products and the additions of the workgroups' partial sums, in any order (a term passes at most
          2 D roundings per component whatever the tree): gamma_D per component, sqrt(2) gamma_D <= gamma_{D+c} for the modulus with
          c = ceil((sqrt(2) - 1) D) + 4 (bound_step's count):
              bound_operand_c = gamma_{D+c} sum_d |H_d| |Z_cd| + sum_d dt_d |Z_cd|.
  half    v_c = sum_d t_d conj(G_cd) is bounded like the sum above, dv_c = gamma_{D+c} sum_d |H_d| |G_cd| + sum_d dt_d |G_cd|, and the
          product with conj(M_k) is one more sum of C complex products, its input error carried through:
              bound_half_c = gamma_{2C+2} sum_j |v_j| |M_jc| + sum_j dv_j |M_jc|        (sqrt(2) gamma_C <= gamma_{2C+2}).
          A bin with cond_ok == 0 reads Yri_k in place of conj(G_k) and skips the product: bound_operand with Z = Yri_k.
  ls      bound_ls_c = gamma_{D+c} sum_d |Hc_d| |Zfix_cd|.
Second-order terms (a gamma times a gamma) are left to the margins above (eps where u would do for the roundings of single values).

The bounds are worst cases; an FP64 step commits about 1e-3 of them (tests/test_sweep_reference_host.py prints the ratio).  The GPU
test therefore holds every row norm-wise to SHARP x max(e, C eps ||row||) as well, e the error of step64 -- an FP64 NumPy step through
the same algebra on the same inputs -- against the longdouble step, SHARP = 8 the factor of tests/test_gpu_factor_chain.py."""
import math

import numpy as np

from synth_reference import CLD, EPS64, LD, f64, gamma, step_ratio, to_cld   # noqa: F401  (step_ratio: re-exported for the tests)

FS = 48000.0
SHARP = 8.0
R_LIMIT = 2.0 ** -30          # the conditioning condition: max dp / |p| over all bins, ears and directions of a case
F_CUT_MIN_FREQ = 1000.0       # lib/getMagLsFilters.m:36


def _ld(a):
    a = np.asarray(a)
    if a.dtype == CLD or a.dtype == LD:
        return a
    return to_cld(a) if np.iscomplexobj(a) else a.astype(np.float64).astype(LD)


def unit_phase(p, habs, nyquist):
    """t = |H| p / |p| in clongdouble, |H| where p == 0, the real part alone at the Nyquist bin"""
    a = np.abs(p)
    h = np.asarray(habs, dtype=np.float64).astype(LD)
    t = np.zeros(p.shape, dtype=CLD)
    nz = a > 0
    t[nz] = h[nz] * p[nz] / a[nz]
    t[~nz] = h[~nz]
    if nyquist:
        t.imag = 0
    return t


def operand_step(w_prev, habs_k, X_k, Z_k, nyquist=False):
    """w_prev [2][C], habs_k [2][D], X_k and Z_k [C][D] (real or complex) -> (W(k,:) [2][C], p [2][D], t [2][D]), clongdouble"""
    p = to_cld(w_prev) @ _ld(X_k)
    t = unit_phase(p, habs_k, nyquist)
    return t @ _ld(Z_k).T, p, t


def half_step(w_prev, habs_k, G_k, M_k, yri_k=None, nyquist=False):
    """w_prev [2][C], habs_k [2][D], G_k [C][D], M_k [C][C]; yri_k [C][D]: a bin with cond_ok == 0 (M_k is not read)
    -> (W(k,:) [2][C], p, t, v [2][C] or None), clongdouble"""
    G = _ld(G_k)
    p = to_cld(w_prev) @ G
    t = unit_phase(p, habs_k, nyquist)
    if yri_k is not None:
        return t @ _ld(yri_k).T, p, t, None
    v = t @ np.conj(G).T
    return v @ np.conj(_ld(M_k)), p, t, v


def ls_rows(Hc, Zfix):
    """Hc [rows][D], Zfix [C][D] -> Hc Zfix^T [rows][C], clongdouble"""
    return to_cld(Hc) @ _ld(Zfix).T


# ---- the same algebra in FP64 NumPy: what the sharper criterion measures the longdouble step with

def unit_phase64(p, habs, nyquist):
    a = np.abs(p)
    h = np.asarray(habs, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(a > 0, h * p / a, h.astype(np.complex128))
    if nyquist:
        t = t.real.astype(np.complex128)
    return t


def operand_step64(w_prev, habs_k, X_k, Z_k, nyquist=False):
    p = np.asarray(w_prev, dtype=np.complex128) @ np.asarray(X_k).astype(np.complex128)
    return unit_phase64(p, habs_k, nyquist) @ np.asarray(Z_k).astype(np.complex128).T


def half_step64(w_prev, habs_k, G_k, M_k, yri_k=None, nyquist=False):
    G = np.asarray(G_k, dtype=np.complex128)
    t = unit_phase64(np.asarray(w_prev, dtype=np.complex128) @ G, habs_k, nyquist)
    if yri_k is not None:
        return t @ np.asarray(yri_k, dtype=np.complex128).T
    return (t @ np.conj(G).T) @ np.conj(np.asarray(M_k, dtype=np.complex128))


# ---- the bounds derived above

def sum_count(D):
    return D + int(math.ceil((math.sqrt(2.0) - 1.0) * D)) + 4


def phase_terms(w_prev, habs_k, X_k, p):
    """(r [2][D] = dp / |p|, dt [2][D]) of the derivation above; X_k [C][D] is the operand p was formed with.  Where p == 0, r is
    inf -- unless dp == 0 as well: every product of the sum is zero (the zero row an array design's chain starts from when it has no
    bin below the cut), the kernel's p is exactly zero too and both take t = |H|."""
    aX = np.abs(np.asarray(X_k)).astype(np.float64)
    C = aX.shape[0]
    dp = gamma(C + 2) * (np.abs(np.asarray(w_prev)).astype(np.float64) @ aX)
    ap = f64(np.abs(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ap > 0, dp / ap, np.where(dp > 0, np.inf, 0.0))
    dphi = np.where(r < 1.0, 2.0 * np.sin(0.5 * np.arcsin(np.minimum(r, 1.0))), 2.0)
    return r, np.asarray(habs_k, dtype=np.float64) * (dphi + 4 * EPS64)


def bound_operand(w_prev, habs_k, X_k, Z_k, p):
    """[2][C], float64; p from operand_step of the same arguments.  Returns (bound, r)."""
    r, dt = phase_terms(w_prev, habs_k, X_k, p)
    aZ = np.abs(np.asarray(Z_k)).astype(np.float64)
    D = aZ.shape[1]
    return gamma(sum_count(D)) * (np.asarray(habs_k, dtype=np.float64) @ aZ.T) + dt @ aZ.T, r


def bound_half(w_prev, habs_k, G_k, M_k, p, v, yri_k=None):
    """[2][C], float64; p, v from half_step of the same arguments.  Returns (bound, r)."""
    if yri_k is not None:
        return bound_operand(w_prev, habs_k, G_k, yri_k, p)
    r, dt = phase_terms(w_prev, habs_k, G_k, p)
    aG = np.abs(np.asarray(G_k)).astype(np.float64)
    aM = np.abs(np.asarray(M_k)).astype(np.float64)
    C, D = aG.shape
    dv = gamma(sum_count(D)) * (np.asarray(habs_k, dtype=np.float64) @ aG.T) + dt @ aG.T
    return gamma(2 * C + 2) * (f64(np.abs(v)) @ aM) + dv @ aM, r


def bound_ls(Hc, Zfix):
    aZ = np.abs(np.asarray(Zfix)).astype(np.float64)
    return gamma(sum_count(aZ.shape[1])) * (np.abs(np.asarray(Hc)).astype(np.float64) @ aZ.T)


def row_errors(w_got, w_ref):
    """||w_got - w_ref||_2 per ear, float64 (w_ref clongdouble)"""
    return np.sqrt(f64((np.abs(to_cld(w_got) - w_ref) ** 2).sum(axis=-1)))


def sharp_limit(e64, w_ref):
    """[2]: SHARP x max(e, C eps ||row||)"""
    C = w_ref.shape[-1]
    nrm = np.sqrt(f64((np.abs(w_ref) ** 2).sum(axis=-1)))
    return SHARP * np.maximum(e64, C * EPS64 * nrm)


def check_step(w_got, step, bound, w64):
    """One checked row of the kernel against the longdouble step `step[0]`: (largest error / bound, largest row error / sharp limit,
    largest row error / e), e the row error of the FP64 NumPy step w64."""
    ref = step[0]
    ratio = float(step_ratio(w_got, ref, bound).max())
    e64 = row_errors(w64, ref)
    err = row_errors(w_got, ref)
    lim = sharp_limit(e64, ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        over_e = float(np.where(e64 > 0, err / e64, np.where(err > 0, np.inf, 0.0)).max())
    return ratio, float((err / lim).max()), over_e


# ---- the cases of tests/test_gpu_sweep_operand_step.py, shared with tests/test_sweep_reference_host.py

def cut_of(kind, order, f_trans=0.0):
    return f_trans if kind == "atf" else max(F_CUT_MIN_FREQ, 500.0 * order)


def bins_of(length, f_cut, fs=FS):
    """(P, kcut0, first swept bin) as plan_setup.hip derives them: nfft = 2 len, k_cut = ceil(f_cut / f(2))"""
    P = length + 1
    k_cut = max(int(math.ceil(f_cut / ((fs / 2.0) / (P - 1)))), 1)
    kcut0 = min(k_cut - 1, P)
    return P, kcut0, max(kcut0, 1)


def shortest_length(kind, order, f_trans=0.0, min_swept=8):
    """The shortest filter length a plan accepts (even, nfft >= 8) that leaves `min_swept` swept bins and, for MagLS, two bins below
    the cut.  A MagLS plan needs one (k_cut >= 2), but a chain that starts from the DC row alone starts from a real row -- H(0,:) is
    real -- and in the real basis stays real through every bin: p real, t = +-|H|, no imaginary part anywhere, and a kernel that kept
    Im t at the Nyquist bin or mishandled the imaginary parts of W would pass.  The second row below the cut is complex.  (An array
    design without a bin below the cut starts from the zero row, t = |H|, and its complex operands make the chain complex at once.)"""
    for length in range(4, 4096, 2):
        P, kcut0, k0 = bins_of(length, cut_of(kind, order, f_trans))
        if (kind != "magls" or kcut0 >= 2) and P - k0 >= min_swept:
            return length
    raise ValueError("no length")


def wide_nwg(D):
    return (D + 63) // 64


def dense_nwg(D, C):
    """(workgroups, slabs per workgroup) of the launch-per-bin forms up to 32 channels (dense_sweep_nwg of sweep.hip)"""
    nslab, cap = (D + 63) // 64, max(1, 16 * 256 // (2 * max(C, 1)))
    spw = (nslab + cap - 1) // cap
    nwg = (nslab + spw - 1) // spw
    return nwg, (nslab + nwg - 1) // nwg


def persist_dpw(D):
    return 64 if D <= 2048 else 96


NO_PERSIST = {"EMAGLS_SWEEP_PERSIST": "0"}
NO_SYNTH = {"EMAGLS_SWEEP_SYNTH": "0"}
# the smallest direction counts the plans accept (found by creating and executing the plan at every count from one below the channel
# count on, as SMALLEST_D of tests/test_gpu_sweep_step.py was): every count from the channel count on runs -- MagLS needs D >= S, and
# the Fibonacci lattice of S points passes the wide path's conditioning certificate (cond(Y)^2 < 1e8); the order-4 eMagLS design
# simulates 20 orders (S = 400) but needs only D >= C = 25 and the 25 columns of its orthonormal route -- and one fewer is refused
SMALLEST_D = {("magls", 4): 25, ("magls", 5): 36, ("emagls", 4): 25}


def case(name, kind, kernel, form, order, basis, D, env=None, nmics=0, radius=0.0, note=""):
    return dict(name=name, kind=kind, kernel=kernel, form=form, order=order, basis=basis, D=D, env=dict(env or {}), nmics=nmics,
                radius=radius, note=note)


def _cases():
    out = []
    # wide, real TX: NG = 24 staged partial sums per lane pair; nWG = 48 fills them, 49 / 50 run the loop behind them once / twice
    for D in (SMALLEST_D[("magls", 5)], 3072, 3073, 3135, 3137):
        out.append(case(f"wide-real-{D}", "magls", "wide", 0, 5, "real", D))
    # wide, complex TX: NG = 12; 24 / 25 workgroups
    for D in (1536, 1537, 1599):
        out.append(case(f"wide-complex-{D}", "magls", "wide", 0, 6, "complex", D))
    out.append(case("wide-emagls2-48", "emagls2", "wide", 0, 4, "real", 1537, nmics=48, radius=0.042))
    # loop: even and odd workgroup counts, tails of 1 and 63 directions
    for order, basis, Ds in ((8, "real", (191, 193)), (9, "complex", (255, 257))):
        for D in Ds:
            out.append(case(f"loop-{basis}-{D}", "magls", "loop", 0, order, basis, D))
    # dense: the four-lane gather's tails (1, 2, 4, 5, 8, 9 workgroups), spw = 1 at its largest grid, spw = 2
    for basis in ("real", "complex"):
        for D in (63, 65, 255, 257, 511, 513, 5184):
            out.append(case(f"dense-{basis}-{D}", "magls", "dense", 0, 4, basis, D, env=NO_PERSIST))
        for D in (5185, 5249):
            out.append(case(f"dense-{basis}-{D}", "magls", "dense", 0, 4, basis, D))
    for D in (64, 65):
        out.append(case(f"dense-atf-{D}", "atf", "dense", 0, 0, "real", D, env=NO_PERSIST, nmics=4))
    # half
    out.append(case("half-emagls-449", "emagls", "half", 0, 4, "real", 449, env={**NO_PERSIST, **NO_SYNTH}, nmics=32, radius=0.042))
    out.append(case("half-emagls-3073", "emagls", "half", 0, 4, "real", 3073, env=NO_SYNTH, nmics=32, radius=0.042))
    # (the SH-domain order-4 design at 2 cm has cond(pwGrid) = 1.5e3 at 2 kHz, its first swept bin -- under COND_LIMIT = 1e4 of
    # dspace.hip, so no swept bin of it can be flagged; the same array's 32 raw microphones, eMagLS2, have 2e5 there)
    out.append(case("half-emagls2-2cm", "emagls2", "half", 0, 4, "real", 449, env={**NO_PERSIST, **NO_SYNTH}, nmics=32, radius=0.02,
                    note="cond_ok"))
    # persistent: slab heights 64 / 96 at 2048 / 2049, the hand-over at 3072
    for basis in ("real", "complex"):
        for D in (SMALLEST_D[("magls", 4)], 2048, 2049, 3071, 3072):
            out.append(case(f"persist-magls-{basis}-{D}", "magls", "persist", 1, 4, basis, D))
        for D in (SMALLEST_D[("emagls", 4)], 2048, 2049, 3071, 3072):
            env = NO_SYNTH if basis == "real" else {**NO_SYNTH, "EMAGLS_REAL_INTERNAL": "0"}
            out.append(case(f"persist-emagls-{basis}-{D}", "emagls", "persist", 1, 4, basis, D, env=env, nmics=32, radius=0.042))
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def length_of(c):
    # the 2 cm array: 12 taps put bin 1 at 2 kHz, below the 3.5 kHz at which the Gram route of 32 channels at this radius starts
    # (emagls_gram_from of plan_setup.hip), so that the first swept bin is a bin of the orthonormal route, which alone can be flagged
    if c["note"] == "cond_ok":
        return 12
    return shortest_length(c["kind"], c["order"], 2000.0 if c["kind"] == "atf" else 0.0)


def scene(c):
    """(azi, zen, hL, hR) of a case: a Fibonacci lattice with rigid-sphere HRIRs of the case's filter length"""
    from emagls_amd import synth
    n = length_of(c)
    azi, zen = synth.fibonacci_grid(c["D"])
    hL, hR = synth.rigid_sphere_hrirs(azi, zen, fs=FS, taps=n, seed=77 + c["D"], centre_delay=n / 4)
    return azi, zen, hL, hR


def microphones(c):
    from emagls_amd import synth
    from synth_reference import jittered_array
    return synth.em32_grid() if c["nmics"] == 32 else jittered_array(c["nmics"])


def atf_set(c):
    from emagls_amd import synth
    return synth.glasses_atfs(natf=c["D"], nmics=c["nmics"], fs=FS, taps=length_of(c))


def host_chain(c):
    """A case's chain on host-made operands of the same shape (the oracle's matrices in place of the plan's buffers), swept in FP64
    NumPy: yields per swept bin (w_prev, habs, operands ..., nyquist) as the step routines take them.  Operand cases yield
    ("operand", w_prev, habs, X, Z, nyq), half cases ("half", w_prev, habs, G, M, yri, nyq)."""
    from oracle import emagls_oracle as O
    azi, zen, hL, hR = scene(c)
    n = length_of(c)
    nfft = 2 * n
    P, kcut0, k0 = bins_of(n, cut_of(c["kind"], c["order"], 2000.0))
    dirs = np.column_stack([azi, zen])
    half = c["kernel"] in ("half", "persist")
    if c["kind"] == "magls":
        Y = O.getSH(c["order"], dirs, c["basis"])
        X = np.ascontiguousarray(Y.conj().T)
        Z = np.ascontiguousarray(np.linalg.pinv(X).T)
        Mfix = np.conj(np.linalg.inv(X @ X.conj().T)) if half else None
        H = np.stack([np.fft.rfft(h, nfft, axis=0) for h in (hL, hR)])
        ops = lambda k: (X, Z, Mfix, None)
    else:
        if c["kind"] == "atf":
            atf, _, _ = atf_set(c)
            pw_all = np.fft.rfft(atf, nfft, axis=0)                    # [P][M][D]: the grids coincide, every direction matches itself
            H = np.stack([np.fft.rfft(h, nfft, axis=0) for h in (hL, hR)])
            pw_of = lambda k: pw_all[k]
        else:
            maz, mzn = microphones(c)
            raw = c["kind"] == "emagls2"
            smair, sim = O.getSMAIRMatrix(O.SMAIR_DEFAULT_ORDER if raw else c["order"], FS, nfft, c["radius"], np.column_stack([maz, mzn]),
                                          "real", returnRawMicSigs=raw)
            Yhc = O.getSH(sim, dirs, "real").conj().T
            HL, HR, _, _ = O._hrir_prologue(hL, hR, nfft, P)
            H = np.stack([HL[:P], HR[:P]])
            pw_of = lambda k: O._matmul(smair[:, :, k], Yhc)

        def ops(k):
            pw = np.ascontiguousarray(pw_of(k))
            U, s, Vh = np.linalg.svd(pw.T, full_matrices=False)
            yri = (np.conj(U) @ ((1.0 / np.maximum(s, O.SVD_REGUL_CONST * s.max()))[:, None] * Vh.conj())).T   # [C][D]
            if not half:
                return pw, np.ascontiguousarray(yri), None, None
            if s.max() > 1e4 * s.min():                                # (COND_LIMIT of dspace.hip: the accurate slab)
                return pw, None, None, np.ascontiguousarray(yri)
            # conj(M) with Y_reg_inv = conj(G)^T conj(M): from the same singular vectors, conj(M) = conj(V) diag(s_reg / s) V^T
            V = Vh.conj().T
            cm = np.conj(V) @ (((1.0 / np.maximum(s, O.SVD_REGUL_CONST * s.max())) / s)[:, None] * V.T)
            return pw, None, np.conj(cm), None
    Xs, Zs, Ms, Ys = ops(max(k0 - 1, 1))
    if c["kind"] == "magls":
        w = H[:, k0 - 1] @ Z.T
    elif kcut0 < 1:    # no bin below the cut: the chain starts from the zero row W(0,:), p == 0 and t = |H| in the first swept bin
        w = np.zeros((2, Xs.shape[0]), dtype=np.complex128)
    else:
        y0 = Zs if Zs is not None else (Ys if Ys is not None else (np.conj(Xs).T @ np.conj(Ms)).T)
        w = H[:, k0 - 1] @ y0.T
    for k in range(k0, P):
        habs = np.abs(H[:, k])
        nyq = k == P - 1
        Xk, Zk, Mk, Yk = ops(k)
        if half:
            yield ("half", w, habs, Xk, Mk, Yk, nyq)
            w = half_step64(w, habs, Xk, Mk, Yk, nyq)
        else:
            yield ("operand", w, habs, Xk, Zk, nyq)
            w = operand_step64(w, habs, Xk, Zk, nyq)
