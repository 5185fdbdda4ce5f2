/* emagls.h -- C ABI of the MI355X-native eMagLS filter-design / binaural-render library.
 *
 * Drop-in boundary for the reference's MATLAB entry points (paths relative to thomasdeppisch/eMagLS):
 *
 *   emagls_get_ls_filters              <-  lib/getLsFilters.m:1-2
 *   emagls_get_magls_filters           <-  lib/getMagLsFilters.m:1-2
 *   emagls_get_emagls_filters          <-  lib/getEMagLsFilters.m:1-2
 *   emagls_get_emagls2_filters         <-  lib/getEMagLs2Filters.m:1-2
 *   emagls_get_emagls_filters_from_atf <-  lib/getEMagLsFiltersFromAtf.m:1
 *   emagls_get_emagls_filters_ema_in_ch <- lib/getEMagLsFiltersEMAinCH.m:1-2  (default chFunction @getCH, dependencies/getCH.m)
 *   emagls_binaural_decode[_complex]   <-  dependencies/binauralDecode.m:1-2 (core loop :33-42,53-64)
 *   emagls_resample                    <-  resample(x, p, q) (Signal Processing Toolbox, call sites dependencies/binauralDecode.m:15,21-22)
 *   emagls_sh_basis                    <-  getSH (polarch/Spherical-Harmonic-Transform, call site lib/getLsFilters.m:30)
 *   emagls_modal_bn                    <-  sphModalCoeffs (polarch/Array-Response-Simulator, call site dependencies/getSMAIRMatrix.m:107)
 *
 * Conventions (identical to the MATLAB side, so a MEX gateway passes mxGetDoubles() pointers through):
 *   - all arrays are column-major FP64; complex arrays are interleaved (re,im) pairs
 *     (MATLAB R2018a+ interleaved complex API, numpy complex128);
 *   - HRIRs are [numSamples x numDirections]; filters come back [len x numChannels];
 *   - angles in radians, zenith (0..pi), not elevation;
 *   - basis: EMAGLS_BASIS_REAL -> real outputs (double), EMAGLS_BASIS_COMPLEX -> complex outputs;
 *   - pointers may be host or device pointers (copies use hipMemcpyDefault); outputs are caller-allocated;
 *   - every function returns EMAGLS_OK or an error code; emagls_last_error() gives the message
 *     (the MEX shim forwards it to mexErrMsgIdAndTxt);
 *   - the default shFunction (@getSH) is built in; a custom MATLAB shFunction handle cannot cross a C ABI: the wrapper
 *     evaluates it and calls the *_with_basis entry points with the resulting matrices.
 *
 * Threading: one host thread per plan; one process per GPU for multi-GPU batches.
 */
#ifndef EMAGLS_H
#define EMAGLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMAGLS_OK 0
#define EMAGLS_ERR_ARG 1         /* invalid argument; mirrors the reference's assert()s, e.g. "len too short" */
#define EMAGLS_ERR_UNSUPPORTED 2 /* shape outside what this build supports */
#define EMAGLS_ERR_HIP 3         /* HIP / hipFFT runtime failure */
#define EMAGLS_ERR_NUMERIC 4     /* e.g. SH Gram matrix of the HRIR grid not positive definite */

#define EMAGLS_BASIS_REAL 0
#define EMAGLS_BASIS_COMPLEX 1

#define EMAGLS_KIND_LS 0
#define EMAGLS_KIND_MAGLS 1
#define EMAGLS_KIND_EMAGLS 2
#define EMAGLS_KIND_EMAGLS2 3
#define EMAGLS_KIND_FROM_ATF 4
#define EMAGLS_KIND_EMA_CH 5   /* equatorial array, output in circular harmonics (2*order+1 channels) */
#define EMAGLS_KIND_MAGLS_2D 6 /* MagLS on a horizontal HRIR set in circular harmonics (2*order+1 channels) */
#define EMAGLS_KIND_EMA_SH 7   /* equatorial array, output in spherical harmonics ((order+1)^2 channels) */

const char* emagls_last_error(void);
int emagls_version(void);
int emagls_device_count(int* count);
int emagls_set_device(int device);

/* The one-shot entry points below keep the plans of their most recent shapes alive (device buffers, captured hipGraphs; at most
 * EMAGLS_PLAN_CACHE plans, default 4, 0 disables), and emagls_binaural_decode its hipFFT plans and work buffers.  This call
 * releases all of it (a MEX gateway registers it with mexAtExit), together with the resident chunks of the job lists and the pool of
 * device-memory blocks that plans and batches hand back. */
int emagls_cache_clear(void);
/* The same without the block pool: every resident plan, batch and job chunk goes, their device memory stays with the library for the
 * next designs (a long-running process that moves on to another study: fresh device memory is what costs -- hipMalloc of a few GB took
 * 0.3 ms on some boxes and seconds on others, profiles/r06_cold_path.md). */
int emagls_cache_release_designs(void);

/* Measured FP64 peak of the current device in TFLOP/s (best of a few launches that keep every CU busy): which = 0 the matrix
 * pipe on v_mfma_f64_16x16x4_f64 (the shape the pipeline's GEMM kernels issue), which = 1 the vector pipe (v_fma_f64), which = 2
 * the matrix pipe on v_mfma_f64_4x4x4_4b_f64 -- on gfx950 the shape that reaches the pipe's nominal rate (75 of 78.6 TFLOP/s; the
 * 16 x 16 x 4 shape sustains 49).  bench.py prices its executed flops against the vector figure. */
int emagls_fp64_peak_tflops(int which, double* tflops);
/* The same with the launch length chosen: burst != 0 times launches of <= 1 ms (before the chip settles at its sustained power
 * state), burst == 0 the ~10 ms launches of the call above; shader_mhz (optional) receives the shader clock the timed loop ran
 * at (in-kernel cycle counter over the 100 MHz wall counter). */
int emagls_fp64_peak_tflops_ex(int which, int burst, double* tflops, double* shader_mhz);
/* Device-side self tests of building blocks that have no entry point of their own.  which = 0: the partial-sum contraction of
 * the register-resident sweep (v_mfma_f64_4x4x4_4b in the sweep's quad layout against a host sum; max_err: largest absolute difference); which = 1 / 2:
 * the LDS-staged Gram tile on v_mfma_f64_16x16x4 / on v_mfma_f64_4x4x4_4b against a host sum (max_err relative to the largest element). */
int emagls_self_test(int which, double* max_err);
/* The operand synthesis of the resident sweeps on the caller's data: bsc [nbins][nord_pad] (interleaved complex) are Chebyshev
 * coefficients, x [nx] the arguments (the kernel doubles them as the sweeps do; no clamping), gs = 2, 3 or 4 the group size of the
 * evaluation.  The kernel stages one bin's row in LDS and calls the sweeps' own evaluation; with E / O the even / odd part of
 * sum_m bsc[k][m] T_m(x): g_plus [nbins][nx] = E + O = g(x) and g_minus [nbins][nx] = E - O = g(-x), what an antipodal microphone
 * pair receives.  nord_pad even, 2 ... 96; nbins 1 ... 65535; nx 1 ... 2^24; otherwise EMAGLS_ERR_ARG.  Host pointers, synchronous. */
int emagls_debug_synth_operand(const void* bsc, int nbins, int nord_pad, const double* x, int64_t nx, int gs, void* g_plus, void* g_minus);
/* The argument of that evaluation as the sweeps form it from the angles: x2 [ndirs][nmics] = 2 cos(angle between HRIR direction d and
 * microphone j), clamped to [-2, 2].  A zenith enters through cos(zen) and sqrt(1 - cos^2(zen)), as it enters the SH matrices: a value a
 * rounding outside [0, pi] is the direction mirrored back.  ndirs 1 ... 2^20, nmics 1 ... 64; host pointers, synchronous. */
int emagls_debug_synth_cosines(const double* dir_azi, const double* dir_zen, int64_t ndirs, const double* mic_azi, const double* mic_zen, int nmics, double* x2);
/* The per-bin factor chain on the caller's matrices: the launchers the designs use (assemble or load B_k, Householder QR, one-sided Jacobi,
 * back-transform to Z_k = conj(U) diag(s_reg) V^T with B_k = U S V^H), with their own choice of kernel for the shape and their own refusals
 * (EMAGLS_ERR_UNSUPPORTED).  All arrays are host arrays, complex ones interleaved; the call is synchronous.
 *   path 0: the forms for up to 32 columns and 4096 rows; path 1: the forms for up to 64 columns; path 2: the tiled form of those (row
 *   blocks and a tree step over their triangles) for up to 32 columns, ldS <= 16384 and nbins <= 8, its workspace filled with the sentinel
 *   first.  Paths 1 and 2 take dense input, reg_mode 0, phases 3, hq_conj 0 and ldS a multiple of 64; they write zeros into the rows
 *   S ... ldS-1 of Z, and form W by the least-squares kernel the designs run behind these factors (the bins below min(ls_end, nbins)).
 *   leaf_rows (path 2 only; 0 elsewhere): 0 = the library's bound of a row block's height, 1024 ... 4096 = this bound in its place.
 *   On path 2 the optional N, R2 and tau are those of the tree step (the factorisation of the stacked triangles).
 *   Input, dense: Xd [nbins][C][ldS], xd_stride = C ldS, or 0 for one matrix read by every bin; kb0 = 0.  Input, assembled (Xd null):
 *   B_k = sum_n bn[k][n] Tn[n], Tn [nOrders][C][ldS] real (tn_cplx = 0) or complex, bn [P][nOrders], for the bins k = kb0 ... kb0+nbins-1;
 *   row s takes the orders n with (n+1)^2 > s only, and bin P-1 (Nyquist) the real part of bn.
 *   reg_mode 0: s_reg = 1 / max(s, reg_c s_max); reg_mode 1: s_reg = 1 / s above tol_dim eps(s_max) and 0 below (MATLAB pinv).
 *   Hq (optional) [2][nbins][ldHq], ldHq >= S: W[e][k][c] = sum_s Hq[e][k-kb0][s] Z_k[c][s] for k < ls_end (hq_conj != 0: Hq holds the
 *   conjugate of those rows).  phases 3: one call of the launcher; 12: its phase 1 (QR, Jacobi) and phase 2 (back-transform) in two calls.
 *   Outputs: Z [nbins][C][ldS] (required) and W [2][P][C] are filled with the quiet NaN of bits EMAGLS_DEBUG_SENTINEL_BITS before the
 *   launch, so what the kernels leave alone shows; optional sv [nbins][C] (unsorted), sweeps [nbins], N and R2 [nbins][C][C], tau [nbins][C].
 * 1 <= S <= ldS <= 4096, 1 <= C <= 64, 1 <= nbins <= 4096, kb0 + nbins <= P <= 8192 (path 2: ldS <= 16384, C <= 32, nbins <= 8), no more
 * than 1 GiB of device memory, the workspace of path 2 included; otherwise EMAGLS_ERR_ARG before the device is touched. */
#define EMAGLS_DEBUG_SENTINEL_BITS 0x7ff8dead0000beefULL
typedef struct {
    int S, C, ldS, nbins, kb0, P;
    const void* Xd;
    int64_t xd_stride;
    const void* Tn;
    int tn_cplx;
    const void* bn;
    int nOrders;
    int reg_mode;
    double reg_c, tol_dim;
    const void* Hq;
    int64_t ldHq;
    int ls_end, hq_conj;
    int phases, path;
    void* Z;
    double* sv;
    int* sweeps;
    void* N;
    void* R2;
    double* tau;
    void* W;
    int leaf_rows;
} emagls_debug_factor_args;
int emagls_debug_factor(const emagls_debug_factor_args* args);
/* Y_reg_inv of the designs with 33 ... 64 channels on the caller's arrays, by the launcher the designs use (launch_wa_yri; the scalar or the
 * matrix-core form by EMAGLS_WA_YRI_MFMA, read per call): Yri[k][c][d] = sum_s Q[d][s] Z[k][c][s], Q [D][ldQ] real, Z [nbins][C][ldS] and
 * Yri [nbins][C][ldD] complex.  Host arrays, synchronous; Yri is filled with the NaN of EMAGLS_DEBUG_SENTINEL_BITS before the launch (the
 * columns D ... ldD-1 keep it).  1 <= C <= 64, 1 <= S <= ldS <= 16384, S <= ldQ <= 16384, 1 <= D <= ldD <= 65536, 1 <= nbins <= 4096, no more
 * than 1 GiB of device memory; otherwise EMAGLS_ERR_ARG before the device is touched. */
int emagls_debug_wa_yri(const double* Q, int64_t ldQ, const void* Z, int S, int C, int ldS, int D, int64_t ldD, int nbins, void* Yri);
/* The Jacobi kernel of that chain in its Gram form, as the Gram route of the designs runs it: A [nbins][C][C] = B_k^H B_k, full Hermitian;
 * route [nbins] = 1 (factor this bin) or 2 (skip it: its M keeps the sentinel, sweeps = -1); a workgroup walks jrun (1 ... 16) neighbouring
 * bins and starts each from the rotations of the one before.  M [nbins][C][C] = V diag(s_reg / s) V^H with s = sqrt(eig(A)) and
 * s_reg = 1 / max(s, reg_c s_max); sv [nbins][C], sweeps [nbins]; status [4]: [2] = 1 and [3] = the highest bin with s_max > cond_limit s_min. */
int emagls_debug_factor_gram(const void* A, int nbins, int C, const int* route, int jrun, double reg_c, double cond_limit, void* M, double* sv, int* sweeps,
                             int* status);
/* The Gram route of the array designs, step by step, on the caller's arrays: the launchers the designs use (launch_gram, launch_gram_kmat,
 * launch_gram_gemm, launch_gram_from_g, launch_gram_solve) with their own dispatch.  Host arrays, row major, complex ones interleaved;
 * synchronous; outputs are filled with the NaN of EMAGLS_DEBUG_SENTINEL_BITS (int outputs with -1) before the launch unless said otherwise;
 * what a plan zero-fills once is zero-filled here, with the plan's padded leading dimensions.  No entry takes more than 1 GiB of device
 * memory; arguments outside the ranges below: EMAGLS_ERR_ARG before the device is touched.  round_up(x, m): the next multiple of m.
 *   emagls_debug_gram: Yc [D][ld], real (is_cplx 0) or complex -> G [S][S] = Yc^H Yc and R [Sh][Sh], its leading block.  The device copy of
 *     Yc has gram_dpad rows, those from D on zero.  G and R hold the upper BLOCK triangle (64 x 64 tiles; inside a diagonal tile both
 *     triangles), zeros below it.  1 <= Sh <= S <= ld <= 8192, 1 <= D <= 65536.
 *   emagls_debug_gram_assemble: A_k = sum_{n,n'} conj(b_n(k)) b_n'(k) K_nn', K_nn' = conj(E_n) Gy[n,n'] E_n'^T, for the bins kb0 ... kb0+nbins-1,
 *     as packed Hermitian rows.  Gy [S][S], S = nOrd^2, only its upper triangle is read; E [C][ldE], ldE >= S; bn [P][nOrd] complex; bin P-1
 *     (Nyquist) takes real(b_n); real or complex arithmetic of Gy and E by is_cplx.  Outputs, with Kp = round_up(nOrd^2, 4),
 *     ldK = round_up(C^2, 64), ldC = round_up(P, 64):
 *       F (optional) [nOrd][C][ldE], F[n][c][s] = sum_{j in order n} Gy(s, j) E[c][j] for s < (n+1)^2, the rest keeps the sentinel;
 *       Kmat [Kp][ldK], zero-filled first: row n = (K_nn + K_nn^H) / 2, rows nOrd + 2 q and nOrd + 2 q + 1 = K_nn' + K_nn'^H and
 *         i (K_nn' - K_nn'^H) for the q-th pair n < n' in lexicographic order; a Hermitian X [C][C] is packed into C^2 reals as
 *         P[c C + c'] = Re X[c][c'] for c <= c' and Im X[c'][c] for c > c';
 *       Cf [Kp][ldC], zero-filled first: Cf[row][k - kb0] = the coefficient of that row, |b_n|^2, Re and Im of conj(b_n) b_n';
 *       Apk [nbins][ldK] = Cf^T Kmat (FP64 MFMA over all Kp rows: the zero rows of Kmat and Cf are part of the product).
 *     Kmat_in non-null (Gy and E null): the product alone, on the caller's Kmat_in [Kp][ldK] taken as it is, pad rows included.
 *     1 <= C <= 32, 1 <= nOrd <= 96, 1 <= nbins, 0 <= kb0, kb0 + nbins <= P <= 8192.
 *   emagls_debug_gram_from_g: G [nbins + kb0 - g0][C][ldD] complex, bin k at slot k - g0 -> Apk [nbins][round_up(C^2, 64)], row k - kb0 the
 *     packed A_k = G_k^H G_k over the D directions.  1 <= C <= 32, 1 <= D <= ldD <= 65536, 0 <= g0 <= kb0, 1 <= nbins <= 8192.
 *   emagls_debug_gram_solve: Apk [nbins][ldA] packed, ldA >= C^2 -> for every bin k = kb0 + i the direct inverse M_k = A_k^-1 (route 2) where
 *     (||A||_F ||A^-1||_F)^2 <= 1 / reg_c^4 certifies cond_2(A_k) <= 1 / reg_c^2, else the unpacked A_k for the Jacobi kernel (route 1).  With
 *     P = kb0 + nbins: Mw and R2w [P][C][C] complex, bin k at slot k - 1; sv [P][C] (route 2: sv[k][0] = ||A||_F^(1/2) >= s_max, the others
 *     ||A^-1||_F^(-1/2) <= s_min); route [P]; sweeps [P] (route 2: 0).  1 <= C <= 32, 1 <= kb0, 1 <= nbins, P <= 8192, 0 < reg_c <= 1. */
int emagls_debug_gram(const void* Yc, int64_t D, int S, int64_t ld, int is_cplx, int Sh, void* G, void* R);
int emagls_debug_gram_assemble(const void* Gy, const void* E, int ldE, const void* bn, int C, int nOrd, int P, int kb0, int nbins, int is_cplx,
                               const double* Kmat_in, void* F, double* Kmat, double* Cf, double* Apk);
int emagls_debug_gram_from_g(const void* G, int D, int C, int64_t ldD, int kb0, int g0, int nbins, double* Apk);
int emagls_debug_gram_solve(const double* Apk, int ldA, int C, int kb0, int nbins, double reg_c, void* Mw, void* R2w, double* sv, int* route,
                            int* sweeps);
/* The transforms at both ends of a design on the caller's arrays: the launchers the designs use, with their own choice of kernel for the
 * shape (radix-2 in LDS for a power of two, wave-private at nfft 1024, direct sums otherwise) and the table of launch_twiddles.  Host
 * arrays, complex ones interleaved; synchronous; every output is filled with the NaN of EMAGLS_DEBUG_SENTINEL_BITS before the launch.
 * Arguments outside the ranges below: EMAGLS_ERR_ARG before the device is touched.
 *   emagls_debug_twiddles: tw [nfft] = exp(-2 pi i j / nfft); 2 <= nfft <= 8192.
 *   emagls_debug_filter_epilogue: W [n_ears][nfft/2+1][C] positive-frequency spectra -> outL, outR [C][len], real (out_cplx 0) or complex.
 *     dc_rule 1: W(0) := Re W(1).  conj_mode 0: Hermitian mirror; 1: W(nfft-k,(n,m)) = (-1)^m conj(W(k,(n,-m))), C a square; 2:
 *     W(nfft-k,m) = conj(W(k,-m)) on the channels [0,-1,+1,-2,+2,...], C odd.  shift_mode 0: delay by nfft/2 (left) and
 *     (nfft/2 + grpd[1]) - grpd[0] (right) as a phase, the Nyquist phase real; 1: rotation by nfft/2.  The len samples around nfft/2 are
 *     kept and faded with hann(2 round(fade_rel len)).  nfft even, 4 ... 4096; len even, 2 ... nfft; 1 <= C <= 1024; n_ears 1 (grpd and
 *     outR may be null) or 2; 0 <= fade_rel <= 0.5.
 *   emagls_debug_hrir_spectra: hL, hR [D_src][L] -> the two group delays (median over the bins of the delay of the sum over all D_src
 *     directions), grpd_out [2], and the delay phases the median kernel leaves behind them, phs [2][nfft/2+1] complex; then the spectra
 *     of the D directions didx [D] selects (null: the first D), delayed by -grpd (mode 0, a phase) or rotated by -round(grpd) (mode 1):
 *     Hc [2][n_c][ldD] complex for the bins below n_c, Habs [2][nfft/2+1-kabs0][ldD] for the bins from kabs0, and optionally HcT [D][ldT],
 *     HcT[d][2 (e n_c + k) + re/im].  Hc, Habs and HcT all null: the delays only (L up to 4096; the spectra take L <= nfft).
 *     grpd_in [2] (optional): these delays instead of the computed ones, phs then keeps the sentinel; not taken at mode 0 with nfft 1024,
 *     where a kernel form reads phs.  nfft even, 4 ... 2048; ldD a multiple of 8; ldT even, >= 4 n_c; |grpd_in| <= 2^20.
 *   emagls_debug_real_spectra: x [ncols_src][L] real -> out [nfft/2+1][ldo] complex, column j = colidx[j] (null: j) of x, zero-padded or
 *     cut to nfft, at (j / inner) ld_inner + j % inner.  nfft even, 4 ... 4096; L <= 8192. */
int emagls_debug_twiddles(int nfft, void* tw);
int emagls_debug_filter_epilogue(const void* W, int C, int nfft, int len, const double* grpd, int conj_mode, int dc_rule, int shift_mode, int out_cplx,
                                 int n_ears, double fade_rel, void* outL, void* outR);
int emagls_debug_hrir_spectra(const double* hL, const double* hR, int64_t L, int64_t D_src, int64_t D, const int64_t* didx, int nfft, int mode, int n_c,
                              int kabs0, const double* grpd_in, int64_t ldD, int ldT, double* grpd_out, void* phs, void* Hc, double* Habs, double* HcT);
int emagls_debug_real_spectra(const double* x, int64_t L, int64_t ncols_src, int64_t ncols, const int64_t* colidx, int nfft, int64_t ldo, int64_t inner,
                              int64_t ld_inner, void* out);

/* ---- kernel-level entry points ------------------------------------------------------------- */

/* Y [ndirs x (order+1)^2], column-major; real (8 B) or interleaved complex (16 B) per entry. */
int emagls_sh_basis(int order, int64_t ndirs, const double* azi, const double* zen, int basis, void* Y);

/* Same kernel on buffers that are already in HBM, enqueued on `stream` (a hipStream_t, NULL = default
 * stream) without any staging copy or synchronisation: used for the bandwidth measurement of the
 * SH-basis assembly and by callers that keep their data on the device. */
int emagls_sh_basis_device(int order, int64_t ndirs, const double* d_azi, const double* d_zen, int basis, void* d_Y,
                           void* stream);

/* bn [nfreq x (order+1)] interleaved complex, column-major: rigid-sphere modal coefficients b_n(kr). */
int emagls_modal_bn(int order, int64_t nfreq, const double* kr, void* bn);

/* ---- one-shot filter design (signatures follow the MATLAB functions) ------------------------ */

int emagls_get_ls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                          const double* hrir_azi, const double* hrir_zen, int order, int basis,
                          void* wL, void* wR /* [nsamp x (order+1)^2] */);

int emagls_get_magls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                             const double* hrir_azi, const double* hrir_zen, int order, double fs, int64_t len,
                             int basis, void* wL, void* wR /* [len x (order+1)^2] */);

int emagls_get_emagls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                              const double* hrir_azi, const double* hrir_zen, double mic_radius,
                              const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                              int64_t len, int basis, void* wL, void* wR /* [len x (order+1)^2] */);

int emagls_get_emagls2_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                               const double* hrir_azi, const double* hrir_zen, double mic_radius,
                               const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                               int64_t len, int basis, void* wL, void* wR /* [len x nmics] */);

/* Equatorial microphone array (all microphones at zenith pi/2), filters in circular harmonics ordered
 * [C_0, C_-1, C_1, ..., C_-N, C_N]: wL, wR [len x (2*order+1)], real or complex like the basis. */
int emagls_get_emagls_filters_ema_in_ch(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                                        const double* hrir_azi, const double* hrir_zen, double mic_radius,
                                        const double* mic_azi, int64_t nmics, int order, double fs, int64_t len, int basis,
                                        void* wL, void* wR);

/* The same designs with a custom shFunction (lib/getEMagLsFilters.m:32,68; dependencies/getSMAIRMatrix.m:101): a function handle
 * cannot cross a C ABI, so the MATLAB-side wrapper evaluates it and passes the matrices -- Y_hrir = shFunction(n, [azi zen],
 * shDefinition) [ndirs x (n+1)^2] and Y_mic = shFunction(n, micGrid, shDefinition) [nmics x (n+1)^2], column-major, real or
 * interleaved complex like `basis`, with n = emagls_simulation_order(kind, order, fs, mic_radius) (n = order for LS / MagLS). */
int emagls_simulation_order(int kind, int order, double fs, double mic_radius);
int emagls_get_ls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir, int order,
                                     int basis, void* wL, void* wR);
int emagls_get_magls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir, int order,
                                        double fs, int64_t len, int basis, void* wL, void* wR);
int emagls_get_emagls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir,
                                         double mic_radius, const void* Y_mic, int64_t nmics, int order, double fs, int64_t len,
                                         int basis, void* wL, void* wR);
int emagls_get_emagls2_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir,
                                          double mic_radius, const void* Y_mic, int64_t nmics, int order, double fs, int64_t len,
                                          int basis, void* wL, void* wR);

/* lib/getEMagLsFiltersEMAinSH.m:1-2 -- [wMlsL, wMlsR] = getEMagLsFiltersEMAinSH(hL, hR, hrirGridAziRad, hrirGridZenRad, micRadius,
 * micGridAziRad, order, fs, len, shDefinition): equatorial array (zenith pi/2 for every microphone), filters [len x (order+1)^2] */
int emagls_get_emagls_filters_ema_in_sh(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                                        const double* zen, double mic_radius, const double* mic_azi, int64_t nmics, int order,
                                        double fs, int64_t len, int basis, void* wL, void* wR);

/* atf_irs [atf_taps x nmics x natf]; outputs real [filter_len x nmics];
 * mean_grid_dev_deg (optional) receives the value the reference prints (getEMagLsFiltersFromAtf.m:96).
 * Up to 64 microphones.  Up to 32, a bin whose matched ATF matrix is well conditioned (cond < 3e4) is solved from its M x M Gram
 * matrix; where a bin is not -- clean or simulated ATFs of a sphere-mounted array at low frequencies -- the bins up to it are
 * factored from the matrix itself (Householder QR + Jacobi SVD, the reference's 1 % clip), at any width and any supported number of
 * matched directions (above 4096 in row blocks with a tree step over their triangles).  The first execute of such a set runs twice; a plan keeps the moved route. */
int emagls_get_emagls_filters_from_atf(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                                       const double* hrir_azi, const double* hrir_zen, const double* atf_irs,
                                       int64_t atf_taps, int64_t nmics, int64_t natf, const double* atf_azi,
                                       const double* atf_zen, double fs, int64_t filter_len, double f_trans,
                                       double* wL, double* wR, double* mean_grid_dev_deg);

/* out [nsamp_out x 2] real, nsamp_out = nsamp (compensate_delay == 0) or nsamp - len/2 + 1 (!= 0).
 * in [nsamp x nch], wL/wR [len x nch], all real. */
int emagls_binaural_decode(const double* in, int64_t nsamp, int64_t nch, const double* wL, const double* wR,
                           int64_t len, int compensate_delay, double* out);

/* Complex-SH rendering (dependencies/binauralDecode.m:39-42,59-64: complex products accumulated, real part kept).
 * in [nsamp x nch] and wL / wR [len x nch] are interleaved complex where the flag says so, real otherwise; out as above, real.
 * imag_abs_sum (optional, [2]) receives sum(abs(imag(.))) of the discarded imaginary part per ear, the two numbers the
 * reference prints in its warning (:61-62) -- over the samples that are returned, i.e. after the compensate_delay cut (:53-57). */
int emagls_binaural_decode_complex(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                   int filters_are_complex, int64_t len, int compensate_delay, double* out, double* imag_abs_sum);

/* The render loop on buffers that are already in HBM (no staging copies, no allocation after the first call of a shape): d_in
 * [nsamp x nch], d_wL / d_wR [len x nch] real or interleaved complex as flagged, d_out [nsamp x 2] real (no delay cut: the caller
 * offsets its read).  Enqueued on `stream` (hipStream_t, NULL = default) and synchronised before returning (the hipFFT work
 * buffers are shared per process).  What bench.py times for north_star item (iii). */
int emagls_binaural_decode_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL, const void* d_wR,
                                  int filters_are_complex, int64_t len, double* d_out, double* imag_abs_sum, void* stream);

/* Channel layouts of the yaw rotation: SH in ACN order, (N+1)^2 channels; CH in getCH's order [C_0, C_-1, C_1, ..., C_-N, C_N],
 * 2N+1 channels (dependencies/getCH.m:17-28). */
#define EMAGLS_LAYOUT_SH 0
#define EMAGLS_LAYOUT_CH 1

/* Yaw rotation of an SH or CH signal (the yaw part of the rotateHOA_N3D call in dependencies/binauralDecode.m:27-31).  OWN
 * SPECIFICATION: rotating by yaw turns the sound field counter-clockwise about z, seen from above, so the
 * signal of a plane wave from azimuth a -- conj(getSH(N, [a zen], basis)) or conj(getCH(N, a, basis)) -- becomes the one of the
 * plane wave from a + yaw.  Only (n, m) and (n, -m) mix, through cos(m yaw) and sin(m yaw); the normalisation does not matter.
 * yaw is reduced modulo 2 pi in FP64 before m yaw is formed.
 * in [nsamp x nch] real or interleaved complex as flagged; yaw [n_yaw], n_yaw = 1 (one angle) or nsamp (one angle per sample);
 * out [nsamp x nch], interleaved complex when in_is_complex or basis == EMAGLS_BASIS_COMPLEX, real otherwise.  A channel count
 * that does not fit the layout is EMAGLS_ERR_ARG. */
int emagls_rotate_yaw(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int layout, int basis, const double* yaw,
                      int64_t n_yaw, void* out);

/* dependencies/binauralDecode.m:1-64 without the resampling (emagls_binaural_decode_render_fs adds it): emagls_binaural_decode_complex's
 * arguments, plus
 *  - the yaw rotation of the input (layout, basis, yaw [n_yaw]; n_yaw = 0: none, 1: one fixed angle, applied to the decoding
 *    filters, nsamp: one angle per input sample, applied to the signal), and
 *  - the source-signal convolution of :44-48 (signal [n_signal], the first column of the reference's `signal`; NULL or
 *    n_signal = 0: none): out(:, e) = fftfilt(ear_e, signal), ear_e being the rendered impulse response of ear e.
 * out [nout x 2] real, nout = (n_signal > 0 ? n_signal : nsamp) - (compensate_delay ? len/2 - 1 : 0): the cut uses the decoding
 * filters' length (:53-57).  imag_abs_sum (optional, [2]) as for emagls_binaural_decode_complex, over the returned samples.
 * Without rotation and signal this is emagls_binaural_decode_complex (emagls_binaural_decode when nothing is complex). */
int emagls_binaural_decode_render(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                  int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                  int64_t n_yaw, const double* signal, int64_t n_signal, double* out, double* imag_abs_sum);

/* emagls_binaural_decode_render on buffers that are already in HBM, on the model of emagls_binaural_decode_device: d_yaw and
 * d_signal are device arrays too; d_out [nout x 2], nout = n_signal > 0 ? n_signal : nsamp, without the delay cut. */
int emagls_binaural_decode_render_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                         const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis,
                                         const double* d_yaw, int64_t n_yaw, const double* d_signal, int64_t n_signal, double* d_out,
                                         double* imag_abs_sum, void* stream);

/* Three-axis rotation of an SH signal (rotateHOA_N3D(in, yaw, pitch, roll), called by dependencies/binauralDecode.m:27-31).  OWN
 * SPECIFICATION: axes of getSH (x front, y left, z up); R = Rz(yaw) Ry(pitch) Rx(roll), each factor a
 * right-handed active rotation about a fixed axis; the signal of a plane wave from u, conj(getSH(N, u, basis)), becomes the one
 * of the plane wave from R u.  yaw = pi/2 moves the front to the left, pitch = pi/2 the front to the floor, roll = pi/2 the left
 * to the top; with pitch = roll = 0 this is emagls_rotate_yaw.  SH orders 0 to 15 ((N+1)^2 channels, ACN); a higher order is
 * EMAGLS_ERR_UNSUPPORTED.
 * M [(N+1)^2 x (N+1)^2] column-major (interleaved complex for the complex basis): the rotation is out_row = in_row M^T; M is
 * block-diagonal by order, orthogonal (real basis) or unitary (complex basis). */
int emagls_sh_rotation_matrix(int order, int basis, double yaw, double pitch, double roll, void* out);

/* in [nsamp x nch] real or interleaved complex as flagged; each of yaw [n_yaw], pitch [n_pitch], roll [n_roll] has 0 (absent: 0),
 * 1 (one angle) or nsamp values (one per sample); out [nsamp x nch], interleaved complex when in_is_complex or basis ==
 * EMAGLS_BASIS_COMPLEX.  When every pitch and roll value is 0 this is emagls_rotate_yaw, bit for bit. */
int emagls_rotate_sh(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int basis, const double* yaw, int64_t n_yaw,
                     const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, void* out);

/* emagls_binaural_decode_render with the three-axis rotation: pitch [n_pitch] and roll [n_roll] as yaw (0, 1 or nsamp values
 * each).  Every count <= 1: a fixed rotation, applied to the decoding filters; otherwise a per-sample pass over the signal.  A CH
 * layout with a nonzero pitch or roll is EMAGLS_ERR_ARG.  When every pitch and roll value is 0 this is
 * emagls_binaural_decode_render, bit for bit. */
int emagls_binaural_decode_render_ypr(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                      int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                      int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll,
                                      const double* signal, int64_t n_signal, double* out, double* imag_abs_sum);

/* emagls_binaural_decode_render_ypr on device buffers (angles and signal included), as emagls_binaural_decode_render_device;
 * n_pitch == n_roll == 0 is emagls_binaural_decode_render_device. */
int emagls_binaural_decode_render_ypr_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                             const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis, const double* d_yaw,
                                             int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                                             const double* d_signal, int64_t n_signal, double* d_out, double* imag_abs_sum, void* stream);

/* Resampling with the semantics of MATLAB's resample(x, p, q) at its defaults N = 10, bta = 5 (the calls of
 * dependencies/binauralDecode.m:12-23).  OWN RESTATEMENT of resample.m: p / q is reduced by their gcd;
 * m = max(p, q), a Kaiser-windowed (bta 5) sinc of 20 m + 1 taps with cut-off 1/(2m), scaled to p / sum; the polyphase filter
 * applied to each column with the alignment of resample.m.  MATLAB's own tap values are not pinned.
 * emagls_resample_length: ceil(nsamp p / q); -1 when nsamp < 0 or p or q < 1. */
int64_t emagls_resample_length(int64_t nsamp, int64_t p, int64_t q);

/* in [nsamp x nch] real or interleaved complex as flagged (complex: the real taps applied to both parts); out
 * [ceil(nsamp p / q) x nch] of the same type.  p, q >= 1 (else EMAGLS_ERR_ARG); max(p, q) > 65536 after reduction is
 * EMAGLS_ERR_UNSUPPORTED; p == q copies.  The taps of a ratio are designed once and kept per device (emagls_cache_clear frees
 * them). */
int emagls_resample(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int64_t p, int64_t q, void* out);

/* emagls_resample on device buffers, enqueued on `stream` (hipStream_t, NULL = default) and not synchronised. */
int emagls_resample_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, int64_t p, int64_t q, void* d_out,
                           void* stream);

/* emagls_binaural_decode_render_ypr plus the three rates of dependencies/binauralDecode.m:1-2 (positive, integer-valued doubles,
 * else EMAGLS_ERR_ARG): the decoding filters are resampled from filter_fs to in_fs (len' = ceil(len in_fs / filter_fs) taps) and
 * the signal from signal_fs to in_fs (n_signal' = ceil(n_signal in_fs / signal_fs) samples; signal_fs is looked at only when there
 * is a signal), on the device, before the rotation (:12-23).  out [nout x 2], nout = (n_signal > 0 ? n_signal' : nsamp) -
 * (compensate_delay ? len'/2 - 1 : 0).  With filter_fs == in_fs and signal_fs == in_fs this is emagls_binaural_decode_render_ypr,
 * bit for bit. */
int emagls_binaural_decode_render_fs(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                     int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                     int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll,
                                     const double* signal, int64_t n_signal, double in_fs, double filter_fs, double signal_fs, double* out,
                                     double* imag_abs_sum);

/* emagls_binaural_decode_render_fs on device buffers, as emagls_binaural_decode_render_ypr_device: d_out [nout x 2], nout =
 * n_signal > 0 ? n_signal' : nsamp, without the delay cut. */
int emagls_binaural_decode_render_fs_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                            const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis, const double* d_yaw,
                                            int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                                            const double* d_signal, int64_t n_signal, double in_fs, double filter_fs, double signal_fs,
                                            double* d_out, double* imag_abs_sum, void* stream);

/* ---- block-streaming decode: a head-tracked renderer gets audio and the head orientation a block at a time ----
 * A decode stream is created once from the decoding filters and then fed consecutive blocks of the input signal, each with the
 * orientation for that block; every push returns the two ear signals of the samples it was given (nothing is held back, and the
 * output depends only on samples already pushed).  With x the concatenation of all pushed blocks and yaw / pitch / roll the
 * concatenation of their per-sample angles, the concatenated outputs equal, to rounding,
 * emagls_binaural_decode_render_ypr(x, ..., compensate_delay = 0, yaw, pitch, roll, no signal): the per-sample rotation of the
 * signal, then sum_c fftfilt(w_c, x_c).  No delay cut (the caller offsets its read), no resampling; a dry source signal goes
 * through its room response in a field stream (emagls_field_stream_*, below), whose output a push here takes as it lies.
 * For complex signals or filters the output is the real part (dependencies/binauralDecode.m:59-64); the stream does NOT report
 * the discarded imaginary sum.
 * Uniformly partitioned overlap-save: block = B samples, a power of two from 64 to 2048 (anything else
 * is EMAGLS_ERR_UNSUPPORTED); 1 <= len <= 16384 (longer: EMAGLS_ERR_UNSUPPORTED); tested up to 256 channels.  The state (a ring of ceil(len / B) pending output spectra
 * per ear, the previous block, the ring position) lives in device memory; pushes of equal size differ only in the caller's
 * pointers; equal pushes on fresh streams give equal bits.
 * wL / wR [len x nch] host arrays, interleaved complex when filters_are_complex.  in_is_complex: the pushed blocks are
 * interleaved complex.  layout / basis: of the rotation (EMAGLS_LAYOUT_*, EMAGLS_BASIS_*).  Every argument is checked before the
 * device is touched.  The stream is bound to the device that is current at creation (without a device the object still exists,
 * so that argument errors can be reported, and its first push fails with EMAGLS_ERR_HIP).  emagls_cache_clear() does not
 * touch a live stream.  One push at a time per stream. */
typedef struct emagls_decode_stream emagls_decode_stream;
int emagls_decode_stream_create(int64_t nch, const void* wL, const void* wR, int filters_are_complex, int64_t len, int in_is_complex,
                                int layout, int basis, int64_t block, emagls_decode_stream** s);

/* in [nsamp x nch] host array, nsamp = k * block (k blocks are run in order inside the call; else EMAGLS_ERR_ARG); each of yaw
 * [n_yaw], pitch [n_pitch], roll [n_roll] has 0 values (absent: 0), 1 (constant over this push) or nsamp (one per sample),
 * anything else is EMAGLS_ERR_ARG; out [nsamp x 2].  Angles need a channel count that fits the layout (EMAGLS_ERR_ARG); a CH
 * layout takes yaw only; pitch or roll above SH order 15 is EMAGLS_ERR_UNSUPPORTED.  When every pitch and roll value of the
 * push is 0 the push takes the yaw rule, as the offline call does. */
int emagls_decode_stream_push(emagls_decode_stream* s, const void* in, int64_t nsamp, const double* yaw, int64_t n_yaw,
                              const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, double* out);

/* emagls_decode_stream_push on device arrays (the angles included), on the model of emagls_binaural_decode_render_ypr_device:
 * enqueued on `stream` (hipStream_t, NULL = default) and NOT synchronised; no allocation, no copy of state.  At most three
 * kernel launches per block (rotation, forward transform with the products, inverse transform).  Device angle arrays are not
 * read by the host: only absent pitch and roll (counts 0) make a push yaw-only. */
int emagls_decode_stream_push_device(emagls_decode_stream* s, const void* d_in, int64_t nsamp, const double* d_yaw, int64_t n_yaw,
                                     const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll, double* d_out,
                                     void* stream);

/* Zero history: what follows equals a fresh stream bit for bit.  Waits for the pushes in flight. */
int emagls_decode_stream_reset(emagls_decode_stream* s);

/* block, partitions = ceil(len / block), state_bytes (ring, previous block and position: what a push reads and writes besides
 * the filter spectra), filter_bytes (the partition spectra, written once) and the kernel launches per block (each output
 * optional). */
int emagls_decode_stream_info(const emagls_decode_stream* s, int64_t* block, int64_t* partitions, int64_t* state_bytes,
                              int64_t* filter_bytes, int* launches_per_block);

int emagls_decode_stream_destroy(emagls_decode_stream* s);

/* ---- a bank of filter sets on a decode stream, cross-faded per block ----
 * Filters that act on raw microphone signals (eMagLS2, FromAtf, EMAinCH) cannot follow the head by rotating the signal: the
 * orientation goes into the FILTERS, one set per orientation, and the renderer changes set as the head moves.  The same serves
 * to switch between designs or HRTF subjects while the sound plays.  A bank stream holds n_sets >= 1 filter sets of one shape;
 * every block t of B samples has a set index s_t.  Sample i of block t (i = 0 .. B - 1) goes to set s_t with the gain 1 when
 * s_t == s_(t-1); otherwise to s_t with r[i] = (i + 1) / B and to s_(t-1) with 1 - r[i]; s_(-1) := s_0 (the first block after
 * creation or reset does not fade).  With x the concatenated (and, where the push has angles, rotated) input and g_s the gain
 * of set s per sample, the concatenated outputs equal, to rounding, sum_s decode(g_s x, wL_s, wR_s): the filter a sample meets
 * is the one of the moment it was pushed, linearly interpolated across the block that changes.  A constant index gives the
 * plain stream's bits.  A block is still at most three kernel launches; a block whose window [x_(t-1), x_t] meets k = 1, 2 or 3
 * distinct sets costs k forward transforms.  Where the host knows that the set stands (the indices of this block and the two
 * before it came from host arrays or were kept, n_set = 0) the block runs the plain stream's kernel on that set; indices given in
 * device memory are decided upon in the kernel.
 * wL / wR: n_sets consecutive [len x nch] arrays.  n_sets < 1: EMAGLS_ERR_ARG; above 65536: EMAGLS_ERR_UNSUPPORTED.  Everything
 * else as emagls_decode_stream_create, which is the bank of one set; push, reset (which also forgets the selection), info
 * (filter_bytes grows with n_sets; state_bytes counts the two previous set indices when n_sets > 1) and destroy are shared. */
int emagls_decode_stream_create_bank(int64_t nch, int64_t n_sets, const void* wL, const void* wR, int filters_are_complex, int64_t len,
                                     int in_is_complex, int layout, int basis, int64_t block, emagls_decode_stream** s);

/* emagls_decode_stream_push with set indices: set [n_set], n_set = 0 (every block keeps the set of the block before it; set 0
 * on a fresh stream), 1 (every block of this push) or nsamp / block (one per block); anything else, a null array with
 * n_set > 0, or an index outside [0, n_sets - 1] is EMAGLS_ERR_ARG, reported before the device is touched.
 * emagls_decode_stream_push is this call with n_set = 0. */
int emagls_decode_stream_push_sets(emagls_decode_stream* s, const void* in, int64_t nsamp, const int32_t* set, int64_t n_set,
                                   const double* yaw, int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll,
                                   int64_t n_roll, double* out);

/* emagls_decode_stream_push_device with set indices in device memory: d_set is not read by the host (the call still only
 * enqueues), so the kernels clamp every index into [0, n_sets - 1] before they form an address from it. */
int emagls_decode_stream_push_sets_device(emagls_decode_stream* s, const void* d_in, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                          const double* d_yaw, int64_t n_yaw, const double* d_pitch, int64_t n_pitch,
                                          const double* d_roll, int64_t n_roll, double* d_out, void* stream);

/* The number of filter sets of the stream's bank. */
int emagls_decode_stream_sets(const emagls_decode_stream* s, int64_t* n_sets);

/* ---- a listener group: many listeners of one sound field in one push ----
 * One bank of n_sets >= 1 filter sets, its spectra stored once, and n_listeners listeners, each with the state a decode stream has
 * (ring, previous block, ring position, the two previous set indices).  One push takes one block of the common signal and, per
 * listener, their angles and their set indices, and returns every listener's pair of ear signals.  DEFINING PROPERTY: listener l's
 * output is, bit for bit, what a decode stream of the same bank returns when it is fed the same blocks with listener l's angles
 * and set indices; the rotation convention, the cross-fade rule and the clamp of device indices are the stream's.  One choice is
 * made per push and not per listener: the push takes the yaw rule when NO listener has a pitch or a roll (host entry: when every
 * pitch and roll value of the push is 0), otherwise every listener goes through the three-axis rotation, as a stream does that is
 * given pitch and roll arrays.  A block is at most three kernel launches for the whole group, whatever n_listeners is.
 * 1 <= n_listeners <= 4096: below, EMAGLS_ERR_ARG; above, EMAGLS_ERR_UNSUPPORTED.  Every other argument and limit as
 * emagls_decode_stream_create_bank; every argument is checked before the device is touched, and the object exists without a
 * device.  emagls_cache_clear() does not touch a live group.  One push at a time per group. */
typedef struct emagls_decode_group emagls_decode_group;
int emagls_decode_group_create(int64_t nch, int64_t n_sets, const void* wL, const void* wR, int filters_are_complex, int64_t len,
                               int in_is_complex, int layout, int basis, int64_t block, int64_t n_listeners, emagls_decode_group** g);

/* in [nsamp x nch], the common signal, nsamp = k * block (else EMAGLS_ERR_ARG); out [L][nsamp x 2], L = n_listeners.  Every array
 * is listener-major.  Each of n_yaw, n_pitch, n_roll is 0 (absent: 0), L (one value per listener, constant over this push) or
 * L * nsamp ([L][nsamp]); n_set is 0 (every listener keeps their set; set 0 on a fresh listener), L (one index per listener for
 * every block of the push) or L * nsamp / block ([L][nsamp / block]).  Any other count, a null array with a positive count, or an
 * index outside [0, n_sets - 1] is EMAGLS_ERR_ARG.  Angles need what a stream's push needs of the layout and the order. */
int emagls_decode_group_push(emagls_decode_group* g, const void* in, int64_t nsamp, const int32_t* set, int64_t n_set, const double* yaw,
                             int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, double* out);

/* emagls_decode_group_push on device arrays: enqueued on `stream` and NOT synchronised; no allocation (the rotated blocks of all
 * listeners have a buffer sized at creation), no copy of state.  Device arrays are not read by the host: only absent pitch and
 * roll make a push yaw-only, and the kernels clamp every set index into [0, n_sets - 1]. */
int emagls_decode_group_push_device(emagls_decode_group* g, const void* d_in, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                    const double* d_yaw, int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll,
                                    int64_t n_roll, double* d_out, void* stream);

/* listener = -1: every listener back to zero history.  0 .. L - 1: that listener alone (ring, overlap, position, selection) -- what
 * a listener who joins gets: what follows equals a fresh stream bit for bit, and the others are untouched.  Anything else is
 * EMAGLS_ERR_ARG.  Waits for the pushes in flight. */
int emagls_decode_group_reset(emagls_decode_group* g, int64_t listener);

/* block, partitions, listeners, state_bytes (grows with the listeners), filter_bytes (does not) and the kernel launches per block
 * of the whole group (each output optional). */
int emagls_decode_group_info(const emagls_decode_group* g, int64_t* block, int64_t* partitions, int64_t* listeners, int64_t* state_bytes,
                             int64_t* filter_bytes, int* launches_per_block);

int emagls_decode_group_destroy(emagls_decode_group* g);

/* ---- the array encoder inside a decode stream or a listener group ----
 * An ENCODED stream (group) is created with an encoder matrix enc [nch x nmics] (column-major like every array here; interleaved
 * complex when enc_is_complex) and is pushed blocks of REAL microphone signals [nsamp x nmics]: the push, push_sets, push_device,
 * push_sets_device and group_push entries above take such blocks on an encoded object, and reset, info, sets and destroy are
 * shared.  DEFINING PROPERTY: its outputs equal, to rounding, those of the stream (group) of the same filters, bank, angles and set
 * indices that is fed x enc^T; a complex enc makes the encoded signal complex, and the stream then runs as one created with
 * in_is_complex.  The encoder runs inside the rotation launch (a push without angles runs it alone), so a block is still at most
 * three launches: the head rotation sits between the encoder and the filters, which is why a head-tracked renderer cannot fold enc
 * into its filters (one that never turns can: w'_m = sum_c enc[c, m] w_c, and a plain stream on nmics channels).
 * The arithmetic is fixed: s_c[t] = sum_m enc[c, m] x[m][t], accumulated from 0 with fma, m ascending, in FP64, the real and the
 * imaginary part as separate chains.  So an identity encoder returns the bits of the plain stream, listener l of an encoded group
 * the bits of an encoded stream, and pushes of one block the bits of pushes of several.
 * 1 <= nmics <= 64 and 1 <= nch <= 64, else EMAGLS_ERR_UNSUPPORTED; nch > nmics is allowed.  A null enc is EMAGLS_ERR_ARG.  nch is
 * the channel count of the filters and of the rotation: a CH layout takes yaw only, pitch or roll needs nch = (N+1)^2.  Everything
 * else as emagls_decode_stream_create_bank / emagls_decode_group_create.  enc is copied at creation and owned by the object
 * (emagls_cache_clear() leaves it alone); info counts it in filter_bytes. */
int emagls_decode_stream_create_encoded(int64_t nmics, const void* enc, int enc_is_complex, int64_t nch, int64_t n_sets, const void* wL,
                                        const void* wR, int filters_are_complex, int64_t len, int layout, int basis, int64_t block,
                                        emagls_decode_stream** s);
int emagls_decode_group_create_encoded(int64_t nmics, const void* enc, int enc_is_complex, int64_t nch, int64_t n_sets, const void* wL,
                                       const void* wR, int filters_are_complex, int64_t len, int layout, int basis, int64_t block,
                                       int64_t n_listeners, emagls_decode_group** g);

/* ---- the field stream: source signals through array room responses, a block at a time ----
 * The auralisation use of the toolbox (testEMagLs.m:66-70, testEMagLsFromAtfs.m:67: fftfilt(srir.rir, sig)) for a head that moves: the
 * rotation sits between the room response and the decoding filters, so the source has to meet the room BEFORE the decode stream.
 * A field stream is created from nsrc room responses rir_q [nr x nch] (q = 0 .. nsrc - 1, one after the other, column-major like
 * every array here; real, or interleaved complex for a complex-SH response) and a block size, and is then fed consecutive blocks
 * of the nsrc REAL source signals, src [nsamp x nsrc] with nsamp = k * block; every push returns the field block [nsamp x nch].
 * DEFINING PROPERTY: with s_q the concatenation of everything pushed for source q, the concatenated outputs equal, to rounding,
 *     x(:, c) = sum_q fftfilt(rir_q(:, c), s_q);
 * nothing is held back, and the output depends only on samples already pushed.  A complex response gives interleaved complex
 * output: its real taps and its imaginary taps each convolved with the real source.  Fed to a decode stream or a listener group
 * (created with in_is_complex in the complex case; responses in the microphone domain feed an encoded one) the chain is
 * source -> room -> rotation -> filters.
 * Uniformly partitioned overlap-save with the state on the device: P = ceil(nr / block) partitions, their spectra written once
 * (response_bytes = nsrc P planes (block + 1) 16, planes = nch, or 2 nch for a complex response), a ring of the last P INPUT
 * spectra per source, the previous block and the ring position (state_bytes).  Two kernel launches per block, no hipFFT, no atomics;
 * the order of every sum is fixed (field_stream.hip), so equal pushes on fresh objects give equal bits, how blocks are grouped into
 * pushes does not change a bit, and pushes of one size differ only in the caller's pointers.
 * Limits, all checked before the device is touched: block a power of two from 64 to 2048; nsrc <= 16; nch <= 256; nr <= 1048576;
 * response_bytes <= 4 GiB -- beyond any of them EMAGLS_ERR_UNSUPPORTED; a count below 1, a null pointer, or nsamp that is not a
 * multiple of block: EMAGLS_ERR_ARG.  The object is bound to the device that is current at creation (without a device it still
 * exists, so that argument errors can be reported and info read, and its first push fails with EMAGLS_ERR_HIP).  It owns its
 * buffers: emagls_cache_clear() leaves it alone.  One push at a time per object. */
typedef struct emagls_field_stream emagls_field_stream;
int emagls_field_stream_create(int64_t nsrc, int64_t nch, const void* rir, int rir_is_complex, int64_t nr, int64_t block,
                               emagls_field_stream** f);

/* src [nsamp x nsrc] host array; out [nsamp x nch], interleaved complex for a complex response.  k = nsamp / block blocks are run in
 * order inside the call; synchronised on return. */
int emagls_field_stream_push(emagls_field_stream* f, const double* src, int64_t nsamp, void* out);

/* The same on device arrays: enqueued on `stream` (hipStream_t, NULL = default) and NOT synchronised; no allocation, no copy of
 * state.  d_out is [nsamp x nch] with the leading dimension nsamp: the d_in of emagls_decode_stream_push_device and
 * emagls_decode_group_push_device as it stands. */
int emagls_field_stream_push_device(emagls_field_stream* f, const double* d_src, int64_t nsamp, void* d_out, void* stream);

/* Zero history: what follows equals a fresh object bit for bit.  Waits for the pushes in flight. */
int emagls_field_stream_reset(emagls_field_stream* f);

/* block, partitions = ceil(nr / block), state_bytes (ring, previous blocks and position), response_bytes (the partition spectra,
 * written once) and the kernel launches per block (each output optional). */
int emagls_field_stream_info(const emagls_field_stream* f, int64_t* block, int64_t* partitions, int64_t* state_bytes,
                             int64_t* response_bytes, int* launches_per_block);

int emagls_field_stream_destroy(emagls_field_stream* f);

/* ---- a bank of room responses on a field stream, cross-faded per block ----
 * A source that moves through measured or simulated positions: the bank holds n_sets >= 1 response sets of one shape, rir[s][q]
 * [nr x nch] (s = 0 .. n_sets - 1, q = 0 .. nsrc - 1), and every source q has its OWN set index per block, s_(q,t).  With
 * r[i] = (i + 1) / block, sample i of block t of source q goes to set s_(q,t) with the gain 1 when s_(q,t) == s_(q,t-1);
 * otherwise to s_(q,t) with r[i] and to s_(q,t-1) with 1 - r[i]; s_(q,-1) := s_(q,0) (the first block after creation or reset
 * does not fade).  DEFINING PROPERTY: with g_(s,q) the gain of set s per sample of source q and x_q everything pushed for it, the
 * concatenated outputs equal, to rounding,
 *     out(:, c) = sum_q sum_s fftfilt(rir[s][q](:, c), g_(s,q) .* x_q):
 * the response a sample meets is that of the moment it was emitted, linearly interpolated across the block that changes.
 * The ring of input spectra holds up to three tagged entries per slot (a window [previous block, block] meets at most the sets of
 * the blocks t - 2, t - 1 and t), each multiplied with the partition spectra of its own set; empty entries are skipped.  Still two
 * launches per block, no atomics, every order fixed.  With every index constant the bank returns the BITS of the plain field stream
 * of that set's responses.  A bank of one set IS the plain field stream: same kernels, same state, same info.
 * rir: n_sets consecutive groups of nsrc [nr x nch] arrays.  n_sets < 1: EMAGLS_ERR_ARG; above 65536: EMAGLS_ERR_UNSUPPORTED; the
 * 4 GiB cap holds for the whole bank's response_bytes = n_sets nsrc P planes (block + 1) 16.  Everything else as
 * emagls_field_stream_create, which is the bank of one set.  With n_sets > 1, state_bytes counts the ring as it is (three entries
 * per slot), the entries' tags (nsrc P 3 int32) and the two previous indices per source; reset also forgets the selection. */
int emagls_field_stream_create_bank(int64_t nsrc, int64_t nch, int64_t n_sets, const void* rir, int rir_is_complex, int64_t nr,
                                    int64_t block, emagls_field_stream** f);

/* emagls_field_stream_push with set indices: set [n_set], n_set = 0 (every source keeps its set; set 0 on a fresh object), nsrc
 * (one index per source for every block of this push) or nsrc * nsamp / block ([nsrc][nsamp / block], source-major).  Any other
 * count, a null array with a positive count, or an index outside [0, n_sets - 1] is EMAGLS_ERR_ARG, reported before the device is
 * touched.  emagls_field_stream_push is this call with n_set = 0. */
int emagls_field_stream_push_sets(emagls_field_stream* f, const double* src, int64_t nsamp, const int32_t* set, int64_t n_set, void* out);

/* emagls_field_stream_push_device with set indices in device memory: d_set is not read by the host (the call still only
 * enqueues), so the kernels clamp every index into [0, n_sets - 1] before they form an address from it.
 * emagls_field_stream_push_device is this call with n_set = 0. */
int emagls_field_stream_push_sets_device(emagls_field_stream* f, const double* d_src, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                         void* d_out, void* stream);

/* The number of response sets of the object's bank. */
int emagls_field_stream_sets(const emagls_field_stream* f, int64_t* n_sets);

/* The three designs with a covariance constraint in the place of the `applyDiffusenessConst` argument the reference's
 * functions used to take after `len` (verifyEMagLs.m:106-114 still shows the call form).  OWN SPECIFICATION, not the reference's
 * implementation: that code is not in the snapshot (CHANGELOG.md:10-12).  Per solved bin the two ears' filters are mixed by the
 * Hermitian positive definite 2x2 matrix M with M Rhat M = R (Rhat: ear covariance of the rendered HRTFs over the HRIR grid,
 * R: that of the time-aligned HRTFs) -- the closed form of Zaunschirm/Schoerkhuber/Hoeldrich 2018's covariance constraint.
 * The reference's surviving *_wDC fixtures agree with it for eMagLS / eMagLS2 (their mixing is predicted to 4e-3) and do NOT
 * for MagLS (interaural cross term off by 6e-2; candidates tried and rejected: DESIGN.md section 7).  Same arguments as the
 * functions without the suffix plus the flag. */
int emagls_get_magls_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                int order, double fs, int64_t len, int apply_diffuseness_const, int basis, void* wL, void* wR);
int emagls_get_emagls_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                 double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                                 int64_t len, int apply_diffuseness_const, int basis, void* wL, void* wR);
int emagls_get_emagls2_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                  double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                                  int64_t len, int apply_diffuseness_const, int basis, void* wL, void* wR);

/* ---- render side: what the reference's harness runs between the recording and the decoder ---- */

/* lib/getMagLsFilters2D.m:1 -- [wMlsL, wMlsR] = getMagLsFilters2D(hLHor, hRHor, horHrirGridAziRad, order, fs, len, chDefinition)
 * hL/hR [nsamp x ndirs]; wL/wR [len x 2*order+1], channels [C_0, C_-1, C_1, ..., C_-N, C_N] (dependencies/getCH.m:17-28),
 * real, or interleaved complex for basis == EMAGLS_BASIS_COMPLEX. */
int emagls_get_magls_filters_2d(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* hrir_azi,
                                int order, double fs, int64_t len, int basis, void* wL, void* wR);

#define EMAGLS_RADIAL_TIKHONOV 0
#define EMAGLS_RADIAL_SOFTLIMIT 1
#define EMAGLS_RADIAL_FULL 2
#define EMAGLS_RADIAL_NONE 3
/* dependencies/getRadialFilter.m:1 -- radFilts = getRadialFilter(params), plane-wave model, rigid sphere.
 * nfft = oversampling * ir_len; rad: interleaved complex [nfft/2+1 x order+1] column-major.  regul_const is read by
 * tikhonov, noise_gain_db by softlimit.  Entries the reference computes as 0/0 or 1/0 (orders > 0 at DC, softlimit / full)
 * come back as NaN / Inf+NaN i like there. */
int emagls_get_radial_filter(int order, double fs, double sma_radius, int64_t ir_len, int oversampling, int filter_type,
                             double regul_const, double noise_gain_db, void* rad);
/* dependencies/applyRadialFilter.m:1 -- outSig = applyRadialFilter(inSig, params) with params.nfft = oversampling * ir_len
 * (verifyEMagLs.m:250).  sig [nsamp x (order+1)^2] real; out [emagls_apply_radial_filter_rows(...) x (order+1)^2]:
 * the signal (zero-padded to nfft if shorter) filtered per SH order, the filter delay nfft/2 removed. */
int64_t emagls_apply_radial_filter_rows(int64_t nsamp, int64_t ir_len, int oversampling);
int emagls_apply_radial_filter(const double* sig, int64_t nsamp, int order, double fs, double sma_radius, int64_t ir_len,
                               int oversampling, int filter_type, double regul_const, double noise_gain_db, double* out);
/* verifyEMagLs.m:235-236 -- E = getSH(order, micGrid, shDefinition).'; shRecording = smaRecording * pinv(E)
 * sig [nsamp x nmics] real; out [nsamp x (order+1)^2], real or interleaved complex like the basis. */
int emagls_sh_encode(const double* sig, int64_t nsamp, int64_t nmics, const double* mic_azi, const double* mic_zen, int order,
                     int basis, void* out);
/* dependencies/getCH.m:1 -- Y = getCH(N, aziRad, basisType): [ndirs x 2N+1] column-major, channels [C_0, C_-1, C_1, ..., C_-N, C_N],
 * real or interleaved complex like the basis */
int emagls_ch_basis(int order, int64_t ndirs, const double* azi, int basis, void* Y);
/* dependencies/getSMAIRMatrix.m:1 -- smairMat = getSMAIRMatrix(params), plane-wave model of a rigid sphere, built-in getSH.
 * The filter designs never form this array (they work on its factors); this entry materialises it for callers that use the
 * array model itself.  nfft = oversampling * ir_len (even); smair: interleaved complex [rows x S x nfft/2+1] column-major,
 * rows = (order+1)^2, or nmics with return_raw_mic_sigs; S = (sim_order+1)^2 with sim_order = max(order, ceil(fs*pi*r/343))
 * returned through sim_order (optional).  radial_filter_type other than EMAGLS_RADIAL_NONE applies getRadialFilter to the
 * SH-domain model (:129-138). */
int emagls_get_smair_matrix(int order, double fs, int64_t ir_len, int oversampling, double sma_radius, const double* mic_azi,
                            const double* mic_zen, int64_t nmics, int basis, int return_raw_mic_sigs, int radial_filter_type,
                            double regul_const, double noise_gain_db, void* smair, int* sim_order);
/* lib/getMagLsSphericalHeadFilter.m:1 -- [wShf, W_Shf] = getMagLsSphericalHeadFilter(micRadius, order, fs, len)
 * w_shf [len]; W_shf (optional) [emagls_eq_filter_nfft(len)] real, the mirrored zero-phase spectrum. */
int64_t emagls_eq_filter_nfft(int64_t len);
int emagls_get_magls_spherical_head_filter(double mic_radius, int order, double fs, int64_t len, double* w_shf, double* W_shf);
/* lib/getMagLsArrayDiffuseFilter.m:1 -- wAdf = getMagLsArrayDiffuseFilter(micRadius, micGridAziRad, micGridZenRad, order, fs,
 * len, shDefinition, shFunction).  Y_hi (optional) replaces the built-in getSH: the caller's shFunction evaluated at the
 * simulation order ceil(fs*pi*micRadius/343), [nmics x (simOrder+1)^2] column-major (the grid may then be NULL).  w_adf [len]. */
int emagls_get_magls_array_diffuse_filter(double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order,
                                          double fs, int64_t len, int basis, const void* Y_hi, double* w_adf);

/* ---- rendered HRTFs of a design (the definition is this project's, the operands are the reference's) ----
 * What a set of decoding filters renders for a plane wave from each of ndirs directions, and how far that is from the HRTFs it
 * was designed against.  With nfft even, len <= nfft (0: min(2048, 2*len)), P = nfft/2+1 and W_e = fft(w_e, nfft) on bins 0..P-1:
 *     Hhat_e(k, d) = sum_c W_e(k, c) pwGrid_k(c, d)
 * -- the product inside the residual the designs minimise (lib/getEMagLsFilters.m:87-103).  `model` fixes pwGrid_k [C x ndirs]:
 *   EMAGLS_MODEL_SH       getSH(order, dirs, shDefinition)' (lib/getMagLsFilters.m), the same for every k; C = (order+1)^2, order <= 15
 *   EMAGLS_MODEL_EMAGLS   smairMat(:,:,k) * getSH(simOrder, dirs, shDefinition)' with getSMAIRMatrix called as
 *                         lib/getEMagLsFilters.m:51-63 calls it (irLen = nfft, oversampling 1, radialFilter 'none', rigid sphere,
 *                         plane wave, real(Bn) in the Nyquist bin, simOrder = max(order, ceil(fs*pi*r/343)) <= 85); C = (order+1)^2,
 *                         order <= 4 (the limit of emagls_get_smair_matrix; above: EMAGLS_ERR_UNSUPPORTED)
 *   EMAGLS_MODEL_EMAGLS2  the same with returnRawMicSigs and params.order left at 4 (lib/getEMagLs2Filters.m:51-63; `order` is not
 *                         looked at); C = nmics <= 64
 *   EMAGLS_MODEL_ATF      pwGrid_k(m, d) = fft(atfIrs, nfft)(k, m, d), atf [atf_taps x nmics x ndirs] column-major GIVEN ON the
 *                         evaluation directions (the caller has matched the grids); C = nmics <= 64, atf_taps <= nfft; dir_azi,
 *                         dir_zen, basis are not looked at
 *   EMAGLS_MODEL_EMA_CH   pinv(getCH(order, micAzi)) * smairMat(:,:,k) * getSH(simOrder, dirs, shDefinition)' with getSMAIRMatrix called
 *                         as lib/getEMagLsFiltersEMAinCH.m:52-65 calls it (raw microphone signals, params.order = order, the microphones at
 *                         zenith pi/2, otherwise as for EMAGLS_MODEL_EMAGLS); C = 2*order+1 in getCH's channel order, order <= 15
 *   EMAGLS_MODEL_EMA_SH   pwGrid_k(:, d) = Rot_d.' * J * pinv(getCH(order, micAzi)) * smairMat(:,:,k) * conj(getSH(simOrder, [azi_d, pi/2])).'
 *                         (lib/getEMagLsFiltersEMAinSH.m:66-100): the same array on the HORIZONTAL projection of the directions, J =
 *                         getChToShExpansionMatrix, Rot_d the SH rotation to the direction's elevation that emagls_get_emagls_filters_ema_in_sh
 *                         uses (the identity where zen_d == pi/2 exactly); C = (order+1)^2, order <= 7, simOrder <= 68 (47 with a complex basis)
 *                         Both EMA models: nmics >= 2*order+1 (fewer: EMAGLS_ERR_UNSUPPORTED); mic_zen is not looked at and may be NULL.
 *                         Value 4 is not assigned.  The scratch of EMAGLS_MODEL_EMA_SH grows with ndirs * C^2 (the rotation fit): the
 *                         24 GiB estimate refuses 65536 directions at order 7 with a complex basis; with a real basis that size
 *                         passes the estimate (about 12 GB) but has NOT been run -- the largest call run is 2702 directions.
 * smairMat is never formed: the call works on its factors.  Arguments a model does not use may be NULL / 0.
 * wL, wR: nsets >= 1 filter sets back to back, each [len x nchan] column-major as the designs return them, real, or interleaved
 * complex with w_is_complex; nchan must equal the model's C.  ndirs <= 65536.
 * Hhat (optional): interleaved complex [nsets][2 ears][P][ndirs], ndirs fastest.  When it is NULL the response never leaves
 * the kernel that computes it.
 * Metrics (each optional) need reference HRIRs hL, hR [nsamp x ndirs] column-major, nsamp <= nfft, on the same directions:
 * nhrir_sets = 1 (one set for all filter sets) or nsets sets back to back.  With H_e = fft(h_e, nfft), w_d = weights / sum(weights)
 * (non-negative; NULL: uniform) and magnitudes clamped below at DBL_MIN before a logarithm, per set and bin k:
 *   mag_err_db [nsets][P][2]   sum_d w_d |20 log10(|Hhat_e| / |H_e|)|
 *   ild_err_db [nsets][P]      sum_d w_d |20 log10(|Hhat_L| / |Hhat_R|) - 20 log10(|H_L| / |H_R|)|
 *   cov_hat, cov_ref [nsets][P][4]   (R_LL, R_RR, Re R_LR, Im R_LR), R_ab = sum_d w_d X_a conj(X_b): the 2 x 2 ear covariances
 *                              of Hhat and of H (interaural coherence = |R_LR| / sqrt(R_LL R_RR))
 * Sums run in a fixed order without atomics: equal calls give equal bits, and set i of a call gives the bits of the call with
 * that set alone.  Every argument is checked before the device is touched. */
#define EMAGLS_MODEL_SH 0
#define EMAGLS_MODEL_EMAGLS 1
#define EMAGLS_MODEL_EMAGLS2 2
#define EMAGLS_MODEL_ATF 3
#define EMAGLS_MODEL_EMA_CH 5
#define EMAGLS_MODEL_EMA_SH 6
int emagls_rendered_hrtfs(int model, const void* wL, const void* wR, int w_is_complex, int64_t len, int64_t nchan, int64_t nsets,
                          const double* dir_azi, const double* dir_zen, int64_t ndirs, double fs, int order, int basis,
                          double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, const double* atf,
                          int64_t atf_taps, int64_t nfft, const double* hL, const double* hR, int64_t nsamp, int64_t nhrir_sets,
                          const double* weights, void* Hhat, double* mag_err_db, double* ild_err_db, double* cov_hat, double* cov_ref);

/* ---- array impulse responses: plane-wave components through the simulated array (this project's) ----
 * The content that goes INTO the field stream: time-domain responses of the rigid-sphere array of getSMAIRMatrix to nsrc sources,
 * each a sum of plane-wave components with a direction, a delay in samples and a real gain.  One component per source: a
 * direction bank for a moving virtual source; many: an array room response from image sources the caller lists.
 * With N = max(order, ceil(fs pi r / 343)) (getSMAIRMatrix.m:95; N <= 85), f_k = k fs / nfft, k = 0 .. nfft/2,
 * beta_n(k) = -b_n(2 pi f_k r / 343) (the rigid sphere, the sign of :107), u_j and v_m the unit vectors of component j and microphone m:
 *   H_q(k, m) = sum_j g_j exp(-2 pi i k (tau_j + pre_delay) / nfft) sum_{n <= N} beta_n(k) (2n+1)/(4 pi) P_n(u_j . v_m)
 * -- by the addition theorem Y_mic(m, :) diag(sh_repToOrder(beta(k))) conj(getSH(N, dir_j)).', the column pwGrid_k(:, dir_j) of the
 * emagls2 operand, in either basis.  In the last bin real(beta_n) is used (:115-117) and the bin's value is the real part of the sum.
 * With an encoder, X_q(k, c) = sum_m enc(c, m) H_q(k, m).  out = irfft over k at length nfft, first nr samples, no window; a complex
 * encoder gives complex taps (the real and the imaginary part of enc transformed separately and joined).
 * mic_azi, mic_zen [nmics], 1 <= nmics <= 64.  enc [nch x nmics] as emagls_decode_stream_create_encoded takes it (column-major,
 * interleaved complex with enc_is_complex), 1 <= nch <= 64; NULL: raw microphones, nch must equal nmics.
 * Sources in CSR form: comp_ptr [nsrc + 1], comp_ptr[0] = 0, non-decreasing; source q owns the components comp_ptr[q] ..
 * comp_ptr[q+1] - 1 of comp_azi, comp_zen, comp_delay (>= 0, fractional allowed; NULL: zeros) and comp_gain (NULL: ones).  A source
 * without components gives zeros.  pre_delay >= 0 samples (fractional allowed) makes the acausal part of the sphere's response
 * causal; a component with tau_j + pre_delay > nfft - 1 would wrap: EMAGLS_ERR_ARG.
 * nfft: a power of two from 8 to 65536; 0: the smallest one >= 2 nr.  nr <= nfft taps are returned.
 * out: nsrc arrays [nr x nch] one after the other, column-major -- the rir of emagls_field_stream_create, or of
 * emagls_field_stream_create_bank for nsrc sets of one source; interleaved complex when enc_is_complex.
 * Sums run in a fixed order without atomics: equal calls give equal bits, and source q of a call gives the bits of the call with
 * that source alone.  Every argument is checked before the device is touched; a call whose device memory estimate passes 24 GiB is
 * EMAGLS_ERR_UNSUPPORTED (split the sources over several calls).  Transforms up to 4096 points run in LDS, longer ones in hipFFT. */
int emagls_array_irs(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                     const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr, const double* comp_azi,
                     const double* comp_zen, const double* comp_delay, const double* comp_gain, double pre_delay, int64_t nfft, int64_t nr,
                     void* out);
/* Device-event time in ms of the main kernel (both forms' launches) of the calling thread's last completed emagls_array_irs call
 * (tools/array_irs_timing.py); EMAGLS_ERR_ARG before the first one. */
int emagls_array_irs_kernel_time(double* ms);

/* ---- array impulse responses with a spectral gain: surfaces and air (this project's) ----
 * emagls_array_irs with a gain that depends on the bin.  With P = nfft / 2 + 1 and k = 0 .. P - 1 a call carries, next to the
 * component lists, nsurf surfaces (0 <= nsurf <= 8) with real reflection spectra surf_refl [nsurf x P] (surface w at surf_refl + w P;
 * every value finite, |R_w(k)| <= 1), per component nsurf integer exponents comp_exp [ncomp x nsurf] (those of component j contiguous
 * at comp_exp + j nsurf; e_jw >= 0), and optionally an attenuation spectrum air_atten [P] (alpha(k) >= 0 in nepers per metre) with a
 * path length per component comp_path [ncomp] (l_j >= 0 in metres): both given or both NULL.  The g_j of emagls_array_irs becomes
 *   G_j(k) = g_j prod_{w < nsurf} R_w(k)^e_jw exp(-alpha(k) l_j).
 * R^0 = 1, also for R = 0; G_j(k) is exactly 0 where some R_w(k) = 0 meets e_jw > 0, and exactly g_j where every e_jw = 0 and there is
 * no air term.  G is real, so the rules for bin 0 and the last bin stand; R_w(0) and alpha(0) are used as given.  Everything else is
 * emagls_array_irs: delays, pre_delay, encoder, transform, the fixed summation order, the per-source choice of the kernel's form, equal
 * bits for equal calls and for source q alone.  nfft must be given (the length of the spectra depends on it): 0 is EMAGLS_ERR_ARG.
 * With nsurf = 0 and no air term the call runs the kernels of emagls_array_irs and returns its bits.  The gain is formed inside the
 * main kernel as one exponential of sum_w e_jw ln|R_w(k)| - alpha(k) l_j with the sign from the parities: it agrees with the direct
 * powers to a few 1e-15 relative.  Every argument is checked before the device is touched; the 24 GiB estimate counts the tables and
 * the per-component arrays.  emagls_array_irs_kernel_time covers the spectral launches. */
int emagls_array_irs_spectral(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                              const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr, const double* comp_azi,
                              const double* comp_zen, const double* comp_delay, const double* comp_gain, int64_t nsurf,
                              const double* surf_refl, const int32_t* comp_exp, const double* air_atten, const double* comp_path,
                              double pre_delay, int64_t nfft, int64_t nr, void* out);

/* ---- array room responses: shoebox image sources (this project's) ----
 * The components of emagls_array_irs, enumerated on the device from a shoebox room: Allen & Berkley's image model with
 * frequency-independent walls.  room_dim [3] = (Lx, Ly, Lz) in metres, all > 0; one corner at the origin, the axes those of getSH
 * (x front, y left, z up) and parallel to the array's.  wall_refl [6]: real amplitude reflection coefficients in [-1, 1] of the walls
 * x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz.  array_pos [3]: the array's centre, the whole sphere inside the room
 * (mic_radius <= array_pos[i] <= room_dim[i] - mic_radius; emagls_shoebox_components has no sphere: radius 0).  src_pos [3 x nsrc], xyz
 * contiguous per source, nsrc >= 1, each strictly inside the room and farther than mic_radius from array_pos.  max_delay: samples,
 * > 0 and finite.  max_order: >= 0, or -1 for no limit on the reflection order.  The speed of sound is 343 m/s.
 * A candidate of a source s is n = (nx, ny, nz), integers, and p = (px, py, pz) in {0, 1}^3.  Per axis i: image_i = (1 - 2 p_i) s_i +
 * 2 n_i L_i; exponents e0_i = |n_i - p_i| (the wall at 0), e1_i = |n_i| (the wall at L_i); reflection order = sum_i (e0_i + e1_i).
 * With v = image - array_pos: d = sqrt((vx vx + vy vy) + vz vz), delay tau = d / 343 fs samples, gain g = prod_i b0_i^e0_i b1_i^e1_i / d
 * (b^0 = 1 also for b = 0; the factors taken in the order x0, x1, y0, y1, z0, z1, then the division: a unit source at 1 m in the
 * free field has gain 1), azi = atan2(vy, vx), zen = acos(vz / d).
 * A candidate is a component iff (max_order < 0 or its reflection order <= max_order) and g != 0 and tau <= max_delay.  The
 * components of a source lie in ascending lexicographic order of (nz, ny, nx, pz, py, px); this fixes the summation order of
 * emagls_array_irs' main kernel, and so the bits of the responses.  No atomics: equal calls give equal lists, and the list of source
 * q is the list of the call with that source alone.
 * The search box is |n_i| <= floor(max_delay 343 / fs / (2 L_i)) + 1, and <= floor((max_order + 1) / 2) with an order limit; a call
 * with more than 2^28 candidates (8 prod_i (2 B_i + 1) per source, times nsrc) is EMAGLS_ERR_UNSUPPORTED.
 * Every argument is checked before the device is touched.  Plane-wave components are a far-field model: the images as point sources at
 * their distances are emagls_array_room_irs_point below; directive sources: emagls_array_room_irs_directive.  Frequency-dependent walls and air
 * absorption: the spectral entries below.
 *
 * emagls_shoebox_components: comp_ptr [nsrc + 1] (host) is always written; comp_azi, comp_zen, comp_delay, comp_gain [capacity] are
 * written only when comp_ptr[nsrc] <= capacity.  NULL arrays with capacity = 0: a count-only call. */
int emagls_shoebox_components(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc, const double* src_pos,
                              double fs, double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_azi,
                              double* comp_zen, double* comp_delay, double* comp_gain);
/* emagls_array_irs of those components without their crossing the bus: the enumeration feeds the main kernel on the device, and only
 * the nsrc + 1 offsets come back to the host (for the main kernel's two source lists).  out and every argument shared with
 * emagls_array_irs as there.  max_delay + pre_delay > nfft - 1 would wrap: EMAGLS_ERR_ARG.  comp_count [nsrc] (optional, NULL for
 * none): the number of components of each source.  The 24 GiB estimate of emagls_array_irs needs the component count: it is applied
 * after the count pass (its part that does not depend on the count before the device is touched).  Source q of a call gives the bits
 * of emagls_array_irs on the list emagls_shoebox_components returns for it. */
int emagls_array_room_irs(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                          const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                          const double* array_pos, int64_t nsrc, const double* src_pos, double max_delay, int max_order, double pre_delay,
                          int64_t nfft, int64_t nr, int64_t* comp_count, void* out);
/* The spectral room: walls with reflection spectra, and air absorption.  The enumeration does not see the walls:
 * a candidate is a component iff (max_order < 0 or its reflection order <= max_order) and tau <= max_delay -- there is no "gain != 0"
 * rule.  emagls_shoebox_images returns per component azi, zen, delay as above, gain = 1 / d, the six exponents comp_exp [capacity x 6]
 * (e0_x, e1_x, e0_y, e1_y, e0_z, e1_z contiguous per component: the walls x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz) and comp_path = d
 * in metres: the lists of emagls_array_irs_spectral with nsurf = 6.  Candidates, search box, cap, order of the list, the absence of
 * atomics and the count-only convention are those of emagls_shoebox_components, and the first four columns are its bits with all six
 * coefficients equal to 1. */
int emagls_shoebox_images(const double* room_dim, const double* array_pos, int64_t nsrc, const double* src_pos, double fs, double max_delay,
                          int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_azi, double* comp_zen, double* comp_delay,
                          double* comp_gain, int32_t* comp_exp, double* comp_path);
/* emagls_array_irs_spectral of those images without their crossing the bus.  wall_refl_spec [6 x P]: the reflection spectra of the six
 * walls in the order above (finite, in [-1, 1]), P = nfft / 2 + 1 with nfft given (0: EMAGLS_ERR_ARG).  air_atten [P] in Np/m, >= 0, or
 * NULL for no air term; with it every component's path length is its d.  Everything else as emagls_array_room_irs.  Source q of a call
 * gives the bits of emagls_array_irs_spectral on the lists emagls_shoebox_images returns for it. */
int emagls_array_room_irs_spectral(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                   const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl_spec,
                                   const double* air_atten, const double* array_pos, int64_t nsrc, const double* src_pos, double max_delay,
                                   int max_order, double pre_delay, int64_t nfft, int64_t nr, int64_t* comp_count, void* out);
/* Device-event time in ms of the enumeration passes (count, scan, write) of the calling thread's last completed
 * emagls_shoebox_components, emagls_shoebox_images or emagls_array_room_irs(_spectral) call; EMAGLS_ERR_ARG before the first one.  A
 * room call also sets the time of emagls_array_irs_kernel_time. */
int emagls_shoebox_kernel_time(double* ms);

/* ---- array impulse responses to point sources at a finite distance (this project's) ----
 * emagls_array_irs_spectral with a distance rho_j in metres per component, comp_dist [ncomp]: every rho_j finite and > mic_radius
 * (EMAGLS_ERR_ARG otherwise; distances are given for all components -- NULL with ncomp > 0 is EMAGLS_ERR_ARG -- and the entries
 * without comp_dist are the calls with none).  With kappa_k = 2 pi f_k / 343 the order-n term of component j gains the factor
 *   F_n(kappa_k rho_j),  F_n(x) = (-i)^(n+1) x e^(ix) h_n^(2)(x) = sum_{m <= n} (n+m)! / (m! (n-m)!) (1 / (2ix))^m,  F_0 = 1, F_n -> 1 as x -> inf:
 *   H_q(k, m) = sum_j G_j(k) exp(-2 pi i k (tau_j + pre_delay) / nfft) sum_{n <= N} beta_n(k) (2n+1)/(4 pi) F_n(kappa_k rho_j) P_n(u_j . v_m).
 * tau_j and g_j stay the caller's: with tau_j = rho_j / 343 fs and g_j = 1 / rho_j the component is the spherical wave
 * e^(-i kappa R) / R of a point source, expanded about the array's centre (the e^(+i omega t), h^(2) convention of b_n).  Bin 0 is the
 * limit kappa -> 0, beta_n (2n+1)/(4 pi) F_n -> -(2n+1)/(n+1) (r/rho_j)^n; in the last bin real(beta_n) is used and the real part of
 * the sum is taken.  N is the plane-wave rule max(order, ceil(fs pi r / 343)): a source close to the sphere needs more orders, which
 * `order` raises (N <= 85).  nsurf = 0 without an air term is allowed (then nfft = 0 also is).  The factors are formed inside the main
 * kernel in a scaled form that stays inside FP64 at every order and bin; a call whose largest x = (pi fs / 343) max_j rho_j has
 * N log10(x) - log10((2N-1)!!) >= 300 is EMAGLS_ERR_UNSUPPORTED (beyond a kilometre at N = 85, no room at N <= 60).  Encoder, transform,
 * layout, the fixed summation order, the per-source form, equal bits for equal calls and for source q alone: emagls_array_irs.  Every
 * argument is checked before the device is touched; the 24 GiB estimate counts the table and the distances;
 * emagls_array_irs_kernel_time covers these launches.  Not built: +inf distances mixed into a call, open or directional spheres,
 * device-pointer outputs.  (Source directivity: emagls_array_irs_directive below.) */
int emagls_array_irs_point(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                           const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr, const double* comp_azi,
                           const double* comp_zen, const double* comp_delay, const double* comp_gain, int64_t nsurf,
                           const double* surf_refl, const int32_t* comp_exp, const double* air_atten, const double* comp_path,
                           const double* comp_dist, double pre_delay, int64_t nfft, int64_t nr, void* out);
/* emagls_shoebox_components with the distance d of every component beside its columns, comp_dist [capacity] in metres: the comp_dist
 * of emagls_array_irs_point, and the bits of emagls_shoebox_images' comp_path on walls of 1.  The four columns keep their bits. */
int emagls_shoebox_components_dist(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc,
                                   const double* src_pos, double fs, double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr,
                                   double* comp_azi, double* comp_zen, double* comp_delay, double* comp_gain, double* comp_dist);
/* The room with its image sources as point sources: every component's rho is its d, handed to the main kernel on the device.
 * wall_is_spectral = 0: wall_refl [6] coefficients (without air_atten the enumeration and the lists of emagls_array_room_irs, with it
 * the coefficients are repeated over the bins); otherwise wall_refl [6 x P] spectra as in emagls_array_room_irs_spectral.  air_atten
 * [P] or NULL.  The overflow rule above is applied to the reach of max_delay, before the device is touched.  Source q of a call gives
 * the bits of emagls_array_irs_point on the lists emagls_shoebox_components_dist (emagls_shoebox_images, path = distance) returns. */
int emagls_array_room_irs_point(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                                int wall_is_spectral, const double* air_atten, const double* array_pos, int64_t nsrc, const double* src_pos,
                                double max_delay, int max_order, double pre_delay, int64_t nfft, int64_t nr, int64_t* comp_count, void* out);

/* ---- array impulse responses of directive, oriented sources (this project's) ----
 * Next to the arguments of emagls_array_irs_point (comp_dist may be NULL: plane waves) a call may carry
 *   dir_order = Nd, 0 <= Nd <= 8 (above: EMAGLS_ERR_UNSUPPORTED), Kd = (Nd + 1)^2, one order for all sources (pad with zeros);
 *   dir_coef [nsrc][Kd][P], interleaved complex doubles, P = nfft / 2 + 1 with nfft given (0: EMAGLS_ERR_ARG): the coefficients
 *     c_{q,i}(k) of source q's directivity in the REAL basis of emagls_get_sh (index n^2 + n + m, orthonormal, Y_0 = 1 / sqrt(4 pi),
 *     m > 0 cosine, m < 0 sine); finite;
 *   src_rot [nsrc][9], row-major R_q whose columns are the source's front (x), left (y) and up (z) axes in room axes; NULL: identity;
 *     max|R^T R - I| > 1e-12 or det < 0 is EMAGLS_ERR_ARG;
 *   comp_emit [ncomp][3], the unit vector e_j in room axes along which the ray of component j left the real source;
 *     | |e|^2 - 1 | > 1e-12 is EMAGLS_ERR_ARG.
 * With w_j = R_q^T e_j, azi = atan2(w_y, w_x), zen = acos(min(1, max(-1, w_z))):  D_j(k) = sum_{i < Kd} c_{q,i}(k) Y_i(azi_j, zen_j),
 * and the gain G_j(k) of emagls_array_irs_spectral (g_j without surfaces and air) becomes G_j(k) D_j(k), inside the main kernel, for
 * plane-wave components and point sources alike.  Delays, pre_delay, encoder, transform, layout, the last bin (Re beta_n and the real
 * part of the sum), the fixed summation order without atomics, the per-source form, equal bits for equal calls and for source q alone:
 * emagls_array_irs.  dir_coef = NULL requires comp_emit = NULL, src_rot = NULL and dir_order = 0 and is the call of
 * emagls_array_irs_point (comp_dist given), emagls_array_irs_spectral (any of its five arguments given) or emagls_array_irs, with
 * its bits.  Every argument is checked before the device is touched; the 24 GiB estimate counts the basis values, the angles and
 * the padded coefficient table; emagls_array_irs_kernel_time covers the basis pass and the main kernel.  Not built: microphone
 * directivity, open or directional spheres, an orientation per component or over time, Nd > 8, coefficients in the complex basis,
 * device-pointer inputs or outputs. */
int emagls_array_irs_directive(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                               const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr, const double* comp_azi,
                               const double* comp_zen, const double* comp_delay, const double* comp_gain, int64_t nsurf,
                               const double* surf_refl, const int32_t* comp_exp, const double* air_atten, const double* comp_path,
                               const double* comp_dist, const double* comp_emit, const double* src_rot, int dir_order, const double* dir_coef,
                               double pre_delay, int64_t nfft, int64_t nr, void* out);
/* The emission vectors of a shoebox room's components, comp_emit [capacity x 3]: for candidate (n, p) with v and d as above, the
 * image's ray to the array, -v / d, mirrored back through the walls it crossed: e_i = -(1 - 2 p_i) v_i / d (the direct sound: from the
 * source to the array).  They do not depend on the source's orientation.  wall_refl NULL: the keep rule and rows of
 * emagls_shoebox_images; otherwise those of emagls_shoebox_components.  comp_ptr and the count-only convention as there. */
int emagls_shoebox_emission(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc, const double* src_pos,
                            double fs, double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_emit);
/* The room with directive sources, no component crossing the bus: the arguments of emagls_array_room_irs_point, point_source (0: plane
 * waves, the lists of emagls_array_room_irs or, with spectra or air, emagls_array_room_irs_spectral; 1: point sources), and src_rot,
 * dir_order, dir_coef as above.  Source q of a call gives the bits of emagls_array_irs_directive on the lists of the matching list
 * entries and emagls_shoebox_emission.  dir_coef = NULL (src_rot NULL, dir_order 0): the matching entry without directivity. */
int emagls_array_room_irs_directive(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                    const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                                    int wall_is_spectral, const double* air_atten, const double* array_pos, int64_t nsrc, const double* src_pos,
                                    double max_delay, int max_order, int point_source, const double* src_rot, int dir_order,
                                    const double* dir_coef, double pre_delay, int64_t nfft, int64_t nr, int64_t* comp_count, void* out);

/* ---- plan API: inputs resident in HBM, repeated execution (benchmarks, batches) ------------- */

typedef struct emagls_plan emagls_plan;

typedef struct emagls_design_desc {
    int kind;            /* EMAGLS_KIND_* */
    int basis;           /* EMAGLS_BASIS_* */
    int order;           /* SH output order N */
    double fs;           /* Hz */
    int64_t len;         /* filter length (ignored for LS) */
    int64_t nsamp;       /* HRIR taps */
    int64_t ndirs;       /* HRIR directions */
    double mic_radius;   /* EMAGLS / EMAGLS2 */
    int64_t nmics;       /* EMAGLS / EMAGLS2 / FROM_ATF */
    double f_trans;      /* FROM_ATF: transition frequency in Hz */
    int64_t atf_taps;    /* FROM_ATF */
    int64_t natf;        /* FROM_ATF: ATF directions */
    int custom_basis;    /* != 0: the SH matrices are supplied by emagls_plan_set_basis (a custom shFunction, lib/getEMagLsFilters.m:32,68) */
    int diffuseness;     /* != 0: apply the covariance constraint (own specification, see emagls_get_magls_filters_dc) in the
                          * place of the applyDiffusenessConst option the reference removed (CHANGELOG.md:10-12,
                          * verifyEMagLs.m:137-145); MAGLS, MAGLS_2D, EMAGLS, EMAGLS2, EMA_CH */
    int sim_order_pad;   /* EMAGLS / EMAGLS2 / EMA_CH, 0 = off: lay the design out for max(its own simulation order, this) SH orders
                          * with b_n = 0 above its own order (dependencies/getSMAIRMatrix.m:95,107: the same sum, the same filters).
                          * Array radii of neighbouring simulation-order classes then have ONE shape and share a lane batch
                          * (emagls_batch_create; BASELINE config 4: 256 radii = 32 batches of 8) */
} emagls_design_desc;

typedef struct emagls_plan_info {
    int nfft, num_pos_freqs, k_cut /* 1-based like the reference */, sim_order, num_sh_sim, num_channels;
    int out_is_complex;
    int64_t out_rows, out_cols;
    double grp_delay_l, grp_delay_r; /* valid after an execute + synchronize */
    double mean_grid_dev_deg;        /* FROM_ATF */
    int num_sweep_launches;
    int64_t device_bytes;
    /* routes of the per-bin factorisation of the array designs (0 elsewhere), 0-based bins: [1, hh_end) orthonormal route
     * (Householder QR + Jacobi SVD) on the lowest hh_orders orders, [gram_from, P) Gram route (gram_from == 0: none);
     * g_first: first bin whose direction-space operand G_k is formed */
    int gram_from, hh_end, hh_orders, g_first;
    int sim_order_own;               /* the design's own simulation order (sim_order is the padded one with sim_order_pad) */
    /* form of the phase sweep the next execute takes: 0 one launch per bin, 1 one resident launch on operands G_k materialised
     * in HBM, 2 one resident launch that evaluates its operands itself from the angles between HRIR directions and microphones
     * (array designs on the built-in SH basis; EMAGLS_SWEEP_SYNTH=0 selects form 1), 3 the same with the operand of a bin held
     * in registers by the waves that run the recurrence (up to 18 units; EMAGLS_SWEEP_REG=0 selects form 2; several such sweeps
     * share the device).  sweep_units: forms 2 and 3, the polynomial evaluations per direction and bin -- antipodal microphone
     * pairs count once (15 pairs + 2 single capsules on the em32). */
    int sweep_form, sweep_units;
} emagls_plan_info;

int emagls_plan_create(const emagls_design_desc* desc, emagls_plan** plan);
int emagls_plan_destroy(emagls_plan* plan);
int emagls_plan_set_hrir_grid(emagls_plan* plan, const double* azi, const double* zen);
/* zen is ignored (may be NULL) for EMAGLS_KIND_EMA_CH: an equatorial array, every microphone at pi/2 */
int emagls_plan_set_mic_grid(emagls_plan* plan, const double* azi, const double* zen);
int emagls_plan_set_hrirs(emagls_plan* plan, const double* hL, const double* hR);
/* custom_basis plans: Y_hrir [ndirs x S] and (array designs) Y_mic [nmics x S], column-major, real or interleaved complex like
 * the plan's basis, S = (emagls_simulation_order(...) + 1)^2; replaces the two grid setters */
int emagls_plan_set_basis(emagls_plan* plan, const void* Y_hrir, const void* Y_mic);
int emagls_plan_set_atfs(emagls_plan* plan, const double* atf_irs, const double* atf_azi, const double* atf_zen);
/* enqueue the whole design (SH basis ... windowed filters) on the plan's stream; returns immediately */
int emagls_plan_execute(emagls_plan* plan);
int emagls_plan_synchronize(emagls_plan* plan);
/* synchronise, check device-side status flags, copy the filters out */
int emagls_plan_get_filters(emagls_plan* plan, void* wL, void* wR);
int emagls_plan_get_info(emagls_plan* plan, emagls_plan_info* info);
/* the sweep form (emagls_plan_info.sweep_form) a batch of `designs` plans shaped like `plan` takes: what bench.py names its
 * dominant kernel by (the form is decided per launch, by the number of designs in it) */
int emagls_plan_sweep_form_in_batch(emagls_plan* plan, int designs, int* form);
/* 1..4: number of HIP streams one design may use (independent branches fork onto side streams; default 3,
 * best for the latency of ONE design; use 1 when several plans are in flight). Drops the captured graph; with more than one
 * stream the plan runs eagerly (a graph is only captured from one stream). */
int emagls_plan_set_streams(emagls_plan* plan, int nstreams);
/* profiling: level 0 none, 1 = HIP events between stages, 2 = additionally around every sweep launch */
int emagls_plan_set_profiling(emagls_plan* plan, int level);
int emagls_plan_num_stages(emagls_plan* plan);
const char* emagls_plan_stage_name(emagls_plan* plan, int stage);
/* after execute + synchronize with profiling >= 1: per-stage milliseconds of the last execute */
int emagls_plan_stage_times(emagls_plan* plan, double* ms, int n);
/* profiling level 2: sum and count of per-launch sweep kernel durations (ms) of the last execute */
int emagls_plan_sweep_kernel_time(emagls_plan* plan, double* total_ms, int* launches);
/* copy an internal device buffer to the host (tests): returns its size in *nbytes when dst == NULL.  "Yls": the kept operand of the
   least-squares rows of the geometry-sharing batch the plan belongs to ([bin 1 .. k_cut-2][channel][padded directions], complex);
   an error when the batch keeps none */
int emagls_plan_debug_buffer(emagls_plan* plan, const char* name, void* dst, size_t* nbytes);
/* the plan's hipStream_t, for callers that interleave their own work */
void* emagls_plan_stream(emagls_plan* plan);

/* ---- batches: several eMagLS / eMagLS2 designs of identical shape (different arrays / HRIR sets) ---------
 * Plans of identical shape (same simulation order: same array radius class) are executed in lane mode: their buffers
 * are moved into one arena at a constant stride and every launch of the pipeline covers all designs (grid.z = design);
 * the sequential sweep is one resident launch in which each design's workgroups occupy one XCD.  Other batches run the
 * per-design stages on the plans' own streams and share only the sweep.  At most 8 plans (one XCD per design in the sweep);
 * with EMAGLS_BATCH_MAX=16 in the environment up to 16 (two designs per XCD, two sweep workgroups per CU: for an otherwise
 * idle device only, see emagls_batch_create in capi.hip); the plans stay owned by the
 * caller and must outlive the batch.  Results: emagls_batch_get_filters, or emagls_plan_get_filters on each plan.
 * LS / MagLS / MagLS-2D plans of one kind, order and basis (up to 32 channels) form batches as well (lib/getLsFilters.m:30,
 * lib/getMagLsFilters.m:30 in a loop over HRIR sets): their stages run on the batch's stream and ONE resident sweep launch serves all designs; with
 * emagls_batch_set_geometry_sharing, sets on one grid compute the SH side once. */
typedef struct emagls_batch emagls_batch;
int emagls_batch_create(emagls_plan** plans, int nplans, emagls_batch** batch);
/* Largest batch emagls_batch_create accepts from now on: 8 by default (EMAGLS_BATCH_MAX in the environment sets the initial
 * value), up to 16 -- two designs per XCD in the resident sweep, two sweep workgroups per CU (154 of 160 KB of LDS): fastest per
 * design when the batch has the device to itself, but kernels of other batches then only find room on the CUs the sweep does not
 * use, so keep 8 when several batches are in flight.  *previous (optional) receives the old value. */
int emagls_set_batch_max(int max_designs, int* previous);
/* Batches of HRIR sets on ONE geometry (the loop over subjects around lib/getEMagLsFilters.m:32 / getEMagLs2Filters.m:32 /
 * getEMagLsFiltersEMAinCH.m:32 with the same grids and array): with sharing enabled, a batch whose plans agree in every
 * geometry input (compared on the device whenever a grid is replaced) runs the SH matrices, the array model, pwGrid_k and its
 * regularised inverses ONCE (plan 0) and per plan only what its HRIRs enter: spectra, least-squares rows, the sweep (on plan
 * 0's operands) and the epilogue.  Off by default: a batch then treats its designs as independent.  Plans that do not agree
 * (or kinds without the option: FromAtf / EMAinSH / more than 32 channels / designs with the covariance constraint) run
 * as before;
 * emagls_batch_shares_geometry reports what the last execute did. */
int emagls_batch_set_geometry_sharing(emagls_batch* batch, int enable);
int emagls_batch_shares_geometry(emagls_batch* batch, int* shared);
/* A sharing batch keeps its geometry stages between executes: the first sharing execute (and the first after a grid was replaced, a
 * recovery, emagls_batch_set_geometry_sharing or an execute of one of its plans on its own) is "cold", the others "warm" -- only what
 * the HRIRs enter, for every plan.  A run becomes the kept one when emagls_batch_get_filters has read its status flags clean.
 * Executes of each form so far (EMAGLS_GEO_KEEP=0 in the environment: every sharing execute is cold). */
int emagls_batch_geometry_runs(emagls_batch* batch, long long* cold, long long* warm);
/* ---- job lists ---------------------------------------------------------------------------------------------------
 * Independent designs are the unit of parallelism of the reference's users: the loop over array radii, HRIR sets or subjects
 * around one of its functions (testEMagLs.m:75-95, testEMagLsFromAtfs.m:72-73).  One job = one design: its descriptor, its inputs
 * and room for its filters.  hL / hR / atf and wL / wR may be host or device buffers of the current device (device buffers are
 * read and written stream-ordered: nothing crosses PCIe); the grids are host arrays. */
typedef struct emagls_job {
    emagls_design_desc desc;
    const double* hL;           /* [nsamp x ndirs] */
    const double* hR;
    const double* hrir_azi;     /* [ndirs] */
    const double* hrir_zen;     /* [ndirs]; NULL: horizontal grid (MAGLS_2D) */
    const double* mic_azi;      /* [nmics], array designs */
    const double* mic_zen;      /* [nmics]; NULL: equatorial array (EMA_CH / EMA_SH) */
    const double* atf;          /* FROM_ATF: [atf_taps x nmics x natf] */
    const double* atf_azi;      /* FROM_ATF: [natf] */
    const double* atf_zen;
    void* wL;                   /* [len x channels] real, or interleaved complex for a complex basis (emagls_plan_info.out_is_complex) */
    void* wR;
} emagls_job;
/* Runs the whole list and returns when every job's filters are in place.  Consecutive jobs of one shape form chunks of up to
 * batch_size designs (<= 0: 32; more than 16 only for array designs that take the register-resident sweep) that run as lane
 * batches -- one launch of every kernel for the chunk, one resident sweep launch --; up to in_flight chunks (<= 0: 4) are between
 * upload and collection at any time, each driven by a thread of the library, so that uploads, launches and the collection of
 * results overlap with the GPU's work on the other chunks.  Plans and batches of chunks whose descriptors repeat stay resident
 * between calls (emagls_cache_clear releases them).  Same filters as the single calls.
 * HRIR sets on one geometry: a chunk whose jobs all have the same descriptor (byte for byte; eMagLS / eMagLS2 / EMAinCH up to 32
 * channels, built-in basis, no covariance constraint) and the same grids (compared on the host, then by the batch on the device) shares
 * its geometry stages WITHOUT being asked: they run once per chunk (emagls_batch_set_geometry_sharing), and a resident chunk keeps
 * them between calls -- after one clean run it enqueues only what an HRIR set enters until a grid is replaced, a run needs a recovery
 * or emagls_cache_clear is called.  A chunk whose jobs do not all agree runs as independent designs.  The shared filters equal the
 * independent designs' to 1e-9 relative (a lane batch warm-starts the Jacobi runs of its per-bin factors by the launch's size;
 * measured at the benchmark's shape: 1.3e-13), and every run of a chunk on the same inputs returns the same bits.
 * flags: EMAGLS_JOBS_INDEPENDENT -- no sharing unless asked: every design computes its own geometry stages.  (EMAGLS_JOBS_AUTO_SHARE=0
 * in the environment does the same.)  EMAGLS_JOBS_SHARE_GEOMETRY -- asks every batch for sharing, also the kinds the scheduler's own
 * rule leaves alone (MagLS / LS sets on one grid); for the designs above it is redundant.  eMagLS / eMagLS2 designs with 33..64
 * channels run plan by plan: with this flag they are cut one per chunk and a plan keeps G_k, the per-bin factors and Y_reg_inv_k
 * from its last clean run while its own grids stay the same (a 64-capsule array: 31 -> 8 ms per set). */
#define EMAGLS_JOBS_SHARE_GEOMETRY 1
#define EMAGLS_JOBS_INDEPENDENT 2
int emagls_jobs_run(const emagls_job* jobs, int64_t njobs, int batch_size, int in_flight, int flags);
/* ---- job lists over several GPUs ------------------------------------------------------------------------------------------
 * Independent jobs shard without any collective on the data path.  emagls_jobs_shard is the split every runner of this
 * library uses (emagls_amd/batch.py restated in C): array-radius studies -- jobs that differ only in mic_radius, up to 32 microphones
 * -- are sorted by simulation order (dependencies/getSMAIRMatrix.m:95), cut into lane batches of equal COST (on average max_batch
 * designs, <= 32; every design of a batch laid out for the batch's highest order: sim_order_pad[j], to be written into
 * desc.sim_order_pad) and whole batches go to ranks by longest processing time; any other job is a unit of its own.  rank_of_job[j]:
 * the rank of job j; order_in_rank[j] (optional): its position in that rank's share (the jobs of a batch adjacent, cheap batches
 * first); sim_order_pad (optional).  Needs no GPU. */
int emagls_jobs_shard(const emagls_job* jobs, int64_t njobs, int world, int max_batch, int* rank_of_job, int* order_in_rank, int* sim_order_pad);
/* The GPUs of ONE process: the list is split with emagls_jobs_shard over `ndevices` devices (their HIP ordinals in `devices`; the
 * same ordinal may appear twice) and every device's share runs through emagls_jobs_run from a host thread of its own.  Inputs and
 * outputs are host arrays (or memory every listed device can reach); there is no gather: each device writes its jobs' filters where
 * the jobs point.  What a MEX caller -- one MATLAB process -- uses for BASELINE config 4's 256 radii or config 5's subjects
 * (emagls_mex('jobs', jobs, batchSize, inFlight, shareGeometry, devices)); one process per GPU with an RCCL gather of device buffers
 * is emagls_amd/batch.py. */
int emagls_jobs_run_devices(const emagls_job* jobs, int64_t njobs, const int* devices, int ndevices, int batch_size, int in_flight, int flags);
/* Shape of a design's filters from its descriptor alone (no plan, no device memory: what a caller needs to allocate wL / wR of a
 * job): rows x cols, real or interleaved complex -- len x channels like the reference's outputs (lib/getEMagLsFilters.m:139-142);
 * LS keeps the HRIR length (lib/getLsFilters.m:33); channels = (N+1)^2 in the SH domain, 2N+1 circular harmonics (MAGLS_2D,
 * EMA_CH), the microphones for EMAGLS2 / FROM_ATF; complex for a complex basis except FROM_ATF.  The same numbers as
 * emagls_plan_info.out_rows / out_cols / out_is_complex of a plan of that descriptor. */
int emagls_design_out_shape(const emagls_design_desc* desc, int64_t* rows, int64_t* cols, int* is_complex);
/* Measurement hooks of the job lists (bench.py's roofline figure): level > 0 makes the chunks' batches bracket their sweep launch
 * with HIP events on the stream it is launched on; emagls_jobs_sweep_times then reports, for every resident chunk that ran since,
 * the duration of its LAST sweep launch (ms) and the designs it covered (count: chunks available, capacity: room in the arrays). */
int emagls_jobs_set_profiling(int level);
int emagls_jobs_sweep_times(double* ms, int* designs, int capacity, int* count);
/* Which form the chunks of the job lists ran in, counted per chunk execute since the last emagls_cache_clear: as independent designs,
 * sharing with the geometry stages run ("cold"), sharing on kept geometry ("warm"). */
int emagls_jobs_geometry_runs(long long* independent, long long* cold, long long* warm);
/* The scheduler's rule for sharing a chunk's geometry, on descriptors and host grids alone (needs no GPU): *share = 1 when the
 * `njobs` jobs would run as one sharing chunk. */
int emagls_jobs_would_share_geometry(const emagls_job* jobs, int njobs, int* share);

/* HRIR sets on ONE grid (and, for the array kinds, ONE array) in one call -- the loop
 *     for i = 1:nsets, [wL(:,:,i), wR(:,:,i)] = getEMagLsFilters(hL(:,:,i), hR(:,:,i), grid..., array..., order, fs, len, shDefinition); end
 * around lib/getLsFilters.m:30 / getMagLsFilters.m:30 / getMagLsFilters2D.m:1 (hrir_zen NULL) / getEMagLsFilters.m:32 /
 * getEMagLs2Filters.m:32 / getEMagLsFiltersEMAinCH.m:32 / getEMagLsFiltersEMAinSH.m:32 (mic_zen NULL; EMAinSH plan by plan), kind =
 * EMAGLS_KIND_LS / _MAGLS / _MAGLS_2D / _EMAGLS / _EMAGLS2 / _EMA_CH / _EMA_SH.  hL, hR [nsamp x ndirs x nsets] (MATLAB 3-D arrays), wL, wR [len x channels x nsets] (LS: nsamp rows; `fs`
 * and `len` are ignored for LS).  Internally: plans and geometry-sharing batches of up to 16 sets (kept for the next call of the
 * same shape; emagls_cache_clear releases them), one resident sweep launch per batch; the same filters as nsets single calls.
 * eMagLS / eMagLS2 with 33..64 channels: the sets pass through two plans that keep their geometry stages between sets. */
int emagls_design_hrir_sets(int kind, const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, int64_t nsets,
                            const double* hrir_azi, const double* hrir_zen, double mic_radius, const double* mic_azi, const double* mic_zen,
                            int64_t nmics, int order, double fs, int64_t len, int basis, void* wL, void* wR);
/* The HRTF subjects of ONE ATF set in one call (BASELINE config 5: the loop over subjects around
 * lib/getEMagLsFiltersFromAtf.m:1): hL, hR [nsamp x ndirs x nsets], the other arguments as emagls_get_emagls_filters_from_atf;
 * wL, wR [filter_len x nmics x nsets].  The ATF set is uploaded once and its side (spectra, matching, per-bin factors) computed
 * once per batch of up to 16 subjects; one resident sweep launch per batch.  The same filters as nsets single calls -- also for
 * ATF sets whose low bins need the dense route (any width up to 32 microphones), whose subjects run plan by plan. */
int emagls_from_atf_hrir_sets(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, int64_t nsets, const double* hrir_azi,
                              const double* hrir_zen, const double* atf_irs, int64_t atf_taps, int64_t nmics, int64_t natf, const double* atf_azi,
                              const double* atf_zen, double fs, int64_t filter_len, double f_trans, double* wL, double* wR, double* mean_dev);
/* A batch may also hold EMAGLS_KIND_FROM_ATF plans of one shape -- the HRTF subjects of one ATF set (BASELINE config 5: 8 subjects).
 * lib/getEMagLsFiltersFromAtf.m:54-95,100-104: the spectra of the matched ATFs and their per-bin factors do not depend on the
 * HRIRs.  When all plans hold the same grids and the same ATF set (compared on the device whenever one of them was replaced) the
 * batch computes that side ONCE, on plan 0, and every subject's prologue, least-squares rows and sweep lane read it; the sweep is
 * one resident launch for all subjects.  Plans with different ATF sets, or ATFs whose low bins need the dense route, run
 * unshared (still one sweep launch).  *shared reports which after an execute. */
int emagls_batch_shares_atf_side(emagls_batch* batch, int* shared);
int emagls_batch_execute(emagls_batch* batch);
int emagls_batch_synchronize(emagls_batch* batch);
/* synchronise once, check every plan's device-side status flags, copy all filters out: wL[j], wR[j] receive the filters of
 * plan j (host or device pointers).  Equivalent to emagls_plan_get_filters on every plan, without the per-plan round trips. */
int emagls_batch_get_filters(emagls_batch* batch, void* const* wL, void* const* wR);
/* profiling: with level >= 1 HIP events bracket the sweep launch of every execute (on the batch stream);
 * emagls_batch_sweep_time returns the duration in ms of the last execute's sweep (synchronises the batch). */
int emagls_batch_set_profiling(emagls_batch* batch, int level);
/* *lanes = 1 when the batch runs in lane mode (one launch of every kernel for all its designs), 0 in stream mode.  Designs of
 * one shape class whose routes differ by a bin or an order (array radii of one simulation order) are given common routes. */
int emagls_batch_lane_mode(emagls_batch* batch, int* lanes);
/* Run the batch on the caller's hipStream_t instead of its own (the caller keeps ownership and must not use the stream while a
 * batch call is in progress).  Why one would: the HIP runtime multiplexes all streams of a process onto 4 hardware queues, and
 * two batches whose streams land on the same queue execute strictly one after the other; a caller that creates its streams
 * first and hands one to each batch in flight decides the mapping itself (bench.py does). */
int emagls_batch_set_stream(emagls_batch* batch, void* hip_stream);
/* A lane batch of more than 8 designs runs the stages before its sweep as two lane groups on two streams (then one sweep launch
 * for all designs).  The second group's stream comes from the library unless the caller hands one over here -- for the same
 * reason as emagls_batch_set_stream: which hardware queue a stream lands on is decided by the order the streams are created in. */
int emagls_batch_set_side_stream(emagls_batch* batch, void* hip_stream);
int emagls_batch_sweep_time(emagls_batch* batch, double* ms);
/* Lane mode: 1..4 HIP streams for the stages before the sweep (default 1).  With more than one the independent branches of the
 * design fork onto side streams and the batch runs eagerly (a graph is only captured from one stream): [HRIR-grid SH matrix,
 * Gram matrix, Cholesky factor, Householder-route factors] | [array model, order terms, G_k of every bin] | [HRIR prologue, least-squares right-hand sides]
 * | [Gram-route factors].  Shortens the path to the batch's sweep from the sum of the kernels to its longest branch (what a
 * short run, a pipeline filling from empty, is bound by); with many batches in flight it only adds queue contention.  A batch with
 * forked stages is taken to have the device to itself: what its sweep does not need -- the Cholesky factor and the orthonormal
 * route of the ill-conditioned low bins, which only feed the filters' rows (lib/getEMagLsFilters.m:94) -- then runs NEXT to the sweep
 * on a stream of its own (designs on the synthesising sweep; EMAGLS_DEFER_HH=0 keeps everything before the sweep). */
int emagls_batch_set_streams(emagls_batch* batch, int nstreams);
/* Lane mode, one stream: the order in which a batch of up to 8 designs issues the stages before its sweep.  0 (default): the
 * order of a single design.  1: the kernels that fill the chip first (HRIR transform, SH Gram matrix, G_k of every bin), the
 * latency-bound chains (Cholesky, per-bin QR / Jacobi) after them.  2: the chains first.  Batches that run side by side in the
 * SAME order meet at the same kernels and add up their times; complementary orders hide one batch's chains behind the other's
 * bandwidth-bound kernels.  The two lane groups of a batch of more than 8 designs take orders 1 and 2 by themselves
 * (EMAGLS_STAGGER=0 switches that off).  Same filters in every order (no arithmetic changes, only the issue order). */
int emagls_batch_set_stage_order(emagls_batch* batch, int order);
int emagls_batch_destroy(emagls_batch* batch);

#ifdef __cplusplus
}
#endif
#endif /* EMAGLS_H */
