// Launcher declarations shared by the kernel translation units and the C ABI (capi.hip and jobs.hip over host_internal.hpp, decode_api.hip, render_api.hip).
#pragma once
#include <algorithm>
#include <functional>

#include "common.hpp"

namespace emagls {

// ---- sh_basis.hip
void launch_zero(void* p, size_t bytes, hipStream_t st);
void launch_compare_words(const void* a, const void* b, size_t bytes, int* differ, hipStream_t st);
void launch_broadcast_lanes(const void* src, size_t bytes, size_t stride, int nlanes, hipStream_t st);
struct LanePtrs { void* p[64]; };   // [2 j + ear] for up to 32 designs
void launch_scatter_lanes(const void* srcL, const void* srcR, size_t stride, size_t bytes, int n, const LanePtrs& dst, hipStream_t st);
void launch_gather_buffers(const LanePtrs& src, const LanePtrs& dst, int nbuf, size_t bytes, hipStream_t st);   // nbuf <= 64 device buffers of `bytes` each
struct BufferMoves { const void* src[96]; void* dst[96]; size_t bytes[96]; int n; };   // device-to-device copies of one launch
void launch_move_buffers(const BufferMoves& m, hipStream_t st);
void launch_ch_basis(int N, int M, const double* azi, bool cplx_basis, void* out, int ld, hipStream_t st, bool out_real = false);
void launch_sh_coeff(int N, double* tab, hipStream_t st);
inline size_t esz(bool c) { return c ? sizeof(cplx) : sizeof(double); }   // element size of a real / complex basis
inline size_t sh_coeff_count(int N) { return (size_t)2 * (N + 1) * (N + 1) + 2 * (N + 1); }
void launch_sh_basis(int N, int64_t D, const double* azi, const double* zen, const double* tab, bool cplx_basis,
                     void* Y, int64_t ld, hipStream_t st);
void launch_transpose_conj(const void* Y, int64_t D, int64_t S, int64_t ldY, void* Yt, int64_t Dpad, int64_t ldYt,
                           bool is_cplx, bool conj_it, hipStream_t st);

// ---- modal.hip
void launch_modal_bn(int N, int64_t nfreq, const double* kr, double kr_scale, double out_scale, void* bn,
                     int64_t stride_k, int64_t stride_n, hipStream_t st, const int* n_valid = nullptr);

// ---- fft.hip
void launch_twiddles(int nfft, void* tw, hipStream_t st);
int hrir_dirsum_chunks(int64_t D);
void launch_hrir_grpdelay(const double* hL, const double* hR, int64_t L, int64_t D, int nfft, const void* tw,
                          double* partial, double* grpd, hipStream_t st);
// HcT (optional): direction-major real copy of the complex rows [D][ldT], HcT[d][2 (e n_c + kb) + re/im]
void launch_hrir_fft(const double* hL, const double* hR, int64_t L, int64_t D, const int64_t* didx, int nfft,
                     const void* tw, const double* grpd, int mode, int n_c, int kabs0, void* Hc, double* Habs,
                     int64_t ldD, hipStream_t st, double* HcT = nullptr, int ldT = 0);
void launch_real_fft_gather(const double* x, int64_t L, int64_t ncols, const int64_t* colidx, int nfft, const void* tw,
                            void* out, int64_t ldo, int64_t inner, int64_t ld_inner, hipStream_t st);
void launch_filter_epilogue(const void* W, int C, int nfft, int len, const void* tw, const double* grpd, int conj_mode,
                            int dc_rule, int shift_mode, int out_cplx, void* outL, void* outR, hipStream_t st, int n_ears = 2,
                            double fade_rel = 0.15);
// ---- fft_debug.hip: the launchers above on host arrays (include/emagls.h: emagls_debug_twiddles ... emagls_debug_real_spectra); synchronous
void twiddles_debug(int nfft, void* tw);
void filter_epilogue_debug(const void* W, int C, int nfft, int len, const double* grpd, int conj_mode, int dc_rule, int shift_mode, int out_cplx,
                           int n_ears, double fade_rel, void* outL, void* outR);
void hrir_spectra_debug(const double* hL, const double* hR, int64_t L, int64_t D_src, int64_t D, const int64_t* didx, int nfft, int mode, int n_c, int kabs0,
                        const double* grpd_in, int64_t ldD, int ldT, double* grpd_out, void* phs, void* Hc, double* Habs, double* HcT);
void real_spectra_debug(const double* x, int64_t L, int64_t ncols_src, int64_t ncols, const int64_t* colidx, int nfft, int64_t ldo, int64_t inner,
                        int64_t ld_inner, void* out);

// ---- gram_chol.hip
int gram_ksplit(int64_t D, int S);
int64_t gram_dpad(int64_t D, int S);
void launch_gram(const void* Yc, int64_t D, int S, int64_t ld, bool is_cplx, void* Gp, void* G, void* R, int Sh, hipStream_t st);
void launch_cholesky(void* G, int S, bool is_cplx, int* flag, hipStream_t st);
void launch_qform(const void* Yc, const void* R, void* Rinv, int S, int64_t D, int64_t ld, bool is_cplx, void* Q, hipStream_t st);
// zs R^H = z for the rows Z[kb][c][:] of the flagged bins (cond_ok[kb] == 0; cond_ok null: every bin of [k0, P)), in place (complex basis)
void launch_zsolve_flagged(void* Z, int ldS, const void* R, const void* Rinv, const double* cond_ok, int S, int C, int P, int k0,
                           hipStream_t st);
void launch_tn(const void* R, const void* E, int S, int C, int ldE, int nOrders, bool is_cplx, void* Tn, int64_t ldS,
               hipStream_t st);
void launch_small_gemm(const void* A, int lda, bool a_cplx, const void* B, int ldb, bool b_cplx, void* Cm, int ldc,
                       bool c_cplx, int M, int N, int K, hipStream_t st);

void launch_magls_m(const void* R, int C, bool is_cplx, int P, void* Mw, double* cond_ok, int* status, hipStream_t st);

// ---- factor.hip
struct FactorArgs;
void launch_factor(const FactorArgs& a, int nbins, bool tn_cplx, hipStream_t st, int phases = 3);
// Jacobi SVD only, on Gram matrices that gram_solve_kernel handed over (route[kb] == 1); bins with route[kb] == 2 are skipped
void launch_factor_jacobi_gram(const FactorArgs& a, int nbins, hipStream_t st);

// ---- gramroute.hip
void launch_gram_kmat(const void* Gy, const void* E, int S, int ldE, int C, int nOrd, bool is_cplx, void* F, int64_t ldF, double* Kmat, int ldK,
                      hipStream_t st);
void launch_gram_gemm(const void* bn, int nOrd, int P, int kb0, int nbins, double* Cf, int ldC, const double* Kmat, int ldK, int C, double* Apk,
                      int ldA, hipStream_t st);
void launch_gram_solve(const double* Apk, int ldA, int C, int kb0, int nbins, double reg_c, void* Mw, void* R2w, double* sv, int* route,
                       int* sweeps_out, hipStream_t st);
// out[r][s] = conj( sum_d H[r][d] conj(Yc[d][s]) ) for the 2 n_c complex rows r = e n_c + kb held direction-major in HcT
// (launch_hrir_fft); Yc [Dpad][ldY] real or complex, rows >= D zero.  Pw: workspace hy_mfma_workspace_doubles(...)
size_t hy_mfma_workspace_doubles(int n_c, int S, bool y_cplx);
int hy_mfma_kpad(int D);   // rows of both operands that the product reads (zero beyond D)
void launch_hy_conj_mfma(const double* HcT, int ldT, int n_c, const void* Yc, int64_t ldY, bool y_cplx, int D, int S, double* Pw, void* out,
                         int ldS, hipStream_t st);
void launch_ls_gram(const void* Hc, int64_t ldH, int n_c, const void* G, int64_t g_stride, int64_t ldD, const void* Mw, int D, int C, int P,
                    int kb_lo, int kb_hi, void* W, hipStream_t st);

// ---- sweep.hip
struct DenseSweepArgs;
struct HalfSweepArgs;
struct HalfSweepMulti;
void launch_sweep_dense(const DenseSweepArgs& a, int kb, bool x_cplx, hipStream_t st);
int dense_sweep_nwg(int D, int C);
void launch_sweep_half(const HalfSweepMulti& m, int kb, hipStream_t st);
void launch_sweep_half_finalize(const HalfSweepMulti& m, int kb_last, hipStream_t st);
// ---- sweep_persist.hip
int persist_sweep_nwg(int D);
bool persist_sweep_supported(int D, int C);
size_t persist_sweep_ll_bytes(int D, int C);
void launch_sweep_persist(const HalfSweepMulti& m, hipStream_t st);
int persist_sweep_dpw(int D);
// residency, decided before a launch: the runtime's occupancy of the kernel variant x the CUs of an XCD (EMAGLS_CU_BUDGET overrides
// the device's CU count) against the workgroups `ndesigns` designs place there
int sweep_cu_budget();
bool persist_sweep_fits(int D, int C, int ndesigns);
bool synth_sweep_fits(int D, int nmics, int nOrd, int ndesigns);
// ---- sweep_synth.hip: the resident sweep with the slab of every bin evaluated inside the launch (Legendre addition theorem)
bool synth_sweep_supported(int D, int nmics, int nOrd);
int synth_nord_pad(int nOrd);
// bsc [P][nord_pad] from bn [P][nOrd]; Pm [32][32] from the complex copy of pinv(Y_lo) (Zlo null: identity, raw microphones)
// smap [34]: the chain's row order of the microphones (row -> microphone), then the numbers of antipodal pairs and of single microphones
void launch_synth_prepare(const void* bn, int nOrd, int P, void* bsc, const void* Zlo, int ldZ, int nOut, int M, const int* smap, double* Pm, hipStream_t st);
// Mt[kb] = Pm^T M_kb Pm for kb in [k0, P) (slot kb - 1 like Mw) and Winit = W(k0-1,:) Pm
void launch_synth_mt(const void* Mw, const double* Pm, int nOut, int M, int k0, int P, const void* W, void* Mt, void* Winit, hipStream_t st);
// W[e][kb][:] = (U[e][kb][:] Pm^T) conj(M_kb) for kb in [k0, P)
void launch_synth_winit(const void* W, const void* Pm, int nOut, int M, int k0, int P, void* Winit, hipStream_t st, bool shared_geometry);
// (shared_geometry: Pm and Mw are ONE design's for every lane of the launch)
void launch_synth_rows(const void* U, int nchunks, const void* Pm, const void* Mw, int nOut, int M, int k_lo, int k_hi, int P, void* W, hipStream_t st,
                       bool shared_geometry = false);
// least-squares bins [kb_lo, kb_hi) of the Gram route: Upart[chunk][e][kb][row] = partial sums of H(kb,:) conj(g_kb) over a chunk of directions
// (synth_ls_chunks(D) chunks; launch_synth_rows with that many chunks turns them into W)
int synth_ls_chunks(int D);
void launch_synth_ls(const void* Hc, int64_t ldH, int n_c, const void* bsc, int nord_pad, const double* dir_azi, const double* dir_zen, const double* mic_azi,
                     const double* mic_zen, const int* smap, int D, int M, int P, int kb_lo, int kb_hi, void* Upart, hipStream_t st, bool shared_geometry = false);
void launch_sweep_synth(const HalfSweepMulti& m, hipStream_t st);
// ---- ls_shared.hip: least-squares rows of the HRIR sets of one geometry from the kept operand Yls [bin 1 .. ls_end-1][C][ldD] = Y_reg_inv_k
// Gram-route bins [kb_lo, kb_hi) of a synthesising design: Yls[kb-1] = conj(g_kb) Pm^T conj(M_kb), g_kb from the angles (ONE design's operands)
void launch_yls_gram(const void* bsc, int nord_pad, const double* dir_azi, const double* dir_zen, const double* mic_azi, const double* mic_zen,
                     const int* smap, const double* Pm, const void* Mw, int D, int nOut, int kb_lo, int kb_hi, void* Yls, int64_t ldD, hipStream_t st);
// W[e][kb][:] = Hc[e][kb][:] Yls[kb-1] for kb in [1, ls_end), for every lane of the launch context in ONE launch (Yls is the same for all)
void launch_ls_shared_rows(const void* Hc, int64_t ldH, int ls_end, const void* Yls, int64_t ldD, int D, int C, int P, void* W, hipStream_t st);
// ---- synth_debug.hip: synth_group<gs> on host arrays (bsc [nbins][nord_pad], x [nx]): g_plus / g_minus [nbins][nx] = E + O / E - O; synchronous
// x2 [ndirs][nmics] = synth_x2 (twice the cosine between direction and microphone, as the sweeps form it) on host arrays; synchronous
void synth_cosines_debug(const double* dir_azi, const double* dir_zen, int64_t ndirs, const double* mic_azi, const double* mic_zen, int nmics, double* x2);
void synth_operand_debug(const void* bsc, int nbins, int nord_pad, const double* x, int64_t nx, int gs, void* g_plus, void* g_minus);
// ---- sweep_reg.hip: the synthesising sweep with the operand in registers (a lane = a direction; no slab in LDS).  Units = antipodal
// microphone pairs + single microphones (smap[32] + smap[33]); argument blocks in device memory (store_sweep_args)
int reg_sweep_max_units();
bool reg_sweep_supported(int D, int nmics, int nunits, int nOrd);
size_t reg_sweep_ll_bytes(int D, int nmics);
int reg_sweep_capacity(int D);                  // designs one launch can keep resident on this device
int reg_sweep_slots_per_xcd();                  // the sweep gate's capacity: thirds of a CU per XCD
int reg_sweep_pick_waves(int D, int ndesigns);  // waves per workgroup of a launch of `ndesigns` designs (4, 8 or 12; 0: cannot be resident)
int reg_sweep_gate_cost(int D, int ndesigns);   // what such a launch takes of the gate's capacity
bool reg_sweep_fits(int D, int nmics, int nunits, int nOrd, int ndesigns);
void launch_sweep_reg(const HalfSweepArgs* args_dev, const HalfSweepArgs& a0, int n, hipStream_t st);
double reg_contract_selftest();
double gram_tile_selftest(bool four);   // gram_chol.hip: the LDS-staged Gram tile kernels against a host sum
void store_sweep_args(const HalfSweepArgs* host, int n, HalfSweepArgs* dev, hipStream_t st);
void launch_sweep_finalize(const void* Wpart, void* W, int nWG, int C, int P, int kb_last, hipStream_t st);
void launch_hy_conj(const void* Hc, int64_t ldD, int nrows, const void* Yc, int64_t ldY, bool y_cplx, int D, int S, void* Pw, void* out,
                    int ldS, hipStream_t st);
size_t hy_workspace_elems(int nrows, int ldS);
void launch_ypinv(const void* Q, int64_t ldQ, bool q_cplx, const void* Zb, int ldS, int D, int S, int C, void* Ypinv,
                  int64_t ldD, hipStream_t st);
void launch_ls_apply(const void* Hc, int64_t ldH, int n_c, const void* Zf, bool z_cplx, int64_t ldD, int D, int C, int P,
                     int kb_lo, int kb_hi, void* W, hipStream_t st);
void launch_ls_filters(const double* hL, const double* hR, int64_t L, int D, const void* Yp, bool cplx_basis, int64_t ldD,
                       int C, void* wL, void* wR, hipStream_t st);
void launch_conj_copy(const void* in, void* out, int64_t n, bool is_cplx, hipStream_t st);
// rows of real-SH coefficients -> complex-SH coefficients in place: W_c = W_r T_N (Y_c = Y_r T_N, sh_basis.hip conventions)
void launch_sh_rows_to_complex(void* W, int C, int nrows, int order, hipStream_t st);
void launch_widen(const void* in, int64_t ldi, bool in_cplx, void* out, int64_t ldo, int rows, int cols, bool transpose,
                  bool upper_only, hipStream_t st);

// ---- wide.hip: LS / MagLS above 32 channels (SH orders 5..7)
void launch_gram_inverse(const void* R, int S, bool is_cplx, void* M, int* status, hipStream_t st, void* work = nullptr);   // work (S > 64): S x S complex + 2 doubles
void launch_ypinv_gram(const void* Ycm, int64_t ldD, bool is_cplx, const void* M, int S, int D, void* Ypinv, hipStream_t st);
void launch_sweep_wide(const DenseSweepArgs& a, int kb, bool x_cplx, hipStream_t st);
void launch_sweep_wide_finalize(const void* Wpart, void* W, int nWG, int C, int P, int kb_last, hipStream_t st);

// ---- wide_array.hip: eMagLS / eMagLS2 with 33..64 channels
void launch_wa_assemble(const void* Tn, const void* bn, int nOrd, int S, int C, int ldS, int P, int kb0, int nbins, void* B, hipStream_t st);
void launch_wa_factor(void* B, void* Vw, int S, int C, int ldS, int nbins, double reg_c, double* tauw, void* R2w, void* Nw, double* sv, int* sweeps,
                      void* Z, hipStream_t st);
// tiled form for S > 4096 rows and up to 32 columns (row blocks + a tree step over their triangles); ws: wa_tiling(...).bytes
struct WaTiling { int leaves, leaf_h, ldT; size_t off_stack, off_vt, off_zt, off_tau, bytes; };
// leaf_bound: 0 = the library's bound of the leaf height (EMAGLS_WA_LEAF_ROWS or its default), else 1024 ... 4096 in its place
WaTiling wa_tiling(int S, int C, int nbins, int leaf_bound = 0);
void launch_wa_factor_tiled(void* B, void* Vw, int S, int C, int ldS, int nbins, double reg_c, double* tauw, void* R2w, void* Nw, double* sv,
                            int* sweeps, void* Z, void* ws, hipStream_t st, int leaf_bound = 0);
void launch_wa_yri(const void* Q, int64_t ldQ, const void* Z, int S, int C, int ldS, int D, int64_t ldD, int nbins, void* Yri, hipStream_t st);
void launch_wa_ls(const void* Hc, int64_t ldH, int n_c, const void* Yri, int64_t ldD, int D, int C, int P, int kb_first, int kb_end, void* W, hipStream_t st);
void launch_wa_lo_gram(const void* Ycm, int M, int nOut, double* Ag, hipStream_t st);
void launch_wa_e(const void* Ycm, int M, int nOut, int S, const void* Minv, void* E, int ldE, hipStream_t st);

// ---- dspace.hip
void launch_qt(const void* Yc, int64_t ldY, const void* E, int ldE, int D, int S, int C, int nOrders, bool is_cplx, void* QT,
               int64_t ldD, hipStream_t st);
// real_mode: complex basis evaluated on the real order terms (sh_order >= 0: channels are SH coefficients up to that order;
// < 0: channels are independent, e.g. microphones)
// k_end (< 0: P): bins [k0, k_end) only -- the designs whose sweep evaluates its operands itself (sweep_synth.hip) need G_k for their
// least-squares bins alone
void launch_dspace_g(const void* QT, int64_t ldD, bool is_cplx, const void* bn, int nOrders, int D, int C, int P, int k0, void* G,
                     hipStream_t st, int real_mode = 0, int sh_order = -1, int k_end = -1);
void launch_cond_flags(const double* sv, int C, int P, int hh_end, double* cond_ok, hipStream_t st);
// (Ycm: the column-major SH matrix [S][ldYcm] of a real basis -- the coalesced form; null: the row-major walk)
// (cond_ok null: every bin of [k0, P), flagged or not -- the least-squares bins of the kept operand Yls, ls_shared.hip)
void launch_yri_accurate(const void* Q, int64_t ldQ, bool is_cplx, const void* Z, int ldS, const double* cond_ok, int D, int S,
                         int C, int P, int k0, void* Yri, int64_t ldD, hipStream_t st, const void* Ycm = nullptr, int64_t ldYcm = 0);

// ---- atf.hip
void launch_grid_match(const double* aziA, const double* zenA, int64_t nA, const double* aziB, const double* zenB,
                       int64_t nB, double* cartB, int64_t* idx, double* dev_deg, double* mean_dev, hipStream_t st);
void launch_atf_colidx(const int64_t* idx, int64_t nA, int M, int64_t* colidx, hipStream_t st);

// ---- microbench.hip
double measure_fp64_peak(int which, int reps, bool burst = false, double* mhz = nullptr);

// ---- decode.hip
void binaural_decode_real(const double* sig, int64_t n, int C, const double* wL, const double* wR, int64_t len,
                          double* out /* [n x 2] column-major */, hipStream_t st,
                          const cplx* sigc = nullptr /* the C / 2 complex channels whose planes are `sig`'s channels, interleaved (wave form only) */);
bool decode_wave_form(int64_t len);
void binaural_decode_complex(const void* sig, bool sig_cplx, int64_t n, int C, const void* wL, const void* wR, bool w_cplx, int64_t len,
                             double* sig2, double* w2L, double* w2R, double* out, double* imag_abs, double* d_tmp, hipStream_t st,
                             int64_t imag_skip = 0 /* samples left out of the imaginary-part sums (the compensateDelay cut) */);
// (with imag_abs: d_tmp [2n + 2] holds the discarded imaginary part [2][n] on return, then its two sums)
void decode_cache_clear();
// out[e] = sum(|x[e*n + i]|, i = skip .. n-1) for the ncols columns of x [ncols][n]
void launch_abs_sum_cols(const double* x, int64_t n, int64_t skip, int ncols, double* out, hipStream_t st);

// ---- rotate.hip
// N of a layout (0: SH, (N+1)^2 channels in ACN order; 1: CH, 2N+1 channels [C_0, C_-1, C_1, ..., C_-N, C_N]); -1 if C fits not
int rotate_order(int layout, int64_t C);
// yaw rotation of in [C][n] (real, or interleaved complex): out [C][n], complex when in_cplx || cplx_basis.  yaw: device, one
// angle (per_sample false) or n angles.  transpose: the filter-side form of a fixed angle (w Rot instead of x Rot^T).
// ld_in / ld_out: elements between the channels of in / out (0: n) -- a block of a longer signal, decode_stream.hip
// L listeners of the one signal `in` (a listener group): listener l takes its angles at yaw + l la and writes out + l lo (elements)
void launch_rotate_yaw(const void* in, bool in_cplx, int64_t n, int C, int layout, bool cplx_basis, const double* yaw, bool per_sample,
                       bool transpose, void* out, hipStream_t st, int64_t ld_in = 0, int64_t ld_out = 0, int L = 1, int64_t la = 0,
                       int64_t lo = 0);
// ---- rotate3.hip
int rotate3_max_order();   // 15: the largest SH order of the three-axis rotation
// rotation R = Rz(yaw) Ry(pitch) Rx(roll) of the SH (ACN) signal in [C][n] (real, or interleaved complex): out [C][n], complex
// when in_cplx || cplx_basis.  Each angle: device pointer, null (0), one value (*_ps false) or n values.  transpose: the
// filter-side form of a fixed rotation (w M instead of x M^T).  C = (N+1)^2 with N <= 15, else Error.  ld_in / ld_out as above.
// L listeners as above, la[3]: the listener strides of yaw, pitch and roll (null: L = 1)
void launch_rotate3(const void* in, bool in_cplx, int64_t n, int C, bool cplx_basis, const double* yaw, bool yaw_ps, const double* pitch,
                    bool pitch_ps, const double* roll, bool roll_ps, bool transpose, void* out, hipStream_t st, int64_t ld_in = 0,
                    int64_t ld_out = 0, int L = 1, const int64_t* la = nullptr, int64_t lo = 0);
// M [(N+1)^2 x (N+1)^2] column-major, out_row = in_row M^T; the same device code as launch_rotate3
void launch_rotate3_matrix(int N, bool cplx_basis, double yaw, double pitch, double roll, void* out, hipStream_t st);
void rotate3_cache_clear();
// ---- the ENC forms of the two rotations (encode_tile.hpp): the array encoder of an encoded decode stream
// inside the rotation launch.  enc [C][M] device, row-major (interleaved complex when enc_cplx), 1 <= M, C <= 64; x: the real
// microphone block, microphone m at x + m ldx.  The encoded signal s_c[t] = sum_m enc[c][m] x[m][t] (fma from 0, m ascending;
// complex when enc_cplx) is what the rotation turns: out, ld_out, L, la, lo as in launch_rotate_yaw / launch_rotate3.
struct EncodeBlock { const double* enc; bool enc_cplx; int M; const double* x; int64_t ldx; };
void launch_rotate_yaw_encoded(const EncodeBlock& e, int64_t n, int C, int layout, bool cplx_basis, const double* yaw, bool per_sample, void* out,
                               hipStream_t st, int64_t ld_out = 0, int L = 1, int64_t la = 0, int64_t lo = 0);
void launch_rotate3_encoded(const EncodeBlock& e, int64_t n, int C, bool cplx_basis, const double* yaw, bool yaw_ps, const double* pitch, bool pitch_ps,
                            const double* roll, bool roll_ps, void* out, hipStream_t st, int64_t ld_out = 0, int L = 1, const int64_t* la = nullptr,
                            int64_t lo = 0);
// the encoder alone: out [C][ld_out] = the encoded block (complex when enc_cplx)
void launch_encode_block(const EncodeBlock& e, int64_t n, int C, void* out, int64_t ld_out, hipStream_t st);
// ---- resample.hip
constexpr int64_t kResampleMaxRatio = 65536;   // the largest max(p, q) after reduction
int64_t resample_length(int64_t n, int64_t p, int64_t q);   // ceil(n p / q)
// MATLAB's resample(x, p, q) of each column of in [nch][n] (real, or interleaved complex): out [nch][ceil(n p / q)], same type.
// p, q reduced, both >= 1; max(p, q) > kResampleMaxRatio: Error(EMAGLS_ERR_UNSUPPORTED)
void launch_resample(const void* in, bool cplx_in, int64_t n, int64_t nch, int64_t p, int64_t q, void* out, hipStream_t st);
void resample_cache_clear();

// ---- decode_stream.hip: the block-streaming decode (uniformly partitioned overlap-save, state in HBM)
struct DecodeStreamState {
    int C = 0;              // channels of the signal
    bool planes2 = false;   // the signal is decoded as 2C real planes [re x; im x] (complex signal, or complex basis with a rotation)
    int B = 0, P = 0;       // block size, partitions
    int S = 1;              // filter sets of the bank
    int L = 1;              // listeners (a listener group; a stream is the group of one)
    cplx* Wf = nullptr;     // [S][2][P][Cp][B + 1] partition spectra, Cp = planes2 ? 2C : C: one bank for all listeners
    cplx* ring = nullptr;   // [L][2][P][B + 1] pending output spectra
    void* hist = nullptr;   // [L][C][B] the previous block (cplx when planes2)
    int* pos = nullptr;     // [L][S > 1 ? 3 : 1] the ring slot of the next output block; with S > 1 followed by the set indices of
                            // the two previous blocks (-1: none yet)
};
bool decode_stream_block_ok(int64_t B);   // a power of two from 64 to 2048
// Wf from the real filter planes wpl [S][2][Cp][len] (device)
void launch_decode_stream_filters(const double* wpl, int Cp, int64_t len, int B, int P, int64_t S, cplx* Wf, hipStream_t st);
// the same kernel on Z sets of Cp real planes of len taps: Wf [Z][P][Cp][B + 1] from wpl [Z][Cp][len] (device)
void launch_partition_spectra(const double* wpl, int Cp, int64_t len, int B, int P, int64_t Z, cplx* Wf, hipStream_t st);
// one block: x + c ldx = channel c of the (rotated) block, B samples (cplx only when planes2); set: device, this block's set index
// (null: the previous block's; not looked at when S == 1); standing: the set the host KNOWS this block and the two before it to be
// on (their window then runs the plain kernel on that set), -1 when it does not know; out[i], out[ldo + i] = the two ears.
// With s.L > 1 listeners (standing = -1): listener l reads its block at x + l lsx (elements; 0: every listener reads x), its
// index at set + l lset, and writes its ears at out + l lso
void launch_decode_stream_block(const DecodeStreamState& s, const void* x, bool x_cplx, int64_t ldx, const int* set, int standing, double* out,
                                int64_t ldo, hipStream_t st, int64_t lsx = 0, int lset = 0, int64_t lso = 0);

// ---- field_stream.hip: source signals through room responses, a block at a time
struct FieldStreamState {
    int nsrc = 0;           // sources
    int planes = 0;         // real output planes: nch, or 2 nch for a complex response (plane 2c = re, 2c + 1 = im of channel c)
    bool out_c = false;     // the output is interleaved complex: a pair of planes is one column
    int B = 0, P = 0;       // block size, partitions
    cplx* Rf = nullptr;     // [nsrc][P][planes][B + 1] partition spectra of the responses
    cplx* ring = nullptr;   // [nsrc][P][B + 1] the spectra of the last P windows [previous block, block] of every source
    double* hist = nullptr; // [nsrc][B] the previous block
    int* pos = nullptr;     // the ring slot of the block pushed last
    // a bank of response sets; with S == 1 none of it exists and the layouts above hold
    int S = 1;              // response sets: Rf [S][nsrc][P][planes][B + 1], ring [nsrc][P][3][B + 1]
    int* tag = nullptr;     // [nsrc][P][3] the set of a ring entry, -1: empty
    int* sel = nullptr;     // [nsrc][2] the set indices of the two previous blocks (-1: none yet)
};
constexpr int kFieldStreamEntries = 3;   // ring entries per slot of a bank: a window meets at most three sets
constexpr int kFieldStreamMaxSources = 16;   // the limit of the C ABI; the bank's source kernel sizes its tables by it
// one block: src + q lds = source q's B samples; out + c ldo = channel c's B samples (doubles, or cplx when s.out_c).  Two launches.
// set (looked at only when s.S > 1): device, source q's set index of this block at set + q lset; null: every source keeps its set
void launch_field_stream_block(const FieldStreamState& s, const double* src, int64_t lds, const int* set, int64_t lset, void* out, int64_t ldo,
                               hipStream_t st);
constexpr int kFieldStreamLaunches = 2;

// ---- decode_api.hip: releases decode.hip's plans, rotate3.hip's tables, resample.hip's taps and the decode family's work buffers
void decode_family_cache_clear();

void filter_channels_by_order(const double* sig, int64_t n_in, int64_t n, int C, const double* ir /* [nOrd][len] */, int nOrd, int64_t len,
                              int64_t skip, double* out /* [C][n-skip] */, hipStream_t st);

// ---- emash.hip (getEMagLsFiltersEMAinSH)
void launch_ema_sh_e0(const void* Ech, int ldS, const void* Ypts, int C, int S, bool cb, void* E0, hipStream_t st);
void launch_rot_points(const double* azi, const double* zen, int D, int npts, double* azr, double* znr, hipStream_t st);
void launch_rot_from_points(const void* A, int64_t ldA, const void* Z, int ldP, int C, int npts, const double* zen, int D, bool cb, void* Rot,
                            hipStream_t st);
void launch_qt_rotate(void* QT, int64_t ldD, int nOrd, int C, int N, int D, const void* Rot, bool cb, hipStream_t st);
void launch_gram_from_g(const void* G, int64_t g_stride, int64_t ldD, int D, int C, int kb0, int nbins, int g0, double* Apk, int ldK,
                        hipStream_t st);

// ---- render.hip
void launch_radial_filter(const void* bn, int nOrd, int P, int type, double regul, double g, bool nyq_abs, bool zero_nan,
                          void* out_kn, void* out_cm, hipStream_t st);
void launch_diffuse_field(const void* bn, int nOrd, int n_lo, int P, double* df_hi, double* df_lo, hipStream_t st);
void launch_array_diffuse(const void* bn, int nOrd, const void* Y, bool y_cplx, int ldY, int S, int M, int nOut, int P,
                          double* df_lo, hipStream_t st);
void launch_eq_spectrum(const double* df_hi, const double* df_lo, const double* df_arr, int P, int mode, void* W, double* W_full,
                        hipStream_t st);
void launch_diffuse_constraint(void* W, const void* G, bool g_cplx, int64_t g_stride, int g0, const void* H, int D, int C, int64_t ldD,
                               int P, hipStream_t st);
void launch_smair(const void* E, bool e_cplx, int ldS, const void* bn, int nOrd, const void* rad, int nRad, int rows, int S, int P, void* out,
                  hipStream_t st);
void launch_sh_encode(const double* sig, int64_t n, int M, const void* Z, int ldZ, int nOut, bool out_cplx, void* out, hipStream_t st);

// ---- response.hip: rendered HRTFs of a design and their error metrics
int rh_num_metrics();            // values per (set, bin) of the reduced metrics: |dB| L, R, |ILD error|, cov_hat [4], cov_ref [4]
int rh_bins_padded(int P);       // bins per set of the product's left operand (whole workgroup tiles)
int rh_gemm_tiles(int64_t D);    // direction tiles of `partial` that launch_rh_gemm / launch_rh_atf write
int rh_atf_tiles(int64_t D);
// complex columns in [ncols][len] -> real planes out [ncols][2][len]; and W[i] = F[2 i] + i F[2 i + 1] for their spectra
void launch_rh_split(const void* in, int64_t ncols, int64_t len, double* out, hipStream_t st);
void launch_rh_join(const void* F, int64_t n, void* W, hipStream_t st);
// Tt [Kpad][ldR] (K = S, or 2 S with a complex basis; the rows K .. Kpad are the caller's to zero) from W [nsets][2][P][C]:
// T = (W A) b_n with A [C][ldA] (null: T = W) and bn [P][nOrd] (null: 1); ldR >= 4 nsets rh_bins_padded(P)
void launch_rh_modes(const void* W, int C, int P, int nsets, const void* A, bool a_cplx, int ldA, const void* bn, int nOrd, int S, bool y_cplx,
                     double* Tt, int64_t ldR, hipStream_t st);
// Tt [Kpad][ldR], K = nOrd C (2 nOrd C with complex order terms): row n C + c = W(k, c) b_n(k), against the UNconjugated right operand
// QT' [nOrd][C][ld] of the EMAinSH model; C <= 64, nOrd <= 86
void launch_rh_order_rows(const void* W, int C, int P, int nsets, const void* bn, int nOrd, bool q_cplx, double* Tt, int64_t ldR, hipStream_t st);
void launch_rh_interleave(const void* Y, int64_t ldi, int S, int64_t D, double* Yk, int64_t ldo, hipStream_t st);
struct RhOut {
    const void* H = nullptr;       // reference spectra [hset][2][P][D] complex (null: no metrics)
    int64_t hset_stride = 0;       // 2 P D, or 0 when one HRIR set serves every filter set
    const double* w = nullptr;     // [D] normalised direction weights
    void* Hhat = nullptr;          // [set][2][P][D] complex (null: not stored)
    double* partial = nullptr;     // [set][P][tiles][rh_num_metrics()]
};
// Yk [Kpad][ldY] with ldY a multiple of 64 >= D and zeros beyond D and K
void launch_rh_gemm(const double* Tt, int64_t ldR, const double* Yk, int64_t ldY, int K, int P, int64_t D, int nsets, const RhOut& o,
                    hipStream_t st);
// W [nsets][2][P][M], A [P][M][D] complex
void launch_rh_atf(const void* W, const void* A, int M, int P, int64_t D, int nsets, const RhOut& o, hipStream_t st);
void launch_rh_reduce(const double* partial, int64_t nrows, int ntile, double* out, hipStream_t st);

// ---- array_irs.hip: plane-wave components through the simulated array, as impulse responses
constexpr int AIR_LANE_SOURCE_MAX = 16;   // a source of at most this many components runs in the lane = source form
int air_bins_padded(int P);               // leading dimension of the bins (whole bin blocks of a wave)
// bn [N+1][Pld] from launch_modal_bn with out_scale = -1/(4 pi), zeros beyond P: times 2n+1, real in the last bin; rec [2 (N+1)]
void launch_air_modes(int N, int P, int64_t Pld, void* bn, double* rec, hipStream_t st);
void launch_air_units(int64_t n, const double* azi, const double* zen, double* u, hipStream_t st);   // u [3][n]
void launch_air_delays(int64_t n, const double* delay, double pre_delay, int nfft, int* dint, double* dfrac, hipStream_t st);
struct AirMain {
    const void* bn; const double* rec;
    const double *u, *v;                   // unit vectors [3][ncomp], [3][M]
    const int* dint; const double* dfrac;  // [ncomp]
    const double* gain;                    // [ncomp], null: ones
    const int64_t* ptr;                    // [Q+1]
    const int *list_long, *list_short;     // sources above / up to AIR_LANE_SOURCE_MAX components
    int n_long, n_short, N, M, P, nfft;
    int64_t Pld, ncomp;
    void* H;                               // [Q][M][Pld] complex
    // the spectral gain: nsurf = 0 and att null is the flat kernel
    int nsurf;                             // surfaces, <= 8
    const double* lnr; const unsigned* neg; const double* att;   // launch_air_spectra's tables [nsurf][Pld], [Pld], [Pld] or null
    const int* exp; const double* path;    // [ncomp][nsurf]; [ncomp] with att
    // point sources: dist null is the plane-wave kernels above
    const double* dist;                    // [ncomp] distances rho_j > mic_radius
    const void* bh; const double* ginv;    // launch_air_point_modes' tables [N+1][Pld] complex, [N+1]
    double mic_radius, kappa_step;         // r; kappa_k = k kappa_step
    // source directivity: dc null is the kernels above
    const double* Yd;                      // [Kd][ncomp] real SH of the emission directions in the sources' frames
    const void* dc;                        // [Q][Kd][Pld] complex coefficients, zeros beyond P
    int Kd;                                // (Nd + 1)^2 <= 81
};
void launch_air_main(const AirMain& m, hipStream_t st);
// azimuth and zenith of w_j = R_q^T e_j: emit [n][3] unit vectors in room axes, rot [nsrc][9] row-major or null (identity), the
// component's source from ptr [nsrc + 1]
void launch_air_emission_angles(int64_t n, int64_t nsrc, const int64_t* ptr, const double* emit, const double* rot, double* azi, double* zen,
                                hipStream_t st);
// the scaled mode table of the point-source kernels: bh [N+1][Pld] = b'_n(k) (2n-1)!! / (i kappa_k r)^n (zeros beyond P, the last bin
// the scaled form of Re b'_n), ginv[n] = 1 / (4 n^2 - 1); kr_step = kappa_step r
void launch_air_point_modes(int N, int P, int64_t Pld, double kr_step, void* bh, double* ginv, hipStream_t st);
// refl [W][P], att [P] or null (attp then unused) -> lnr [W][Pld], neg [Pld], attp [Pld]
void launch_air_spectra(int W, int P, int64_t Pld, const double* refl, const double* att, double* lnr, unsigned* neg, double* attp,
                        hipStream_t st);
// out [Q][C][nr], real or (enc_im given) interleaved complex; enc_re null: C = M raw microphones.  nfft <= 4096
void launch_air_irfft(const void* H, int64_t Pld, const double* enc_re, const double* enc_im, int C, int M, int64_t Q, int nfft,
                      const void* tw, int nr, void* out, hipStream_t st);
// X [Q][C][np][P], np = 2 with enc_im; and the first nr samples of y [rows][np][nfft] over nfft
void launch_air_encode(const void* H, int64_t Pld, const double* enc_re, const double* enc_im, int C, int M, int64_t Q, int P, void* X,
                       hipStream_t st);
void launch_air_pick(const double* y, int64_t rows, int np, int nfft, int nr, void* out, hipStream_t st);

// ---- shoebox.hip: image sources of a shoebox room as the component lists of array_irs.hip
constexpr int SBX_TILE = 256;              // candidates per workgroup: four waves, one ballot word each
struct ShoeboxArgs {
    double L[3], beta[6], pos[3];          // room, walls (x=0, x=Lx, y=0, y=Ly, z=0, z=Lz), array centre
    double fs, max_delay;
    int max_order;                         // < 0: no limit
    int B[3], W[3];                        // the search box |n_i| <= B_i, W_i = 2 B_i + 1
    int64_t ncand, tiles;                  // candidates and tiles of ONE source: 8 Wx Wy Wz, ceil(ncand / SBX_TILE)
};
// mask [nsrc tiles][SBX_TILE / 64], cnt [nsrc tiles]; base [nsrc tiles + 1], comp_ptr [nsrc + 1]; src [nsrc][3]
void launch_shoebox_count(const ShoeboxArgs& a, int64_t nsrc, const double* src, uint64_t* mask, int* cnt, hipStream_t st);
void launch_shoebox_scan(const ShoeboxArgs& a, int64_t nsrc, const int* cnt, int64_t* base, int64_t* comp_ptr, hipStream_t st);
void launch_shoebox_write(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                          double* zen, double* delay, double* gain, hipStream_t st);
// the same lists, and the distance dist [n] of every component beside them (section 14)
void launch_shoebox_write_dist(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                               double* zen, double* delay, double* gain, double* dist, hipStream_t st);
// the same with the six exponents exp [n][6] (x0, x1, y0, y1, z0, z1) and the distance path [n] of every component (section 13)
void launch_shoebox_write_images(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                                 double* zen, double* delay, double* gain, int* exp, double* path, hipStream_t st);
// any of the three forms above (exp and path given, path alone, neither) with the emission vectors emit [n][3] beside them (section 15)
void launch_shoebox_write_emit(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                               double* zen, double* delay, double* gain, int* exp, double* path, double* emit, hipStream_t st);

// ---- host_pools.hip: process-wide stream pool (streams are recycled, never destroyed: see StreamPool in host_internal.hpp)
hipStream_t pool_stream_take();
void pool_stream_give(hipStream_t st);
// ---- host_pools.hip: runs f, maps exceptions to the C status codes and records the message for emagls_last_error()
int guarded_call(const std::function<void()>& f);

}  // namespace emagls

// full definitions of the argument structs (kept in their kernel files' header section)
#include "args.hpp"
