// Debug entries of the transforms at both ends of a design (emagls_debug_twiddles, emagls_debug_filter_epilogue, emagls_debug_hrir_spectra,
// emagls_debug_real_spectra): the launchers of fft.hip -- launch_twiddles, launch_hrir_grpdelay, launch_hrir_fft, launch_real_fft_gather and
// launch_filter_epilogue, with their own choice of kernel for the shape -- on arrays the caller supplies, so that a test can hold the HRIR
// prologue, the ATF spectra and the filter epilogue against a transform of higher precision shape by shape.  No kernel is launched from
// here and no dispatch is repeated here: an entry validates, allocates, copies, calls the launchers, synchronises, copies back and frees.
// Every output is filled with the sentinel of debug_common.hpp on the device before the launch, so what the kernels leave alone shows.
#include <cmath>

#include "debug_common.hpp"
#include "kernels.hpp"

namespace emagls {

using debug::copy;
using debug::filled;
using debug::sentinel;

namespace {

constexpr size_t kMaxBytes = (size_t)1 << 30;
bool is_square(int c) {
    const int r = (int)std::lround(std::sqrt((double)c));
    return r * r == c;
}
void check_indices(const int64_t* idx, int64_t n, int64_t bound, const char* what) {
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= bound) throw Error(1, what);
}

}  // namespace

void twiddles_debug(int nfft, void* tw) {
    if (!tw) throw Error(1, "null pointer");
    if (nfft < 2 || nfft > 8192) throw Error(1, "debug twiddles: 2 <= nfft <= 8192");
    Scratch b;
    cplx* d_tw = filled<cplx>(b, (size_t)nfft, sentinel());
    launch_twiddles(nfft, d_tw, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(tw, d_tw, (size_t)nfft * sizeof(cplx), hipMemcpyDeviceToHost));
}

void filter_epilogue_debug(const void* W, int C, int nfft, int len, const double* grpd, int conj_mode, int dc_rule, int shift_mode, int out_cplx,
                           int n_ears, double fade_rel, void* outL, void* outR) {
    if (!W || !outL) throw Error(1, "null pointer");
    if (n_ears != 1 && n_ears != 2) throw Error(1, "debug filter epilogue: n_ears is 1 or 2");
    if (n_ears == 2 && (!outR || !grpd)) throw Error(1, "debug filter epilogue: two ears need outR and grpd");
    if (nfft < 4 || nfft > 4096 || (nfft & 1)) throw Error(1, "debug filter epilogue: nfft is even, 4 ... 4096");
    if (len < 2 || len > nfft || (len & 1)) throw Error(1, "debug filter epilogue: len is even, 2 ... nfft");
    if (C < 1 || C > 1024) throw Error(1, "debug filter epilogue: 1 <= C <= 1024");
    if (conj_mode < 0 || conj_mode > 2) throw Error(1, "debug filter epilogue: conj_mode is 0 (Hermitian), 1 (SH rule) or 2 (CH rule)");
    if (conj_mode == 1 && !is_square(C)) throw Error(1, "debug filter epilogue: the SH rule (conj_mode 1) needs C = (N + 1)^2");
    if (conj_mode == 2 && !(C & 1)) throw Error(1, "debug filter epilogue: the CH rule (conj_mode 2) needs C = 2 N + 1");
    if ((dc_rule | 1) != 1 || (shift_mode | 1) != 1 || (out_cplx | 1) != 1) throw Error(1, "debug filter epilogue: dc_rule, shift_mode and out_cplx are 0 or 1");
    if (!(fade_rel >= 0.0) || !(fade_rel <= 0.5)) throw Error(1, "debug filter epilogue: 0 <= fade_rel <= 0.5");
    if (grpd && (!std::isfinite(grpd[0]) || !std::isfinite(grpd[1]))) throw Error(1, "debug filter epilogue: grpd is finite");
    const int P = nfft / 2 + 1;
    const size_t nout = (size_t)C * len * (out_cplx ? 2 : 1);   // doubles per ear
    Scratch b;
    cplx* d_W = copy<cplx>(b, W, (size_t)n_ears * P * C);
    cplx* d_tw = b.get<cplx>(sizeof(cplx) * (size_t)nfft);
    double* d_g = grpd ? copy<double>(b, grpd, 2) : nullptr;
    double* d_L = filled<double>(b, nout, sentinel());
    double* d_R = n_ears == 2 ? filled<double>(b, nout, sentinel()) : nullptr;
    launch_twiddles(nfft, d_tw, nullptr);
    launch_filter_epilogue(d_W, C, nfft, len, d_tw, d_g, conj_mode, dc_rule, shift_mode, out_cplx, d_L, d_R, nullptr, n_ears, fade_rel);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(outL, d_L, nout * sizeof(double), hipMemcpyDeviceToHost));
    if (d_R) HIP_CHECK(hipMemcpy(outR, d_R, nout * sizeof(double), hipMemcpyDeviceToHost));
}

// grpd_in and the delay phases: the wave form of nfft = 1024 (hrir_fft_wave_kernel) multiplies the spectra of mode 0 with the table
// grpdelay_median_kernel leaves behind the two delays, and only that kernel writes it.  Delays the caller supplies are therefore taken
// where no form reads the table -- mode 1 at every nfft, mode 0 at every nfft but 1024 (the LDS and the direct form evaluate the
// phases themselves) -- and refused at mode 0, nfft 1024, whichever form the switches select.  The table is returned as the
// sentinel then.
void hrir_spectra_debug(const double* hL, const double* hR, int64_t L, int64_t D_src, int64_t D, const int64_t* didx, int nfft, int mode, int n_c, int kabs0,
                        const double* grpd_in, int64_t ldD, int ldT, double* grpd_out, void* phs, void* Hc, double* Habs, double* HcT) {
    if (!hL || !hR) throw Error(1, "null pointer");
    if (nfft < 4 || nfft > 2048 || (nfft & 1)) throw Error(1, "debug hrir spectra: nfft is even, 4 ... 2048");
    if (L < 1 || L > 4096 || D_src < 1 || D_src > 65536) throw Error(1, "debug hrir spectra: 1 <= L <= 4096 and 1 <= D_src <= 65536");
    if (mode != 0 && mode != 1) throw Error(1, "debug hrir spectra: mode is 0 (fractional delay) or 1 (integer shift)");
    const int P = nfft / 2 + 1;
    const bool spectra = Hc != nullptr || Habs != nullptr || HcT != nullptr;
    if (!spectra && (grpd_in || !grpd_out)) throw Error(1, "debug hrir spectra: without spectra the call returns the delays it computes (grpd_out, no grpd_in)");
    if (spectra) {
        if (!Hc || !Habs) throw Error(1, "debug hrir spectra: Hc and Habs come together");
        if (L > nfft) throw Error(1, "debug hrir spectra: the spectra take at most nfft taps");
        if (D < 1 || D > 65536 || (!didx && D > D_src)) throw Error(1, "debug hrir spectra: 1 <= D <= 65536, and D <= D_src without didx");
        if (ldD < D || ldD > 131072 || ldD % 8 != 0) throw Error(1, "debug hrir spectra: ldD is a multiple of 8, D <= ldD <= 131072");
        if (n_c < 0 || n_c > P || kabs0 < 0 || kabs0 > P) throw Error(1, "debug hrir spectra: 0 <= n_c <= P and 0 <= kabs0 <= P");
        if (HcT && (ldT < 4 * n_c || ldT > 8192 || (ldT & 1))) throw Error(1, "debug hrir spectra: ldT is even, 4 n_c <= ldT <= 8192");
        if (didx) check_indices(didx, D, D_src, "debug hrir spectra: didx holds rows of the input, 0 ... D_src-1");
    }
    if (grpd_in) {
        if (!(std::fabs(grpd_in[0]) <= 1048576.0) || !(std::fabs(grpd_in[1]) <= 1048576.0)) throw Error(1, "debug hrir spectra: |grpd_in| <= 2^20");
        if (mode == 0 && nfft == 1024) throw Error(1, "debug hrir spectra: grpd_in at mode 0 and nfft 1024 is not taken (the wave form reads the median kernel's table)");
    }
    const size_t ng = 2 + 4 * (size_t)P;
    const size_t n_hc = spectra ? (size_t)2 * n_c * ldD : 0, n_ha = spectra ? (size_t)2 * (P - kabs0) * ldD : 0, n_t = HcT ? (size_t)D * ldT : 0;
    if (2 * (size_t)D_src * L * sizeof(double) + n_hc * sizeof(cplx) + (n_ha + n_t) * sizeof(double) > kMaxBytes) throw Error(1, "debug hrir spectra: more than 1 GiB of device memory");
    Scratch b;
    const double* d_hL = copy<double>(b, hL, (size_t)D_src * L);
    const double* d_hR = copy<double>(b, hR, (size_t)D_src * L);
    cplx* d_tw = b.get<cplx>(sizeof(cplx) * (size_t)nfft);
    double* d_g = filled<double>(b, ng, sentinel());
    launch_twiddles(nfft, d_tw, nullptr);
    if (grpd_in) {
        HIP_CHECK(hipMemcpy(d_g, grpd_in, 2 * sizeof(double), hipMemcpyHostToDevice));
    } else {
        double* d_part = filled<double>(b, (size_t)hrir_dirsum_chunks(D_src) * 2 * L, sentinel());
        launch_hrir_grpdelay(d_hL, d_hR, L, D_src, nfft, d_tw, d_part, d_g, nullptr);
    }
    cplx* d_Hc = nullptr;
    double *d_Ha = nullptr, *d_T = nullptr;
    if (spectra) {
        const int64_t* d_idx = didx ? copy<int64_t>(b, didx, (size_t)D) : nullptr;
        d_Hc = filled<cplx>(b, n_hc, sentinel());
        d_Ha = filled<double>(b, n_ha, sentinel());
        if (HcT) d_T = filled<double>(b, n_t, sentinel());
        launch_hrir_fft(d_hL, d_hR, L, D, d_idx, nfft, d_tw, d_g, mode, n_c, kabs0, d_Hc, d_Ha, ldD, nullptr, d_T, ldT);
    }
    HIP_CHECK(hipDeviceSynchronize());
    if (grpd_out) HIP_CHECK(hipMemcpy(grpd_out, d_g, 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (phs) HIP_CHECK(hipMemcpy(phs, d_g + 2, 4 * (size_t)P * sizeof(double), hipMemcpyDeviceToHost));
    if (spectra) {
        HIP_CHECK(hipMemcpy(Hc, d_Hc, n_hc * sizeof(cplx), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(Habs, d_Ha, n_ha * sizeof(double), hipMemcpyDeviceToHost));
        if (HcT) HIP_CHECK(hipMemcpy(HcT, d_T, n_t * sizeof(double), hipMemcpyDeviceToHost));
    }
}

void real_spectra_debug(const double* x, int64_t L, int64_t ncols_src, int64_t ncols, const int64_t* colidx, int nfft, int64_t ldo, int64_t inner,
                        int64_t ld_inner, void* out) {
    if (!x || !out) throw Error(1, "null pointer");
    if (nfft < 4 || nfft > 4096 || (nfft & 1)) throw Error(1, "debug real spectra: nfft is even, 4 ... 4096");
    if (L < 1 || L > 8192) throw Error(1, "debug real spectra: 1 <= L <= 8192");
    if (ncols_src < 1 || ncols_src > 65536 || ncols < 1 || ncols > 65536 || (!colidx && ncols > ncols_src))
        throw Error(1, "debug real spectra: 1 <= ncols, ncols_src <= 65536, and ncols <= ncols_src without colidx");
    if (inner < 1 || ld_inner < inner || ld_inner > 131072) throw Error(1, "debug real spectra: 1 <= inner <= ld_inner <= 131072");
    if (ldo > 1048576 || ((ncols - 1) / inner) * ld_inner + (ncols - 1) % inner >= ldo) throw Error(1, "debug real spectra: ldo holds every column's place, at most 2^20");
    if (colidx) check_indices(colidx, ncols, ncols_src, "debug real spectra: colidx holds columns of the input, 0 ... ncols_src-1");
    const int P = nfft / 2 + 1;
    if ((size_t)ncols_src * L * sizeof(double) + (size_t)P * ldo * sizeof(cplx) > kMaxBytes) throw Error(1, "debug real spectra: more than 1 GiB of device memory");
    Scratch b;
    const double* d_x = copy<double>(b, x, (size_t)ncols_src * L);
    const int64_t* d_idx = colidx ? copy<int64_t>(b, colidx, (size_t)ncols) : nullptr;
    cplx* d_tw = b.get<cplx>(sizeof(cplx) * (size_t)nfft);
    cplx* d_out = filled<cplx>(b, (size_t)P * ldo, sentinel());
    launch_twiddles(nfft, d_tw, nullptr);
    launch_real_fft_gather(d_x, L, ncols, d_idx, nfft, d_tw, d_out, ldo, inner, ld_inner, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d_out, (size_t)P * ldo * sizeof(cplx), hipMemcpyDeviceToHost));
}

}  // namespace emagls
