// C ABI of the rendered HRTFs of a design (include/emagls.h, emagls_rendered_hrtfs).  Host arrays in, host
// arrays out; every argument is checked before the device is touched (rh_check), and every array operation runs in the kernels of
// response.hip, fft.hip (the spectra), sh_basis.hip, modal.hip and factor.hip (pinv(Y_lo)).  The array models -- encoder, EMAinSH
// operands, scalars -- are the designs' own: the one definition of array_model.hpp (kernels: emash.hip, dspace.hip, wide_array.hip).
// No CPU fallback.
#include <cmath>
#include <vector>

#include "../../include/emagls.h"
#include "array_model.hpp"

using namespace emagls;

namespace {

constexpr int RH_NFFT_MAX = 2048;          // the designs' own limit (lib/getEMagLsFilters.m:41)
constexpr int RH_SIM_ORDER_MAX = 85;
constexpr int64_t RH_DIRS_MAX = 65536;
constexpr size_t RH_SCRATCH_MAX = (size_t)24 << 30;
constexpr size_t RH_QT_LDS = (size_t)150 * 1024;   // launch_qt: four rows of conj(Y) per workgroup at the least

// what the checked arguments of a call come to: the model, the sizes that follow from it, and the host tables it uploads
struct RhCall {
    bool ema_ch, ema_sh, is_ema, is_sh, is_atf, is_array, raw, metrics, cb;
    int nfft, P, C, S, simOrder, nOut, M;
    int64_t D;
    std::vector<double> wn, equator, na;   // normalised direction weights; pi/2 (an EMA's microphones, the projected grid); ema_sh_channel_azimuths
    // sizes
    int NM, Pp, nOrd, Kre, K, Kpad, ntile;   // Kre: inner dimension of the product -- the simulation's SH channels, or (ema_sh) the order terms of every output channel
    int64_t ldR, ldY, ldA;                    // ldA: the ema_sh rotation fit's rotated points (array_model.hpp)
    size_t nW;
};

RhCall rh_check(int model, const void* wL, const void* wR, int w_is_complex, int64_t len, int64_t nchan, int64_t nsets, const double* dir_azi,
                const double* dir_zen, int64_t ndirs, double fs, int order, int basis, double mic_radius, const double* mic_azi,
                const double* mic_zen, int64_t nmics, const double* atf, int64_t atf_taps, int64_t nfft_in, const double* hL, const double* hR,
                int64_t nsamp, int64_t nhrir_sets, const double* weights, const void* Hhat, const double* mag_err_db, const double* ild_err_db,
                const double* cov_hat, const double* cov_ref) {
    RhCall c{};
    const bool ema_ch = c.ema_ch = model == EMAGLS_MODEL_EMA_CH, ema_sh = c.ema_sh = model == EMAGLS_MODEL_EMA_SH, is_ema = c.is_ema = ema_ch || ema_sh;
    if ((model < EMAGLS_MODEL_SH || model > EMAGLS_MODEL_ATF) && !is_ema) throw Error(EMAGLS_ERR_ARG, "unknown model");
    const bool is_sh = c.is_sh = model == EMAGLS_MODEL_SH, is_atf = c.is_atf = model == EMAGLS_MODEL_ATF, is_array = c.is_array = !is_sh && !is_atf;
    const bool raw = c.raw = model == EMAGLS_MODEL_EMAGLS2;
    if (!wL || !wR) throw Error(EMAGLS_ERR_ARG, "null pointer: decoding filters");
    if (!is_atf && (!dir_azi || !dir_zen)) throw Error(EMAGLS_ERR_ARG, "null pointer: evaluation directions");
    if (is_array && (!mic_azi || (!mic_zen && !is_ema))) throw Error(EMAGLS_ERR_ARG, "null pointer: microphone grid");
    if (is_atf && !atf) throw Error(EMAGLS_ERR_ARG, "null pointer: ATFs");
    const bool metrics = c.metrics = mag_err_db || ild_err_db || cov_hat || cov_ref;
    if (!Hhat && !metrics) throw Error(EMAGLS_ERR_ARG, "null pointer: no output is asked for");
    if (metrics && (!hL || !hR)) throw Error(EMAGLS_ERR_ARG, "null pointer: the metrics need reference HRIRs");
    if (len < 1 || nchan < 1 || nsets < 1 || ndirs < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
    if (nsets > 65535) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 65535 filter sets in one call are not supported");
    if (ndirs > RH_DIRS_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 65536 evaluation directions are not supported");
    const int64_t nfft64 = nfft_in > 0 ? nfft_in : std::min<int64_t>(RH_NFFT_MAX, 2 * len);
    if (nfft_in < 0) throw Error(EMAGLS_ERR_ARG, "nfft must be positive (0: min(2048, 2*len))");
    if (nfft64 % 2) throw Error(EMAGLS_ERR_ARG, "nfft must be even");
    if (len > nfft64) throw Error(EMAGLS_ERR_ARG, "len exceeds nfft");
    if (nfft64 < 8) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft below 8 is not supported");
    if (nfft64 > RH_NFFT_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft above 2048 is not supported in this build");
    const int nfft = c.nfft = (int)nfft64, P = c.P = nfft / 2 + 1;
    const bool cb = c.cb = basis == EMAGLS_BASIS_COMPLEX;
    if (!is_atf && basis != EMAGLS_BASIS_REAL && basis != EMAGLS_BASIS_COMPLEX) throw Error(EMAGLS_ERR_ARG, "shDefinition must be 'real' or 'complex'");
    int C = 0, S = 0, simOrder = 0, nOut = 0, M = 0;
    if (is_sh) {
        if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
        if (order > 15) throw Error(EMAGLS_ERR_UNSUPPORTED, "SH order above 15 is not supported for the sh model");
        C = S = (order + 1) * (order + 1);
    } else {
        if (nmics < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nmics");
        if (nmics > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 microphones are not supported");
        M = (int)nmics;
        C = M;
    }
    if (is_array) {
        if (!(fs > 0) || !(mic_radius > 0)) throw Error(EMAGLS_ERR_ARG, "fs and micRadius must be positive");
        int ord = 4;                                      // lib/getEMagLs2Filters.m:51-63 leaves params.order at its default
        if (is_ema) {
            // lib/getEMagLsFiltersEMAinCH.m:52-65, lib/getEMagLsFiltersEMAinSH.m:66-100: 2 order + 1 circular harmonics of the microphones
            if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
            if (ema_ch && order > 15) throw Error(EMAGLS_ERR_UNSUPPORTED, "the ema_ch model is limited to order 15 (31 circular harmonics)");
            if (ema_sh && order > 7) throw Error(EMAGLS_ERR_UNSUPPORTED, "the ema_sh model is limited to SH order 7");
            ord = order;
            nOut = 2 * order + 1;
            if (M < nOut) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer microphones than circular harmonics (2*order+1)");
            C = ema_ch ? nOut : (order + 1) * (order + 1);
        } else if (!raw) {
            if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
            if (order > 4)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "the emagls model is limited to SH order 4 (pinv(Y_lo) of emagls_get_smair_matrix); orders 5..7 are not supported");
            ord = order;
            nOut = (order + 1) * (order + 1);
            if (M < nOut) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer microphones than SH channels");
            C = nOut;
        }
        simOrder = smair_sim_order(ord, fs, mic_radius);
        if (simOrder > RH_SIM_ORDER_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "simulation order above 85 is not supported");
        S = (simOrder + 1) * (simOrder + 1);
        if (ema_sh && 4 * esz(cb) * (size_t)(S + 1) > RH_QT_LDS)
            throw Error(EMAGLS_ERR_UNSUPPORTED, cb ? "the ema_sh model is limited to simulation order 47 with a complex basis (the order terms' tile)"
                                                   : "the ema_sh model is limited to simulation order 68 (the order terms' tile)");
    }
    if (is_atf) {
        if (atf_taps < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: atf_taps");
        if (atf_taps > nfft) throw Error(EMAGLS_ERR_ARG, "atf_taps exceeds nfft");
    }
    if (nchan != C) throw Error(EMAGLS_ERR_ARG, "the filters' channel count does not match the model");
    if (hL || hR) {
        if (!hL || !hR) throw Error(EMAGLS_ERR_ARG, "null pointer: one of hL, hR");
        if (nsamp < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nsamp");
        if (nsamp > nfft) throw Error(EMAGLS_ERR_ARG, "nsamp exceeds nfft");
        if (nhrir_sets != 1 && nhrir_sets != nsets) throw Error(EMAGLS_ERR_ARG, "the number of HRIR sets must be 1 or nsets");
    }
    const int64_t D = c.D = ndirs;
    c.C = C; c.S = S; c.simOrder = simOrder; c.nOut = nOut; c.M = M;
    if (is_ema) c.equator.assign((size_t)std::max<int64_t>(M, ema_sh ? std::max<int64_t>(D, C) : 0), kPi / 2.0);
    if (ema_sh) c.na = ema_sh_channel_azimuths(C, cb);
    if (metrics) {
        c.wn.assign((size_t)D, 1.0 / (double)D);
        if (weights) {
            double sum = 0.0;
            for (int64_t d = 0; d < D; ++d) {
                if (!(weights[d] >= 0.0) || !std::isfinite(weights[d])) throw Error(EMAGLS_ERR_ARG, "direction weights must be non-negative and finite");
                sum += weights[d];
            }
            if (!(sum > 0.0) || !std::isfinite(sum)) throw Error(EMAGLS_ERR_ARG, "direction weights must not all be zero");
            for (int64_t d = 0; d < D; ++d) c.wn[(size_t)d] = weights[d] / sum;
        }
    }
    // ---- sizes
    c.NM = rh_num_metrics(); c.Pp = rh_bins_padded(P);
    c.nOrd = simOrder + 1; c.Kre = ema_sh ? c.nOrd * C : S;
    c.K = (cb && !is_atf) ? 2 * c.Kre : c.Kre; c.Kpad = (int)(ceil_div(c.K, 4) * 4);
    c.ldR = (int64_t)nsets * c.Pp * 4; c.ldY = ceil_div(D, 64) * 64;
    c.ntile = is_atf ? rh_atf_tiles(D) : rh_gemm_tiles(D);
    c.nW = (size_t)nsets * 2 * P * C;
    // ema_sh: the rotation fit (rotated points, their SH matrix, Rot), conj(Y) of the projected grid twice, complex order terms
    c.ldA = ceil_div((int64_t)(D + 1) * ema_sh_npts(C), 64) * 64;
    const int64_t ldSs = ceil_div((int64_t)S, 64) * 64;
    const size_t need_ema = !ema_sh ? 0 : esz(cb) * ((size_t)C * c.ldA + (size_t)D * C * C + (size_t)S * c.ldY + (size_t)D * ldSs) +
                                              (size_t)c.ldA * 16 + (cb ? (size_t)c.Kre * c.ldY * 16 : 0);
    const size_t need = c.nW * 16 * (w_is_complex ? 4 : 2) + (is_atf ? (size_t)P * M * D * 16 + (size_t)atf_taps * M * D * 8
                                                                      : (size_t)c.Kpad * (c.ldR + c.ldY) * 8 + (cb && !ema_sh ? (size_t)S * D * 16 : 0)) + need_ema +
                        (metrics ? (size_t)nhrir_sets * 2 * D * (nsamp * 8 + (size_t)P * 16) + (size_t)nsets * P * c.ntile * c.NM * 8 : 0) +
                        (Hhat ? (size_t)nsets * 2 * P * D * 16 : 0);
    if (need > RH_SCRATCH_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "the call needs more than 24 GiB of device memory; split the filter sets over several calls");
    return c;
}

}  // namespace

extern "C" int emagls_rendered_hrtfs(int model, const void* wL, const void* wR, int w_is_complex, int64_t len, int64_t nchan, int64_t nsets,
                                     const double* dir_azi, const double* dir_zen, int64_t ndirs, double fs, int order, int basis,
                                     double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, const double* atf,
                                     int64_t atf_taps, int64_t nfft_in, const double* hL, const double* hR, int64_t nsamp,
                                     int64_t nhrir_sets, const double* weights, void* Hhat, double* mag_err_db, double* ild_err_db,
                                     double* cov_hat, double* cov_ref) {
    return guarded_call([&] {
        // ---- arguments (nothing below this line fails on what the caller passed)
        const RhCall c = rh_check(model, wL, wR, w_is_complex, len, nchan, nsets, dir_azi, dir_zen, ndirs, fs, order, basis, mic_radius, mic_azi, mic_zen,
                                  nmics, atf, atf_taps, nfft_in, hL, hR, nsamp, nhrir_sets, weights, Hhat, mag_err_db, ild_err_db, cov_hat, cov_ref);
        const bool cb = c.cb, metrics = c.metrics;
        const int nfft = c.nfft, P = c.P, C = c.C, S = c.S, simOrder = c.simOrder, M = c.M, NM = c.NM, K = c.K, Kpad = c.Kpad;
        const int64_t D = c.D, ldR = c.ldR, ldY = c.ldY;
        const size_t nW = c.nW;

        // ---- device
        Scratch s;
        cplx* tw = s.get<cplx>(sizeof(cplx) * (size_t)nfft);
        launch_twiddles(nfft, tw, s.st);
        // 1. filter spectra W [set][2][P][C]: columns (set, ear, c[, re/im]) of one real array
        cplx* W = s.get<cplx>(sizeof(cplx) * nW);
        {
            const size_t esz_w = w_is_complex ? sizeof(cplx) : sizeof(double);
            const size_t per_ear = (size_t)C * len;
            char* taps = s.get<char>(esz_w * (size_t)nsets * 2 * per_ear);
            for (int64_t i = 0; i < nsets; ++i)
                for (int e = 0; e < 2; ++e)
                    HIP_CHECK(hipMemcpyAsync(taps + esz_w * ((size_t)i * 2 + e) * per_ear, (const char*)(e ? wR : wL) + esz_w * (size_t)i * per_ear,
                                             esz_w * per_ear, hipMemcpyHostToDevice, s.st));
            const int64_t ncols = (int64_t)nsets * 2 * C;
            if (!w_is_complex) {
                launch_real_fft_gather((const double*)taps, len, ncols, nullptr, nfft, tw, W, C, C, (int64_t)P * C, s.st);
            } else {
                double* planes = s.get<double>(sizeof(double) * (size_t)ncols * 2 * len);
                cplx* F = s.get<cplx>(sizeof(cplx) * nW * 2);
                launch_rh_split(taps, ncols, len, planes, s.st);
                launch_real_fft_gather(planes, len, 2 * ncols, nullptr, nfft, tw, F, 2 * C, 2 * C, (int64_t)P * 2 * C, s.st);
                launch_rh_join(F, (int64_t)nW, W, s.st);
            }
        }
        // reference spectra H [hset][2][P][D], weights, partial sums
        RhOut o{};
        double* d_red = nullptr;
        if (metrics) {
            const size_t per_ear = (size_t)D * nsamp;
            double* h = s.get<double>(sizeof(double) * (size_t)nhrir_sets * 2 * per_ear);
            for (int64_t i = 0; i < nhrir_sets; ++i)
                for (int e = 0; e < 2; ++e)
                    HIP_CHECK(hipMemcpyAsync(h + ((size_t)i * 2 + e) * per_ear, (e ? hR : hL) + (size_t)i * per_ear, sizeof(double) * per_ear,
                                             hipMemcpyHostToDevice, s.st));
            cplx* H = s.get<cplx>(sizeof(cplx) * (size_t)nhrir_sets * 2 * P * D);
            launch_real_fft_gather(h, nsamp, nhrir_sets * 2 * D, nullptr, nfft, tw, H, D, D, (int64_t)P * D, s.st);
            o.H = H;
            o.hset_stride = nhrir_sets > 1 ? (int64_t)2 * P * D : 0;
            o.w = s.put(c.wn.data(), (size_t)D);
            o.partial = s.get<double>(sizeof(double) * (size_t)nsets * P * c.ntile * NM);
            d_red = s.get<double>(sizeof(double) * (size_t)nsets * P * NM);
        }
        const size_t hhat_bytes = sizeof(cplx) * (size_t)nsets * 2 * P * D;
        if (Hhat) o.Hhat = s.get(hhat_bytes);

        if (c.is_atf) {
            // pwGrid_k(m, d) = fft(atfIrs, nfft)(k, m, d): A [P][M][D] through a column gather (atfIrs is [taps x M x D])
            const double* d_atf = s.put(atf, (size_t)atf_taps * M * D);
            std::vector<int64_t> colidx((size_t)M * D);
            for (int m = 0; m < M; ++m)
                for (int64_t d = 0; d < D; ++d) colidx[(size_t)m * D + d] = d * M + m;
            const int64_t* d_col = s.put(colidx.data(), colidx.size());
            cplx* A = s.get<cplx>(sizeof(cplx) * (size_t)P * M * D);
            launch_real_fft_gather(d_atf, atf_taps, (int64_t)M * D, d_col, nfft, tw, A, (int64_t)M * D, (int64_t)M * D, 0, s.st);
            launch_rh_atf(W, A, M, P, D, (int)nsets, o, s.st);
            s.sync();   // (colidx lives on the host until its copy has run)
        } else {
            // conj(Y(dirs)) as real rows Yk [Kpad][ldY]  (ema_sh: the rotated order terms QT' in their place, below)
            const int N = c.is_sh ? order : simOrder;
            const double* d_azi = s.put(dir_azi, (size_t)D);
            const double* d_zen = s.put(dir_zen, (size_t)D);
            double* tab = s.get<double>(sizeof(double) * sh_coeff_count(N));
            launch_sh_coeff(N, tab, s.st);
            double* Yk = s.get<double>(sizeof(double) * (size_t)Kpad * ldY, true);
            if (!c.ema_sh && !cb) {
                launch_sh_basis(N, D, d_azi, d_zen, tab, false, Yk, ldY, s.st);
            } else if (!c.ema_sh) {
                void* Yc = s.get(sizeof(cplx) * (size_t)S * D);
                launch_sh_basis(N, D, d_azi, d_zen, tab, true, Yc, D, s.st);
                launch_rh_interleave(Yc, D, S, D, Yk, ldY, s.st);
            }
            // 2. mode coefficients
            double* Tt = s.get<double>(sizeof(double) * (size_t)Kpad * ldR);
            if (Kpad > K) HIP_CHECK(hipMemsetAsync(Tt + (size_t)K * ldR, 0, sizeof(double) * (size_t)(Kpad - K) * ldR, s.st));
            if (c.is_sh) {
                launch_rh_modes(W, C, P, (int)nsets, nullptr, false, 0, nullptr, 0, S, cb, Tt, ldR, s.st);
            } else {
                // E = Y_mic for raw microphone signals, pinv(Y_lo) Y_mic, or (EMAs) pinv(getCH(order, micAzi)) Y_mic; bnAll (getSMAIRMatrix.m:107)
                const int ldM = round_up(M, 64), ldS = round_up(S, 64);
                const double* m_azi = s.put(mic_azi, (size_t)M);
                const double* m_zen = s.put(c.is_ema ? c.equator.data() : mic_zen, (size_t)M);
                void* Ycm = s.get(esz(cb) * (size_t)S * M);
                void* Yrm = s.get(esz(cb) * (size_t)ldM * ldS, true);
                launch_sh_basis(simOrder, M, m_azi, m_zen, tab, cb, Ycm, M, s.st);
                void* E = c.raw ? Yrm : s.get(esz(cb) * (size_t)c.nOut * ldS, true);
                array_encoder(c.raw ? Encoder::RAW : c.is_ema ? Encoder::CH_PINV : Encoder::SH_PINV, Ycm, M, S, ldS, cb, order, m_azi, Yrm,
                              c.raw ? PinvWs{} : pinv_scratch(s, c.nOut, ldM), E, s.st);
                cplx* bn = s.get<cplx>(sizeof(cplx) * (size_t)P * c.nOrd);
                launch_modal_bn(simOrder, P, nullptr, kr_bin_step(fs, P, mic_radius), -1.0, bn, c.nOrd, 1, s.st);
                if (!c.ema_sh) {
                    launch_rh_modes(W, C, P, (int)nsets, E, cb, ldS, bn, c.nOrd, S, cb, Tt, ldR, s.st);
                } else {
                    // E0 = J E (EMAinSH.m:77-82), the per-direction rotations (:85-100) and the rotated order terms QT' [nOrd][C][ldY]
                    const int ldP = round_up(ema_sh_npts(C), 64);
                    const double* zen_eq = s.put(c.equator.data(), (size_t)std::max<int64_t>(D, C));
                    double* tab_lo = s.get<double>(sizeof(double) * sh_coeff_count(order));
                    void* Ypts = s.get(esz(cb) * (size_t)C * C);
                    void* E0 = s.get(esz(cb) * (size_t)C * ldS, true);
                    ema_sh_e0(order, C, S, ldS, cb, s.put(c.na.data(), (size_t)C), zen_eq, tab_lo, Ypts, E, E0, s.st);
                    const EmaShRot r{s.get<double>(sizeof(double) * (size_t)c.ldA), s.get<double>(sizeof(double) * (size_t)c.ldA), s.get(esz(cb) * (size_t)C * c.ldA),
                                     pinv_scratch(s, C, ldP), s.get<double>(sizeof(double) * C), s.get<int>(sizeof(int) * 4), s.get(esz(cb) * (size_t)D * C * C)};
                    ema_sh_rotations(r, order, C, (int)D, cb, d_azi, d_zen, tab_lo, s.st);
                    void* Yh = s.get(esz(cb) * (size_t)S * ldY);
                    void* Yc = s.get(esz(cb) * (size_t)D * ldS);
                    void* QT = cb ? s.get(sizeof(cplx) * (size_t)c.Kre * ldY, true) : (void*)Yk;   // (real basis: Yk itself, zero beyond D and K)
                    ema_sh_order_terms(simOrder, order, (int)D, C, S, ldS, cb, d_azi, zen_eq, tab, Yh, ldY, Yc, D, E0, r.Rot, QT, s.st);
                    if (cb) launch_rh_interleave(QT, ldY, c.Kre, D, Yk, ldY, s.st);
                    launch_rh_order_rows(W, C, P, (int)nsets, bn, c.nOrd, cb, Tt, ldR, s.st);
                }
            }
            // 3. the product and its epilogue
            launch_rh_gemm(Tt, ldR, Yk, ldY, Kpad, P, D, (int)nsets, o, s.st);
        }
        // 5. direction tiles in tile order
        std::vector<double> red;
        if (metrics) {
            launch_rh_reduce(o.partial, (int64_t)nsets * P, c.ntile, d_red, s.st);
            red.resize((size_t)nsets * P * NM);
            HIP_CHECK(hipMemcpyAsync(red.data(), d_red, sizeof(double) * red.size(), hipMemcpyDeviceToHost, s.st));
        }
        if (Hhat) HIP_CHECK(hipMemcpyAsync(Hhat, o.Hhat, hhat_bytes, hipMemcpyDeviceToHost, s.st));
        s.sync();
        for (size_t r = 0; metrics && r < (size_t)nsets * P; ++r) {
            const double* v = red.data() + r * NM;
            if (mag_err_db) { mag_err_db[2 * r] = v[0]; mag_err_db[2 * r + 1] = v[1]; }
            if (ild_err_db) ild_err_db[r] = v[2];
            for (int j = 0; j < 4; ++j) {
                if (cov_hat) cov_hat[4 * r + j] = v[3 + j];
                if (cov_ref) cov_ref[4 * r + j] = v[7 + j];
            }
        }
    });
}
