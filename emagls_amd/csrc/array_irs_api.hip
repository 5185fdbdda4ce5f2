// C ABI of the array impulse responses (include/emagls.h, emagls_array_irs).  Host arrays in, host array out;
// every argument is checked before the device is touched, and every array operation runs in the kernels of array_irs.hip, modal.hip
// and fft.hip (the twiddles), with hipFFT's Z2D above 4096 points (the precedent of decode.hip above 2048 taps).  No CPU fallback.
#include <hipfft/hipfft.h>

#include <cmath>
#include <vector>

#include "../../include/emagls.h"
#include "kernels.hpp"
#include "device_mem.hpp"

using namespace emagls;

namespace {

constexpr double C_SOUND = 343.0;          // dependencies/getSMAIRMatrix.m:95
constexpr int AIR_SIM_ORDER_MAX = 85;
constexpr int64_t AIR_NFFT_MAX = 65536;
constexpr int AIR_NFFT_LDS_MAX = 4096;     // the LDS transforms of lds_fft.hpp; hipFFT above
constexpr size_t AIR_SCRATCH_MAX = (size_t)24 << 30;

void fft_check(hipfftResult r, const char* what) {
    if (r != HIPFFT_SUCCESS) throw Error(EMAGLS_ERR_HIP, std::string("hipFFT error ") + std::to_string((int)r) + " in " + what);
}

// device events around the main kernel of a call, read after the call's synchronisation (emagls_array_irs_kernel_time)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() { HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b)); }
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
};
thread_local double g_main_ms = -1.0;

}  // namespace

extern "C" int emagls_array_irs(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr,
                                const double* comp_azi, const double* comp_zen, const double* comp_delay, const double* comp_gain,
                                double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    return guarded_call([&] {
        // ---- arguments (nothing below this block fails on what the caller passed)
        if (!mic_azi || !mic_zen) throw Error(EMAGLS_ERR_ARG, "null pointer: microphone grid");
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (!out) throw Error(EMAGLS_ERR_ARG, "null pointer: out");
        if (nsrc < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nsrc");
        if (nmics < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nmics");
        if (nmics > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 microphones are not supported");
        if (nch < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nch");
        if (nch > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 channels are not supported");
        if (!enc && nch != nmics) throw Error(EMAGLS_ERR_ARG, "without an encoder nch must equal nmics (raw microphone responses)");
        if (!(fs > 0) || !(mic_radius > 0) || !std::isfinite(fs) || !std::isfinite(mic_radius)) throw Error(EMAGLS_ERR_ARG, "fs and micRadius must be positive");
        if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
        if (nr < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nr");
        if (nfft_in < 0) throw Error(EMAGLS_ERR_ARG, "nfft must be positive (0: the smallest power of two from 2*nr)");
        int64_t nfft64 = nfft_in;
        if (nfft64 == 0) {
            nfft64 = 8;
            while (nfft64 < 2 * nr && nfft64 <= AIR_NFFT_MAX) nfft64 *= 2;
        }
        if (nfft64 & (nfft64 - 1)) throw Error(EMAGLS_ERR_ARG, "nfft must be a power of two");
        if (nfft64 < 8) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft below 8 is not supported");
        if (nfft64 > AIR_NFFT_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft above 65536 is not supported");
        if (nr > nfft64) throw Error(EMAGLS_ERR_ARG, "nr exceeds nfft");
        if (!(pre_delay >= 0.0) || !std::isfinite(pre_delay)) throw Error(EMAGLS_ERR_ARG, "pre_delay must be non-negative and finite");
        if (comp_ptr[0] != 0) throw Error(EMAGLS_ERR_ARG, "comp_ptr must start at 0");
        for (int64_t q = 0; q < nsrc; ++q)
            if (comp_ptr[q + 1] < comp_ptr[q]) throw Error(EMAGLS_ERR_ARG, "comp_ptr must not decrease");
        const int64_t ncomp = comp_ptr[nsrc];
        if (ncomp > 0 && (!comp_azi || !comp_zen)) throw Error(EMAGLS_ERR_ARG, "null pointer: component directions");
        const int nfft = (int)nfft64, P = nfft / 2 + 1, M = (int)nmics, C = (int)nch;
        if (pre_delay > (double)(nfft - 1)) throw Error(EMAGLS_ERR_ARG, "pre_delay beyond nfft - 1 would wrap");
        for (int64_t j = 0; comp_delay && j < ncomp; ++j) {
            if (!(comp_delay[j] >= 0.0) || !std::isfinite(comp_delay[j])) throw Error(EMAGLS_ERR_ARG, "component delays must be non-negative and finite");
            if (comp_delay[j] + pre_delay > (double)(nfft - 1)) throw Error(EMAGLS_ERR_ARG, "a component's delay plus pre_delay beyond nfft - 1 would wrap");
        }
        for (int64_t j = 0; comp_gain && j < ncomp; ++j)
            if (!std::isfinite(comp_gain[j])) throw Error(EMAGLS_ERR_ARG, "component gains must be finite");
        const int N = std::max(order, (int)std::ceil(fs * kPi * mic_radius / C_SOUND));     // getSMAIRMatrix.m:95
        if (N > AIR_SIM_ORDER_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "simulation order above 85 is not supported");
        // ---- sizes
        const bool ec = enc && enc_is_complex, lds = nfft <= AIR_NFFT_LDS_MAX;
        const int np = ec ? 2 : 1;
        const int64_t Pld = air_bins_padded(P), rows = nsrc * C;
        const size_t out_bytes = esz(ec) * (size_t)rows * nr;
        {
            // (in long double: the counts of a refused call may overflow 64 bits)
            const long double need = (long double)nsrc * M * Pld * 16 + (long double)(N + 1) * Pld * 16 + (long double)ncomp * 52 +
                                     (long double)nsrc * 12 + (long double)out_bytes +
                                     (lds ? 0.0L : (enc ? (long double)rows * np * P * 16 : 0.0L) + (long double)rows * np * nfft * 8);
            if (need > (long double)AIR_SCRATCH_MAX)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "the call needs more than 24 GiB of device memory; split the sources over several calls");
        }
        // the two forms' source lists (array_irs.hip): by each source's own count
        std::vector<int> list_long, list_short;
        for (int64_t q = 0; q < nsrc; ++q) (comp_ptr[q + 1] - comp_ptr[q] > AIR_LANE_SOURCE_MAX ? list_long : list_short).push_back((int)q);
        std::vector<double> e_re, e_im;
        if (enc) {
            const double* e = (const double*)enc;
            e_re.resize((size_t)C * M);
            if (ec) e_im.resize((size_t)C * M);
            for (size_t i = 0; i < (size_t)C * M; ++i) {
                e_re[i] = ec ? e[2 * i] : e[i];
                if (ec) e_im[i] = e[2 * i + 1];
            }
        }

        // ---- device
        Scratch s;
        // 1. mode coefficients b'_n(k) = -b_n (2n+1) / (4 pi) as rows [N+1][Pld]
        cplx* bn = s.get<cplx>(sizeof(cplx) * (size_t)(N + 1) * Pld, true);
        double* rec = s.get<double>(sizeof(double) * 2 * (N + 1));
        const double kr_step = 2.0 * kPi * (fs / (double)nfft) / C_SOUND * mic_radius;
        launch_modal_bn(N, P, nullptr, kr_step, -1.0 / (4.0 * kPi), bn, 1, Pld, s.st);     // bnAll = -sphModalCoeffs(...)  (:107)
        launch_air_modes(N, P, Pld, bn, rec, s.st);
        // 2. components and microphones
        AirMain m{};
        double* v = s.get<double>(sizeof(double) * 3 * M);
        launch_air_units(M, s.put(mic_azi, (size_t)M), s.put(mic_zen, (size_t)M), v, s.st);
        if (ncomp > 0) {
            double* u = s.get<double>(sizeof(double) * 3 * (size_t)ncomp);
            int* dint = s.get<int>(sizeof(int) * (size_t)ncomp);
            double* dfrac = s.get<double>(sizeof(double) * (size_t)ncomp);
            launch_air_units(ncomp, s.put(comp_azi, (size_t)ncomp), s.put(comp_zen, (size_t)ncomp), u, s.st);
            launch_air_delays(ncomp, s.put_opt(comp_delay, (size_t)ncomp), pre_delay, nfft, dint, dfrac, s.st);
            m.u = u; m.dint = dint; m.dfrac = dfrac;
            m.gain = s.put_opt(comp_gain, (size_t)ncomp);
        }
        m.bn = bn; m.rec = rec; m.v = v;
        m.ptr = s.put(comp_ptr, (size_t)nsrc + 1);
        m.list_long = s.put_opt(list_long.data(), list_long.size());
        m.list_short = s.put_opt(list_short.data(), list_short.size());
        m.n_long = (int)list_long.size(); m.n_short = (int)list_short.size();
        m.N = N; m.M = M; m.P = P; m.nfft = nfft; m.Pld = Pld; m.ncomp = ncomp;
        cplx* H = s.get<cplx>(sizeof(cplx) * (size_t)nsrc * M * Pld);
        m.H = H;
        // 3. the main kernel
        EventPair ev;
        HIP_CHECK(hipEventRecord(ev.a, s.st));
        launch_air_main(m, s.st);
        HIP_CHECK(hipEventRecord(ev.b, s.st));
        // 4. encoder and inverse real transform
        const double* d_re = s.put_opt(e_re.data(), e_re.size());
        const double* d_im = s.put_opt(e_im.data(), e_im.size());
        void* d_out = s.get(out_bytes);
        FftPlan plan;
        if (lds) {
            cplx* tw = s.get<cplx>(sizeof(cplx) * (size_t)nfft);
            launch_twiddles(nfft, tw, s.st);
            launch_air_irfft(H, Pld, d_re, d_im, C, M, nsrc, nfft, tw, (int)nr, d_out, s.st);
        } else {
            cplx* X = H;
            int64_t ldx = Pld;
            if (enc) {
                X = s.get<cplx>(sizeof(cplx) * (size_t)rows * np * P);
                ldx = P;
                launch_air_encode(H, Pld, d_re, d_im, C, M, nsrc, P, X, s.st);
            }
            double* y = s.get<double>(sizeof(double) * (size_t)rows * np * nfft);
            int nn[1] = {nfft}, inembed[1] = {P}, onembed[1] = {nfft};
            fft_check(hipfftPlanMany(plan.fresh(), 1, nn, inembed, 1, (int)ldx, onembed, 1, nfft, HIPFFT_Z2D, (int)(rows * np)), "plan Z2D");
            fft_check(hipfftSetStream(plan, s.st), "set stream");
            fft_check(hipfftExecZ2D(plan, (hipfftDoubleComplex*)X, y), "exec Z2D");
            launch_air_pick(y, rows, np, nfft, (int)nr, d_out, s.st);
        }
        HIP_CHECK(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, s.st));
        s.sync();   // (the host vectors above live until their copies have run)
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
        g_main_ms = (double)ms;
    });
}

extern "C" int emagls_array_irs_kernel_time(double* ms) {
    return guarded_call([&] {
        if (!ms) throw Error(EMAGLS_ERR_ARG, "null pointer: ms");
        if (g_main_ms < 0.0) throw Error(EMAGLS_ERR_ARG, "no emagls_array_irs call has completed on this thread");
        *ms = g_main_ms;
    });
}
