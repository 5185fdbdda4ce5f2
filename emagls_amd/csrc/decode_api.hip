// C ABI of binauralDecode, the SH rotations and the resampler (include/emagls.h: emagls_binaural_decode*, emagls_rotate_yaw,
// emagls_rotate_sh, emagls_sh_rotation_matrix, emagls_resample*, emagls_decode_stream_*, emagls_decode_group_*): the argument check, host staging, the work buffers and the
// choice of kernels, once for the whole family.  The kernels are decode.hip's, decode_stream.hip's, rotate.hip's, rotate3.hip's and
// resample.hip's.  The stream and the group stand on the host skeleton they share with the field stream (BlockStreamObject,
// block_stream.hpp); one-call scratch and the work buffers are device_mem.hpp's owners.
// No CPU fallback.
#include <algorithm>
#include <initializer_list>
#include <memory>
#include <numeric>
#include <vector>

#include "../../include/emagls.h"
#include "block_stream.hpp"

using namespace emagls;

namespace {

// The head rotation of a call: each angle absent (0 values), one value or one value per input sample.  Yaw-only means
// n_pitch == n_roll == 0: such a call takes rotate.hip's kernel (SH or CH), any other rotate3.hip's (SH, orders 0 to 15).
struct Angles {
    const double* yaw = nullptr;
    int64_t n_yaw = 0;
    const double* pitch = nullptr;
    int64_t n_pitch = 0;
    const double* roll = nullptr;
    int64_t n_roll = 0;
    bool yaw_only() const { return n_pitch == 0 && n_roll == 0; }
    bool any() const { return n_yaw != 0 || !yaw_only(); }
    bool fixed() const { return n_yaw <= 1 && n_pitch <= 1 && n_roll <= 1; }
};

Angles put_angles(Scratch& s, const Angles& a) {   // device copies of the angle arrays that are there
    return {s.put_opt(a.yaw, (size_t)a.n_yaw), a.n_yaw, s.put_opt(a.pitch, (size_t)a.n_pitch), a.n_pitch, s.put_opt(a.roll, (size_t)a.n_roll), a.n_roll};
}

// work buffers of the device-resident body, grown on demand and kept (released by decode_family_cache_clear); one decode at a
// time per process, like decode.hip's plans.  Never destroyed (device_mem.hpp)
struct Work {
    enum { RS_SIG, RS_WL, RS_WR, ROT_SIG, ROT_WL, ROT_WR, SIG2, W2L, W2R, TMP, IR, YIM, NBUF };
    std::mutex mu;
    int device = -1;
    DevMem buf[NBUF];
    static Work& instance() { static Work* p = new Work; return *p; }
    void release() {
        for (DevMem& m : buf) m.reset();
        device = -1;
    }
    template <typename T = void> T* get(int i, size_t bytes) {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        if (dev != device) { release(); device = dev; }
        buf[i].grow(bytes);
        return buf[i].get<T>();
    }
};
Work& g_work = Work::instance();

// A sample-rate conversion of dependencies/binauralDecode.m:12-23, MATLAB's resample(x, p, q) with p / q reduced by their gcd
struct Ratio {
    int64_t p = 1, q = 1;
    bool identity() const { return p == q; }
    int64_t length(int64_t n) const { return resample_length(n, p, q); }
};

Ratio reduce_ratio(int64_t p, int64_t q) {
    if (p < 1 || q < 1) throw Error(EMAGLS_ERR_ARG, "resample needs positive integer rates p and q");
    const int64_t g = std::gcd(p, q);
    const Ratio r{p / g, q / g};
    if (std::max(r.p, r.q) > kResampleMaxRatio)
        throw Error(EMAGLS_ERR_UNSUPPORTED, "resample supports max(p, q) <= 65536 after reduction by their gcd");
    return r;
}

// to_fs / from_fs: sample rates given as doubles, which must be positive and integer-valued (MATLAB's resample requires it)
Ratio rate_ratio(double to_fs, double from_fs, const char* what) {
    auto integral = [](double f) { return std::isfinite(f) && f >= 1.0 && f <= 9.0e15 && std::floor(f) == f; };
    if (!integral(to_fs) || !integral(from_fs))
        throw Error(EMAGLS_ERR_ARG, std::string("resampling the ") + what + " needs positive integer-valued sample rates");
    return reduce_ratio((int64_t)to_fs, (int64_t)from_fs);
}

bool all_zero(const double* a, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (a[i] != 0.0) return false;
    return true;
}

// Host entry points drop pitch and roll arrays that hold only zeros, so such a call is yaw-only: bit for bit the yaw path.
// (Device arrays are not read: there only absent pitch and roll make a call yaw-only.)
Angles host_angles(Angles a) {
    auto zero = [](const double* p, int64_t n) { return n == 0 || (p && n > 0 && all_zero(p, n)); };
    if (zero(a.pitch, a.n_pitch) && zero(a.roll, a.n_roll)) { a.pitch = a.roll = nullptr; a.n_pitch = a.n_roll = 0; }
    return a;
}

void check_basis(int basis) {
    if (basis != EMAGLS_BASIS_REAL && basis != EMAGLS_BASIS_COMPLEX) throw Error(EMAGLS_ERR_ARG, "shDefinition must be 'real' or 'complex'");
}

void check_order3(int N) {
    if (N > rotate3_max_order()) throw Error(EMAGLS_ERR_UNSUPPORTED, "the three-axis rotation supports SH orders 0 to 15");
}

void check_angles(int64_t nsamp, const double* p, int64_t n, const char* name) {
    if (n < 0 || (n > 1 && n != nsamp)) throw Error(EMAGLS_ERR_ARG, std::string(name) + " needs no value, one value or one value per input sample");
    if (n > 0 && !p) throw Error(EMAGLS_ERR_ARG, "null pointer");
}

// The argument check of every entry point, in the order in which they have always reported (the messages and the statuses are
// part of the ABI).  decode: a decode with filters of length len and a signal of n_signal samples, rather than a rotation alone,
// which needs an angle.
void check_args(bool decode, std::initializer_list<const void*> ptrs, int64_t nsamp, int64_t nch, int64_t len, int64_t n_signal,
                int layout, int basis, const Angles& a) {
    static const char* const count = "the rotation needs one angle or one angle per input sample";
    for (const void* p : ptrs)
        if (!p) throw Error(EMAGLS_ERR_ARG, "null pointer");
    if (nsamp < 0 || nch < 1 || (decode && (len < 1 || n_signal < 0 || (a.yaw_only() && a.n_yaw < 0))))
        throw Error(EMAGLS_ERR_ARG, "invalid shape");
    if (a.yaw_only()) {
        if (!decode && a.n_yaw < 1) throw Error(EMAGLS_ERR_ARG, count);
        if (a.n_yaw == 0) return;
        if (!a.yaw) throw Error(EMAGLS_ERR_ARG, "null pointer");
        check_basis(basis);
        if (layout != EMAGLS_LAYOUT_SH && layout != EMAGLS_LAYOUT_CH) throw Error(EMAGLS_ERR_ARG, "layout must be EMAGLS_LAYOUT_SH or EMAGLS_LAYOUT_CH");
        if (a.n_yaw != 1 && a.n_yaw != nsamp) throw Error(EMAGLS_ERR_ARG, count);
        if (rotate_order(layout, nch) < 0)
            throw Error(EMAGLS_ERR_ARG, layout == EMAGLS_LAYOUT_SH ? "the rotation needs (N+1)^2 SH channels" : "the rotation needs 2N+1 CH channels");
        return;
    }
    check_angles(nsamp, a.yaw, a.n_yaw, "yaw");
    check_angles(nsamp, a.pitch, a.n_pitch, "pitch");
    check_angles(nsamp, a.roll, a.n_roll, "roll");
    if (layout == EMAGLS_LAYOUT_CH) throw Error(EMAGLS_ERR_ARG, "a CH signal can only be turned about z: pitch and roll must be 0");
    if (layout != EMAGLS_LAYOUT_SH) throw Error(EMAGLS_ERR_ARG, "layout must be EMAGLS_LAYOUT_SH or EMAGLS_LAYOUT_CH");
    check_basis(basis);
    const int N = rotate_order(EMAGLS_LAYOUT_SH, nch);
    if (N < 0) throw Error(EMAGLS_ERR_ARG, "the three-axis rotation needs (N+1)^2 SH channels in ACN order");
    check_order3(N);
}

// in [C][n] -> out [C][n] (complex when in_c or cb) by rotate.hip's kernel for a yaw-only rotation, rotate3.hip's otherwise;
// transpose: the filter-side form of a fixed rotation (w Rot instead of x Rot^T)
// ld_in / ld_out: elements between the channels of in / out (0: n)
// L listeners of the one signal (a listener group): la[3] the listener strides of the three angle arrays, lo of out
void launch_rotation(const Angles& a, const void* in, bool in_c, int64_t n, int nch, int layout, bool cb, bool transpose, void* out,
                     hipStream_t st, int64_t ld_in = 0, int64_t ld_out = 0, int L = 1, const int64_t* la = nullptr, int64_t lo = 0) {
    if (a.yaw_only())
        launch_rotate_yaw(in, in_c, n, nch, layout, cb, a.yaw, a.n_yaw > 1, transpose, out, st, ld_in, ld_out, L, la ? la[0] : 0, lo);
    else
        launch_rotate3(in, in_c, n, nch, cb, a.n_yaw ? a.yaw : nullptr, a.n_yaw > 1, a.n_pitch ? a.pitch : nullptr, a.n_pitch > 1,
                       a.n_roll ? a.roll : nullptr, a.n_roll > 1, transpose, out, st, ld_in, ld_out, L, la, lo);
}

// the same on the microphone block of an encoded stream: the encoder runs inside the rotation launch
void launch_rotation_encoded(const Angles& a, const EncodeBlock& e, int64_t n, int nch, int layout, bool cb, void* out, hipStream_t st,
                             int64_t ld_out, int L = 1, const int64_t* la = nullptr, int64_t lo = 0) {
    if (a.yaw_only())
        launch_rotate_yaw_encoded(e, n, nch, layout, cb, a.yaw, a.n_yaw > 1, out, st, ld_out, L, la ? la[0] : 0, lo);
    else
        launch_rotate3_encoded(e, n, nch, cb, a.n_yaw ? a.yaw : nullptr, a.n_yaw > 1, a.n_pitch ? a.pitch : nullptr, a.n_pitch > 1,
                               a.n_roll ? a.roll : nullptr, a.n_roll > 1, out, st, ld_out, L, la, lo);
}

// The rotation before the decode.  A fixed one (every count <= 1) turns the decoding filters, sum_i w_i * (x Rot^T)_i =
// sum_j (w Rot)_j * x_j; a trajectory is a pass over the signal into ROT_SIG.  The operands it replaces
// are complex from here on in the complex basis.  (g_work.mu held)
void rotate_step(const Angles& a, int layout, bool cb, int64_t nsamp, int nch, int64_t len, const void*& d_in, bool& in_c,
                 const void*& d_wL, const void*& d_wR, bool& w_c, hipStream_t st) {
    if (a.fixed()) {
        const bool wc2 = w_c || cb;
        void* rL = g_work.get(Work::ROT_WL, esz(wc2) * (size_t)len * nch);
        void* rR = g_work.get(Work::ROT_WR, esz(wc2) * (size_t)len * nch);
        launch_rotation(a, d_wL, w_c, len, nch, layout, cb, true, rL, st);
        launch_rotation(a, d_wR, w_c, len, nch, layout, cb, true, rR, st);
        d_wL = rL; d_wR = rR; w_c = wc2;
    } else {
        const bool ic2 = in_c || cb;
        void* x = g_work.get(Work::ROT_SIG, esz(ic2) * (size_t)nsamp * nch);
        launch_rotation(a, d_in, in_c, nsamp, nch, layout, cb, false, x, st);
        d_in = x; in_c = ic2;
    }
}

// The resampling of dependencies/binauralDecode.m:12-23 before everything else: the decoding filters by rf into RS_WL / RS_WR,
// the source signal by rs into RS_SIG; len and nsig become the resampled lengths.  (g_work.mu held)
void resample_step(const Ratio& rf, const Ratio& rs, int nch, const void*& d_wL, const void*& d_wR, bool w_c, int64_t& len,
                   const double*& d_sig, int64_t& nsig, hipStream_t st) {
    if (!rf.identity()) {
        const int64_t len2 = rf.length(len);
        void* rL = g_work.get(Work::RS_WL, esz(w_c) * (size_t)len2 * nch);
        void* rR = g_work.get(Work::RS_WR, esz(w_c) * (size_t)len2 * nch);
        launch_resample(d_wL, w_c, len, nch, rf.p, rf.q, rL, st);
        launch_resample(d_wR, w_c, len, nch, rf.p, rf.q, rR, st);
        d_wL = rL; d_wR = rR; len = len2;
    }
    if (nsig > 0 && !rs.identity()) {
        const int64_t n2 = rs.length(nsig);
        double* s2 = g_work.get<double>(Work::RS_SIG, sizeof(double) * (size_t)n2);
        launch_resample(d_sig, false, nsig, 1, rs.p, rs.q, s2, st);
        d_sig = s2; nsig = n2;
    }
}

// The device-resident body of every decode entry (nsamp > 0): the resampling, the rotation, the real or complex decode, and the
// source-signal convolution of dependencies/binauralDecode.m:44-48 with its imaginary-part sums.  d_out [nout][2], nout = the
// resampled nsig if there is a signal, else nsamp, without the delay cut; `cut` only moves the start of the imaginary-part sums.
// Returns with st synchronised (every binaural_decode_real call synchronises it).
void decode_body(const void* d_in, bool in_c, int64_t nsamp, int nch, const void* d_wL, const void* d_wR, bool w_c, int64_t len, int layout,
                 bool cb, const Angles& a, const double* d_sig, int64_t nsig, int64_t cut, double* d_out, double* imag_abs, hipStream_t st,
                 const Ratio& rf = {}, const Ratio& rs = {}) {
    std::lock_guard<std::mutex> lk(g_work.mu);
    resample_step(rf, rs, nch, d_wL, d_wR, w_c, len, d_sig, nsig, st);
    if (a.any()) rotate_step(a, layout, cb, nsamp, nch, len, d_in, in_c, d_wL, d_wR, w_c, st);
    const bool any_c = in_c || w_c, want_imag = imag_abs && any_c;
    double* stage1 = nsig > 0 ? g_work.get<double>(Work::IR, sizeof(double) * 2 * (size_t)nsamp) : d_out;
    double* tmp = want_imag ? g_work.get<double>(Work::TMP, sizeof(double) * (2 * (size_t)nsamp + 2)) : nullptr;
    double im1[2] = {0.0, 0.0};
    if (!any_c) {
        binaural_decode_real((const double*)d_in, nsamp, nch, (const double*)d_wL, (const double*)d_wR, len, stage1, st);
    } else {
        double* sig2 = g_work.get<double>(Work::SIG2, sizeof(double) * 2 * (size_t)nsamp * nch);
        double* w2L = g_work.get<double>(Work::W2L, sizeof(double) * 2 * (size_t)len * nch);
        double* w2R = g_work.get<double>(Work::W2R, sizeof(double) * 2 * (size_t)len * nch);
        // (the reference sums the discarded imaginary part after binauralOut(del:end,:), binauralDecode.m:53-62)
        binaural_decode_complex(d_in, in_c, nsamp, nch, d_wL, d_wR, w_c, len, sig2, w2L, w2R, stage1,
                                want_imag ? (nsig > 0 ? im1 : imag_abs) : nullptr, tmp, st, nsig > 0 ? 0 : std::min(cut, nsamp));
    }
    if (nsig > 0) {   // the two ears of the first stage are the filters of a one-channel overlap-save over the signal
        binaural_decode_real(d_sig, nsig, 1, stage1, stage1 + nsamp, nsamp, d_out, st);
        if (want_imag) {   // real(conv(e, s)) = conv(real(e), s); the imaginary part only feeds the two warning sums
            double* yim = g_work.get<double>(Work::YIM, sizeof(double) * (2 * (size_t)nsig + 2));
            binaural_decode_real(d_sig, nsig, 1, tmp, tmp + nsamp, nsamp, yim, st);
            launch_abs_sum_cols(yim, nsig, std::min(cut, nsig), 2, yim + 2 * nsig, st);
            HIP_CHECK(hipMemcpyAsync(imag_abs, yim + 2 * nsig, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
    }
}

// The two rate conversions of a decode: fs = {in_fs, filter_fs, signal_fs}, or null for none.  signal_fs is looked at only when
// there is a signal (binauralDecode.m:12-17).
void decode_ratios(const double* fs, int64_t nsig, Ratio& rf, Ratio& rs) {
    if (!fs) return;
    rf = rate_ratio(fs[0], fs[1], "decoding filters");
    if (nsig > 0) rs = rate_ratio(fs[0], fs[2], "signal");
}

// The host decode entries: staging, the body, and the compensate_delay cut on the way back (binauralOut(del:end,:), del = len/2 of
// the resampled filters, dependencies/binauralDecode.m:53-57): out [nout - (len/2 - 1)][2].
int host_decode(const void* in, bool ic, int64_t nsamp, int64_t nch, const void* wL, const void* wR, bool wc, int64_t len, int compensate_delay,
                int layout, int basis, const Angles& a, const double* signal, int64_t n_signal, double* out, double* imag_abs_sum,
                const double* fs = nullptr) {
    return guarded_call([&] {
        const int64_t nsig = signal ? n_signal : 0;
        // (without rotation and signal, the checks of emagls_binaural_decode_complex: they never looked at n_signal)
        check_args(true, {in, wL, wR, out}, nsamp, nch, len, a.any() || nsig ? n_signal : 0, layout, basis, a);
        Ratio rf, rs;
        decode_ratios(fs, nsig, rf, rs);
        if (imag_abs_sum) imag_abs_sum[0] = imag_abs_sum[1] = 0.0;
        const int64_t len2 = rf.length(len);
        const int64_t nout = nsig > 0 ? rs.length(nsig) : nsamp;
        const int64_t cut = (compensate_delay && len2 / 2 > 0) ? len2 / 2 - 1 : 0;
        const int64_t rows = nout - cut;
        if (nsamp == 0) {   // the rendered impulse response is empty: so is its convolution with the signal
            if (rows > 0) std::fill(out, out + 2 * rows, 0.0);
            return;
        }
        Scratch s;
        const void* d_in = s.put((const char*)in, esz(ic) * (size_t)nsamp * nch);
        const void* d_wL = s.put((const char*)wL, esz(wc) * (size_t)len * nch);
        const void* d_wR = s.put((const char*)wR, esz(wc) * (size_t)len * nch);
        double* d_out = s.get<double>(sizeof(double) * 2 * nout);
        decode_body(d_in, ic, nsamp, (int)nch, d_wL, d_wR, wc, len, layout, basis == EMAGLS_BASIS_COMPLEX, put_angles(s, a), s.put_opt(signal, (size_t)nsig),
                    nsig, cut, d_out, imag_abs_sum, s.st, rf, rs);
        if (rows > 0) {
            HIP_CHECK(hipMemcpyAsync(out, d_out + cut, sizeof(double) * rows, hipMemcpyDefault, s.st));
            HIP_CHECK(hipMemcpyAsync(out + rows, d_out + nout + cut, sizeof(double) * rows, hipMemcpyDefault, s.st));
            HIP_CHECK(hipStreamSynchronize(s.st));
        }
    });
}

// The two host rotation entries: staging, the rotation, the result back
int host_rotate(const void* in, bool ic, int64_t nsamp, int64_t nch, int layout, int basis, const Angles& a, void* out) {
    return guarded_call([&] {
        check_args(false, {in, out}, nsamp, nch, 0, 0, layout, basis, a);
        if (nsamp == 0) return;
        const bool cb = basis == EMAGLS_BASIS_COMPLEX;
        const size_t bout = esz(ic || cb) * (size_t)nsamp * nch;
        Scratch s;
        const void* d_in = s.put((const char*)in, esz(ic) * (size_t)nsamp * nch);
        void* d_out = s.get(bout);
        launch_rotation(put_angles(s, a), d_in, ic, nsamp, (int)nch, layout, cb, false, d_out, s.st);
        HIP_CHECK(hipMemcpyAsync(out, d_out, bout, hipMemcpyDefault, s.st));
        HIP_CHECK(hipStreamSynchronize(s.st));
    });
}

}  // namespace

void emagls::decode_family_cache_clear() {
    decode_cache_clear();
    rotate3_cache_clear();
    resample_cache_clear();
    std::lock_guard<std::mutex> lk(g_work.mu);
    g_work.release();
}

extern "C" {

int emagls_binaural_decode(const double* in, int64_t nsamp, int64_t nch, const double* wL, const double* wR, int64_t len,
                           int compensate_delay, double* out) {
    return host_decode(in, false, nsamp, nch, wL, wR, false, len, compensate_delay, EMAGLS_LAYOUT_SH, EMAGLS_BASIS_REAL, {}, nullptr, 0,
                       out, nullptr);
}

int emagls_binaural_decode_complex(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                   int filters_are_complex, int64_t len, int compensate_delay, double* out, double* imag_abs_sum) {
    return host_decode(in, in_is_complex != 0, nsamp, nch, wL, wR, filters_are_complex != 0, len, compensate_delay, EMAGLS_LAYOUT_SH,
                       EMAGLS_BASIS_REAL, {}, nullptr, 0, out, imag_abs_sum);
}

int emagls_binaural_decode_render_ypr(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                      int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                      int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll,
                                      const double* signal, int64_t n_signal, double* out, double* imag_abs_sum) {
    const Angles a = host_angles({yaw, n_yaw, pitch, n_pitch, roll, n_roll});
    // (without rotation and signal, with nothing complex, this is emagls_binaural_decode: imag_abs_sum is left alone)
    const bool plain_real = !a.any() && !(signal && n_signal) && !in_is_complex && !filters_are_complex;
    return host_decode(in, in_is_complex != 0, nsamp, nch, wL, wR, filters_are_complex != 0, len, compensate_delay, layout, basis, a, signal,
                       n_signal, out, plain_real ? nullptr : imag_abs_sum);
}

int emagls_binaural_decode_render(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                  int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                  int64_t n_yaw, const double* signal, int64_t n_signal, double* out, double* imag_abs_sum) {
    return emagls_binaural_decode_render_ypr(in, in_is_complex, nsamp, nch, wL, wR, filters_are_complex, len, compensate_delay, layout, basis,
                                             yaw, n_yaw, nullptr, 0, nullptr, 0, signal, n_signal, out, imag_abs_sum);
}

int emagls_binaural_decode_render_fs(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                     int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                     int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll,
                                     const double* signal, int64_t n_signal, double in_fs, double filter_fs, double signal_fs, double* out,
                                     double* imag_abs_sum) {
    const Angles a = host_angles({yaw, n_yaw, pitch, n_pitch, roll, n_roll});
    const bool plain_real = !a.any() && !(signal && n_signal) && !in_is_complex && !filters_are_complex;
    const double fs[3] = {in_fs, filter_fs, signal_fs};
    return host_decode(in, in_is_complex != 0, nsamp, nch, wL, wR, filters_are_complex != 0, len, compensate_delay, layout, basis, a, signal,
                       n_signal, out, plain_real ? nullptr : imag_abs_sum, fs);
}

static int device_decode(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL, const void* d_wR,
                         int filters_are_complex, int64_t len, int layout, int basis, const Angles& a, const double* d_signal, int64_t n_signal,
                         const double* fs, double* d_out, double* imag_abs_sum, void* stream) {
    return guarded_call([&] {
        check_args(true, {d_in, d_wL, d_wR, d_out}, nsamp, nch, len, n_signal, layout, basis, a);
        const int64_t nsig = d_signal ? n_signal : 0;
        Ratio rf, rs;
        decode_ratios(fs, nsig, rf, rs);
        if (imag_abs_sum) imag_abs_sum[0] = imag_abs_sum[1] = 0.0;
        hipStream_t st = (hipStream_t)stream;
        if (nsamp == 0) {
            if (nsig > 0) HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(double) * 2 * rs.length(nsig), st));
            HIP_CHECK(hipStreamSynchronize(st));
            return;
        }
        decode_body(d_in, in_is_complex != 0, nsamp, (int)nch, d_wL, d_wR, filters_are_complex != 0, len, layout, basis == EMAGLS_BASIS_COMPLEX,
                    a, d_signal, nsig, 0, d_out, imag_abs_sum, st, rf, rs);
    });
}

int emagls_binaural_decode_render_ypr_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                             const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis, const double* d_yaw,
                                             int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                                             const double* d_signal, int64_t n_signal, double* d_out, double* imag_abs_sum, void* stream) {
    return device_decode(d_in, in_is_complex, nsamp, nch, d_wL, d_wR, filters_are_complex, len, layout, basis,
                         {d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll}, d_signal, n_signal, nullptr, d_out, imag_abs_sum, stream);
}

int emagls_binaural_decode_render_fs_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                            const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis, const double* d_yaw,
                                            int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                                            const double* d_signal, int64_t n_signal, double in_fs, double filter_fs, double signal_fs,
                                            double* d_out, double* imag_abs_sum, void* stream) {
    const double fs[3] = {in_fs, filter_fs, signal_fs};
    return device_decode(d_in, in_is_complex, nsamp, nch, d_wL, d_wR, filters_are_complex, len, layout, basis,
                         {d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll}, d_signal, n_signal, fs, d_out, imag_abs_sum, stream);
}

int64_t emagls_resample_length(int64_t nsamp, int64_t p, int64_t q) {
    if (nsamp < 0 || p < 1 || q < 1) return -1;
    const int64_t g = std::gcd(p, q);
    return resample_length(nsamp, p / g, q / g);
}

int emagls_resample(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int64_t p, int64_t q, void* out) {
    return guarded_call([&] {
        if (!in || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nsamp < 0 || nch < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        const Ratio r = reduce_ratio(p, q);
        if (nsamp == 0) return;
        const bool c = in_is_complex != 0;
        const size_t bout = esz(c) * (size_t)r.length(nsamp) * nch;
        Scratch s;
        const void* d_in = s.put((const char*)in, esz(c) * (size_t)nsamp * nch);
        void* d_out = s.get(bout);
        launch_resample(d_in, c, nsamp, nch, r.p, r.q, d_out, s.st);
        HIP_CHECK(hipMemcpyAsync(out, d_out, bout, hipMemcpyDefault, s.st));
        HIP_CHECK(hipStreamSynchronize(s.st));
    });
}

int emagls_resample_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, int64_t p, int64_t q, void* d_out, void* stream) {
    return guarded_call([&] {
        if (!d_in || !d_out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nsamp < 0 || nch < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        const Ratio r = reduce_ratio(p, q);
        launch_resample(d_in, in_is_complex != 0, nsamp, nch, r.p, r.q, d_out, (hipStream_t)stream);
    });
}

int emagls_binaural_decode_render_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                         const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis,
                                         const double* d_yaw, int64_t n_yaw, const double* d_signal, int64_t n_signal, double* d_out,
                                         double* imag_abs_sum, void* stream) {
    return emagls_binaural_decode_render_ypr_device(d_in, in_is_complex, nsamp, nch, d_wL, d_wR, filters_are_complex, len, layout, basis,
                                                    d_yaw, n_yaw, nullptr, 0, nullptr, 0, d_signal, n_signal, d_out, imag_abs_sum, stream);
}

int emagls_binaural_decode_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL, const void* d_wR,
                                  int filters_are_complex, int64_t len, double* d_out, double* imag_abs_sum, void* stream) {
    return emagls_binaural_decode_render_ypr_device(d_in, in_is_complex, nsamp, nch, d_wL, d_wR, filters_are_complex, len, EMAGLS_LAYOUT_SH,
                                                    EMAGLS_BASIS_REAL, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, d_out, imag_abs_sum,
                                                    stream);
}

int emagls_rotate_yaw(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int layout, int basis, const double* yaw,
                      int64_t n_yaw, void* out) {
    return host_rotate(in, in_is_complex != 0, nsamp, nch, layout, basis, {yaw, n_yaw}, out);
}

int emagls_rotate_sh(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int basis, const double* yaw, int64_t n_yaw,
                     const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, void* out) {
    Angles a{yaw, n_yaw, pitch, n_pitch, roll, n_roll};
    auto counted = [&](int64_t n) { return n >= 0 && (n <= 1 || n == nsamp); };
    if (counted(n_pitch) && counted(n_roll)) a = host_angles(a);   // (zeros in a count that does not fit are reported, not dropped)
    const double zero = 0.0;
    if (a.yaw_only() && a.n_yaw == 0) { a.yaw = &zero; a.n_yaw = 1; }   // (an absent yaw is 0)
    return host_rotate(in, in_is_complex != 0, nsamp, nch, EMAGLS_LAYOUT_SH, basis, a, out);
}

int emagls_sh_rotation_matrix(int order, int basis, double yaw, double pitch, double roll, void* out) {
    return guarded_call([&] {
        if (!out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
        check_order3(order);
        check_basis(basis);
        const size_t C = (size_t)(order + 1) * (order + 1), bytes = esz(basis == EMAGLS_BASIS_COMPLEX) * C * C;
        Scratch s;
        void* d = s.get(bytes);
        launch_rotate3_matrix(order, basis == EMAGLS_BASIS_COMPLEX, yaw, pitch, roll, d, s.st);
        HIP_CHECK(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s.st));
        HIP_CHECK(hipStreamSynchronize(s.st));
    });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// The decode stream (decode_stream.hip; DESIGN.md sections 9.3 and 9.4) and the listener group (section 9.5): one object with d.L
// listeners, the per-listener state L times over, the bank once, and one host path for both.  A stream is the object with
// d.L == 1; emagls_decode_group is the ABI's second name for it, and the two sets of entry points differ in the wording of
// some errors (Kind) and in nothing else.  The object owns its device buffers: emagls_cache_clear() does not reach them.
// ---------------------------------------------------------------------------------------------
struct emagls_decode_stream : BlockStreamObject<emagls_decode_stream, 4> {   // stage: the push's input, angles, output and set indices
    int64_t nch = 0, len = 0;
    int layout = 0, basis = 0;
    bool in_c = false;            // the signal the rotation and the filters meet is complex (an encoded stream: its encoder is)
    int64_t nmics = 0;            // an encoded stream: the microphones of a pushed block; 0: blocks are SH / CH
    std::vector<double> enc_host; // [nch][nmics] row-major, interleaved complex when in_c
    std::vector<double> wpl;      // [S][2][Cp][len] the real filter planes [re w; -im w], until the device has their spectra
    DecodeStreamState d;          // the launchers' view of mem
    // xrot [L][nch][B]: the rotated block of every listener (cplx when the signal or the basis is complex); enc: enc_host's device copy
    struct Mem { DevMem Wf, ring, hist, pos, xrot, enc; } mem;
    void* xrot = nullptr;
    double* enc = nullptr;
    int known[2] = {-1, -1};      // d.L == 1: what the host knows of the selection state on the device: the set indices of the two
                                  // previous blocks, -1: none yet, -2: not known (a push took its indices from device memory)
    int cp() const { return d.planes2 ? 2 * d.C : d.C; }
    // a pushed block: [nsamp x block_cols()], complex when block_c()
    int64_t block_cols() const { return nmics ? nmics : nch; }
    bool block_c() const { return nmics ? false : in_c; }
    size_t enc_bytes() const { return sizeof(double) * enc_host.size(); }
    // per listener:
    size_t ring_bytes() const { return sizeof(cplx) * 2 * (size_t)d.P * (d.B + 1); }
    size_t hist_bytes() const { return esz(d.planes2) * (size_t)d.C * d.B; }
    size_t pos_bytes() const { return sizeof(int) * (d.S > 1 ? 3 : 1); }   // the ring position; with a bank, the two previous set indices
    size_t state_bytes() const { return (size_t)d.L * (ring_bytes() + hist_bytes() + pos_bytes()); }
    // once, whatever the number of listeners:
    size_t filter_bytes() const { return sizeof(cplx) * (size_t)d.S * 2 * (size_t)d.P * cp() * (d.B + 1) + enc_bytes(); }
    size_t spectra_bytes() const { return filter_bytes() - enc_bytes(); }
    void bind() {
        d.Wf = mem.Wf.get<cplx>(); d.ring = mem.ring.get<cplx>(); d.hist = mem.hist.get(); d.pos = mem.pos.get<int>();
        xrot = mem.xrot.get(); enc = mem.enc.get<double>();
    }
    // the listeners first .. first + count - 1 back to a fresh stream's state
    void zero_state(hipStream_t st, int64_t first, int64_t count) {
        const size_t n = (size_t)count, pb = pos_bytes();
        HIP_CHECK(hipMemsetAsync((char*)d.ring + (size_t)first * ring_bytes(), 0, n * ring_bytes(), st));
        HIP_CHECK(hipMemsetAsync((char*)d.hist + (size_t)first * hist_bytes(), 0, n * hist_bytes(), st));
        char* pos = (char*)d.pos + (size_t)first * pb;
        HIP_CHECK(hipMemset2DAsync(pos, pb, 0, sizeof(int), n, st));
        if (d.S > 1) HIP_CHECK(hipMemset2DAsync(pos + sizeof(int), pb, 0xff, 2 * sizeof(int), n, st));   // -1: no block yet
        known[0] = known[1] = -1;
    }
    void build_device() {
        mem.Wf.alloc(spectra_bytes());
        mem.ring.alloc(d.L * ring_bytes());
        mem.hist.alloc(d.L * hist_bytes());
        mem.pos.alloc(d.L * pos_bytes());
        mem.xrot.alloc(esz(d.planes2) * (size_t)d.L * d.C * d.B);   // (a rotated block is complex exactly when planes2)
        Scratch s;
        if (nmics) {
            mem.enc.alloc(enc_bytes());
            HIP_CHECK(hipMemcpyAsync(mem.enc.get(), enc_host.data(), enc_bytes(), hipMemcpyHostToDevice, s.st));
        }
        bind();
        launch_decode_stream_filters(s.put(wpl.data(), wpl.size()), cp(), len, d.B, d.P, d.S, d.Wf, s.st);
        zero_state(s.st, 0, d.L);
        s.sync();
        wpl = std::vector<double>();
    }
    void drop_device() { mem = Mem(); bind(); }
};

namespace {

constexpr int64_t kDecodeStreamMaxSets = 65536;
constexpr int64_t kDecodeGroupMaxListeners = 4096;   // well under the grid's limit; keeps xrot and the rings of large shapes bounded

// The two names of the object, where their errors differ (the texts and their order are part of the ABI).  angle_count: a wrong
// angle count is reported by check_push, in the group's wording; null: a stream's is left to check_args, in the rotation's.
struct Kind { const char* null_handle; const char* set_count; const char* angle_count; const char* outside_bank; };
const Kind kStream{"null decode stream", "a push takes 0 set indices, 1, or one per block", nullptr, "set index outside the stream's bank"};
const Kind kGroup{"null decode group", "a group push takes 0 set indices, one per listener, or one per listener and block",
                  "a group push takes no value of an angle, one per listener, or one per listener and sample",
                  "set index outside the group's bank"};

emagls_decode_stream* object_of(emagls_decode_group* g) { return reinterpret_cast<emagls_decode_stream*>(g); }
const emagls_decode_stream* object_of(const emagls_decode_group* g) { return reinterpret_cast<const emagls_decode_stream*>(g); }

// the set indices of a push; host: the same values, where the host has them
struct Sets { const int32_t* p = nullptr; int64_t n = 0; const int32_t* host = nullptr; };

// A count of a push, arrays listener-major: 0, L (one value per listener) or L * per (per = nsamp for an angle, nsamp / block for
// a set index).  With L == 1 that is a stream's 0, 1 or one per sample / per block.  Returns what one listener has.
int64_t push_count(int64_t n, int64_t L, int64_t per, const void* p, const char* wrong) {
    if (n != 0 && n != L && n != L * per) throw Error(EMAGLS_ERR_ARG, wrong);
    if (n > 0 && !p) throw Error(EMAGLS_ERR_ARG, "null pointer");
    return n == 0 ? 0 : (per != 1 && n == L * per) ? per : 1;
}

// what one listener has of each array of a push
struct Push { Angles one; int64_t set_per = 0; };

Push check_push(const Kind& k, const emagls_decode_stream* s, const void* in, const void* out, int64_t nsamp, const Angles& a, const Sets& sets) {
    if (!s) throw Error(EMAGLS_ERR_ARG, k.null_handle);
    const int64_t B = s->d.B, L = s->d.L;
    if (nsamp < 0 || nsamp % B) throw Error(EMAGLS_ERR_ARG, "a push needs a multiple of the block size of samples");
    Push r;
    r.set_per = push_count(sets.n, L, nsamp / B, sets.p, k.set_count);
    r.one = a;
    if (k.angle_count) {
        r.one.n_yaw = push_count(a.n_yaw, L, nsamp, a.yaw, k.angle_count);
        r.one.n_pitch = push_count(a.n_pitch, L, nsamp, a.pitch, k.angle_count);
        r.one.n_roll = push_count(a.n_roll, L, nsamp, a.roll, k.angle_count);
    }
    check_args(true, {in, out}, nsamp, s->nch, s->len, 0, s->layout, s->basis, r.one);
    return r;
}

// The blocks of a push in order on st, at most three launches each whatever L is; device pointers; not synchronised (s->mu held,
// device current).  Per-sample angles are [L][nsamp], set indices per block [L][nsamp / B], d_out [L][2][nsamp].
void push_blocks(emagls_decode_stream* s, const void* d_in, int64_t nsamp, const Push& p, const Sets& sets, double* d_out, hipStream_t st) {
    s->ensure_device();
    const int64_t B = s->d.B, C = s->d.C, nb = nsamp / B;
    const int L = s->d.L;
    const bool cb = s->basis == EMAGLS_BASIS_COMPLEX;
    const Angles& a = p.one;
    const bool turned = a.any();
    // block b of listener l's angles at + l nsamp + b B; one value per listener: [L]  (the kernels index by the listener: 0 when L == 1)
    const int64_t la[3] = {a.n_yaw > 1 ? nsamp : 1, a.n_pitch > 1 ? nsamp : 1, a.n_roll > 1 ? nsamp : 1};
    auto at = [&](const double* q, int64_t n, int64_t b) { return n > 1 ? q + b * B : q; };
    for (int64_t b = 0; b < nb; ++b) {
        const void* x = (const char*)d_in + esz(s->block_c()) * (size_t)(b * B);
        bool x_c = s->in_c;
        int64_t ldx = nsamp, lsx = 0;   // without angles every listener reads the common block
        const Angles blk{at(a.yaw, a.n_yaw, b), a.n_yaw > 1 ? B : a.n_yaw, at(a.pitch, a.n_pitch, b), a.n_pitch > 1 ? B : a.n_pitch,
                         at(a.roll, a.n_roll, b), a.n_roll > 1 ? B : a.n_roll};
        if (s->nmics) {   // the encoder inside the rotation launch, in every listener's workgroups; without angles, alone and once
            const EncodeBlock e{s->enc, s->in_c, (int)s->nmics, (const double*)x, nsamp};
            if (turned) launch_rotation_encoded(blk, e, B, (int)C, s->layout, cb, s->xrot, st, B, L, la, C * B);
            else launch_encode_block(e, B, (int)C, s->xrot, B, st);
            x = s->xrot; x_c = x_c || (turned && cb); ldx = B; lsx = turned ? C * B : 0;
        } else if (turned) {
            launch_rotation(blk, x, x_c, B, (int)C, s->layout, cb, false, s->xrot, st, nsamp, B, L, la, C * B);
            x = s->xrot; x_c = x_c || cb; ldx = B; lsx = C * B;
        }
        // One listener: the host's copy of the selection, moved on as the kernels move theirs; three equal known indices are a
        // standing set, which runs the plain instance.  More: the kernels decide for every listener (section 9.4: the same bits)
        int standing = -1;
        if (L == 1) {
            int cur = -2;
            if (p.set_per == 0) cur = s->known[0] == -2 ? -2 : std::max(s->known[0], 0);
            else if (sets.host) cur = sets.host[p.set_per > 1 ? b : 0];
            if (cur >= 0) {
                const int s1 = s->known[0] == -1 ? cur : s->known[0], s2 = s->known[1] == -1 ? s1 : s->known[1];
                if (s1 == cur && s2 == cur) standing = cur;
            }
            s->known[1] = s->known[0] == -1 ? cur : s->known[0];
            s->known[0] = cur;
        }
        const int32_t* set = p.set_per > 1 ? sets.p + b : p.set_per ? sets.p : nullptr;
        launch_decode_stream_block(s->d, x, x_c, ldx, set, standing, d_out + b * B, nsamp, st, lsx, (int)(p.set_per > 1 ? nb : 1), 2 * nsamp);
    }
}

// A push of device arrays on the caller's stream (the kernels clamp the indices: the host never sees them)
int device_push(const Kind& k, emagls_decode_stream* s, const void* d_in, int64_t nsamp, const Sets& sets, const Angles& a, double* d_out,
                void* stream) {
    return guarded_call([&] {
        const Push p = check_push(k, s, d_in, d_out, nsamp, a, sets);
        if (nsamp == 0) return;
        s->device_frame([&] { push_blocks(s, d_in, nsamp, p, sets, d_out, (hipStream_t)stream); });
    });
}

// A push of host arrays: staged on a pool stream, pushed, the result back, synchronised
int host_push(const Kind& k, emagls_decode_stream* s, const void* in, int64_t nsamp, const int32_t* set, int64_t n_set, Angles a, double* out) {
    return guarded_call([&] {
        if (s) {   // (zeros in a count that does not fit are reported, not dropped)
            auto counted = [&](int64_t n) { return n == 0 || n == s->d.L || n == s->d.L * nsamp; };
            if (counted(a.n_pitch) && counted(a.n_roll)) a = host_angles(a);
        }
        const Push p = check_push(k, s, in, out, nsamp, a, {set, n_set});
        for (int64_t i = 0; i < n_set; ++i)
            if (set[i] < 0 || set[i] >= s->d.S) throw Error(EMAGLS_ERR_ARG, k.outside_bank);
        if (nsamp == 0) return;
        s->host_frame([&](hipStream_t st) {
            const size_t L = (size_t)s->d.L, bin = esz(s->block_c()) * (size_t)nsamp * s->block_cols();
            char* d_in = s->staged<char>(0, bin);
            double* d_ang = s->staged<double>(1, sizeof(double) * 3 * L * (size_t)nsamp);
            double* d_out = s->staged<double>(2, sizeof(double) * 2 * L * (size_t)nsamp);
            HIP_CHECK(hipMemcpyAsync(d_in, in, bin, hipMemcpyHostToDevice, st));
            auto up = [&](const double* q, int64_t n, int slot) -> const double* {
                if (!n) return nullptr;
                double* dst = d_ang + (size_t)slot * L * nsamp;
                HIP_CHECK(hipMemcpyAsync(dst, q, sizeof(double) * n, hipMemcpyHostToDevice, st));
                return dst;
            };
            Push dp = p;
            dp.one.yaw = up(a.yaw, a.n_yaw, 0); dp.one.pitch = up(a.pitch, a.n_pitch, 1); dp.one.roll = up(a.roll, a.n_roll, 2);
            Sets dsets{nullptr, n_set, set};
            if (n_set) {
                int32_t* d_set = s->staged<int32_t>(3, sizeof(int32_t) * (size_t)n_set);
                HIP_CHECK(hipMemcpyAsync(d_set, set, sizeof(int32_t) * (size_t)n_set, hipMemcpyHostToDevice, st));
                dsets.p = d_set;
            }
            push_blocks(s, d_in, nsamp, dp, dsets, d_out, st);
            HIP_CHECK(hipMemcpyAsync(out, d_out, sizeof(double) * 2 * L * nsamp, hipMemcpyDeviceToHost, st));
        });
    });
}

// listener: one listener, or -1: all of them
int reset_object(const Kind& k, emagls_decode_stream* s, int64_t listener) {
    return guarded_call([&] {
        if (!s) throw Error(EMAGLS_ERR_ARG, k.null_handle);
        if (listener < -1 || listener >= s->d.L) throw Error(EMAGLS_ERR_ARG, "listener outside the group (-1: all of them)");
        s->reset_frame([&](hipStream_t st) {
            if (listener < 0) s->zero_state(st, 0, s->d.L);
            else s->zero_state(st, listener, 1);
        });
    });
}

int info_object(const Kind& k, const emagls_decode_stream* s, int64_t* block, int64_t* partitions, int64_t* listeners, int64_t* state_bytes,
                int64_t* filter_bytes, int* launches_per_block) {
    return guarded_call([&] {
        if (!s) throw Error(EMAGLS_ERR_ARG, k.null_handle);
        if (block) *block = s->d.B;
        if (partitions) *partitions = s->d.P;
        if (listeners) *listeners = s->d.L;
        if (state_bytes) *state_bytes = (int64_t)s->state_bytes();
        if (filter_bytes) *filter_bytes = (int64_t)s->filter_bytes();
        // for all listeners: rotation (encoded: with the encoder, or the encoder alone), forward transform with the products, inverse transform
        if (launches_per_block) *launches_per_block = 3;
    });
}

// The creation of the object, every argument checked before the device is touched
// encoded: nmics microphones, enc [nch x nmics] column-major (interleaved complex when in_is_complex, which then says what the
// ENCODED signal is; the pushed microphone blocks are real)
int create_object(bool encoded, int64_t nmics, const void* enc, int64_t nch, int64_t n_sets, const void* wL, const void* wR,
                  int filters_are_complex, int64_t len, int in_is_complex, int layout, int basis, int64_t block, int64_t listeners,
                  emagls_decode_stream** out) {
    return guarded_call([&] {
        if (!wL || !wR || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *out = nullptr;
        if (encoded) {
            if (nmics < 1 || nmics > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "an encoded decode stream supports 1 to 64 microphones");
            if (nch < 1 || nch > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "an encoded decode stream supports 1 to 64 channels");
            if (!enc) throw Error(EMAGLS_ERR_ARG, "null pointer");
        }
        if (nch < 1 || len < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        if (n_sets < 1) throw Error(EMAGLS_ERR_ARG, "a decode stream needs at least one filter set");
        if (n_sets > kDecodeStreamMaxSets) throw Error(EMAGLS_ERR_UNSUPPORTED, "the decode stream supports banks of up to 65536 filter sets");
        if (listeners < 1) throw Error(EMAGLS_ERR_ARG, "a listener group needs at least one listener");
        if (listeners > kDecodeGroupMaxListeners) throw Error(EMAGLS_ERR_UNSUPPORTED, "a listener group supports up to 4096 listeners");
        if (layout != EMAGLS_LAYOUT_SH && layout != EMAGLS_LAYOUT_CH) throw Error(EMAGLS_ERR_ARG, "layout must be EMAGLS_LAYOUT_SH or EMAGLS_LAYOUT_CH");
        check_basis(basis);
        if (!decode_stream_block_ok(block))
            throw Error(EMAGLS_ERR_UNSUPPORTED, "the decode stream supports block sizes 64, 128, 256, 512, 1024 and 2048");
        if (len > 16384) throw Error(EMAGLS_ERR_UNSUPPORTED, "the decode stream supports filters of up to 16384 taps");
        std::unique_ptr<emagls_decode_stream> s(new emagls_decode_stream);
        s->nch = nch; s->len = len; s->layout = layout; s->basis = basis; s->in_c = in_is_complex != 0;
        s->d.C = (int)nch; s->d.B = (int)block; s->d.P = (int)ceil_div(len, block); s->d.S = (int)n_sets; s->d.L = (int)listeners;
        // a rotation in the complex basis makes a real signal complex: such a stream runs on 2C planes from the start
        s->d.planes2 = s->in_c || (basis == EMAGLS_BASIS_COMPLEX && rotate_order(layout, nch) >= 0);
        if (encoded) {
            const int k = s->in_c ? 2 : 1;
            const double* e = reinterpret_cast<const double*>(enc);
            s->nmics = nmics;
            s->enc_host.resize((size_t)nch * nmics * k);
            for (int64_t c = 0; c < nch; ++c)
                for (int64_t m = 0; m < nmics; ++m)
                    for (int i = 0; i < k; ++i) s->enc_host[(size_t)(c * nmics + m) * k + i] = e[(size_t)(m * nch + c) * k + i];
        }
        const int Cp = s->cp();
        const bool wc = filters_are_complex != 0;
        s->wpl.assign((size_t)n_sets * 2 * Cp * len, 0.0);
        for (int64_t set = 0; set < n_sets; ++set)
            for (int e = 0; e < 2; ++e) {
                const double* w = reinterpret_cast<const double*>(e ? wR : wL) + (size_t)set * nch * len * (wc ? 2 : 1);
                double* pl = s->wpl.data() + ((size_t)set * 2 + e) * Cp * len;
                for (int64_t c = 0; c < nch; ++c)
                    for (int64_t t = 0; t < len; ++t) {
                        const size_t i = (size_t)(c * len + t);
                        pl[(size_t)c * len + t] = wc ? w[2 * i] : w[i];
                        if (wc && s->d.planes2) pl[(size_t)(nch + c) * len + t] = -w[2 * i + 1];
                    }
            }
        s->create_device_side();
        *out = s.release();
    });
}

}  // namespace

extern "C" {

int emagls_decode_stream_create(int64_t nch, const void* wL, const void* wR, int filters_are_complex, int64_t len, int in_is_complex,
                                int layout, int basis, int64_t block, emagls_decode_stream** out) {
    return create_object(false, 0, nullptr, nch, 1, wL, wR, filters_are_complex, len, in_is_complex, layout, basis, block, 1, out);
}

int emagls_decode_stream_create_bank(int64_t nch, int64_t n_sets, const void* wL, const void* wR, int filters_are_complex, int64_t len,
                                     int in_is_complex, int layout, int basis, int64_t block, emagls_decode_stream** out) {
    return create_object(false, 0, nullptr, nch, n_sets, wL, wR, filters_are_complex, len, in_is_complex, layout, basis, block, 1, out);
}

int emagls_decode_stream_create_encoded(int64_t nmics, const void* enc, int enc_is_complex, int64_t nch, int64_t n_sets, const void* wL,
                                        const void* wR, int filters_are_complex, int64_t len, int layout, int basis, int64_t block,
                                        emagls_decode_stream** out) {
    return create_object(true, nmics, enc, nch, n_sets, wL, wR, filters_are_complex, len, enc_is_complex, layout, basis, block, 1, out);
}

int emagls_decode_group_create(int64_t nch, int64_t n_sets, const void* wL, const void* wR, int filters_are_complex, int64_t len,
                               int in_is_complex, int layout, int basis, int64_t block, int64_t n_listeners, emagls_decode_group** out) {
    return create_object(false, 0, nullptr, nch, n_sets, wL, wR, filters_are_complex, len, in_is_complex, layout, basis, block, n_listeners,
                         reinterpret_cast<emagls_decode_stream**>(out));
}

int emagls_decode_group_create_encoded(int64_t nmics, const void* enc, int enc_is_complex, int64_t nch, int64_t n_sets, const void* wL,
                                       const void* wR, int filters_are_complex, int64_t len, int layout, int basis, int64_t block,
                                       int64_t n_listeners, emagls_decode_group** out) {
    return create_object(true, nmics, enc, nch, n_sets, wL, wR, filters_are_complex, len, enc_is_complex, layout, basis, block, n_listeners,
                         reinterpret_cast<emagls_decode_stream**>(out));
}

int emagls_decode_stream_push_device(emagls_decode_stream* s, const void* d_in, int64_t nsamp, const double* d_yaw, int64_t n_yaw,
                                     const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll, double* d_out,
                                     void* stream) {
    return device_push(kStream, s, d_in, nsamp, {}, {d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll}, d_out, stream);
}

int emagls_decode_stream_push_sets_device(emagls_decode_stream* s, const void* d_in, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                          const double* d_yaw, int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll,
                                          int64_t n_roll, double* d_out, void* stream) {
    return device_push(kStream, s, d_in, nsamp, {d_set, n_set}, {d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll}, d_out, stream);
}

int emagls_decode_group_push_device(emagls_decode_group* g, const void* d_in, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                    const double* d_yaw, int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll,
                                    int64_t n_roll, double* d_out, void* stream) {
    return device_push(kGroup, object_of(g), d_in, nsamp, {d_set, n_set}, {d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll}, d_out, stream);
}

int emagls_decode_stream_push(emagls_decode_stream* s, const void* in, int64_t nsamp, const double* yaw, int64_t n_yaw, const double* pitch,
                              int64_t n_pitch, const double* roll, int64_t n_roll, double* out) {
    return host_push(kStream, s, in, nsamp, nullptr, 0, {yaw, n_yaw, pitch, n_pitch, roll, n_roll}, out);
}

int emagls_decode_stream_push_sets(emagls_decode_stream* s, const void* in, int64_t nsamp, const int32_t* set, int64_t n_set,
                                   const double* yaw, int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll,
                                   int64_t n_roll, double* out) {
    return host_push(kStream, s, in, nsamp, set, n_set, {yaw, n_yaw, pitch, n_pitch, roll, n_roll}, out);
}

int emagls_decode_group_push(emagls_decode_group* g, const void* in, int64_t nsamp, const int32_t* set, int64_t n_set, const double* yaw,
                             int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, double* out) {
    return host_push(kGroup, object_of(g), in, nsamp, set, n_set, {yaw, n_yaw, pitch, n_pitch, roll, n_roll}, out);
}

int emagls_decode_stream_reset(emagls_decode_stream* s) { return reset_object(kStream, s, -1); }

int emagls_decode_group_reset(emagls_decode_group* g, int64_t listener) { return reset_object(kGroup, object_of(g), listener); }

int emagls_decode_stream_info(const emagls_decode_stream* s, int64_t* block, int64_t* partitions, int64_t* state_bytes, int64_t* filter_bytes,
                              int* launches_per_block) {
    return info_object(kStream, s, block, partitions, nullptr, state_bytes, filter_bytes, launches_per_block);
}

int emagls_decode_group_info(const emagls_decode_group* g, int64_t* block, int64_t* partitions, int64_t* listeners,
                             int64_t* state_bytes, int64_t* filter_bytes, int* launches_per_block) {
    return info_object(kGroup, object_of(g), block, partitions, listeners, state_bytes, filter_bytes, launches_per_block);
}

int emagls_decode_stream_sets(const emagls_decode_stream* s, int64_t* n_sets) {
    return guarded_call([&] {
        if (!s) throw Error(EMAGLS_ERR_ARG, "null decode stream");
        if (!n_sets) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *n_sets = s->d.S;
    });
}

int emagls_decode_stream_destroy(emagls_decode_stream* s) { return emagls_decode_stream::destroy(s); }

int emagls_decode_group_destroy(emagls_decode_group* g) { return emagls_decode_stream::destroy(object_of(g)); }

}  // extern "C"
