// C ABI of the three-axis rotation (include/emagls.h, "three-axis rotation"): emagls_sh_rotation_matrix, emagls_rotate_sh and
// the binauralDecode entry points with yaw, pitch and roll.  The rotation runs in rotate3.hip, the decode in capi.hip's
// render_core.  Calls whose pitch and roll are all zero take the yaw entry points of capi.hip.  No CPU fallback.
#include <vector>

#include "../../include/emagls.h"
#include "kernels.hpp"

using namespace emagls;

namespace {

struct Scratch {   // device buffers of one call, freed on every exit path
    std::vector<void*> ptrs;
    hipStream_t st = nullptr;
    Scratch() { st = pool_stream_take(); }
    ~Scratch() {
        for (void* p : ptrs) hipFree(p);
        pool_stream_give(st);
    }
    template <typename T = void> T* get(size_t bytes) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
        ptrs.push_back(p);
        return reinterpret_cast<T*>(p);
    }
    template <typename T> T* put(const T* host, size_t count) {
        if (!host || !count) return nullptr;
        T* p = get<T>(sizeof(T) * count);
        HIP_CHECK(hipMemcpyAsync(p, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
        return p;
    }
};

bool all_zero(const double* a, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (a[i] != 0.0) return false;
    return true;
}

void check_angles(int64_t nsamp, const double* p, int64_t n, const char* name) {
    if (n < 0 || (n > 1 && n != nsamp)) throw Error(EMAGLS_ERR_ARG, std::string(name) + " needs no value, one value or one value per input sample");
    if (n > 0 && !p) throw Error(EMAGLS_ERR_ARG, "null pointer");
}

// the SH order of nch channels for the three-axis rotation; layout CH only when pitch and roll are absent (checked by the caller)
int sh_order3(int64_t nch) {
    const int N = rotate_order(EMAGLS_LAYOUT_SH, nch);
    if (N < 0) throw Error(EMAGLS_ERR_ARG, "the three-axis rotation needs (N+1)^2 SH channels in ACN order");
    if (N > rotate3_max_order()) throw Error(EMAGLS_ERR_UNSUPPORTED, "the three-axis rotation supports SH orders 0 to 15");
    return N;
}

void check_basis(int basis) {
    if (basis != EMAGLS_BASIS_REAL && basis != EMAGLS_BASIS_COMPLEX) throw Error(EMAGLS_ERR_ARG, "shDefinition must be 'real' or 'complex'");
}

// the rotation before the decode: a fixed one (every count <= 1) turns the filters (transposed form), a trajectory the signal
// (into the ROT_SIG work buffer); then the decode forms of render_core run unchanged.  (render_scratch_mutex() held)
void ypr_render(const void* d_in, bool in_c, int64_t nsamp, int nch, const void* d_wL, const void* d_wR, bool w_c, int64_t len, bool cb,
                const double* d_yaw, int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                const double* d_sig, int64_t nsig, int64_t cut, double* d_out, double* imag_abs, hipStream_t st) {
    const double* yaw = n_yaw ? d_yaw : nullptr;
    const double* pitch = n_pitch ? d_pitch : nullptr;
    const double* roll = n_roll ? d_roll : nullptr;
    if (n_yaw <= 1 && n_pitch <= 1 && n_roll <= 1) {
        const bool wc2 = w_c || cb;
        void* rL = render_scratch(RENDER_ROT_WL, esz(wc2) * (size_t)len * nch);
        void* rR = render_scratch(RENDER_ROT_WR, esz(wc2) * (size_t)len * nch);
        launch_rotate3(d_wL, w_c, len, nch, cb, yaw, false, pitch, false, roll, false, true, rL, st);
        launch_rotate3(d_wR, w_c, len, nch, cb, yaw, false, pitch, false, roll, false, true, rR, st);
        d_wL = rL; d_wR = rR; w_c = wc2;
    } else {
        const bool ic2 = in_c || cb;
        void* x = render_scratch(RENDER_ROT_SIG, esz(ic2) * (size_t)nsamp * nch);
        launch_rotate3(d_in, in_c, nsamp, nch, cb, yaw, n_yaw > 1, pitch, n_pitch > 1, roll, n_roll > 1, false, x, st);
        d_in = x; in_c = ic2;
    }
    render_core(d_in, in_c, nsamp, nch, d_wL, d_wR, w_c, len, EMAGLS_LAYOUT_SH, cb, nullptr, 0, d_sig, nsig, cut, d_out, imag_abs, st);
}

void check_ypr(int64_t nsamp, int64_t nch, int layout, int basis, const double* yaw, int64_t n_yaw, const double* pitch, int64_t n_pitch,
               const double* roll, int64_t n_roll) {
    check_angles(nsamp, yaw, n_yaw, "yaw");
    check_angles(nsamp, pitch, n_pitch, "pitch");
    check_angles(nsamp, roll, n_roll, "roll");
    if (layout == EMAGLS_LAYOUT_CH) throw Error(EMAGLS_ERR_ARG, "a CH signal can only be turned about z: pitch and roll must be 0");
    if (layout != EMAGLS_LAYOUT_SH) throw Error(EMAGLS_ERR_ARG, "layout must be EMAGLS_LAYOUT_SH or EMAGLS_LAYOUT_CH");
    check_basis(basis);
    sh_order3(nch);
}

}  // namespace

extern "C" {

int emagls_sh_rotation_matrix(int order, int basis, double yaw, double pitch, double roll, void* out) {
    return guarded_call([&] {
        if (!out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
        if (order > rotate3_max_order()) throw Error(EMAGLS_ERR_UNSUPPORTED, "the three-axis rotation supports SH orders 0 to 15");
        check_basis(basis);
        const size_t C = (size_t)(order + 1) * (order + 1), bytes = esz(basis == EMAGLS_BASIS_COMPLEX) * C * C;
        Scratch s;
        void* d = s.get(bytes);
        launch_rotate3_matrix(order, basis == EMAGLS_BASIS_COMPLEX, yaw, pitch, roll, d, s.st);
        HIP_CHECK(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s.st));
        HIP_CHECK(hipStreamSynchronize(s.st));
    });
}

int emagls_rotate_sh(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, int basis, const double* yaw, int64_t n_yaw,
                     const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll, void* out) {
    if (in && out && nsamp >= 0 && (n_pitch == 0 || pitch) && (n_roll == 0 || roll) && n_pitch >= 0 && n_roll >= 0 &&
        (n_pitch <= 1 || n_pitch == nsamp) && (n_roll <= 1 || n_roll == nsamp) && all_zero(pitch, n_pitch) && all_zero(roll, n_roll)) {
        const double zero = 0.0;   // yaw only: the yaw entry point, bit for bit
        return emagls_rotate_yaw(in, in_is_complex, nsamp, nch, EMAGLS_LAYOUT_SH, basis, n_yaw ? yaw : &zero, n_yaw ? n_yaw : 1, out);
    }
    return guarded_call([&] {
        if (!in || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nsamp < 0 || nch < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        check_ypr(nsamp, nch, EMAGLS_LAYOUT_SH, basis, yaw, n_yaw, pitch, n_pitch, roll, n_roll);
        if (nsamp == 0) return;
        const bool ic = in_is_complex != 0, cb = basis == EMAGLS_BASIS_COMPLEX;
        const size_t bin = esz(ic) * (size_t)nsamp * nch, bout = esz(ic || cb) * (size_t)nsamp * nch;
        Scratch s;
        void* d_in = s.get(bin);
        void* d_out = s.get(bout);
        HIP_CHECK(hipMemcpyAsync(d_in, in, bin, hipMemcpyHostToDevice, s.st));
        const double *d_yaw = s.put(yaw, n_yaw), *d_pitch = s.put(pitch, n_pitch), *d_roll = s.put(roll, n_roll);
        launch_rotate3(d_in, ic, nsamp, (int)nch, cb, d_yaw, n_yaw > 1, d_pitch, n_pitch > 1, d_roll, n_roll > 1, false, d_out, s.st);
        HIP_CHECK(hipMemcpyAsync(out, d_out, bout, hipMemcpyDeviceToHost, s.st));
        HIP_CHECK(hipStreamSynchronize(s.st));
    });
}

int emagls_binaural_decode_render_ypr(const void* in, int in_is_complex, int64_t nsamp, int64_t nch, const void* wL, const void* wR,
                                      int filters_are_complex, int64_t len, int compensate_delay, int layout, int basis, const double* yaw,
                                      int64_t n_yaw, const double* pitch, int64_t n_pitch, const double* roll, int64_t n_roll,
                                      const double* signal, int64_t n_signal, double* out, double* imag_abs_sum) {
    if ((n_pitch == 0 || (pitch && n_pitch > 0 && all_zero(pitch, n_pitch))) && (n_roll == 0 || (roll && n_roll > 0 && all_zero(roll, n_roll))))
        return emagls_binaural_decode_render(in, in_is_complex, nsamp, nch, wL, wR, filters_are_complex, len, compensate_delay, layout,
                                             basis, yaw, n_yaw, signal, n_signal, out, imag_abs_sum);   // yaw only, bit for bit
    return guarded_call([&] {
        if (!in || !wL || !wR || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nsamp < 0 || nch < 1 || len < 1 || n_signal < 0) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        check_ypr(nsamp, nch, layout, basis, yaw, n_yaw, pitch, n_pitch, roll, n_roll);
        if (imag_abs_sum) imag_abs_sum[0] = imag_abs_sum[1] = 0.0;
        const int64_t nsig = signal ? n_signal : 0;
        const int64_t nout = nsig > 0 ? nsig : nsamp;
        const int64_t skip = (compensate_delay && len / 2 > 0) ? len / 2 - 1 : 0;    // binauralOut(del:end,:), del = len/2 (:53-57)
        if (nsamp == 0) {
            if (nout - skip > 0) std::fill(out, out + 2 * (nout - skip), 0.0);
            return;
        }
        const bool ic = in_is_complex != 0, wc = filters_are_complex != 0;
        const size_t bin = esz(ic) * (size_t)nsamp * nch, bw = esz(wc) * (size_t)len * nch;
        Scratch s;
        void* d_in = s.get(bin);
        void* d_wL = s.get(bw);
        void* d_wR = s.get(bw);
        double* d_out = s.get<double>(sizeof(double) * 2 * nout);
        HIP_CHECK(hipMemcpyAsync(d_in, in, bin, hipMemcpyHostToDevice, s.st));
        HIP_CHECK(hipMemcpyAsync(d_wL, wL, bw, hipMemcpyHostToDevice, s.st));
        HIP_CHECK(hipMemcpyAsync(d_wR, wR, bw, hipMemcpyHostToDevice, s.st));
        const double *d_yaw = s.put(yaw, n_yaw), *d_pitch = s.put(pitch, n_pitch), *d_roll = s.put(roll, n_roll);
        const double* d_sig = s.put(signal, (size_t)nsig);
        {
            std::lock_guard<std::mutex> lk(render_scratch_mutex());
            ypr_render(d_in, ic, nsamp, (int)nch, d_wL, d_wR, wc, len, basis == EMAGLS_BASIS_COMPLEX, d_yaw, n_yaw, d_pitch, n_pitch, d_roll,
                       n_roll, d_sig, nsig, skip, d_out, imag_abs_sum, s.st);
        }
        const int64_t rows = nout - skip;
        if (rows > 0) {
            HIP_CHECK(hipMemcpy(out, d_out + skip, sizeof(double) * rows, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out + rows, d_out + nout + skip, sizeof(double) * rows, hipMemcpyDeviceToHost));
        }
    });
}

int emagls_binaural_decode_render_ypr_device(const void* d_in, int in_is_complex, int64_t nsamp, int64_t nch, const void* d_wL,
                                             const void* d_wR, int filters_are_complex, int64_t len, int layout, int basis, const double* d_yaw,
                                             int64_t n_yaw, const double* d_pitch, int64_t n_pitch, const double* d_roll, int64_t n_roll,
                                             const double* d_signal, int64_t n_signal, double* d_out, double* imag_abs_sum, void* stream) {
    if (n_pitch == 0 && n_roll == 0)
        return emagls_binaural_decode_render_device(d_in, in_is_complex, nsamp, nch, d_wL, d_wR, filters_are_complex, len, layout, basis,
                                                    d_yaw, n_yaw, d_signal, n_signal, d_out, imag_abs_sum, stream);
    return guarded_call([&] {
        if (!d_in || !d_wL || !d_wR || !d_out) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nsamp < 0 || nch < 1 || len < 1 || n_signal < 0) throw Error(EMAGLS_ERR_ARG, "invalid shape");
        check_ypr(nsamp, nch, layout, basis, d_yaw, n_yaw, d_pitch, n_pitch, d_roll, n_roll);
        if (imag_abs_sum) imag_abs_sum[0] = imag_abs_sum[1] = 0.0;
        const int64_t nsig = d_signal ? n_signal : 0;
        hipStream_t st = (hipStream_t)stream;
        if (nsamp == 0) {
            if (nsig > 0) HIP_CHECK(hipMemsetAsync(d_out, 0, sizeof(double) * 2 * nsig, st));
            HIP_CHECK(hipStreamSynchronize(st));
            return;
        }
        std::lock_guard<std::mutex> lk(render_scratch_mutex());
        ypr_render(d_in, in_is_complex != 0, nsamp, (int)nch, d_wL, d_wR, filters_are_complex != 0, len, basis == EMAGLS_BASIS_COMPLEX, d_yaw,
                   n_yaw, d_pitch, n_pitch, d_roll, n_roll, d_signal, nsig, 0, d_out, imag_abs_sum, st);
    });
}

}  // extern "C"
