// Yaw rotation of SH / CH signals (the yaw part of rotateHOA_N3D, called by dependencies/binauralDecode.m:27-31).  OWN
// SPECIFICATION: rotating by theta turns the sound field counter-clockwise about z, so the signal of a
// plane wave from azimuth a, conj(getSH(N, [a zen])) / conj(getCH(N, a)), becomes the one of the plane wave from a + theta.
// Only the channels (n, m) and (n, -m) mix:
//   real basis      out(n, m) = cos(m t) x(n, m) - sin(m t) x(n, -m),  out(n, -m) = cos(m t) x(n, -m) + sin(m t) x(n, m)   (m > 0)
//   complex basis   out(n, m) = exp(-i m t) x(n, m)                                                                    (any m)
// whatever the normalisation.  theta is reduced modulo 2 pi in FP64 before m theta is formed.
#include "kernels.hpp"
#include "encode_tile.hpp"

namespace emagls {

int rotate_order(int layout, int64_t C) {
    if (C < 1) return -1;
    if (layout == 0) {   // SH, ACN: (N + 1)^2 channels
        int64_t N = (int64_t)std::llround(std::sqrt((double)C)) - 1;
        return (N >= 0 && (N + 1) * (N + 1) == C) ? (int)N : -1;
    }
    if (layout == 1) return (C % 2) ? (int)((C - 1) / 2) : -1;   // CH: [C_0, C_-1, C_1, ..., C_-N, C_N], 2N + 1 channels
    return -1;
}

namespace {

template <bool C_> struct Val;
template <> struct Val<false> { using T = double; };
template <> struct Val<true> { using T = cplx; };

__device__ __forceinline__ cplx widen(double v) { return mk(v, 0.0); }
__device__ __forceinline__ cplx widen(cplx v) { return v; }

// one thread = one sample (row) of every channel; columns are channel planes of n values, so a wave's loads are contiguous
// IC / OC: input / output complex (OC = IC || complex basis).  sgn = -1 applies the transpose of the real-basis rotation
// (the decoding filters of a fixed angle: sum_i w_i * (x Rot^T)_i = sum_j (w Rot)_j * x_j); the complex basis is diagonal.
// grid (., L): listener l = blockIdx.y turns the one signal by its angles, yaw_ + l la, into out_ + l lo (a listener group)
template <bool IC, bool OC>
__global__ void __launch_bounds__(256) rotate_yaw_kernel(const void* __restrict__ in_, int64_t n, int N, int layout, int cb,
                                                         const double* __restrict__ yaw_, int per_sample, double sgn, void* __restrict__ out_, int64_t ldi, int64_t ldo,
                                                         int64_t la, int64_t lo) {
    using TI = typename Val<IC>::T;
    using TO = typename Val<OC>::T;
    const TI* __restrict__ in = reinterpret_cast<const TI*>(in_);
    TO* __restrict__ out = reinterpret_cast<TO*>(out_) + (int64_t)blockIdx.y * lo;
    const double* __restrict__ yaw = yaw_ + (int64_t)blockIdx.y * la;
    const int nl = layout == 0 ? N + 1 : 1;   // channels of one |m|: SH orders n = m..N, CH one pair
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const double th = fmod(yaw[per_sample ? t : 0], 2.0 * kPi);
        for (int j = 0; j < nl; ++j) {          // m = 0: unchanged
            const int64_t k = layout == 0 ? (int64_t)j * j + j : 0;
            if constexpr (OC) out[k * ldo + t] = widen(in[k * ldi + t]);
            else out[k * ldo + t] = in[k * ldi + t];
        }
        for (int m = 1; m <= N; ++m) {
            double s, c;
            sincos((double)m * th, &s, &c);
            for (int nn = layout == 0 ? m : 0; nn < (layout == 0 ? N + 1 : 1); ++nn) {
                const int64_t p = layout == 0 ? (int64_t)nn * nn + nn + m : 2 * m;        // (n, m)
                const int64_t q = layout == 0 ? (int64_t)nn * nn + nn - m : 2 * m - 1;    // (n, -m)
                const TI a = in[p * ldi + t], b = in[q * ldi + t];
                if constexpr (OC) {
                    const cplx ac = widen(a), bc = widen(b);
                    if (cb) {   // exp(-i m t) and exp(+i m t)
                        out[p * ldo + t] = mk(c * ac.x + s * ac.y, c * ac.y - s * ac.x);
                        out[q * ldo + t] = mk(c * bc.x - s * bc.y, c * bc.y + s * bc.x);
                    } else {
                        const double ss = sgn * s;
                        out[p * ldo + t] = mk(c * ac.x - ss * bc.x, c * ac.y - ss * bc.y);
                        out[q * ldo + t] = mk(c * bc.x + ss * ac.x, c * bc.y + ss * ac.y);
                    }
                } else {
                    const double ss = sgn * s;
                    out[p * ldo + t] = c * a - ss * b;
                    out[q * ldo + t] = c * b + ss * a;
                }
            }
        }
    }
}

// The loop body of the kernel above as a function of its own, for the ENC form below: row ti of in (channel planes ldi apart)
// turned by th into row to of out, expression for expression what the kernel does (the build does not contract, so the bits are
// the kernel's).  The kernel keeps its body: called from there, this function changes the schedule of its complex instance.
template <bool IC, bool OC>
__device__ __forceinline__ void yaw_sample(const typename Val<IC>::T* in, int64_t ldi, int64_t ti, typename Val<OC>::T* out,
                                           int64_t ldo, int64_t to, double th, int N, int layout, int nl, int cb, double sgn) {
    using TI = typename Val<IC>::T;
    for (int j = 0; j < nl; ++j) {          // m = 0: unchanged
        const int64_t k = layout == 0 ? (int64_t)j * j + j : 0;
        if constexpr (OC) out[k * ldo + to] = widen(in[k * ldi + ti]);
        else out[k * ldo + to] = in[k * ldi + ti];
    }
    for (int m = 1; m <= N; ++m) {
        double s, c;
        sincos((double)m * th, &s, &c);
        for (int nn = layout == 0 ? m : 0; nn < (layout == 0 ? N + 1 : 1); ++nn) {
            const int64_t p = layout == 0 ? (int64_t)nn * nn + nn + m : 2 * m;        // (n, m)
            const int64_t q = layout == 0 ? (int64_t)nn * nn + nn - m : 2 * m - 1;    // (n, -m)
            const TI a = in[p * ldi + ti], b = in[q * ldi + ti];
            if constexpr (OC) {
                const cplx ac = widen(a), bc = widen(b);
                if (cb) {   // exp(-i m t) and exp(+i m t)
                    out[p * ldo + to] = mk(c * ac.x + s * ac.y, c * ac.y - s * ac.x);
                    out[q * ldo + to] = mk(c * bc.x - s * bc.y, c * bc.y + s * bc.x);
                } else {
                    const double ss = sgn * s;
                    out[p * ldo + to] = mk(c * ac.x - ss * bc.x, c * ac.y - ss * bc.y);
                    out[q * ldo + to] = mk(c * bc.x + ss * ac.x, c * bc.y + ss * ac.y);
                }
            } else {
                const double ss = sgn * s;
                out[p * ldo + to] = c * a - ss * b;
                out[q * ldo + to] = c * b + ss * a;
            }
        }
    }
}

// The ENC form (encode_tile.hpp): the workgroup encodes its tile of ENC_T samples of the microphone block
// into LDS and its first ENC_T threads turn the tile from there, one sample each, with the arithmetic of the kernel above.
// EC: complex encoder, so a complex encoded signal.  grid (n / ENC_T, L); dynamic LDS enc_lds_bytes(C, M, EC, true)
template <bool EC, bool OC>
__global__ void __launch_bounds__(ENC_NT) rotate_yaw_enc_kernel(EncIn e, int C, int64_t n, int N, int layout, int cb, const double* __restrict__ yaw_,
                                                                int per_sample, void* __restrict__ out_, int64_t ldo, int64_t la, int64_t lo) {
    using TI = typename Val<EC>::T;
    using TO = typename Val<OC>::T;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    TI* enc_s = reinterpret_cast<TI*>(dyn);
    TI* tile = enc_s + C * e.M;   // [C][ENC_T]
    const int64_t t0 = (int64_t)blockIdx.x * ENC_T;
    encode_tile<EC>(e, C, t0, n, enc_s, [&](int c, int t, TI v) { tile[c * ENC_T + t] = v; });
    __syncthreads();
    const int64_t t = t0 + threadIdx.x;
    if (threadIdx.x >= ENC_T || t >= n) return;
    TO* __restrict__ out = reinterpret_cast<TO*>(out_) + (int64_t)blockIdx.y * lo;
    const double* __restrict__ yaw = yaw_ + (int64_t)blockIdx.y * la;
    const double th = fmod(yaw[per_sample ? t : 0], 2.0 * kPi);
    yaw_sample<EC, OC>(tile, ENC_T, threadIdx.x, out, ldo, t, th, N, layout, layout == 0 ? N + 1 : 1, cb, 1.0);
}

// the encoder alone (a push without angles): the encoded samples go from the registers to out [C][ldo].  grid (n / ENC_T)
template <bool EC>
__global__ void __launch_bounds__(ENC_NT) encode_kernel(EncIn e, int C, int64_t n, void* __restrict__ out_, int64_t ldo) {
    using TI = typename Val<EC>::T;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    TI* __restrict__ out = reinterpret_cast<TI*>(out_);
    const int64_t t0 = (int64_t)blockIdx.x * ENC_T;
    encode_tile<EC>(e, C, t0, n, reinterpret_cast<TI*>(dyn), [&](int c, int t, TI v) { out[(int64_t)c * ldo + t0 + t] = v; });
}

void enc_attributes() {
    static PerDeviceOnce once;
    if (!once.first()) return;
#define EMAGLS_ENC_ATTR(K) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024))
    EMAGLS_ENC_ATTR((rotate_yaw_enc_kernel<false, false>));
    EMAGLS_ENC_ATTR((rotate_yaw_enc_kernel<false, true>));
    EMAGLS_ENC_ATTR((rotate_yaw_enc_kernel<true, true>));
    EMAGLS_ENC_ATTR(encode_kernel<false>);
    EMAGLS_ENC_ATTR(encode_kernel<true>);
#undef EMAGLS_ENC_ATTR
}

void enc_check(const EncodeBlock& e, int C) {
    if (e.M < 1 || e.M > ENC_MAX || C < 1 || C > ENC_MAX) throw Error(2, "the stream's encoder supports 1 to 64 microphones and 1 to 64 channels");
}

}  // namespace

void launch_rotate_yaw(const void* in, bool in_cplx, int64_t n, int C, int layout, bool cplx_basis, const double* yaw, bool per_sample,
                       bool transpose, void* out, hipStream_t st, int64_t ld_in, int64_t ld_out, int L, int64_t la, int64_t lo) {
    if (n <= 0) return;
    const int64_t ldi = ld_in ? ld_in : n, ldo = ld_out ? ld_out : n;
    const int N = rotate_order(layout, C);
    if (N < 0) throw Error(1, "rotate_yaw: the channel count fits neither (N+1)^2 (SH) nor 2N+1 (CH)");
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 256), 65536), (unsigned)L);
    const double sgn = (transpose && !cplx_basis) ? -1.0 : 1.0;
    const int cb = cplx_basis ? 1 : 0, ps = per_sample ? 1 : 0;
    if (in_cplx) rotate_yaw_kernel<true, true><<<grid, 256, 0, st>>>(in, n, N, layout, cb, yaw, ps, sgn, out, ldi, ldo, la, lo);
    else if (cplx_basis) rotate_yaw_kernel<false, true><<<grid, 256, 0, st>>>(in, n, N, layout, cb, yaw, ps, sgn, out, ldi, ldo, la, lo);
    else rotate_yaw_kernel<false, false><<<grid, 256, 0, st>>>(in, n, N, layout, cb, yaw, ps, sgn, out, ldi, ldo, la, lo);
    KERNEL_CHECK();
}

void launch_encode_block(const EncodeBlock& e, int64_t n, int C, void* out, int64_t ld_out, hipStream_t st) {
    if (n <= 0) return;
    enc_check(e, C);
    enc_attributes();
    const EncIn in{e.enc, e.M, e.x, e.ldx};
    const unsigned grid = (unsigned)ceil_div(n, ENC_T);
    const size_t dyn = enc_lds_bytes(C, e.M, e.enc_cplx, false);
    if (e.enc_cplx) encode_kernel<true><<<grid, ENC_NT, dyn, st>>>(in, C, n, out, ld_out ? ld_out : n);
    else encode_kernel<false><<<grid, ENC_NT, dyn, st>>>(in, C, n, out, ld_out ? ld_out : n);
    KERNEL_CHECK();
}

void launch_rotate_yaw_encoded(const EncodeBlock& e, int64_t n, int C, int layout, bool cplx_basis, const double* yaw, bool per_sample, void* out,
                               hipStream_t st, int64_t ld_out, int L, int64_t la, int64_t lo) {
    if (n <= 0) return;
    enc_check(e, C);
    const int N = rotate_order(layout, C);
    if (N < 0) throw Error(1, "rotate_yaw: the channel count fits neither (N+1)^2 (SH) nor 2N+1 (CH)");
    enc_attributes();
    const EncIn in{e.enc, e.M, e.x, e.ldx};
    const dim3 grid((unsigned)ceil_div(n, ENC_T), (unsigned)L);
    const size_t dyn = enc_lds_bytes(C, e.M, e.enc_cplx, true);
    const int64_t ldo = ld_out ? ld_out : n;
    const int cb = cplx_basis ? 1 : 0, ps = per_sample ? 1 : 0;
    if (e.enc_cplx) rotate_yaw_enc_kernel<true, true><<<grid, ENC_NT, dyn, st>>>(in, C, n, N, layout, cb, yaw, ps, out, ldo, la, lo);
    else if (cplx_basis) rotate_yaw_enc_kernel<false, true><<<grid, ENC_NT, dyn, st>>>(in, C, n, N, layout, cb, yaw, ps, out, ldo, la, lo);
    else rotate_yaw_enc_kernel<false, false><<<grid, ENC_NT, dyn, st>>>(in, C, n, N, layout, cb, yaw, ps, out, ldo, la, lo);
    KERNEL_CHECK();
}

}  // namespace emagls
