// Rendered HRTFs of a design: Hhat_e(k, d) = sum_c W_e(k, c) pwGrid_k(c, d) for every bin, direction and
// ear, and the error metrics against reference HRTFs, reduced in the product's epilogue.
//   rh_split / rh_join   complex taps as two real planes through the real FFTs of fft.hip, and back
//   rh_modes             T(k, s) = (sum_c W(k, c) A(c, s)) b_n(s)(k), written as the K-major real operand of the product
//   rh_order_rows        T(k, (n, c)) = W(k, c) b_n(k): the left operand against the rotated order terms QT' of the EMAinSH model
//   rh_interleave        a complex right operand as real rows [2 s + re/im][d]
//   rh_gemm              Hhat = T conj(Y) on v_mfma_f64_16x16x4_f64 with the metric epilogue
//   rh_atf               the [2 x M] [M x D] product of the ATF model, thread = direction, the same epilogue
//   rh_reduce            partial sums over direction tiles, in tile order (no floating-point atomics anywhere)
#include <cfloat>

#include "kernels.hpp"

namespace emagls {

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) rh_split_kernel(const cplx* __restrict__ in, int64_t ncols, int64_t len, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ncols * len) return;
    const int64_t col = idx / len, t = idx - col * len;
    const cplx v = in[idx];
    out[(2 * col) * len + t] = v.x;
    out[(2 * col + 1) * len + t] = v.y;
}

// W[i] = F[2 i] + i F[2 i + 1]: the spectra of the real and the imaginary plane of one complex column
__global__ void __launch_bounds__(256) rh_join_kernel(const cplx* __restrict__ F, int64_t n, cplx* __restrict__ W) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cplx a = F[2 * i], b = F[2 * i + 1];
    W[i] = mk(a.x - b.y, a.y + b.x);
}

// Real rows of the product's left operand.  The four bins k = 4 t + q of tile t and their four components comp = (L re, L im,
// R re, R im) are the 16 rows 16 t + q + 4 comp: in the C/D layout of the 16 x 16 x 4 FP64 MFMA (row = (lane >> 4) + 4 reg) a
// lane then holds both ears of ONE bin and direction in its four registers, and the epilogue needs no lane exchange.
// Tt [Kpad][ldR], K-major like gemm_tn_f64's operands.  A complex basis doubles K: row 2 s meets Re Y_s, row 2 s + 1 meets Im Y_s,
//   Re Hhat = Re T Re Y + Im T Im Y,   Im Hhat = Im T Re Y - Re T Im Y      (Hhat = T conj(Y)).
// A (null: T = W, the SH model) is E of emagls_get_smair_matrix, [C][ldA]; bn [P][nOrd] with the sign of getSMAIRMatrix.m:107,
// real(b_n) in the last bin (:115-117).  Workgroup = one tile of one set; the bins past P are written as zeros.
template <typename TA>
__global__ void __launch_bounds__(256) rh_modes_kernel(const cplx* __restrict__ W, int C, int P, int Pp, const TA* __restrict__ A, int ldA,
                                                       const cplx* __restrict__ bn, int nOrd, int S, int y_cplx, double* __restrict__ Tt,
                                                       int64_t ldR) {
    __shared__ cplx Ws[8 * 256];   // C <= 256: SH order 15
    const int tile = blockIdx.x, set = blockIdx.y, k0 = 4 * tile;
    for (int i = threadIdx.x; i < 8 * C; i += blockDim.x) {
        const int c = i % C, qe = i / C, q = qe >> 1, ear = qe & 1, k = k0 + q;
        Ws[i] = k < P ? W[(((int64_t)set * 2 + ear) * P + k) * C + c] : mk(0.0, 0.0);
    }
    __syncthreads();
    const int r16 = threadIdx.x & 15, q = r16 & 3, comp = r16 >> 2, ear = comp >> 1, part = comp & 1, k = k0 + q;
    const cplx* w = Ws + (q * 2 + ear) * C;
    const int64_t row = ((int64_t)set * (Pp / 4) + tile) * 16 + r16;
    for (int s = threadIdx.x >> 4; s < S; s += 16) {
        cplx v = mk(0.0, 0.0);
        if (k < P) {
            if (A) {
                for (int c = 0; c < C; ++c) cfma(v, w[c], A[(size_t)c * ldA + s]);
            } else {
                v = w[s];
            }
            if (bn) {
                int n = (int)sqrt((double)s);
                while (n * n > s) --n;
                while ((n + 1) * (n + 1) <= s) ++n;
                cplx b = bn[(size_t)k * nOrd + n];
                if (k == P - 1) b.y = 0.0;
                v = v * b;
            }
        }
        if (!y_cplx) {
            Tt[(int64_t)s * ldR + row] = part ? v.y : v.x;
        } else {
            Tt[(int64_t)(2 * s) * ldR + row] = part ? v.y : v.x;
            Tt[(int64_t)(2 * s + 1) * ldR + row] = part ? -v.x : v.y;
        }
    }
}

// Left operand of the EMAinSH model (emash.hip): Hhat(k, d) = sum_n b_n(k) sum_c W(k, c) QT'_n(c, d), so row j = n C + c of the product
// holds W(k, c) b_n(k) in the row layout of rh_modes_kernel, bn as there.  QT' enters the product as it is, NOT conjugated like Y:
//   Re Hhat = Re T Re Q - Im T Im Q,   Im Hhat = Im T Re Q + Re T Im Q,
// so with a complex basis row 2 j + 1 (the one that meets Im Q_j) carries the opposite sign of rh_modes_kernel's.
// Workgroup = one tile of one set; the bins past P are written as zeros.
constexpr int RH_OR_CMAX = 64, RH_OR_NMAX = 86;   // SH order 7; simulation order 85, the entry point's limit
__global__ void __launch_bounds__(256) rh_order_rows_kernel(const cplx* __restrict__ W, int C, int P, int Pp, const cplx* __restrict__ bn, int nOrd,
                                                            int q_cplx, double* __restrict__ Tt, int64_t ldR) {
    __shared__ cplx Ws[8 * RH_OR_CMAX];
    __shared__ cplx Bs[4 * RH_OR_NMAX];
    const int tile = blockIdx.x, set = blockIdx.y, k0 = 4 * tile;
    for (int i = threadIdx.x; i < 8 * C; i += blockDim.x) {
        const int c = i % C, qe = i / C, q = qe >> 1, ear = qe & 1, k = k0 + q;
        Ws[i] = k < P ? W[(((int64_t)set * 2 + ear) * P + k) * C + c] : mk(0.0, 0.0);
    }
    for (int i = threadIdx.x; i < 4 * nOrd; i += blockDim.x) {
        const int n = i % nOrd, k = k0 + i / nOrd;
        cplx b = k < P ? bn[(size_t)k * nOrd + n] : mk(0.0, 0.0);
        if (k == P - 1) b.y = 0.0;
        Bs[i] = b;
    }
    __syncthreads();
    const int r16 = threadIdx.x & 15, q = r16 & 3, comp = r16 >> 2, ear = comp >> 1, part = comp & 1;
    const cplx* w = Ws + (q * 2 + ear) * C;
    const cplx* b = Bs + q * nOrd;
    const int64_t row = ((int64_t)set * (Pp / 4) + tile) * 16 + r16;
    const int J = nOrd * C;
    for (int j = threadIdx.x >> 4; j < J; j += 16) {
        const int n = j / C, c = j - n * C;
        const cplx v = w[c] * b[n];
        if (!q_cplx) {
            Tt[(int64_t)j * ldR + row] = part ? v.y : v.x;
        } else {
            Tt[(int64_t)(2 * j) * ldR + row] = part ? v.y : v.x;
            Tt[(int64_t)(2 * j + 1) * ldR + row] = part ? v.x : -v.y;
        }
    }
}

// Yk[2 s + re/im][d] from the complex basis Y [S][ldi]
__global__ void __launch_bounds__(256) rh_interleave_kernel(const cplx* __restrict__ Y, int64_t ldi, int S, int64_t D, double* __restrict__ Yk,
                                                            int64_t ldo) {
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = blockIdx.y;
    if (d >= D || s >= S) return;
    const cplx v = Y[(int64_t)s * ldi + d];
    Yk[(int64_t)(2 * s) * ldo + d] = v.x;
    Yk[(int64_t)(2 * s + 1) * ldo + d] = v.y;
}

// what the epilogue of either product needs
struct RhEpi {
    const cplx* H;          // reference spectra [hset][2][P][D] (null: no metrics)
    int64_t hset_stride;    // elements between the HRIR sets (0: one set for every filter set)
    const double* w;        // direction weights [D], normalised
    cplx* Hhat;             // [set][2][P][D] (null: not stored)
    double* partial;        // [set][P][ntile][RH_NM]
    int ntile, P;
    int64_t D;
};

constexpr int RH_NM = 11;   // |dB| L, |dB| R, |ILD error|, cov_hat (LL, RR, Re LR, Im LR), cov_ref (the same four)

__device__ __forceinline__ double rh_db(cplx v) { return 20.0 * log10(fmax(cabs(v), DBL_MIN)); }

// t += w (the RH_NM terms of one direction)
__device__ __forceinline__ void rh_terms(cplx aL, cplx aR, cplx hL, cplx hR, double w, double* t) {
    const double daL = rh_db(aL), daR = rh_db(aR), dhL = rh_db(hL), dhR = rh_db(hR);
    t[0] += w * fabs(daL - dhL);
    t[1] += w * fabs(daR - dhR);
    t[2] += w * fabs((daL - daR) - (dhL - dhR));
    t[3] += w * norm2(aL);
    t[4] += w * norm2(aR);
    t[5] += w * (aL.x * aR.x + aL.y * aR.y);     // aL conj(aR)
    t[6] += w * (aL.y * aR.x - aL.x * aR.y);
    t[7] += w * norm2(hL);
    t[8] += w * norm2(hR);
    t[9] += w * (hL.x * hR.x + hL.y * hR.y);
    t[10] += w * (hL.y * hR.x - hL.x * hR.y);
}

// Hhat = T conj(Y) as ONE real product: rows = the real rows of rh_modes_kernel, K = S (real basis) or 2 S.  Workgroup = 4 waves =
// 16 bins of one set x 64 directions, each wave 2 x 2 tiles of v_mfma_f64_16x16x4_f64 (8 bins x 32 directions) with the operands
// straight from global memory, as gemm_tn_f64_kernel reads them: 16 lanes of an operand read 128 contiguous bytes.  Both operands
// are this call's scratch, padded with zeros to whole tiles and K to a multiple of 4, so the loop carries no bounds test; the
// caller's arrays (Hhat, H, weights) are touched under a predicate.
// The tile is gemm_tn_f64's.  DESIGN.md section 5 measured that the 4x4x4_4b shape outruns this one on gfx950; whether the
// epilogue's registers (11 partial sums, four logarithms in flight next to 16 accumulators) leave room for a wider tile has NOT
// been measured -- this is the smallest tile that keeps the two ears of a bin in one lane.
// A wave reduces its 32 directions itself (DPP inside the 16-lane row of a bin, the two column tiles in the lane), so a direction
// tile of `partial` is one wave's and no LDS is used.
__global__ void __launch_bounds__(256) rh_gemm_kernel(const double* __restrict__ Tt, int64_t ldR, const double* __restrict__ Yk, int64_t ldY,
                                                      int K, int Pp, RhEpi e) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ii = lane & 15, kk = lane >> 4;
    const int set = blockIdx.z;
    const int kb0 = (int)blockIdx.y * 16 + (wave >> 1) * 8;
    const int64_t d0 = (int64_t)blockIdx.x * 64 + (wave & 1) * 32;
    double4_t acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = double4_t{0.0, 0.0, 0.0, 0.0};
    const double* pa = Tt + (int64_t)kk * ldR + ((int64_t)set * Pp + kb0) * 4 + ii;
    const double* pb = Yk + (int64_t)kk * ldY + d0 + ii;
#pragma unroll 4
    for (int k = 0; k < K; k += 4) {
        const double a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
        pa += 4 * ldR; pb += 4 * ldY;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    const cplx* H = e.H ? e.H + (int64_t)set * e.hset_stride : nullptr;
    const int tileD = (int)blockIdx.x * 2 + (wave & 1);
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int k = kb0 + 4 * x + kk;
        double t[RH_NM];
#pragma unroll
        for (int m = 0; m < RH_NM; ++m) t[m] = 0.0;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int64_t d = d0 + 16 * y + ii;
            if (k >= e.P || d >= e.D) continue;
            const cplx aL = mk(acc[x][y][0], acc[x][y][1]), aR = mk(acc[x][y][2], acc[x][y][3]);
            const int64_t iL = ((int64_t)k) * e.D + d, iR = ((int64_t)e.P + k) * e.D + d;
            if (e.Hhat) {
                cplx* o = e.Hhat + (int64_t)set * 2 * e.P * e.D;
                stream_store(o + iL, aL);
                stream_store(o + iR, aR);
            }
            if (H) rh_terms(aL, aR, H[iL], H[iR], e.w[d], t);
        }
        if (H) {   // (uniform: every lane takes part in the row sums)
#pragma unroll
            for (int m = 0; m < RH_NM; ++m) t[m] = group_sum<16>(t[m]);
            if (ii == 0 && k < e.P) {
                double* p = e.partial + (((int64_t)set * e.P + k) * e.ntile + tileD) * RH_NM;
#pragma unroll
                for (int m = 0; m < RH_NM; ++m) p[m] = t[m];
            }
        }
    }
}

// ATF model: Hhat_e(k, d) = sum_m W_e(k, m) A(k, m, d).  A [P][M][D], W [set][2][P][M]; thread = direction, bin = blockIdx.y,
// set = blockIdx.z; a direction tile of `partial` is one wave's 64 directions.
__global__ void __launch_bounds__(256) rh_atf_kernel(const cplx* __restrict__ W, const cplx* __restrict__ A, int M, RhEpi e) {
    __shared__ cplx Ws[2 * 64];
    const int k = blockIdx.y, set = blockIdx.z;
    for (int i = threadIdx.x; i < 2 * M; i += blockDim.x) {
        const int ear = i / M, m = i - ear * M;
        Ws[i] = W[(((int64_t)set * 2 + ear) * e.P + k) * M + m];
    }
    __syncthreads();
    const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = d < e.D;
    cplx aL = mk(0.0, 0.0), aR = mk(0.0, 0.0);
    double t[RH_NM];
#pragma unroll
    for (int m = 0; m < RH_NM; ++m) t[m] = 0.0;
    const cplx* H = e.H ? e.H + (int64_t)set * e.hset_stride : nullptr;
    if (valid) {
        const cplx* a = A + (int64_t)k * M * e.D + d;
        for (int m = 0; m < M; ++m) {
            const cplx v = a[(int64_t)m * e.D];
            cfma(aL, Ws[m], v);
            cfma(aR, Ws[M + m], v);
        }
        const int64_t iL = ((int64_t)k) * e.D + d, iR = ((int64_t)e.P + k) * e.D + d;
        if (e.Hhat) {
            cplx* o = e.Hhat + (int64_t)set * 2 * e.P * e.D;
            stream_store(o + iL, aL);
            stream_store(o + iR, aR);
        }
        if (H) rh_terms(aL, aR, H[iL], H[iR], e.w[d], t);
    }
    if (H) {
#pragma unroll
        for (int m = 0; m < RH_NM; ++m) t[m] = wave_sum(t[m]);
        if ((threadIdx.x & 63) == 0) {
            double* p = e.partial + (((int64_t)set * e.P + k) * e.ntile + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RH_NM;
#pragma unroll
            for (int m = 0; m < RH_NM; ++m) p[m] = t[m];
        }
    }
}

// out[(set P + k) RH_NM + m] = the direction tiles of partial summed in tile order: one thread per (set, k, m)
__global__ void __launch_bounds__(256) rh_reduce_kernel(const double* __restrict__ partial, int64_t n, int ntile, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int64_t sk = idx / RH_NM;
    const int m = (int)(idx - sk * RH_NM);
    const double* p = partial + sk * ntile * RH_NM + m;
    double acc = 0.0;
    for (int t = 0; t < ntile; ++t) acc += p[(int64_t)t * RH_NM];
    out[idx] = acc;
}

}  // namespace

int rh_num_metrics() { return RH_NM; }
int rh_bins_padded(int P) { return (int)(ceil_div(P, 16) * 16); }
int rh_gemm_tiles(int64_t D) { return (int)(2 * ceil_div(D, 64)); }
int rh_atf_tiles(int64_t D) { return (int)(4 * ceil_div(D, 256)); }

void launch_rh_split(const void* in, int64_t ncols, int64_t len, double* out, hipStream_t st) {
    rh_split_kernel<<<(unsigned)ceil_div(ncols * len, 256), 256, 0, st>>>((const cplx*)in, ncols, len, out);
    KERNEL_CHECK();
}

void launch_rh_join(const void* F, int64_t n, void* W, hipStream_t st) {
    rh_join_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>((const cplx*)F, n, (cplx*)W);
    KERNEL_CHECK();
}

void launch_rh_modes(const void* W, int C, int P, int nsets, const void* A, bool a_cplx, int ldA, const void* bn, int nOrd, int S, bool y_cplx,
                     double* Tt, int64_t ldR, hipStream_t st) {
    const int Pp = rh_bins_padded(P);
    const dim3 grid(Pp / 4, nsets);
    if (a_cplx)
        rh_modes_kernel<cplx><<<grid, 256, 0, st>>>((const cplx*)W, C, P, Pp, (const cplx*)A, ldA, (const cplx*)bn, nOrd, S, y_cplx ? 1 : 0, Tt, ldR);
    else
        rh_modes_kernel<double><<<grid, 256, 0, st>>>((const cplx*)W, C, P, Pp, (const double*)A, ldA, (const cplx*)bn, nOrd, S, y_cplx ? 1 : 0, Tt, ldR);
    KERNEL_CHECK();
}

void launch_rh_order_rows(const void* W, int C, int P, int nsets, const void* bn, int nOrd, bool q_cplx, double* Tt, int64_t ldR, hipStream_t st) {
    if (C > RH_OR_CMAX || nOrd > RH_OR_NMAX) throw Error(2, "rendered HRTFs: order rows of more than 64 channels or 86 orders");
    const int Pp = rh_bins_padded(P);
    rh_order_rows_kernel<<<dim3(Pp / 4, nsets), 256, 0, st>>>((const cplx*)W, C, P, Pp, (const cplx*)bn, nOrd, q_cplx ? 1 : 0, Tt, ldR);
    KERNEL_CHECK();
}

void launch_rh_interleave(const void* Y, int64_t ldi, int S, int64_t D, double* Yk, int64_t ldo, hipStream_t st) {
    rh_interleave_kernel<<<dim3((unsigned)ceil_div(D, 256), S), 256, 0, st>>>((const cplx*)Y, ldi, S, D, Yk, ldo);
    KERNEL_CHECK();
}

static RhEpi rh_epi(const RhOut& o, int ntile, int P, int64_t D) {
    RhEpi e{};
    e.H = (const cplx*)o.H; e.hset_stride = o.hset_stride; e.w = o.w; e.Hhat = (cplx*)o.Hhat; e.partial = o.partial;
    e.ntile = ntile; e.P = P; e.D = D;
    return e;
}

void launch_rh_gemm(const double* Tt, int64_t ldR, const double* Yk, int64_t ldY, int K, int P, int64_t D, int nsets, const RhOut& o,
                    hipStream_t st) {
    const int Pp = rh_bins_padded(P);
    const dim3 grid((unsigned)ceil_div(D, 64), Pp / 16, nsets);
    rh_gemm_kernel<<<grid, 256, 0, st>>>(Tt, ldR, Yk, ldY, K, Pp, rh_epi(o, rh_gemm_tiles(D), P, D));
    KERNEL_CHECK();
}

void launch_rh_atf(const void* W, const void* A, int M, int P, int64_t D, int nsets, const RhOut& o, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(D, 256), P, nsets);
    rh_atf_kernel<<<grid, 256, 0, st>>>((const cplx*)W, (const cplx*)A, M, rh_epi(o, rh_atf_tiles(D), P, D));
    KERNEL_CHECK();
}

void launch_rh_reduce(const double* partial, int64_t nrows, int ntile, double* out, hipStream_t st) {
    const int64_t n = nrows * RH_NM;
    rh_reduce_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(partial, n, ntile, out);
    KERNEL_CHECK();
}

}  // namespace emagls
