// Array impulse responses: plane-wave components through the simulated rigid-sphere array (the host entry is
// array_irs_api.hip).  Per source q, microphone m and bin k
//
//   H_q(k, m) = sum_j g_j exp(-2 pi i k d_j / nfft) sum_{n <= N} b'_n(k) P_n(u_j . v_m),    b'_n(k) = -b_n(k r) (2n+1) / (4 pi),
//
// the column pwGrid_k(:, dir_j) of the emagls2 operand by the addition theorem (dependencies/getSMAIRMatrix.m:102-121), delayed by
// d_j = tau_j + tau_0 samples.  The work is ncomp * M * P * (N+1) complex-by-real multiply-adds in FP64, so the main kernel is a vector
// kernel in the manner of sweep_reg.hip: a wave owns one microphone and AIR_R consecutive bins, the b' of those bins come through
// wave-uniform loads (the four waves of a workgroup share the bins and take four microphones), and one three-term Legendre
// recurrence per component feeds AIR_R complex accumulators.  Then the phases: one sincospi for the block's first bin, one for the
// step, AIR_R - 1 complex products; the integer part of d_j is multiplied with k modulo nfft in integers, so the argument is exact
// at nfft = 65536.
//
// TWO FORMS, chosen PER SOURCE by its own component count J_q (so that a source's bits do not depend on its neighbours):
//   J_q >  AIR_LANE_SOURCE_MAX   lane = component: a lane sums the components j = lane, lane + 64, ... in that order, one wave
//                                reduction (wave_sum: DPP inside the rows, then the four rows in a fixed order) per bin
//   J_q <= AIR_LANE_SOURCE_MAX   lane = source: the short sources of a call are listed, a lane walks its own source's components in
//                                order, no reduction (a direction bank is J = 1 for thousands of sources; an empty source gives zeros)
// No atomics; every order is fixed.
//
// THE SPECTRAL GAIN: with W <= 8 surfaces of real reflection spectra R_w(k), integer exponents e_jw >= 0 per
// component, and optionally an attenuation alpha(k) in Np/m and a path length l_j, g_j becomes
//   G_j(k) = g_j prod_w R_w(k)^e_jw exp(-alpha(k) l_j) = g_j (-1)^(number of w with R_w(k) < 0 and e_jw odd) exp(sum_w e_jw ln|R_w(k)| - alpha(k) l_j).
// It depends on component and bin, so it is formed inside the main kernel, in a kernel of its own (air_two_mics_kernel, both forms;
// the flat kernels are not touched): the per-bin tables ln|R_w|, the sign bits and alpha come wave-uniformly next to b'
// (air_spectra_kernel writes them with the padding of Pld), the exponents and the path are per-lane loads, and one exp per
// (component, bin) does the rest.  ln|0| is stored as AIR_LN_ZERO, large, finite and negative: e = 0 gives the factor exp(-0) = 1,
// e > 0 gives exp(-huge) = 0 exactly.  A wave owns TWO microphones there, which share G, the phases and the loads of b': measured
// against one microphone per wave and against binary powers per surface in profiles/r27_room_spectral.md.  Per microphone the
// operations and their order are those of the flat kernel with G_r w_r in the place of (g w)_r.
//
// POINT SOURCES (section 14) and SOURCE DIRECTIVITY (section 15) have main kernels of their own further down, each with a heading
// that says what it adds; the kernels above them are not touched by either.
//
// The rest of the chain: air_modes_kernel (the factor (2n+1) on launch_modal_bn's output, real part in the last bin, and the
// recurrence's coefficients), air_prepare_kernel (unit vectors, delays split into integer and fraction), and the inverse real
// transform per (source, channel) with the encoder in its load: on the LDS passes of lds_fft.hpp up to nfft = 4096
// (air_irfft_kernel), through hipFFT's Z2D above (air_encode_kernel, air_pick_kernel around it).
#include "kernels.hpp"
#include "lds_fft.hpp"

namespace emagls {

constexpr int AIR_R = 8;   // bins per wave

// rec[2 n] = (2n+1)/(n+1), rec[2 n + 1] = n/(n+1): P_(n+1) = rec[2n] x P_n - rec[2n+1] P_(n-1).  bn [N+1][Pld] comes as
// -b_n / (4 pi) (launch_modal_bn's out_scale) with zeros beyond P.
__global__ void __launch_bounds__(256) air_modes_kernel(int N, int P, int64_t Pld, cplx* __restrict__ bn, double* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= N) {
        rec[2 * i] = (double)(2 * i + 1) / (double)(i + 1);
        rec[2 * i + 1] = (double)i / (double)(i + 1);
    }
    if (i >= (int64_t)(N + 1) * P) return;
    const int n = (int)(i / P), k = (int)(i % P);
    cplx v = bn[(int64_t)n * Pld + k];
    const double s = (double)(2 * n + 1);
    v.x *= s;
    v.y = k == P - 1 ? 0.0 : v.y * s;   // getSMAIRMatrix.m:115-117
    bn[(int64_t)n * Pld + k] = v;
}

// unit vectors [3][n] of directions (azimuth, zenith)
__global__ void __launch_bounds__(256) air_units_kernel(int64_t n, const double* __restrict__ azi, const double* __restrict__ zen,
                                                       double* __restrict__ u) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sa, ca, sz, cz;
    sincos(azi[i], &sa, &ca);
    sincos(zen[i], &sz, &cz);
    u[i] = sz * ca; u[n + i] = sz * sa; u[2 * n + i] = cz;
}

// d_j = tau_j + tau_0 as an integer below nfft and a fraction in [0, 1): the integer parts are added as integers, the fractions as
// doubles (the host has checked 0 <= d_j <= nfft - 1)
__global__ void __launch_bounds__(256) air_delays_kernel(int64_t n, const double* __restrict__ delay, double pre_delay, int nfft,
                                                        int* __restrict__ dint, double* __restrict__ dfrac) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = delay ? delay[i] : 0.0;
    const double ti = floor(t), pi = floor(pre_delay);
    const double f = (t - ti) + (pre_delay - pi), fi = floor(f);
    dint[i] = (int)(((int64_t)ti + (int64_t)pi + (int64_t)fi) & (nfft - 1));
    dfrac[i] = f - fi;
}

struct AirArgs {
    const cplx* bn;        // [N+1][Pld]
    const double* rec;     // [2 (N+1)]
    const double* u;       // [3][ncomp]
    const double* v;       // [3][M]
    const int* dint;       // [ncomp]
    const double* dfrac;   // [ncomp]
    const double* gain;    // [ncomp] or null
    const int64_t* ptr;    // [Q+1]
    const int* list;       // the sources of this launch
    int nlist, N, M, P, nfft;
    int64_t Pld, ncomp;
    cplx* H;               // [Q][M][Pld]
};

constexpr double AIR_LN_ZERO = -1.0e300;   // stands for ln|0|: 0 * AIR_LN_ZERO = -0, e * AIR_LN_ZERO <= -1e300 for e >= 1

struct AirArgsSpectral : AirArgs {
    const double* lnr;     // [W][Pld] ln|R_w(k)|, AIR_LN_ZERO where R_w(k) = 0, zeros beyond P
    const unsigned* neg;   // [Pld] bit w: R_w(k) < 0
    const double* att;     // [Pld] alpha(k), zeros beyond P; null (with path): no air term
    const int* exp;        // [ncomp][W]
    const double* path;    // [ncomp]
    int W;
};

// the tables of the spectral gain from refl [W][P] and att [P] (or null); grid over Pld
__global__ void __launch_bounds__(256) air_spectra_kernel(int W, int P, int64_t Pld, const double* __restrict__ refl, const double* __restrict__ att,
                                                         double* __restrict__ lnr, unsigned* __restrict__ neg, double* __restrict__ attp) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= Pld) return;
    unsigned bits = 0;
    for (int w = 0; w < W; ++w) {
        const double r = k < P ? refl[(int64_t)w * P + k] : 1.0;
        if (r < 0.0) bits |= 1u << w;
        lnr[(int64_t)w * Pld + k] = r == 0.0 ? AIR_LN_ZERO : log(fabs(r));
    }
    neg[k] = bits;
    if (att) attp[k] = k < P ? att[k] : 0.0;
}

// the spectral gains of component j in the AIR_R bins from k0: G[r] = +-g exp(sum_w e_w ln|R_w(k0 + r)| - alpha(k0 + r) l), the
// arguments summed first (the surfaces ascending on top of the air term), the sign from the bins' masks and the exponents' parities
__device__ __forceinline__ void air_gains(const AirArgsSpectral& a, int k0, int64_t j, double g, double (&G)[AIR_R]) {
    const double len = a.att ? a.path[j] : 0.0;
    const int* __restrict__ e = a.exp + j * a.W;
    const double* __restrict__ l = a.lnr + k0;
    double arg[AIR_R];
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) arg[r] = a.att ? -(a.att[k0 + r] * len) : 0.0;
    unsigned odd = 0;
    for (int t = 0; t < a.W; ++t, l += a.Pld) {
        const int et = e[t];
        const double ed = (double)et;
        odd |= (unsigned)(et & 1) << t;
#pragma unroll
        for (int r = 0; r < AIR_R; ++r) arg[r] = fma(ed, l[r], arg[r]);
    }
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) G[r] = ((__popc(a.neg[k0 + r] & odd) & 1) ? -g : g) * exp(arg[r]);
}

// the same for the two microphones of a wave, which share G, the phases and the loads of b': sum[i][r] += G_r w_r sum_n b'_n P_n(x_i)
__device__ __forceinline__ void air_component2(const AirArgsSpectral& a, int k0, int64_t j, const double (&vx)[2], const double (&vy)[2],
                                               const double (&vz)[2], cplx (&sum)[2][AIR_R]) {
    const double ux = a.u[j], uy = a.u[a.ncomp + j], uz = a.u[2 * a.ncomp + j];
    const double x0 = fma(uz, vz[0], fma(uy, vy[0], ux * vx[0])), x1 = fma(uz, vz[1], fma(uy, vy[1], ux * vx[1]));
    cplx acc0[AIR_R], acc1[AIR_R];
    const cplx* __restrict__ b = a.bn + k0;
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) acc0[r] = acc1[r] = b[r];   // n = 0: P_0 = 1
    double p0 = 1.0, p1 = x0, q0 = 1.0, q1 = x1;
    for (int n = 1; n <= a.N; ++n) {
        b += a.Pld;
#pragma unroll
        for (int r = 0; r < AIR_R; ++r) { cfma(acc0[r], b[r], p1); cfma(acc1[r], b[r], q1); }
        const double p2 = fma(a.rec[2 * n] * x0, p1, -(a.rec[2 * n + 1] * p0)), q2 = fma(a.rec[2 * n] * x1, q1, -(a.rec[2 * n + 1] * q0));
        p0 = p1; p1 = p2; q0 = q1; q1 = q2;
    }
    const unsigned di = (unsigned)a.dint[j];
    const double df = a.dfrac[j], inv = 1.0 / (double)a.nfft, g = a.gain ? a.gain[j] : 1.0;
    const unsigned ki = ((unsigned)k0 * di) & (unsigned)(a.nfft - 1);
    cplx w, s;
    sincospi(-2.0 * (((double)ki + (double)k0 * df) * inv), &w.y, &w.x);
    sincospi(-2.0 * (((double)di + df) * inv), &s.y, &s.x);
    double G[AIR_R];
    air_gains(a, k0, j, g, G);
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) {
        const cplx gw = G[r] * w;
        cfma(sum[0][r], gw, acc0[r]);
        cfma(sum[1][r], gw, acc1[r]);
        w = w * s;
    }
}

// the two forms with two microphones per wave: grid.y = ceil(M / 8), wave w takes the microphones 8 blockIdx.y + 2 w and the next
// (an odd M's last wave computes its one microphone twice and stores it once)
template <bool LANE_IS_SOURCE>
__global__ void __launch_bounds__(256) air_two_mics_kernel(AirArgsSpectral a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m0 = blockIdx.y * 8 + 2 * wave;
    if (m0 >= a.M) return;
    const int m1 = m0 + 1 < a.M ? m0 + 1 : m0, k0 = blockIdx.x * AIR_R;
    int q;
    if (LANE_IS_SOURCE) {
        const int i = blockIdx.z * 64 + lane;
        if (i >= a.nlist) return;
        q = a.list[i];
    } else {
        q = a.list[blockIdx.z];
    }
    const double vx[2] = {a.v[m0], a.v[m1]}, vy[2] = {a.v[a.M + m0], a.v[a.M + m1]}, vz[2] = {a.v[2 * a.M + m0], a.v[2 * a.M + m1]};
    cplx sum[2][AIR_R];
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) sum[0][r] = sum[1][r] = mk(0.0, 0.0);
    const int64_t j1 = a.ptr[q + 1];
    for (int64_t j = a.ptr[q] + (LANE_IS_SOURCE ? 0 : lane); j < j1; j += LANE_IS_SOURCE ? 1 : 64) air_component2(a, k0, j, vx, vy, vz, sum);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (i == 1 && m1 == m0) break;
        cplx* out = a.H + ((int64_t)q * a.M + (i ? m1 : m0)) * a.Pld;
#pragma unroll
        for (int r = 0; r < AIR_R; ++r) {
            cplx t = LANE_IS_SOURCE ? sum[i][r] : wave_sum(sum[i][r]);
            const int k = k0 + r;
            if (k == a.P - 1) t.y = 0.0;   // the last bin's value is the real part of the sum
            if ((LANE_IS_SOURCE || lane == 0) && k < a.P) out[k] = t;
        }
    }
}

// one component's terms of the AIR_R bins from k0: sum[r] += g w_r sum_n b'_n(k0 + r) P_n(x)
__device__ __forceinline__ void air_component(const AirArgs& a, int k0, int64_t j, double vx, double vy, double vz, cplx (&sum)[AIR_R]) {
    const double x = fma(a.u[2 * a.ncomp + j], vz, fma(a.u[a.ncomp + j], vy, a.u[j] * vx));
    cplx acc[AIR_R];
    const cplx* __restrict__ b = a.bn + k0;
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) acc[r] = b[r];   // n = 0: P_0 = 1
    double p0 = 1.0, p1 = x;
    for (int n = 1; n <= a.N; ++n) {
        b += a.Pld;
#pragma unroll
        for (int r = 0; r < AIR_R; ++r) cfma(acc[r], b[r], p1);
        const double p2 = fma(a.rec[2 * n] * x, p1, -(a.rec[2 * n + 1] * p0));
        p0 = p1; p1 = p2;
    }
    // phases in half turns: -2 ((k dint mod nfft) + k dfrac) / nfft
    const unsigned di = (unsigned)a.dint[j];
    const double df = a.dfrac[j], inv = 1.0 / (double)a.nfft, g = a.gain ? a.gain[j] : 1.0;
    const unsigned ki = ((unsigned)k0 * di) & (unsigned)(a.nfft - 1);
    cplx w, s;
    sincospi(-2.0 * (((double)ki + (double)k0 * df) * inv), &w.y, &w.x);
    sincospi(-2.0 * (((double)di + df) * inv), &s.y, &s.x);
    w = g * w;
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) {
        cfma(sum[r], w, acc[r]);
        w = w * s;
    }
}

// grid (bin blocks, ceil(M / 4), sources of the list); 256 threads: wave w takes the microphone 4 blockIdx.y + w
__global__ void __launch_bounds__(256) air_lane_component_kernel(AirArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = blockIdx.y * 4 + wave;
    if (m >= a.M) return;
    const int q = a.list[blockIdx.z], k0 = blockIdx.x * AIR_R;
    const double vx = a.v[m], vy = a.v[a.M + m], vz = a.v[2 * a.M + m];
    cplx sum[AIR_R];
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) sum[r] = mk(0.0, 0.0);
    const int64_t j1 = a.ptr[q + 1];
    for (int64_t j = a.ptr[q] + lane; j < j1; j += 64) air_component(a, k0, j, vx, vy, vz, sum);
    cplx* out = a.H + ((int64_t)q * a.M + m) * a.Pld;
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) {
        cplx t = wave_sum(sum[r]);
        const int k = k0 + r;
        if (k == a.P - 1) t.y = 0.0;   // the last bin's value is the real part of the sum
        if (lane == 0 && k < a.P) out[k] = t;
    }
}

// grid (bin blocks, ceil(M / 4), ceil(nlist / 64)): lane l takes the source list[64 blockIdx.z + l]
__global__ void __launch_bounds__(256) air_lane_source_kernel(AirArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m = blockIdx.y * 4 + wave;
    if (m >= a.M) return;
    const int i = blockIdx.z * 64 + lane, k0 = blockIdx.x * AIR_R;
    if (i >= a.nlist) return;
    const int q = a.list[i];
    const double vx = a.v[m], vy = a.v[a.M + m], vz = a.v[2 * a.M + m];
    cplx sum[AIR_R];
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) sum[r] = mk(0.0, 0.0);
    const int64_t j1 = a.ptr[q + 1];
    for (int64_t j = a.ptr[q]; j < j1; ++j) air_component(a, k0, j, vx, vy, vz, sum);
    cplx* out = a.H + ((int64_t)q * a.M + m) * a.Pld;
#pragma unroll
    for (int r = 0; r < AIR_R; ++r) {
        const int k = k0 + r;
        if (k == a.P - 1) sum[r].y = 0.0;
        if (k < a.P) out[k] = sum[r];
    }
}

// ---------------------------------------------------------------------------------------------
// POINT SOURCES: component j at the finite distance rho_j.  The order-n term gains the factor
//   F_n(x) = (-i)^(n+1) x e^(ix) h_n^(2)(x),  x = kappa_k rho_j,
// which turns "plane wave times e^(-i kappa rho) / rho" into the spherical wave about the array's centre.  F_n grows like
// (2n-1)!! / x^n below x = n and b'_n shrinks like (kappa r)^n / (2n+1)!!, so the kernel multiplies three tame numbers instead:
//   b'_n F_n P_n = bh_n(k) G_n(kappa_k rho_j) [(r / rho_j)^n P_n],    G_n(x) = F_n(x) (ix)^n / (2n-1)!!,  bh_n = b'_n (2n-1)!! / (i kappa r)^n,
//   G_0 = 1, G_1 = 1 + ix, G_(n+1) = G_n - x^2 / (4n^2 - 1) G_(n-1)    (the forward Hankel recurrence, real coefficient, exact at x = 0),
//   bh_0 = -e^(ix) / (1 + ix), bh_n = (2n+1) e^(ix) / (x^2 G_(n-1)(x) / (2n-1) - (n+1) G_n(x)),  x = kappa r    (no b_n, no y_n),
// and (r / rho)^n rides on the Legendre recurrence.  Bin 0 is x = 0: G = 1, bh_n = -(2n+1)/(n+1), the limit of the definition.
// A kernel of its own in both forms, the spectral gain a compile-time option; the plane-wave kernels above are not touched.
// ---------------------------------------------------------------------------------------------
#ifndef AIR_POINT_BINS
#define AIR_POINT_BINS 4      // bins per wave (divides AIR_R, the padding of Pld)
#endif
#ifndef AIR_POINT_MICS
#define AIR_POINT_MICS 4      // microphones per wave: they share G_n, bh_n G_n, the gain and the phases (measured against 1 and 2, and
                              // 4 bins against 2 and 8, in profiles/r28_point_sources.md)
#endif
constexpr int APT_R = AIR_POINT_BINS, APT_M = AIR_POINT_MICS;
static_assert(AIR_R % APT_R == 0, "the bins of a wave must divide the padding of Pld");

// one thread per bin of Pld: bh [N+1][Pld], ginv [N+1]
__global__ void __launch_bounds__(256) air_point_modes_kernel(int N, int P, int64_t Pld, double kr_step, cplx* __restrict__ bh,
                                                             double* __restrict__ ginv) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= N) ginv[k] = 1.0 / (4.0 * (double)k * (double)k - 1.0);
    if (k >= Pld) return;
    if (k >= P) {
        for (int n = 0; n <= N; ++n) bh[(int64_t)n * Pld + k] = mk(0.0, 0.0);
        return;
    }
    const double x = (double)k * kr_step, x2 = x * x;
    const bool last = k == P - 1;
    cplx e;
    sincos(x, &e.y, &e.x);
    cplx g0 = mk(1.0, 0.0), g1 = mk(1.0, x);
    cplx b = cdiv(-e, g1);
    if (last) b.y = 0.0;
    bh[k] = b;
    for (int n = 1; n <= N; ++n) {
        const double c = x2 / (double)(2 * n - 1), m = (double)(n + 1);
        const cplx den = mk(fma(c, g0.x, -(m * g1.x)), fma(c, g0.y, -(m * g1.y)));
        b = cdiv((double)(2 * n + 1) * e, den);
        if (last) { if (n & 1) b.x = 0.0; else b.y = 0.0; }   // (-i)^n Re(i^n bh_n): Re b'_n in the scaled form
        bh[(int64_t)n * Pld + k] = b;
        const double s = x2 / (4.0 * (double)n * (double)n - 1.0);
        const cplx g2 = mk(fma(-s, g0.x, g1.x), fma(-s, g0.y, g1.y));
        g0 = g1; g1 = g2;
    }
}

struct AirArgsPoint : AirArgsSpectral {
    const cplx* bh;        // [N+1][Pld]
    const double* ginv;    // [N+1]
    const double* dist;    // [ncomp]
    double r, kappa_step;
};

// air_gains for the APT_R bins of a point-source wave: the same operations in the same order per bin
__device__ __forceinline__ void air_point_gains(const AirArgsPoint& a, int k0, int64_t j, double g, double (&G)[APT_R]) {
    const double len = a.att ? a.path[j] : 0.0;
    const int* __restrict__ e = a.exp + j * a.W;
    const double* __restrict__ l = a.lnr + k0;
    double arg[APT_R];
#pragma unroll
    for (int r = 0; r < APT_R; ++r) arg[r] = a.att ? -(a.att[k0 + r] * len) : 0.0;
    unsigned odd = 0;
    for (int t = 0; t < a.W; ++t, l += a.Pld) {
        const int et = e[t];
        const double ed = (double)et;
        odd |= (unsigned)(et & 1) << t;
#pragma unroll
        for (int r = 0; r < APT_R; ++r) arg[r] = fma(ed, l[r], arg[r]);
    }
#pragma unroll
    for (int r = 0; r < APT_R; ++r) G[r] = ((__popc(a.neg[k0 + r] & odd) & 1) ? -g : g) * exp(arg[r]);
}

// one component's terms of the APT_R bins from k0 at the APT_M microphones of the wave:
// sum[i][r] += G_r w_r sum_n (bh_n(k0 + r) G_n(kappa_(k0 + r) rho)) (t^n P_n(x_i)),  t = r / rho
template <bool SPECTRAL>
__device__ __forceinline__ void air_point_component(const AirArgsPoint& a, int k0, int64_t j, const double (&vx)[APT_M], const double (&vy)[APT_M],
                                                    const double (&vz)[APT_M], cplx (&sum)[APT_M][APT_R]) {
    const double ux = a.u[j], uy = a.u[a.ncomp + j], uz = a.u[2 * a.ncomp + j];
    const double rho = a.dist[j], t = a.r / rho, t2 = t * t;
    double xm[APT_M], p0[APT_M], p1[APT_M];
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        xm[i] = t * fma(uz, vz[i], fma(uy, vy[i], ux * vx[i]));   // t x: t^(n+1) P_(n+1) = rec[2n] (t x) (t^n P_n) - rec[2n+1] t^2 (t^(n-1) P_(n-1))
        p0[i] = 1.0; p1[i] = xm[i];
    }
    const cplx* __restrict__ b = a.bh + k0;
    double x2[APT_R];
    cplx g0[APT_R], g1[APT_R], acc[APT_M][APT_R];
#pragma unroll
    for (int r = 0; r < APT_R; ++r) {
        const double x = ((double)(k0 + r) * a.kappa_step) * rho;
        x2[r] = x * x;
        g0[r] = mk(1.0, 0.0); g1[r] = mk(1.0, x);
#pragma unroll
        for (int i = 0; i < APT_M; ++i) acc[i][r] = b[r];   // n = 0: G_0 = 1, P_0 = 1
    }
    for (int n = 1; n <= a.N; ++n) {
        b += a.Pld;
        const double s = a.ginv[n];
#pragma unroll
        for (int r = 0; r < APT_R; ++r) {
            const cplx c = b[r] * g1[r];
#pragma unroll
            for (int i = 0; i < APT_M; ++i) cfma(acc[i][r], c, p1[i]);
            const double f = x2[r] * s;
            const cplx g2 = mk(fma(-f, g0[r].x, g1[r].x), fma(-f, g0[r].y, g1[r].y));
            g0[r] = g1[r]; g1[r] = g2;
        }
        const double ra = a.rec[2 * n], rb = a.rec[2 * n + 1] * t2;
#pragma unroll
        for (int i = 0; i < APT_M; ++i) {
            const double p2 = fma(ra * xm[i], p1[i], -(rb * p0[i]));
            p0[i] = p1[i]; p1[i] = p2;
        }
    }
    const unsigned di = (unsigned)a.dint[j];
    const double df = a.dfrac[j], inv = 1.0 / (double)a.nfft, g = a.gain ? a.gain[j] : 1.0;
    const unsigned ki = ((unsigned)k0 * di) & (unsigned)(a.nfft - 1);
    cplx w, s;
    sincospi(-2.0 * (((double)ki + (double)k0 * df) * inv), &w.y, &w.x);
    sincospi(-2.0 * (((double)di + df) * inv), &s.y, &s.x);
    double G[APT_R];
    if (SPECTRAL) {
        air_point_gains(a, k0, j, g, G);
    } else {
#pragma unroll
        for (int r = 0; r < APT_R; ++r) G[r] = g;
    }
#pragma unroll
    for (int r = 0; r < APT_R; ++r) {
        const cplx gw = G[r] * w;
#pragma unroll
        for (int i = 0; i < APT_M; ++i) cfma(sum[i][r], gw, acc[i][r]);
        w = w * s;
    }
}

// both forms: grid (Pld / APT_R, ceil(M / (4 APT_M)), sources of the list or ceil(nlist / 64)); wave w takes the microphones
// (4 blockIdx.y + w) APT_M + i (beyond M: the last one again, computed and not stored)
template <bool LANE_IS_SOURCE, bool SPECTRAL>
__global__ void __launch_bounds__(256) air_point_kernel(AirArgsPoint a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m0 = (blockIdx.y * 4 + wave) * APT_M;
    if (m0 >= a.M) return;
    const int k0 = blockIdx.x * APT_R;
    int q;
    if (LANE_IS_SOURCE) {
        const int i = blockIdx.z * 64 + lane;
        if (i >= a.nlist) return;
        q = a.list[i];
    } else {
        q = a.list[blockIdx.z];
    }
    double vx[APT_M], vy[APT_M], vz[APT_M];
    cplx sum[APT_M][APT_R];
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        const int m = m0 + i < a.M ? m0 + i : a.M - 1;
        vx[i] = a.v[m]; vy[i] = a.v[a.M + m]; vz[i] = a.v[2 * a.M + m];
#pragma unroll
        for (int r = 0; r < APT_R; ++r) sum[i][r] = mk(0.0, 0.0);
    }
    const int64_t j1 = a.ptr[q + 1];
    for (int64_t j = a.ptr[q] + (LANE_IS_SOURCE ? 0 : lane); j < j1; j += LANE_IS_SOURCE ? 1 : 64)
        air_point_component<SPECTRAL>(a, k0, j, vx, vy, vz, sum);
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        if (m0 + i >= a.M) break;
        cplx* out = a.H + ((int64_t)q * a.M + m0 + i) * a.Pld;
#pragma unroll
        for (int r = 0; r < APT_R; ++r) {
            cplx t = LANE_IS_SOURCE ? sum[i][r] : wave_sum(sum[i][r]);
            const int k = k0 + r;
            if (k == a.P - 1) t.y = 0.0;   // the last bin's value is the real part of the sum
            if ((LANE_IS_SOURCE || lane == 0) && k < a.P) out[k] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// SOURCE DIRECTIVITY: component j left its real source along the unit vector e_j (room axes); in the frame
// of source q, w_j = R_q^T e_j, and the component's gain gains the factor
//   D_j(k) = sum_{i < Kd} c_{q,i}(k) Y_i(w_j),    Y the real basis of sh_basis_kernel<false>, Kd = (Nd + 1)^2.
// air_emission_angles_kernel turns e_j into the angles of w_j, launch_sh_basis writes Yd [Kd][ncomp] from them (no second SH
// evaluator), and the main kernel forms D for the bins of its wave AFTER the order loop, when the accumulators' operands are dead:
// Kd steps of one per-lane load of Yd and one complex-by-real multiply-add per bin, the coefficients [Q][Kd][Pld] wave-uniform in
// the lane = component form and per lane in the lane = source form.  D depends on neither microphone nor order, so the APT_M
// microphones of a wave share it.  A kernel of its own with the point kernel's shape (APT_R bins, APT_M microphones per wave), in
// both forms, the spectral gain and the point-source factor compile-time options; the kernels above are not touched.
// ---------------------------------------------------------------------------------------------
struct AirArgsDir : AirArgsPoint {
    const double* Yd;      // [Kd][ncomp]
    const cplx* dc;        // [Q][Kd][Pld]
    int Kd;
};

// one thread per component: the source by bisection in ptr (ptr[q] <= j < ptr[q + 1]), then the angles of R_q^T e_j
__global__ void __launch_bounds__(256) air_emission_angles_kernel(int64_t n, int64_t nsrc, const int64_t* __restrict__ ptr,
                                                                 const double* __restrict__ emit, const double* __restrict__ rot,
                                                                 double* __restrict__ azi, double* __restrict__ zen) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    int64_t lo = 0, hi = nsrc;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= j) lo = mid; else hi = mid;
    }
    const double ex = emit[3 * j], ey = emit[3 * j + 1], ez = emit[3 * j + 2];
    double wx = ex, wy = ey, wz = ez;
    if (rot) {
        const double* __restrict__ R = rot + 9 * lo;   // the columns of R are the source's axes
        wx = fma(R[6], ez, fma(R[3], ey, R[0] * ex));
        wy = fma(R[7], ez, fma(R[4], ey, R[1] * ex));
        wz = fma(R[8], ez, fma(R[5], ey, R[2] * ex));
    }
    azi[j] = atan2(wy, wx);
    zen[j] = acos(fmin(1.0, fmax(-1.0, wz)));
}

#ifndef AIR_DIR_UNROLL
#define AIR_DIR_UNROLL 4       // steps of the D loop in flight together: left rolled (1) the loop waits for each step's two loads before its
                               // eight FMAs and costs twice as much at Nd = 8 (measured against 1 and 8 in profiles/r29_source_directivity.md);
                               // the order of the additions, and so the bits, do not depend on it
#endif
// D[r] = sum_i c_i(k0 + r) Y_i of component j: y walks Yd + j by ncomp, c walks the source's coefficients + k0 by Pld
__device__ __forceinline__ void air_directivity(const double* __restrict__ y, int64_t ncomp, const cplx* __restrict__ c, int64_t Pld, int Kd,
                                                cplx (&D)[APT_R]) {
#pragma unroll
    for (int r = 0; r < APT_R; ++r) D[r] = mk(0.0, 0.0);
#pragma unroll AIR_DIR_UNROLL
    for (int i = 0; i < Kd; ++i, y += ncomp, c += Pld) {
        const double yi = *y;
#pragma unroll
        for (int r = 0; r < APT_R; ++r) cfma(D[r], c[r], yi);
    }
}

// one component's terms of the APT_R bins from k0 at the APT_M microphones of the wave, plane wave or (POINT) point source:
// sum[i][r] += (G_r w_r) D_r acc[i][r], acc the order sum of the flat kernel or of air_point_component; dc: the coefficients of
// the component's source at bin k0
template <bool SPECTRAL, bool POINT>
__device__ __forceinline__ void air_directive_component(const AirArgsDir& a, int k0, int64_t j, const cplx* __restrict__ dc,
                                                        const double (&vx)[APT_M], const double (&vy)[APT_M], const double (&vz)[APT_M],
                                                        cplx (&sum)[APT_M][APT_R]) {
    const double ux = a.u[j], uy = a.u[a.ncomp + j], uz = a.u[2 * a.ncomp + j];
    const double rho = POINT ? a.dist[j] : 1.0, t = POINT ? a.r / rho : 1.0, t2 = t * t;
    double xm[APT_M], p0[APT_M], p1[APT_M];
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        const double x = fma(uz, vz[i], fma(uy, vy[i], ux * vx[i]));
        xm[i] = POINT ? t * x : x;
        p0[i] = 1.0; p1[i] = xm[i];
    }
    const cplx* __restrict__ b = (POINT ? a.bh : a.bn) + k0;
    double x2[APT_R];
    cplx g0[APT_R], g1[APT_R], acc[APT_M][APT_R];
#pragma unroll
    for (int r = 0; r < APT_R; ++r) {
        if constexpr (POINT) {
            const double x = ((double)(k0 + r) * a.kappa_step) * rho;
            x2[r] = x * x;
            g0[r] = mk(1.0, 0.0); g1[r] = mk(1.0, x);
        }
#pragma unroll
        for (int i = 0; i < APT_M; ++i) acc[i][r] = b[r];   // n = 0
    }
    for (int n = 1; n <= a.N; ++n) {
        b += a.Pld;
        if constexpr (POINT) {
            const double s = a.ginv[n];
#pragma unroll
            for (int r = 0; r < APT_R; ++r) {
                const cplx c = b[r] * g1[r];
#pragma unroll
                for (int i = 0; i < APT_M; ++i) cfma(acc[i][r], c, p1[i]);
                const double f = x2[r] * s;
                const cplx g2 = mk(fma(-f, g0[r].x, g1[r].x), fma(-f, g0[r].y, g1[r].y));
                g0[r] = g1[r]; g1[r] = g2;
            }
        } else {
#pragma unroll
            for (int r = 0; r < APT_R; ++r) {
#pragma unroll
                for (int i = 0; i < APT_M; ++i) cfma(acc[i][r], b[r], p1[i]);
            }
        }
        const double ra = a.rec[2 * n], rb = POINT ? a.rec[2 * n + 1] * t2 : a.rec[2 * n + 1];
#pragma unroll
        for (int i = 0; i < APT_M; ++i) {
            const double p2 = fma(ra * xm[i], p1[i], -(rb * p0[i]));
            p0[i] = p1[i]; p1[i] = p2;
        }
    }
    const unsigned di = (unsigned)a.dint[j];
    const double df = a.dfrac[j], inv = 1.0 / (double)a.nfft, g = a.gain ? a.gain[j] : 1.0;
    const unsigned ki = ((unsigned)k0 * di) & (unsigned)(a.nfft - 1);
    cplx w, s;
    sincospi(-2.0 * (((double)ki + (double)k0 * df) * inv), &w.y, &w.x);
    sincospi(-2.0 * (((double)di + df) * inv), &s.y, &s.x);
    double G[APT_R];
    if (SPECTRAL) {
        air_point_gains(a, k0, j, g, G);
    } else {
#pragma unroll
        for (int r = 0; r < APT_R; ++r) G[r] = g;
    }
    cplx D[APT_R];
    air_directivity(a.Yd + j, a.ncomp, dc, a.Pld, a.Kd, D);
#pragma unroll
    for (int r = 0; r < APT_R; ++r) {
        const cplx gw = (G[r] * w) * D[r];
#pragma unroll
        for (int i = 0; i < APT_M; ++i) cfma(sum[i][r], gw, acc[i][r]);
        w = w * s;
    }
}

// both forms, the grid and the microphones of a wave as in air_point_kernel
template <bool LANE_IS_SOURCE, bool SPECTRAL, bool POINT>
__global__ void __launch_bounds__(256) air_directive_kernel(AirArgsDir a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int m0 = (blockIdx.y * 4 + wave) * APT_M;
    if (m0 >= a.M) return;
    const int k0 = blockIdx.x * APT_R;
    int q;
    if (LANE_IS_SOURCE) {
        const int i = blockIdx.z * 64 + lane;
        if (i >= a.nlist) return;
        q = a.list[i];
    } else {
        q = a.list[blockIdx.z];
    }
    const cplx* __restrict__ dc = a.dc + (int64_t)q * a.Kd * a.Pld + k0;
    double vx[APT_M], vy[APT_M], vz[APT_M];
    cplx sum[APT_M][APT_R];
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        const int m = m0 + i < a.M ? m0 + i : a.M - 1;
        vx[i] = a.v[m]; vy[i] = a.v[a.M + m]; vz[i] = a.v[2 * a.M + m];
#pragma unroll
        for (int r = 0; r < APT_R; ++r) sum[i][r] = mk(0.0, 0.0);
    }
    const int64_t j1 = a.ptr[q + 1];
    for (int64_t j = a.ptr[q] + (LANE_IS_SOURCE ? 0 : lane); j < j1; j += LANE_IS_SOURCE ? 1 : 64)
        air_directive_component<SPECTRAL, POINT>(a, k0, j, dc, vx, vy, vz, sum);
#pragma unroll
    for (int i = 0; i < APT_M; ++i) {
        if (m0 + i >= a.M) break;
        cplx* out = a.H + ((int64_t)q * a.M + m0 + i) * a.Pld;
#pragma unroll
        for (int r = 0; r < APT_R; ++r) {
            cplx t = LANE_IS_SOURCE ? sum[i][r] : wave_sum(sum[i][r]);
            const int k = k0 + r;
            if (k == a.P - 1) t.y = 0.0;   // the last bin's value is the real part of the sum
            if ((LANE_IS_SOURCE || lane == 0) && k < a.P) out[k] = t;
        }
    }
}

// the encoder in a load: X(k) = sum_m enc(c, m) H(k, m), m ascending, accumulated from 0 with fma; the real and the imaginary part of
// enc as separate chains.  enc_re null: X = H(:, c)
struct AirEnc {
    const double* re;   // [C][M] column-major: enc(c, m) at c + C m
    const double* im;   // null: a real encoder
    int C, M;
};
__device__ __forceinline__ void air_encoded(const AirEnc& e, const cplx* __restrict__ Hq, int64_t Pld, int c, int k, cplx& zr, cplx& zi) {
    zi = mk(0.0, 0.0);
    if (!e.re) { zr = Hq[(int64_t)c * Pld + k]; return; }
    zr = mk(0.0, 0.0);
    for (int m = 0; m < e.M; ++m) {
        const cplx h = Hq[(int64_t)m * Pld + k];
        cfma(zr, e.re[c + e.C * m], h);
        if (e.im) cfma(zi, e.im[c + e.C * m], h);
    }
}

// out [Q][C][nr] (real, or interleaved complex with a complex encoder) = irfft over k at length nfft, first nr samples: one complex
// inverse transform of Z = X_re + i X_im, both Hermitian-extended (the imaginary parts of bin 0 and of the last bin do not enter, as
// in every inverse real transform).  grid (C, Q); LDS: the padded buffer and nfft / 2 twiddles
__global__ void __launch_bounds__(512) air_irfft_kernel(const cplx* __restrict__ H, int64_t Pld, AirEnc e, int nfft, int log2n,
                                                       const cplx* __restrict__ tw, int nr, void* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char air_smem[];
    cplx* buf = reinterpret_cast<cplx*>(air_smem);
    cplx* tws = buf + lds_fft_ix<true>(nfft);
    const int c = blockIdx.x, half = nfft >> 1;
    const int64_t q = blockIdx.y;
    const cplx* Hq = H + q * e.M * Pld;
    for (int j = threadIdx.x; j < half; j += blockDim.x) tws[j] = tw[j];
    for (int k = threadIdx.x; k <= half; k += blockDim.x) {
        cplx zr, zi;
        air_encoded(e, Hq, Pld, c, k, zr, zi);
        if (k == 0 || k == half) { zr.y = 0.0; zi.y = 0.0; }
        buf[lds_fft_ix<true>((int)bitrev((unsigned)k, log2n))] = mk(zr.x - zi.y, zr.y + zi.x);
        if (k > 0 && k < half) buf[lds_fft_ix<true>((int)bitrev((unsigned)(nfft - k), log2n))] = mk(zr.x + zi.y, zi.x - zr.y);
    }
    __syncthreads();
    lds_fft_stages<true, true>(buf, tws, nfft, log2n, 1);
    const double inv = 1.0 / (double)nfft;
    const int64_t o = (q * e.C + c) * nr;
    for (int t = threadIdx.x; t < nr; t += blockDim.x) {
        const cplx v = buf[lds_fft_ix<true>(t)];
        if (e.im) reinterpret_cast<cplx*>(out)[o + t] = mk(v.x * inv, v.y * inv);
        else reinterpret_cast<double*>(out)[o + t] = v.x * inv;
    }
}

// the long transforms: X [Q][planes][P] for hipFFT (planes = C, or 2 C: every channel's real-encoder and imaginary-encoder spectrum)
__global__ void __launch_bounds__(256) air_encode_kernel(const cplx* __restrict__ H, int64_t Pld, AirEnc e, int P, cplx* __restrict__ X) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, c = blockIdx.y, np = e.im ? 2 : 1;
    const int64_t q = blockIdx.z;
    if (k >= P) return;
    cplx zr, zi;
    air_encoded(e, H + q * e.M * Pld, Pld, c, k, zr, zi);
    if (k == 0 || k == P - 1) { zr.y = 0.0; zi.y = 0.0; }
    X[((q * e.C + c) * np) * P + k] = zr;
    if (e.im) X[((q * e.C + c) * np + 1) * P + k] = zi;
}

// y [Q C][np][nfft] (unscaled inverse transforms) -> out [Q C][nr], real (np = 1) or interleaved complex (np = 2)
__global__ void __launch_bounds__(256) air_pick_kernel(const double* __restrict__ y, int64_t rows, int np, int nfft, int nr, void* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = blockIdx.y;
    if (t >= nr || row >= rows) return;
    const double inv = 1.0 / (double)nfft;
    const double* yr = y + row * np * nfft;
    if (np == 2) reinterpret_cast<cplx*>(out)[row * nr + t] = mk(yr[t] * inv, yr[nfft + t] * inv);
    else reinterpret_cast<double*>(out)[row * nr + t] = yr[t] * inv;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
int air_bins_padded(int P) { return (int)(ceil_div(P, AIR_R) * AIR_R); }

void launch_air_modes(int N, int P, int64_t Pld, void* bn, double* rec, hipStream_t st) {
    air_modes_kernel<<<(unsigned)ceil_div(std::max<int64_t>((int64_t)(N + 1) * P, N + 1), 256), 256, 0, st>>>(N, P, Pld, (cplx*)bn, rec);
    KERNEL_CHECK();
}

void launch_air_units(int64_t n, const double* azi, const double* zen, double* u, hipStream_t st) {
    if (n <= 0) return;
    air_units_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, azi, zen, u);
    KERNEL_CHECK();
}

void launch_air_delays(int64_t n, const double* delay, double pre_delay, int nfft, int* dint, double* dfrac, hipStream_t st) {
    if (n <= 0) return;
    air_delays_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, delay, pre_delay, nfft, dint, dfrac);
    KERNEL_CHECK();
}

void launch_air_spectra(int W, int P, int64_t Pld, const double* refl, const double* att, double* lnr, unsigned* neg, double* attp,
                        hipStream_t st) {
    air_spectra_kernel<<<(unsigned)ceil_div(Pld, 256), 256, 0, st>>>(W, P, Pld, refl, att, lnr, neg, attp);
    KERNEL_CHECK();
}

// the source lists of both forms in slices (grid.z stops at 65535): kernel_long on slices of the long sources, kernel_short on 64
// short sources per grid.z
template <class Args, class KL, class KS>
static void air_main_launches(Args& a, const AirMain& m, unsigned gy, KL kernel_long, KS kernel_short, hipStream_t st, int bins = AIR_R) {
    a.bn = (const cplx*)m.bn; a.rec = m.rec; a.u = m.u; a.v = m.v; a.dint = m.dint; a.dfrac = m.dfrac; a.gain = m.gain; a.ptr = m.ptr;
    a.N = m.N; a.M = m.M; a.P = m.P; a.nfft = m.nfft; a.Pld = m.Pld; a.ncomp = m.ncomp; a.H = (cplx*)m.H;
    const unsigned gx = (unsigned)(m.Pld / bins);
    for (int i0 = 0; i0 < m.n_long; i0 += 65535) {
        a.list = m.list_long + i0; a.nlist = std::min(65535, m.n_long - i0);
        kernel_long<<<dim3(gx, gy, (unsigned)a.nlist), 256, 0, st>>>(a);
        KERNEL_CHECK();
    }
    for (int i0 = 0; i0 < m.n_short; i0 += 65535 * 64) {
        a.list = m.list_short + i0; a.nlist = std::min(65535 * 64, m.n_short - i0);
        kernel_short<<<dim3(gx, gy, (unsigned)ceil_div(a.nlist, 64)), 256, 0, st>>>(a);
        KERNEL_CHECK();
    }
}

void launch_air_point_modes(int N, int P, int64_t Pld, double kr_step, void* bh, double* ginv, hipStream_t st) {
    air_point_modes_kernel<<<(unsigned)ceil_div(std::max<int64_t>(Pld, N + 1), 256), 256, 0, st>>>(N, P, Pld, kr_step, (cplx*)bh, ginv);
    KERNEL_CHECK();
}

void launch_air_emission_angles(int64_t n, int64_t nsrc, const int64_t* ptr, const double* emit, const double* rot, double* azi, double* zen,
                                hipStream_t st) {
    if (n <= 0) return;
    air_emission_angles_kernel<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(n, nsrc, ptr, emit, rot, azi, zen);
    KERNEL_CHECK();
}

template <bool SPECTRAL, bool POINT>
static void air_directive_launches(AirArgsDir& a, const AirMain& m, hipStream_t st) {
    air_main_launches(a, m, (unsigned)ceil_div(m.M, 4 * APT_M), air_directive_kernel<false, SPECTRAL, POINT>, air_directive_kernel<true, SPECTRAL, POINT>,
                      st, APT_R);
}

void launch_air_main(const AirMain& m, hipStream_t st) {
    if (m.dc) {                                        // source directivity: one kernel, spectral gain and point sources its options
        AirArgsDir a{};
        a.lnr = m.lnr; a.neg = m.neg; a.att = m.att; a.exp = m.exp; a.path = m.path; a.W = m.nsurf;
        a.bh = (const cplx*)m.bh; a.ginv = m.ginv; a.dist = m.dist; a.r = m.mic_radius; a.kappa_step = m.kappa_step;
        a.Yd = m.Yd; a.dc = (const cplx*)m.dc; a.Kd = m.Kd;
        const bool spectral = m.nsurf > 0 || m.att;
        if (m.dist) spectral ? air_directive_launches<true, true>(a, m, st) : air_directive_launches<false, true>(a, m, st);
        else spectral ? air_directive_launches<true, false>(a, m, st) : air_directive_launches<false, false>(a, m, st);
    } else if (m.dist) {                                     // point sources: one kernel, the spectral gain its option
        AirArgsPoint a{};
        a.lnr = m.lnr; a.neg = m.neg; a.att = m.att; a.exp = m.exp; a.path = m.path; a.W = m.nsurf;
        a.bh = (const cplx*)m.bh; a.ginv = m.ginv; a.dist = m.dist; a.r = m.mic_radius; a.kappa_step = m.kappa_step;
        const unsigned gy = (unsigned)ceil_div(m.M, 4 * APT_M);
        if (m.nsurf > 0 || m.att) air_main_launches(a, m, gy, air_point_kernel<false, true>, air_point_kernel<true, true>, st, APT_R);
        else air_main_launches(a, m, gy, air_point_kernel<false, false>, air_point_kernel<true, false>, st, APT_R);
    } else if (m.nsurf > 0 || m.att) {
        AirArgsSpectral a{};
        a.lnr = m.lnr; a.neg = m.neg; a.att = m.att; a.exp = m.exp; a.path = m.path; a.W = m.nsurf;
        air_main_launches(a, m, (unsigned)ceil_div(m.M, 8), air_two_mics_kernel<false>, air_two_mics_kernel<true>, st);
    } else {
        AirArgs a{};
        air_main_launches(a, m, (unsigned)ceil_div(m.M, 4), air_lane_component_kernel, air_lane_source_kernel, st);
    }
}

static int air_log2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

void launch_air_irfft(const void* H, int64_t Pld, const double* enc_re, const double* enc_im, int C, int M, int64_t Q, int nfft,
                      const void* tw, int nr, void* out, hipStream_t st) {
    const AirEnc e{enc_re, enc_im, C, M};
    const size_t sm = sizeof(cplx) * ((size_t)nfft + (nfft >> 4) + (size_t)nfft / 2);   // (lds_fft_ix<true>(nfft) elements, and the twiddles)
    static PerDeviceOnce attr_once;   // (function attributes are per device)
    if (attr_once.first()) HIP_CHECK(hipFuncSetAttribute((const void*)air_irfft_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int threads = nfft >= 2048 ? 512 : nfft >= 512 ? 256 : 64;
    for (int64_t q0 = 0; q0 < Q; q0 += 65535) {
        const int64_t nq = std::min<int64_t>(65535, Q - q0);
        air_irfft_kernel<<<dim3((unsigned)C, (unsigned)nq), threads, sm, st>>>((const cplx*)H + q0 * M * Pld, Pld, e, nfft, air_log2(nfft),
                                                                             (const cplx*)tw, nr, (char*)out + (size_t)q0 * C * nr * esz(enc_im != nullptr));
        KERNEL_CHECK();
    }
}

void launch_air_encode(const void* H, int64_t Pld, const double* enc_re, const double* enc_im, int C, int M, int64_t Q, int P, void* X,
                       hipStream_t st) {
    const AirEnc e{enc_re, enc_im, C, M};
    const int np = enc_im ? 2 : 1;
    for (int64_t q0 = 0; q0 < Q; q0 += 65535) {
        const int64_t nq = std::min<int64_t>(65535, Q - q0);
        air_encode_kernel<<<dim3((unsigned)ceil_div(P, 256), (unsigned)C, (unsigned)nq), 256, 0, st>>>((const cplx*)H + q0 * M * Pld, Pld, e, P,
                                                                                                     (cplx*)X + q0 * C * np * P);
        KERNEL_CHECK();
    }
}

void launch_air_pick(const double* y, int64_t rows, int np, int nfft, int nr, void* out, hipStream_t st) {
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
        const int64_t n = std::min<int64_t>(65535, rows - r0);
        air_pick_kernel<<<dim3((unsigned)ceil_div(nr, 256), (unsigned)n), 256, 0, st>>>(y + r0 * np * nfft, n, np, nfft, nr,
                                                                                       (char*)out + (size_t)r0 * nr * esz(np == 2));
        KERNEL_CHECK();
    }
}

}  // namespace emagls
