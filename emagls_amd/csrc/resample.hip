// Polyphase FIR resampling with the semantics of MATLAB's resample(x, p, q) at its defaults N = 10, bta = 5 (called by
// dependencies/binauralDecode.m:12-23).  OWN RESTATEMENT of resample.m: m = max(p, q), L = 20 m + 1,
// h0[n] = sinc((n - 10 m) / m) / m * kaiser(L, 5)[n], h = p h0 / sum(h0), nz = q - (10 m mod q) zeros in front of h,
// delay = (10 m + nz) / q.  Output k of a column is
//     y[k] = sum_r h[ph + p r] x[t0 - r],   n = k + delay,  t0 = floor(n q / p),  ph = n q mod p,
// x = 0 outside [0, nx), h = 0 beyond its end.  The sum runs r = 0 .. R-1 in that order with fused multiply-adds, so results are
// deterministic.  The taps are designed on the host in FP64 once per (p, q) and kept per device (resample_cache_clear frees them).
#include <map>
#include <tuple>
#include <vector>

#include "kernels.hpp"

namespace emagls {

namespace {

constexpr int RS_THREADS = 256;
constexpr int64_t RS_TAPS_LDS = 4096;       // doubles: a bank of up to 32 KiB is staged in LDS, a larger one read through the caches
constexpr int64_t RS_X_LDS = 32768;         // bytes of a workgroup's input span in LDS
constexpr int64_t RS_TILE_MAX = 2048;       // outputs per workgroup tile

double bessel_i0(double x) {   // power series; the argument never exceeds bta = 5 here
    const double y = 0.25 * x * x;
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 100 && t > 1e-18 * s; ++k) {
        t *= y / ((double)k * k);
        s += t;
    }
    return s;
}

// bank [R * p]: h with its nz leading zeros, zero-padded to R = ceil((L + nz) / p) taps per phase; tap r of phase ph is
// bank[r p + ph], so lanes of neighbouring outputs (neighbouring phases) read neighbouring words
struct Design {
    std::vector<double> bank;
    int64_t R = 0, delay = 0;
};

Design design(int64_t p, int64_t q) {
    const int64_t m = std::max(p, q), L = 20 * m + 1, half = 10 * m;
    std::vector<double> h0(L);
    const double i0b = bessel_i0(5.0);
    double sum = 0.0;
    for (int64_t n = 0; n < L; ++n) {
        const double u = (double)(n - half), a = u / (double)m, r = u / (double)half;
        const double sinc = n == half ? 1.0 : std::sin(kPi * a) / (kPi * a);
        const double w = bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        h0[n] = sinc / (double)m * w;
        sum += h0[n];
    }
    const int64_t nz = q - half % q;
    Design d;
    d.delay = (half + nz) / q;
    d.R = ceil_div(L + nz, p);
    d.bank.assign((size_t)(d.R * p), 0.0);
    for (int64_t n = 0; n < L; ++n) d.bank[(size_t)(n + nz)] = (double)p * h0[n] / sum;
    return d;
}

struct Taps {
    double* d = nullptr;
    int64_t R = 0, delay = 0;
};

std::mutex g_rs_mu;
std::map<std::tuple<int, int64_t, int64_t>, Taps> g_rs_taps;   // (device, p, q) -> bank in HBM

Taps taps_for(int64_t p, int64_t q) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_rs_mu);
    auto it = g_rs_taps.find({dev, p, q});
    if (it != g_rs_taps.end()) return it->second;
    const Design ds = design(p, q);
    Taps t{nullptr, ds.R, ds.delay};
    HIP_CHECK(hipMalloc(&t.d, sizeof(double) * ds.bank.size()));
    const hipError_t e = hipMemcpy(t.d, ds.bank.data(), sizeof(double) * ds.bank.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(t.d); HIP_CHECK(e); }
    g_rs_taps[{dev, p, q}] = t;
    return t;
}

__device__ __forceinline__ void fmav(double a, double x, double& acc) { acc = fma(a, x, acc); }
__device__ __forceinline__ void fmav(double a, const cplx& x, cplx& acc) { acc.x = fma(a, x.x, acc.x); acc.y = fma(a, x.y, acc.y); }

// Workgroups stride over tiles of T outputs of one column.  X_LDS: the tile's input span x[t0(k0) - R + 1 .. t0(k0 + T - 1)] is
// staged in LDS by coalesced loads; otherwise (a span beyond RS_X_LDS) every lane reads its inputs from global memory.
// TAPS_LDS: the bank is staged once per workgroup; otherwise it is read through L1 / L2.  Complex input: the real taps applied to
// the real and the imaginary part.
template <typename V, bool X_LDS, bool TAPS_LDS>
__global__ void __launch_bounds__(RS_THREADS) resample_kernel(const V* __restrict__ x, int64_t nx, int64_t nch, const double* __restrict__ bank,
                                                              int p, int q, int R, int64_t delay, int64_t ny, int T, V* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double rs_lds[];
    V* xs = reinterpret_cast<V*>(rs_lds + (TAPS_LDS ? ((int64_t)p * R + 1) / 2 * 2 : 0));
    const double* tp0 = bank;
    if constexpr (TAPS_LDS) {
        for (int i = threadIdx.x; i < p * R; i += RS_THREADS) rs_lds[i] = bank[i];
        tp0 = rs_lds;
    }
    const int64_t tiles = (ny + T - 1) / T;
    for (int64_t tile = blockIdx.x; tile < tiles * nch; tile += gridDim.x) {
        const int64_t col = tile / tiles, k0 = (tile - col * tiles) * T, kend = min(k0 + (int64_t)T, ny);
        const V* __restrict__ xc = x + col * nx;
        V* __restrict__ yc = y + col * ny;
        const int64_t tb = ((k0 + delay) * q) / p - (R - 1);   // x index of xs[0]
        if constexpr (X_LDS) {
            const int64_t cnt = ((kend - 1 + delay) * q) / p - tb + 1;
            __syncthreads();   // (the previous tile's reads are done)
            for (int64_t i = threadIdx.x; i < cnt; i += RS_THREADS) {
                const int64_t t = tb + i;
                xs[i] = (t >= 0 && t < nx) ? xc[t] : V{};
            }
        }
        __syncthreads();
        for (int64_t k = k0 + threadIdx.x; k < kend; k += RS_THREADS) {
            const int64_t nq = (k + delay) * q, t0 = nq / p;
            const double* __restrict__ tp = tp0 + (nq - t0 * p);
            V acc{};
            if constexpr (X_LDS) {
                const V* xp = xs + (t0 - tb);
                for (int r = 0; r < R; ++r) fmav(tp[(int64_t)r * p], xp[-r], acc);
            } else {   // only the taps whose input lies in [0, nx): r in [t0 - nx + 1, t0]
                const int r0 = (int)max((int64_t)0, t0 - nx + 1), r1 = (int)min((int64_t)R, t0 + 1);
                for (int r = r0; r < r1; ++r) fmav(tp[(int64_t)r * p], xc[t0 - r], acc);
            }
            yc[k] = acc;
        }
    }
}

template <typename V>
void launch_typed(const V* x, int64_t nx, int64_t nch, int64_t p, int64_t q, V* y, hipStream_t st) {
    const Taps tp = taps_for(p, q);
    const int64_t ny = resample_length(nx, p, q), R = tp.R;
    // the largest tile (a multiple of the workgroup) whose input span fits RS_X_LDS; none: the inputs come from global memory
    auto span = [&](int64_t T) { return ((T - 1) * q + p - 1) / p + R + 1; };
    int64_t T = RS_TILE_MAX;
    while (T > RS_THREADS && span(T) * (int64_t)sizeof(V) > RS_X_LDS) T /= 2;
    const bool x_lds = span(T) * (int64_t)sizeof(V) <= RS_X_LDS;
    const bool taps_lds = p * R <= RS_TAPS_LDS;
    const size_t lds = (taps_lds ? sizeof(double) * (size_t)((p * R + 1) / 2 * 2) : 0) + (x_lds ? sizeof(V) * (size_t)span(T) : 0);
    const int64_t work = ceil_div(ny, T) * nch;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(work, 2048));
    const int ip = (int)p, iq = (int)q, iR = (int)R, iT = (int)T;
    if (x_lds && taps_lds)
        resample_kernel<V, true, true><<<grid, RS_THREADS, lds, st>>>(x, nx, nch, tp.d, ip, iq, iR, tp.delay, ny, iT, y);
    else if (x_lds)
        resample_kernel<V, true, false><<<grid, RS_THREADS, lds, st>>>(x, nx, nch, tp.d, ip, iq, iR, tp.delay, ny, iT, y);
    else if (taps_lds)
        resample_kernel<V, false, true><<<grid, RS_THREADS, lds, st>>>(x, nx, nch, tp.d, ip, iq, iR, tp.delay, ny, iT, y);
    else
        resample_kernel<V, false, false><<<grid, RS_THREADS, lds, st>>>(x, nx, nch, tp.d, ip, iq, iR, tp.delay, ny, iT, y);
    KERNEL_CHECK();
}

}  // namespace

int64_t resample_length(int64_t n, int64_t p, int64_t q) { return (int64_t)(((__int128)n * p + q - 1) / q); }

void launch_resample(const void* in, bool cplx_in, int64_t n, int64_t nch, int64_t p, int64_t q, void* out, hipStream_t st) {
    if (n <= 0 || nch <= 0) return;
    if (p == 1 && q == 1) {
        HIP_CHECK(hipMemcpyAsync(out, in, esz(cplx_in) * (size_t)n * nch, hipMemcpyDeviceToDevice, st));
        return;
    }
    if (std::max(p, q) > kResampleMaxRatio) throw Error(2, "resample supports max(p, q) <= 65536 after reduction");
    if (cplx_in) launch_typed((const cplx*)in, n, nch, p, q, (cplx*)out, st);
    else launch_typed((const double*)in, n, nch, p, q, (double*)out, st);
}

void resample_cache_clear() {
    std::lock_guard<std::mutex> lk(g_rs_mu);
    for (auto& kv : g_rs_taps) hipFree(kv.second.d);
    g_rs_taps.clear();
}

}  // namespace emagls
