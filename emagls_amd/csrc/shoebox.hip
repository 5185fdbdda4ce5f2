// Shoebox image sources (DESIGN.md sections 12 and 13; the host entries are in array_irs_api.hip): Allen & Berkley's image model,
// with frequency-independent walls in the gain or -- the write pass's IMAGES form -- with the exponents and the path beside it, enumerated on the device into the component lists of section 11 (azi, zen, delay, gain per component,
// CSR offsets per source), in an order that is part of the definition.
//
// A candidate of a source s is an integer triple n = (nx, ny, nz) and a parity triple p = (px, py, pz) in {0, 1}^3:
//   image_i = (1 - 2 p_i) s_i + 2 n_i L_i,   e0_i = |n_i - p_i| (the wall at 0),   e1_i = |n_i| (the wall at L_i),
//   reflection order = sum_i (e0_i + e1_i),   v = image - array_pos,   d = sqrt((vx vx + vy vy) + vz vz),   tau = d / 343 fs,
//   g = ((((((1 b0x^e0x) b1x^e1x) b0y^e0y) b1y^e1y) b0z^e0z) b1z^e1z) / d  (b^e by binary powers, b^0 = 1),
//   azi = atan2(vy, vx),   zen = acos(vz / d)   (d >= |vz| in IEEE arithmetic, and d > 0: the host has checked the geometry).
// It is KEPT iff (max_order < 0 or its reflection order <= max_order) and g != 0 and tau <= max_delay.  The kept candidates of a
// source lie in ascending lexicographic order of (nz, ny, nx, pz, py, px): the candidate index inside the search box
// |n_i| <= B_i is c = ((((nz + Bz) Wy + (ny + By)) Wx + (nx + Bx)) 8 + 4 pz + 2 py + px, W_i = 2 B_i + 1, and the order of the kept
// ones does not depend on the box.  Every source of a call has the same box, so the same number of candidates ncand.
//
// lane = candidate; a workgroup of four waves owns a tile of SBX_TILE = 256 consecutive candidates of one source.
//   count   shoebox_eval decides; the decision of a wave is one 64-bit __ballot word (mask [tile][4]), the tile's count the four
//           population counts combined in wave order through LDS
//   scan    one workgroup: exclusive scan of the tile counts (64-bit) -> tile_base [ntiles + 1] and comp_ptr [nsrc + 1]
//   write   reads the mask -- it does not decide again --: place = tile base + the population counts of the tile's lower waves'
//           words + the population count of the lane's lower bits in its own word; evaluates the definition once more and writes
//           azi, zen, delay, gain there (and, by its form, exponents, path, and the emission vectors of DESIGN.md section 15)
// No atomics: the place of a component is a function of the masks alone, so equal calls give equal lists in equal order, and the
// list of source q is the list of the call with that source alone.
#include "kernels.hpp"

namespace emagls {

struct SbxCand {
    double vx, vy, vz, d, tau, gain;
};

__device__ __forceinline__ double sbx_ipow(double b, int e) {
    double r = 1.0;
    while (e) {
        if (e & 1) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// candidate c (< a.ncand) of the source at s[0..2]: the definition above; returns "kept"
__device__ __forceinline__ bool shoebox_eval(const ShoeboxArgs& a, const double* __restrict__ s, int64_t c, SbxCand& o) {
    const int p = (int)(c & 7);
    int64_t t = c >> 3;
    int n[3], par[3] = {p & 1, (p >> 1) & 1, (p >> 2) & 1};
    n[0] = (int)(t % a.W[0]) - a.B[0]; t /= a.W[0];
    n[1] = (int)(t % a.W[1]) - a.B[1]; t /= a.W[1];
    n[2] = (int)t - a.B[2];
    double v[3], g = 1.0;
    int ord = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int e0 = abs(n[i] - par[i]), e1 = abs(n[i]);
        ord += e0 + e1;
        g *= sbx_ipow(a.beta[2 * i], e0);
        g *= sbx_ipow(a.beta[2 * i + 1], e1);
        const double img = (double)(1 - 2 * par[i]) * s[i] + (double)(2 * n[i]) * a.L[i];
        v[i] = img - a.pos[i];
    }
    o.vx = v[0]; o.vy = v[1]; o.vz = v[2];
    o.d = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    o.tau = o.d / 343.0 * a.fs;
    o.gain = g / o.d;
    return (a.max_order < 0 || ord <= a.max_order) && o.gain != 0.0 && o.tau <= a.max_delay;
}

// grid nsrc * tiles; mask [ntiles][4], cnt [ntiles]
__global__ void __launch_bounds__(SBX_TILE) shoebox_count_kernel(ShoeboxArgs a, const double* __restrict__ src, uint64_t* __restrict__ mask,
                                                                int* __restrict__ cnt) {
    __shared__ int wc[SBX_TILE / 64];
    const int64_t tile = blockIdx.x, q = tile / a.tiles, c = (tile % a.tiles) * SBX_TILE + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool kept = false;
    if (c < a.ncand) {
        SbxCand o;
        kept = shoebox_eval(a, src + 3 * q, c, o);
    }
    const uint64_t m = __ballot(kept);
    if (lane == 0) {
        mask[tile * (SBX_TILE / 64) + wave] = m;
        wc[wave] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) cnt[tile] = ((wc[0] + wc[1]) + wc[2]) + wc[3];
}

// one workgroup of 1024 threads: thread t sums the run [t run, (t + 1) run) of the tile counts, the 1024 sums are scanned in LDS,
// and the thread writes its run's bases; comp_ptr[q] is the base of source q's first tile
__global__ void __launch_bounds__(1024) shoebox_scan_kernel(int64_t ntiles, int64_t tiles, const int* __restrict__ cnt, int64_t* __restrict__ base,
                                                            int64_t* __restrict__ comp_ptr) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t run = (ntiles + 1023) / 1024, i0 = std::min<int64_t>(t * run, ntiles), i1 = std::min<int64_t>(i0 + run, ntiles);
    int64_t s = 0;
    for (int64_t i = i0; i < i1; ++i) s += cnt[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int64_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t b = part[t] - s;
    for (int64_t i = i0; i < i1; ++i) {
        base[i] = b;
        if (i % tiles == 0) comp_ptr[i / tiles] = b;
        b += cnt[i];
    }
    if (t == 1023) {
        base[ntiles] = part[1023];
        comp_ptr[ntiles / tiles] = part[1023];
    }
}

// grid nsrc * tiles; azi, zen, delay, gain [base[ntiles]]; IMAGES: also exp [base[ntiles]][6] and path [base[ntiles]] (the spectral
// room of DESIGN.md section 13, whose a.beta are ones: the walls enter in the responses' main kernel); PATH without IMAGES: the
// flat lists and path alone (the distances of the point-source responses, section 14)
template <bool IMAGES, bool PATH = IMAGES>
__global__ void __launch_bounds__(SBX_TILE) shoebox_write_kernel(ShoeboxArgs a, const double* __restrict__ src, const uint64_t* __restrict__ mask,
                                                                const int64_t* __restrict__ base, double* __restrict__ azi,
                                                                double* __restrict__ zen, double* __restrict__ delay, double* __restrict__ gain,
                                                                int* __restrict__ exp, double* __restrict__ path) {
    // (shoebox_write_emit_kernel below restates this body: a change here is a change there)
    const int64_t tile = blockIdx.x, q = tile / a.tiles, c = (tile % a.tiles) * SBX_TILE + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t* __restrict__ mw = mask + tile * (SBX_TILE / 64);
    const uint64_t m = mw[wave];
    if (!((m >> lane) & 1)) return;   // (a set bit implies c < ncand)
    int64_t r = base[tile] + __popcll(m & (((uint64_t)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) r += __popcll(mw[w]);
    SbxCand o;
    (void)shoebox_eval(a, src + 3 * q, c, o);
    azi[r] = atan2(o.vy, o.vx);
    zen[r] = acos(o.vz / o.d);
    delay[r] = o.tau;
    gain[r] = o.gain;
    if constexpr (IMAGES) {
        int64_t t = c >> 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int n = (int)(i < 2 ? t % a.W[i] : t) - a.B[i], par = (int)(c >> i) & 1;
            if (i < 2) t /= a.W[i];
            exp[6 * r + 2 * i] = abs(n - par);
            exp[6 * r + 2 * i + 1] = abs(n);
        }
    }
    if constexpr (PATH) path[r] = o.d;
}

// The forms that also write emit [base[ntiles]][3]: the unit vector along which the component's ray left the
// real source -- the image's ray to the array, -v / d, mirrored back through the walls it crossed, e_i = -(1 - 2 p_i) v_i / d.  A
// kernel of its own with the body of shoebox_write_kernel restated: the forms above keep their text, so that their instruction
// streams stay what they were (through a shared function the IMAGES form came out with other registers).
template <bool IMAGES, bool PATH>
__global__ void __launch_bounds__(SBX_TILE) shoebox_write_emit_kernel(ShoeboxArgs a, const double* __restrict__ src, const uint64_t* __restrict__ mask,
                                                                     const int64_t* __restrict__ base, double* __restrict__ azi,
                                                                     double* __restrict__ zen, double* __restrict__ delay, double* __restrict__ gain,
                                                                     int* __restrict__ exp, double* __restrict__ path, double* __restrict__ emit) {
    const int64_t tile = blockIdx.x, q = tile / a.tiles, c = (tile % a.tiles) * SBX_TILE + threadIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t* __restrict__ mw = mask + tile * (SBX_TILE / 64);
    const uint64_t m = mw[wave];
    if (!((m >> lane) & 1)) return;   // (a set bit implies c < ncand)
    int64_t r = base[tile] + __popcll(m & (((uint64_t)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) r += __popcll(mw[w]);
    SbxCand o;
    (void)shoebox_eval(a, src + 3 * q, c, o);
    azi[r] = atan2(o.vy, o.vx);
    zen[r] = acos(o.vz / o.d);
    delay[r] = o.tau;
    gain[r] = o.gain;
    if constexpr (IMAGES) {
        int64_t t = c >> 3;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int n = (int)(i < 2 ? t % a.W[i] : t) - a.B[i], par = (int)(c >> i) & 1;
            if (i < 2) t /= a.W[i];
            exp[6 * r + 2 * i] = abs(n - par);
            exp[6 * r + 2 * i + 1] = abs(n);
        }
    }
    if constexpr (PATH) path[r] = o.d;
    emit[3 * r] = ((c & 1) ? o.vx : -o.vx) / o.d;
    emit[3 * r + 1] = ((c & 2) ? o.vy : -o.vy) / o.d;
    emit[3 * r + 2] = ((c & 4) ? o.vz : -o.vz) / o.d;
}

void launch_shoebox_count(const ShoeboxArgs& a, int64_t nsrc, const double* src, uint64_t* mask, int* cnt, hipStream_t st) {
    shoebox_count_kernel<<<(unsigned)(nsrc * a.tiles), SBX_TILE, 0, st>>>(a, src, mask, cnt);
    KERNEL_CHECK();
}

void launch_shoebox_scan(const ShoeboxArgs& a, int64_t nsrc, const int* cnt, int64_t* base, int64_t* comp_ptr, hipStream_t st) {
    shoebox_scan_kernel<<<1, 1024, 0, st>>>(nsrc * a.tiles, a.tiles, cnt, base, comp_ptr);
    KERNEL_CHECK();
}

void launch_shoebox_write(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                          double* zen, double* delay, double* gain, hipStream_t st) {
    shoebox_write_kernel<false><<<(unsigned)(nsrc * a.tiles), SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, nullptr, nullptr);
    KERNEL_CHECK();
}

void launch_shoebox_write_dist(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                               double* zen, double* delay, double* gain, double* dist, hipStream_t st) {
    shoebox_write_kernel<false, true><<<(unsigned)(nsrc * a.tiles), SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, nullptr, dist);
    KERNEL_CHECK();
}

void launch_shoebox_write_images(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                                 double* zen, double* delay, double* gain, int* exp, double* path, hipStream_t st) {
    shoebox_write_kernel<true><<<(unsigned)(nsrc * a.tiles), SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, exp, path);
    KERNEL_CHECK();
}

void launch_shoebox_write_emit(const ShoeboxArgs& a, int64_t nsrc, const double* src, const uint64_t* mask, const int64_t* base, double* azi,
                               double* zen, double* delay, double* gain, int* exp, double* path, double* emit, hipStream_t st) {
    const unsigned grid = (unsigned)(nsrc * a.tiles);
    if (exp) shoebox_write_emit_kernel<true, true><<<grid, SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, exp, path, emit);
    else if (path) shoebox_write_emit_kernel<false, true><<<grid, SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, nullptr, path, emit);
    else shoebox_write_emit_kernel<false, false><<<grid, SBX_TILE, 0, st>>>(a, src, mask, base, azi, zen, delay, gain, nullptr, nullptr, emit);
    KERNEL_CHECK();
}

}  // namespace emagls
