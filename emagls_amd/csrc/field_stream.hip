// The field stream (include/emagls.h: emagls_field_stream_*): nsrc dry source signals through nsrc room
// responses of nch channels each, out(:, c) = sum_q fftfilt(rir_q(:, c), s_q), fed a block of B samples at a time, with the state of
// the convolution kept in HBM between the calls.  What it writes lies as the decode stream and the listener group read their input.
//
// Uniformly partitioned overlap-save, the mirror image of decode_stream.hip.  The responses are cut into P = ceil(nr / B) partitions
// of B taps and transformed once at Nf = 2B (ds_filter_kernel of decode_stream.hip, through launch_partition_spectra):
// Rf [nsrc][P][planes][B + 1], planes = nch real channels, or 2 nch for a complex response (plane 2c its real, 2c + 1 its imaginary
// taps: each is convolved with the real source).  Block j of source q, behind its predecessor, has the spectrum
// X_q,j = FFT([s_q,(j-1), s_q,j]), and
//     y_j(:, plane) = last B samples of IFFT( sum_q sum_p X_q,(j-p) Rf[q][p][plane] ).
// The state is the GATHERED form: a ring of the last P INPUT spectra per source.  With one channel in and many out it is `planes`
// times smaller than a ring of pending outputs, and its history serves every output channel.  A slot of a block not yet pushed is
// zero (creation, reset) and contributes nothing.
//
// Per block:
//   fs_source_kernel    ONE workgroup: the windows [hist_q, block_q] of all sources, two real sources per packed transform, their
//                       spectra into ring slot pos + 1, hist <- block, pos <- pos + 1 (mod P).  The position has one writer and no
//                       reader in another workgroup of the launch.
//   fs_product_kernel   one workgroup per pair of planes (two real channels, or the real and the imaginary plane of one complex
//                       channel; an odd plane count leaves the last pair half empty), thread = frequency bin: both planes'
//                       sums over the sources and the partitions against the SAME ring value, then A + iB back in one packed
//                       inverse transform and the last B samples out: two columns, or one interleaved complex column.  It
//                       writes nothing another workgroup reads.
// The order of the sums is fixed.  With B + 1 <= 256 the G = floor(512 / (B + 1)) thread groups of a workgroup share the partitions:
// group g takes the partitions p = g, g + G, ...; within a group the sources ascend and, within a source, the partitions; a
// product is accumulated with cfma's four fused multiply-adds; the groups' sums meet in LDS and are added in group order,
// ((g0 + g1) + g2) + ...  With B + 1 > 256 there is one group and a thread takes several bins (KU).  No atomics: equal pushes on
// fresh objects give equal bits, and how blocks are grouped into pushes changes nothing.
// A bank of response sets (n_sets > 1) runs the two kernels' bank forms further down; one set runs these.
#include "kernels.hpp"
#include "stream_fft.hpp"

namespace emagls {

namespace {

// grid 1.  src + q lds: the block of source q; hist [nsrc][B]; ring [nsrc][P][B + 1]
__global__ void __launch_bounds__(DS_NT) fs_source_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ hist, int nsrc, int B,
                                                          int log2n, int P, int* __restrict__ pos_p, cplx* __restrict__ ring) {
    constexpr int NLD = DS_ELEMS / DS_NT;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1, mask = Nf - 1;
    const int NTP = DS_ELEMS >> log2n;              // transforms per round
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [NTP][Nf], padded
    cplx* tws = buf + (DS_ELEMS + DS_ELEMS / 16);   // [Nf / 2]
    const int tid = threadIdx.x, npairs = (nsrc + 1) / 2;
    const int pos = *pos_p;
    const int slot = pos + 1 >= P ? 0 : pos + 1;
    ds_twiddles(tws, Nf);
#pragma unroll 1
    for (int p0 = 0; p0 < npairs; p0 += NTP) {
        const int np = min(NTP, npairs - p0);
        double xb[NLD][2];
        __syncthreads();   // the previous round's spectra have been read (first round: nothing yet)
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + DS_NT * j;
            const int t = idx >> log2n, i = idx & mask;
            xb[j][0] = xb[j][1] = 0.0;
            if (t < np) {
                const int qa = 2 * (p0 + t), qb = qa + 1;
                if (i < B) {
                    xb[j][0] = hist[(int64_t)qa * B + i];
                    if (qb < nsrc) xb[j][1] = hist[(int64_t)qb * B + i];
                } else {
                    xb[j][0] = src[(int64_t)qa * lds + (i - B)];
                    if (qb < nsrc) xb[j][1] = src[(int64_t)qb * lds + (i - B)];
                }
                buf[lds_fft_ix<true>((t << log2n) + (int)bitrev((unsigned)i, log2n))] = mk(xb[j][0], xb[j][1]);
            }
        }
        __syncthreads();   // every read of this round's hist lies behind: the block becomes the next overlap
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + DS_NT * j;
            const int t = idx >> log2n, i = idx & mask;
            if (t < np && i >= B) {
                const int qa = 2 * (p0 + t), qb = qa + 1;
                hist[(int64_t)qa * B + (i - B)] = xb[j][0];
                if (qb < nsrc) hist[(int64_t)qb * B + (i - B)] = xb[j][1];
            }
        }
        lds_fft_stages<false, true>(buf, tws, Nf, log2n, np);
        for (int idx = tid; idx < np * Pf; idx += DS_NT) {
            const int t = idx / Pf, k = idx - t * Pf;
            const int qa = 2 * (p0 + t), qb = qa + 1;
            cplx pa, pb;
            ds_unpack(buf[lds_fft_ix<true>((t << log2n) + k)], conj(buf[lds_fft_ix<true>((t << log2n) + ((Nf - k) & mask))]), pa, pb);
            ring[((int64_t)qa * P + slot) * Pf + k] = pa;
            if (qb < nsrc) ring[((int64_t)qb * P + slot) * Pf + k] = pb;
        }
    }
    if (tid == 0) *pos_p = slot;   // (every thread read the position ahead of the first barrier)
}

// grid (pairs of planes).  Rf [nsrc][P][planes][B + 1]; out: plane c at out + c ldo (doubles), or with out_cplx pair c at out + c ldo
// (cplx).  KU: frequency bins per thread (B + 1 <= KU * DS_NT)
template <int KU>
__global__ void __launch_bounds__(DS_NT) fs_product_kernel(const cplx* __restrict__ ring, const cplx* __restrict__ Rf, int nsrc, int planes, int B,
                                                           int log2n, int P, const int* __restrict__ pos_p, void* __restrict__ out_, int out_cplx,
                                                           int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1;
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [Nf], padded
    cplx* tws = buf + (Nf + Nf / 16);               // [Nf / 2]
    cplx* part = tws + Nf / 2;                      // [G - 1][2][Pf] the partial sums of the groups 1 .. G - 1
    const int tid = threadIdx.x, pair = blockIdx.x;
    const int ca = 2 * pair;
    const bool has_b = ca + 1 < planes;
    const int64_t offb = has_b ? Pf : 0;            // (a half-empty pair reads plane ca twice and drops the second sum)
    const int G = Pf <= DS_NT ? DS_NT / Pf : 1;     // groups of threads that share the partitions (short transforms)
    const int pos = *pos_p;                         // the slot of the block fs_source_kernel has just written
    ds_twiddles(tws, Nf);
    cplx accA[KU], accB[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        accA[u] = mk(0, 0); accB[u] = mk(0, 0);
        const int idx = tid + DS_NT * u;
        const int g = idx / Pf, k = idx - g * Pf;
        if (g < G) {
#pragma unroll 1
            for (int q = 0; q < nsrc; ++q) {
                const cplx* rq = ring + (int64_t)q * P * Pf + k;
                const cplx* wq = Rf + ((int64_t)q * P * planes + ca) * Pf + k;
                int slot = pos - g;
                if (slot < 0) slot += P;
#pragma unroll 4
                for (int p = g; p < P; p += G) {
                    const cplx x = rq[(int64_t)slot * Pf];
                    const cplx* w = wq + (int64_t)p * planes * Pf;
                    const cplx wa = w[0], wb = w[offb];
                    cfma(accA[u], x, wa);
                    cfma(accB[u], x, wb);
                    slot -= G;
                    if (slot < 0) slot += P;
                }
            }
        }
        if (!has_b) accB[u] = mk(0, 0);
    }
    if (G > 1) {   // the groups' partial sums meet in LDS; group 0 adds them in the order of the groups
        const int g = tid / Pf, k = tid - g * Pf;
        if (g > 0 && g < G) { part[((g - 1) * 2 + 0) * Pf + k] = accA[0]; part[((g - 1) * 2 + 1) * Pf + k] = accB[0]; }
        __syncthreads();
        if (g == 0) {
            for (int o = 1; o < G; ++o) {
                const cplx a = part[((o - 1) * 2 + 0) * Pf + k], b = part[((o - 1) * 2 + 1) * Pf + k];
                accA[0].x += a.x; accA[0].y += a.y;
                accB[0].x += b.x; accB[0].y += b.y;
            }
        }
    }
    // Y_a + i Y_b with Y[N - k] = conj(Y[k]), as ds_inverse_kernel packs the two ears
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const int k = tid + DS_NT * u;
        if (k < Pf) {
            const cplx a = accA[u], b = accB[u];
            buf[lds_fft_ix<true>((int)bitrev((unsigned)k, log2n))] = mk(a.x - b.y, a.y + b.x);
            if (k > 0 && k < B) buf[lds_fft_ix<true>((int)bitrev((unsigned)(Nf - k), log2n))] = mk(a.x + b.y, b.x - a.y);
        }
    }
    __syncthreads();
    lds_fft_stages<true, true>(buf, tws, Nf, log2n, 1);
    const double scale = 1.0 / (double)Nf;
    if (out_cplx) {
        cplx* out = reinterpret_cast<cplx*>(out_) + (int64_t)pair * ldo;
        for (int i = tid; i < B; i += DS_NT) {
            const cplx y = buf[lds_fft_ix<true>(B + i)];
            out[i] = mk(y.x * scale, y.y * scale);
        }
    } else {
        double* out = reinterpret_cast<double*>(out_) + (int64_t)ca * ldo;
        for (int i = tid; i < B; i += DS_NT) {
            const cplx y = buf[lds_fft_ix<true>(B + i)];
            out[i] = y.x * scale;
            if (has_b) out[ldo + i] = y.y * scale;
        }
    }
}

// ---- a bank of response sets, cross-faded per block on the input side.  Every source has a set index per
// block.  The window [hist_q, block_q] of block t meets the distinct sets among s_(t-2), s_(t-1), s_t of its source; under each of
// them it is transformed with that set's gains over its two halves (each one of 0, 1, r[i] = (i + 1) / B, 1 - r[i], applied to the
// registers between the global load and the LDS store; a gain of 1 is not multiplied) and becomes one ENTRY of the ring slot, tagged
// with its set: ring [nsrc][P][3][B + 1], tag [nsrc][P][3] (-1: empty).  The product kernel multiplies every live entry with the
// partition spectra of ITS set, Rf [S][nsrc][P][planes][B + 1].  hist holds the raw previous block.
enum { FS_G_ZERO = 0, FS_G_ONE = 1, FS_G_R = 2, FS_G_1MR = 3 };   // gain of a set over a block
constexpr int FS_E = kFieldStreamEntries;
constexpr int FS_MAX_SRC = kFieldStreamMaxSources;   // the size of the source kernel's tables
constexpr int FS_U = 4;          // partitions per pass of the product kernel's loop

// grid 1.  As fs_source_kernel, and: set_p + q lset: source q's index of this block (null: it keeps its set; 0 on a fresh object),
// clamped into [0, S - 1] before any use; sel [nsrc][2]: the indices of the blocks t - 1 and t - 2 (-1: none yet, the block then
// does not fade).  The pairing of the windows is fixed: entry e of source 2j with entry e of source 2j + 1 (the plain kernel's
// pairs, so that a constant index gives its bits); a transform both of whose windows are empty is left out, and the live ones are
// taken in the order (j, e) ascending, DS_ELEMS / Nf per round.
__global__ void __launch_bounds__(DS_NT) fs_source_bank_kernel(const double* __restrict__ src, int64_t lds, double* __restrict__ hist, int nsrc,
                                                               int B, int log2n, int P, int* __restrict__ pos_p, cplx* __restrict__ ring,
                                                               const int* __restrict__ set_p, int64_t lset, int S, int* __restrict__ sel,
                                                               int* __restrict__ tag) {
    constexpr int NLD = DS_ELEMS / DS_NT;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    __shared__ int meta[FS_MAX_SRC][FS_E];            // (set << 4) | (gain of the first half << 2) | gain of the second; -1: empty
    __shared__ int live[FS_MAX_SRC / 2 * FS_E + 1];   // the live transforms j * FS_E + e; [last]: their number
    const int Nf = 2 * B, Pf = B + 1, mask = Nf - 1;
    const int NTP = DS_ELEMS >> log2n;              // transforms per round
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [NTP][Nf], padded
    cplx* tws = buf + (DS_ELEMS + DS_ELEMS / 16);   // [Nf / 2]
    const int tid = threadIdx.x, npairs = (nsrc + 1) / 2;
    const int pos = *pos_p;
    const int slot = pos + 1 >= P ? 0 : pos + 1;
    int s0 = 0, s1 = 0;                             // (thread q < nsrc: sigma_t and sigma_(t-1) of source q)
    if (tid < nsrc) {
        const int p1 = min(sel[2 * tid], S - 1), p2 = min(sel[2 * tid + 1], S - 1);
        s0 = set_p ? min(max(set_p[(int64_t)tid * lset], 0), S - 1) : max(p1, 0);
        s1 = p1 < 0 ? s0 : p1;
        const int s2 = p2 < 0 ? s1 : p2;
        // the distinct sets of the window, oldest role first
        int u[FS_E] = {s2, -1, -1};
        if (s1 != s2) { u[1] = s1; if (s0 != s1 && s0 != s2) u[2] = s0; }
        else if (s0 != s1) u[1] = s0;
#pragma unroll
        for (int e = 0; e < FS_E; ++e) {
            const int set = u[e];
            const int ga = set == s1 ? (s1 == s2 ? FS_G_ONE : FS_G_R) : set == s2 ? FS_G_1MR : FS_G_ZERO;
            const int gb = set == s0 ? (s0 == s1 ? FS_G_ONE : FS_G_R) : set == s1 ? FS_G_1MR : FS_G_ZERO;
            meta[tid][e] = set < 0 || (ga == FS_G_ZERO && gb == FS_G_ZERO) ? -1 : (set << 4) | (ga << 2) | gb;
        }
    }
    ds_twiddles(tws, Nf);
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < npairs; ++j)
            for (int e = 0; e < FS_E; ++e)
                if (meta[2 * j][e] >= 0 || (2 * j + 1 < nsrc && meta[2 * j + 1][e] >= 0)) live[n++] = j * FS_E + e;
        live[FS_MAX_SRC / 2 * FS_E] = n;
    }
    __syncthreads();
    const int nlive = live[FS_MAX_SRC / 2 * FS_E];
    const double invB = 1.0 / (double)B;
    // sample i of the window of source q under a gain shape
    auto sample = [&](int q, int shape, int i) __attribute__((always_inline)) {
        if (shape == FS_G_ZERO) return 0.0;
        double v = i < B ? hist[(int64_t)q * B + i] : src[(int64_t)q * lds + (i - B)];
        if (shape != FS_G_ONE) {
            const double r = (double)((i & (B - 1)) + 1) * invB;   // exact: B is a power of two
            v *= shape == FS_G_R ? r : 1.0 - r;
        }
        return v;
    };
#pragma unroll 1
    for (int r0 = 0; r0 < nlive; r0 += NTP) {
        const int np = min(NTP, nlive - r0);
        if (r0 > 0) __syncthreads();   // the previous round's spectra have been read
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + DS_NT * j;
            const int t = idx >> log2n, i = idx & mask;
            if (t < np) {
                const int item = live[r0 + t];
                const int pr = item / FS_E, e = item - pr * FS_E;
                const int qa = 2 * pr, qb = qa + 1;
                const int ma = meta[qa][e], mb = qb < nsrc ? meta[qb][e] : -1;
                const int sh = i < B ? 2 : 0;
                const double xa = sample(qa, ma < 0 ? FS_G_ZERO : (ma >> sh) & 3, i);
                const double xb = sample(qb, mb < 0 ? FS_G_ZERO : (mb >> sh) & 3, i);
                buf[lds_fft_ix<true>((t << log2n) + (int)bitrev((unsigned)i, log2n))] = mk(xa, xb);
            }
        }
        __syncthreads();
        lds_fft_stages<false, true>(buf, tws, Nf, log2n, np);
        for (int idx = tid; idx < np * Pf; idx += DS_NT) {
            const int t = idx / Pf, k = idx - t * Pf;
            const int item = live[r0 + t];
            const int pr = item / FS_E, e = item - pr * FS_E;
            const int qa = 2 * pr, qb = qa + 1;
            cplx pa, pb;
            ds_unpack(buf[lds_fft_ix<true>((t << log2n) + k)], conj(buf[lds_fft_ix<true>((t << log2n) + ((Nf - k) & mask))]), pa, pb);
            if (meta[qa][e] >= 0) ring[(((int64_t)qa * P + slot) * FS_E + e) * Pf + k] = pa;
            if (qb < nsrc && meta[qb][e] >= 0) ring[(((int64_t)qb * P + slot) * FS_E + e) * Pf + k] = pb;
        }
    }
    __syncthreads();   // every read of hist lies behind: the raw block becomes the next overlap
    for (int idx = tid; idx < nsrc * B; idx += DS_NT) {
        const int q = idx / B, i = idx - q * B;
        hist[(int64_t)q * B + i] = src[(int64_t)q * lds + i];
    }
    if (tid < nsrc * FS_E) {
        const int q = tid / FS_E, e = tid - q * FS_E;
        const int m = meta[q][e];
        tag[((int64_t)q * P + slot) * FS_E + e] = m < 0 ? -1 : m >> 4;
    }
    if (tid < nsrc) { sel[2 * tid] = s0; sel[2 * tid + 1] = s1; }   // (the thread that read them)
    if (tid == 0) *pos_p = slot;   // (every thread read the position ahead of the first barrier)
}

// grid (pairs of planes).  As fs_product_kernel on ring [nsrc][P][3][B + 1] and Rf [S][nsrc][P][planes][B + 1]: within a (source,
// slot) the live entries in slot order, each against the spectra of its tag's set; an empty entry is skipped.  The tag is clamped
// again before it forms an address.
template <int KU>
__global__ void __launch_bounds__(DS_NT) fs_product_bank_kernel(const cplx* __restrict__ ring, const int* __restrict__ tag, const cplx* __restrict__ Rf,
                                                                int S, int nsrc, int planes, int B, int log2n, int P,
                                                                const int* __restrict__ pos_p, void* __restrict__ out_, int out_cplx, int64_t ldo) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1;
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [Nf], padded
    cplx* tws = buf + (Nf + Nf / 16);               // [Nf / 2]
    cplx* part = tws + Nf / 2;                      // [G - 1][2][Pf] the partial sums of the groups 1 .. G - 1
    const int tid = threadIdx.x, pair = blockIdx.x;
    const int ca = 2 * pair;
    const bool has_b = ca + 1 < planes;
    const int64_t offb = has_b ? Pf : 0;            // (a half-empty pair reads plane ca twice and drops the second sum)
    const int G = Pf <= DS_NT ? DS_NT / Pf : 1;     // groups of threads that share the partitions (short transforms)
    const int pos = *pos_p;                         // the slot of the block fs_source_bank_kernel has just written
    const int64_t set_stride = (int64_t)nsrc * P * planes * Pf;
    ds_twiddles(tws, Nf);
    cplx accA[KU], accB[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        accA[u] = mk(0, 0); accB[u] = mk(0, 0);
        const int idx = tid + DS_NT * u;
        const int g = idx / Pf, k = idx - g * Pf;
        if (g < G) {
#pragma unroll 1
            for (int q = 0; q < nsrc; ++q) {
                const cplx* rq = ring + (int64_t)q * P * FS_E * Pf + k;
                const int* tq = tag + (int64_t)q * P * FS_E;
                const cplx* wq = Rf + ((int64_t)q * P * planes + ca) * Pf + k;
                // FS_U partitions per pass, in three steps that keep the loads of a pass in flight together: the live entries' values
                // of this pass, the tags of the NEXT pass (nothing depends on them yet), then the products in the fixed order
                int tg[FS_U][FS_E], tn[FS_U][FS_E];
                auto tags = [&](int p0, int (&t)[FS_U][FS_E]) __attribute__((always_inline)) {
#pragma unroll
                    for (int j = 0; j < FS_U; ++j) {
                        const int pj = p0 + j * G;
                        int slot = pos - min(pj, P - 1);
                        if (slot < 0) slot += P;
                        const int* ts = tq + (int64_t)slot * FS_E;
#pragma unroll
                        for (int e = 0; e < FS_E; ++e) t[j][e] = pj < P ? ts[e] : -1;
                    }
                };
                tags(g, tn);
#pragma unroll 1
                for (int p = g; p < P; p += FS_U * G) {
                    cplx x[FS_U][FS_E], wa[FS_U][FS_E], wb[FS_U][FS_E];
#pragma unroll
                    for (int j = 0; j < FS_U; ++j) {
                        const int pj = p + j * G;
                        int slot = pos - min(pj, P - 1);
                        if (slot < 0) slot += P;
                        const cplx* xs = rq + (int64_t)slot * FS_E * Pf;
                        const cplx* wp = wq + (int64_t)pj * planes * Pf;
#pragma unroll
                        for (int e = 0; e < FS_E; ++e) {
                            tg[j][e] = tn[j][e];
                            x[j][e] = wa[j][e] = wb[j][e] = mk(0, 0);
                            if (tg[j][e] >= 0) {
                                const cplx* w = wp + (int64_t)min(tg[j][e], S - 1) * set_stride;
                                x[j][e] = xs[(int64_t)e * Pf];
                                wa[j][e] = w[0];
                                wb[j][e] = w[offb];
                            }
                        }
                    }
                    if (p + FS_U * G < P) tags(p + FS_U * G, tn);
#pragma unroll
                    for (int j = 0; j < FS_U; ++j)
#pragma unroll
                        for (int e = 0; e < FS_E; ++e)
                            if (tg[j][e] >= 0) {
                                cfma(accA[u], x[j][e], wa[j][e]);
                                cfma(accB[u], x[j][e], wb[j][e]);
                            }
                }
            }
        }
        if (!has_b) accB[u] = mk(0, 0);
    }
    if (G > 1) {   // the groups' partial sums meet in LDS; group 0 adds them in the order of the groups
        const int g = tid / Pf, k = tid - g * Pf;
        if (g > 0 && g < G) { part[((g - 1) * 2 + 0) * Pf + k] = accA[0]; part[((g - 1) * 2 + 1) * Pf + k] = accB[0]; }
        __syncthreads();
        if (g == 0) {
            for (int o = 1; o < G; ++o) {
                const cplx a = part[((o - 1) * 2 + 0) * Pf + k], b = part[((o - 1) * 2 + 1) * Pf + k];
                accA[0].x += a.x; accA[0].y += a.y;
                accB[0].x += b.x; accB[0].y += b.y;
            }
        }
    }
    // Y_a + i Y_b with Y[N - k] = conj(Y[k]), as ds_inverse_kernel packs the two ears
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const int k = tid + DS_NT * u;
        if (k < Pf) {
            const cplx a = accA[u], b = accB[u];
            buf[lds_fft_ix<true>((int)bitrev((unsigned)k, log2n))] = mk(a.x - b.y, a.y + b.x);
            if (k > 0 && k < B) buf[lds_fft_ix<true>((int)bitrev((unsigned)(Nf - k), log2n))] = mk(a.x + b.y, b.x - a.y);
        }
    }
    __syncthreads();
    lds_fft_stages<true, true>(buf, tws, Nf, log2n, 1);
    const double scale = 1.0 / (double)Nf;
    if (out_cplx) {
        cplx* out = reinterpret_cast<cplx*>(out_) + (int64_t)pair * ldo;
        for (int i = tid; i < B; i += DS_NT) {
            const cplx y = buf[lds_fft_ix<true>(B + i)];
            out[i] = mk(y.x * scale, y.y * scale);
        }
    } else {
        double* out = reinterpret_cast<double*>(out_) + (int64_t)ca * ldo;
        for (int i = tid; i < B; i += DS_NT) {
            const cplx y = buf[lds_fft_ix<true>(B + i)];
            out[i] = y.x * scale;
            if (has_b) out[ldo + i] = y.y * scale;
        }
    }
}

size_t fs_product_lds(int B) {
    const int Pf = B + 1, G = Pf <= DS_NT ? DS_NT / Pf : 1;
    return ds_single_lds(B) + sizeof(cplx) * (size_t)(G - 1) * 2 * Pf;
}

void fs_attributes() {
    static PerDeviceOnce once;
    if (!once.first()) return;
#define EMAGLS_FS_ATTR(K) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024))
    EMAGLS_FS_ATTR(fs_source_kernel);
    EMAGLS_FS_ATTR(fs_product_kernel<1>);
    EMAGLS_FS_ATTR(fs_product_kernel<2>);
    EMAGLS_FS_ATTR(fs_product_kernel<3>);
    EMAGLS_FS_ATTR(fs_product_kernel<5>);
    EMAGLS_FS_ATTR(fs_source_bank_kernel);
    EMAGLS_FS_ATTR(fs_product_bank_kernel<1>);
    EMAGLS_FS_ATTR(fs_product_bank_kernel<2>);
    EMAGLS_FS_ATTR(fs_product_bank_kernel<3>);
    EMAGLS_FS_ATTR(fs_product_bank_kernel<5>);
#undef EMAGLS_FS_ATTR
}

}  // namespace

void launch_field_stream_block(const FieldStreamState& s, const double* src, int64_t lds, const int* set, int64_t lset, void* out, int64_t ldo,
                               hipStream_t st) {
    fs_attributes();
    const int log2n = ds_log2(2 * s.B), Pf = s.B + 1, ku = (Pf + DS_NT - 1) / DS_NT;
    const unsigned grid = (unsigned)((s.planes + 1) / 2);
    const size_t dyn = fs_product_lds(s.B);
    if (s.S > 1) {
        fs_source_bank_kernel<<<1, DS_NT, ds_forward_lds(s.B), st>>>(src, lds, s.hist, s.nsrc, s.B, log2n, s.P, s.pos, s.ring, set, lset, s.S, s.sel,
                                                                     s.tag);
        KERNEL_CHECK();
#define EMAGLS_FS_GO(KU) \
    fs_product_bank_kernel<KU><<<grid, DS_NT, dyn, st>>>(s.ring, s.tag, s.Rf, s.S, s.nsrc, s.planes, s.B, log2n, s.P, s.pos, out, s.out_c ? 1 : 0, ldo)
        if (ku == 1) EMAGLS_FS_GO(1); else if (ku == 2) EMAGLS_FS_GO(2); else if (ku == 3) EMAGLS_FS_GO(3); else EMAGLS_FS_GO(5);
#undef EMAGLS_FS_GO
        KERNEL_CHECK();
        return;
    }
    fs_source_kernel<<<1, DS_NT, ds_forward_lds(s.B), st>>>(src, lds, s.hist, s.nsrc, s.B, log2n, s.P, s.pos, s.ring);
    KERNEL_CHECK();
#define EMAGLS_FS_GO(KU) fs_product_kernel<KU><<<grid, DS_NT, dyn, st>>>(s.ring, s.Rf, s.nsrc, s.planes, s.B, log2n, s.P, s.pos, out, s.out_c ? 1 : 0, ldo)
    if (ku == 1) EMAGLS_FS_GO(1); else if (ku == 2) EMAGLS_FS_GO(2); else if (ku == 3) EMAGLS_FS_GO(3); else EMAGLS_FS_GO(5);
#undef EMAGLS_FS_GO
    KERNEL_CHECK();
}

}  // namespace emagls
