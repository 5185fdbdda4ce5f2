// Block-streaming binauralDecode (include/emagls.h: emagls_decode_stream_*): out(:, ear) = sum_c fftfilt(w_ear(:, c), x(:, c)) fed a
// block of B samples at a time, with the state of the convolution kept in HBM between the calls.
//
// Uniformly partitioned overlap-save.  The filters are cut into P = ceil(len / B) partitions of B taps, w_p, and transformed once at
// length Nf = 2B: W_p = FFT([w_p, 0]).  Block j of the signal, behind its predecessor, has the spectrum X_j = FFT([x_(j-1), x_j]), and
//     y_j = last B samples of IFFT( sum_p sum_c X_(j-p),c W_p,c ).
// The state is the SCATTERED form: a ring of P pending output spectra per ear.  Block j adds X_j W_p into the slot of output block
// j + p, for every p, and then takes its own slot out.  Nothing of the input's past is read again but the previous block (the
// overlap), and the ring is C times smaller than a ring of input spectra.
//
// Per block (after the rotation kernel of rotate.hip / rotate3.hip, when the push has angles):
//   ds_forward_kernel   grid (P, 2 ears): every workgroup transforms the block's channels itself (two real channels, or one complex
//                       one, per packed transform, in LDS) and accumulates its partition over the channels, thread = frequency bin,
//                       into ITS ring slot.  A slot has one writer per launch and the channel order is fixed: no atomics, equal
//                       pushes give equal bits.  Partition P - 1 lands in the slot the previous block just gave up and stores
//                       instead of adding, so a slot needs no clearing.
//   ds_inverse_kernel   workgroup 0: the block's slot, both ears in one packed inverse transform, the last B samples out, and the
//                       ring position (device memory) one step on; the other workgroups keep the block as the next overlap.
// A complex signal (or a real one turned in the complex basis) is decoded as 2C real planes [re x; im x] against the filters
// [re w; -im w] (decode.hip, binaural_decode_complex): a complex sample IS the packed pair of its two planes, so it is read as it lies.
//
// A bank of S filter sets: every block t has a set index s_t, and a change of set is cross-faded on the INPUT
// side over the block that changes: its sample i goes to the new set with the gain r[i] = (i + 1) / B and to the old one with
// 1 - r[i].  The window [x_(t-1), x_t] therefore meets up to three sets, s_(t-2), s_(t-1), s_t; for every distinct one, oldest role
// first, the forward kernel transforms the window under that set's gains (each half one of 0, 1, r, 1 - r, applied to the registers
// the samples wait in between global memory and LDS) and accumulates with that set's spectra into the same sums.  Three equal
// indices are one pass without a gain: the plain stream's arithmetic.  The indices of the two previous blocks live beside the ring
// position and move on with it.
//
// A listener group: L listeners of one sound field, each with a state of their own (ring, hist, pos, sel, one
// after the other in the same buffers) and all on one bank Wf.  The listener is one more grid dimension of the two kernels: a
// workgroup forms its pointers from its listener index and the listener strides and then does what it does for a single stream.
// A push without angles has the input stride 0: every listener reads the common block.  The listener form is instantiated beside
// the single stream's (GROUP): folded into one, the pointer arithmetic ahead of the first loads cost the single stream 0.3 to
// 0.6 us per block (profiles/r12_decode_group.md); with GROUP = false the kernels are the single stream's, instruction for
// instruction, and a group of one listener runs those.
#include "kernels.hpp"
#include "stream_fft.hpp"

namespace emagls {

namespace {

enum { DS_G_ZERO = 0, DS_G_ONE = 1, DS_G_R = 2, DS_G_1MR = 3 };   // gain of a set over a block: 0, 1, r[i] = (i + 1) / B, 1 - r[i]

// the listener strides of a group's launch: of the block (elements of its type; 0: the common block), of pos / sel, of the set
// index, of the output; hist [L][C][B] and ring [L][2][P][B + 1] follow from the shapes.  A single stream's launch has none.
struct DsListeners { int64_t lsx; int lpos, lset; int64_t lso; };
struct DsSingle {};
template <bool GROUP> using DsStrides = std::conditional_t<GROUP, DsListeners, DsSingle>;

// Wf[z][p][c][k] (k <= B) = FFT([w_z,c(pB .. pB + B - 1), 0])[k], z = 2 set + ear; wpl [Z][Cp][len] real planes.
// grid (pairs of planes, P, Z): Z = the (set, ear) pairs of this launch (the launcher cuts a large bank into several); the field
// stream's response spectra are the same thing with Z = its sources (field_stream.hip)
__global__ void __launch_bounds__(DS_NT) ds_filter_kernel(const double* __restrict__ wpl, int Cp, int64_t len, int B, int log2n, int P,
                                                          cplx* __restrict__ Wf) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1, mask = Nf - 1;
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [Nf], padded
    cplx* tws = buf + (Nf + Nf / 16);               // [Nf / 2]
    const int tid = threadIdx.x, p = blockIdx.y, e = blockIdx.z;
    const int ca = 2 * blockIdx.x, cb = ca + 1;
    ds_twiddles(tws, Nf);
    const double* wa = wpl + ((int64_t)e * Cp + ca) * len;
    const double* wb = wpl + ((int64_t)e * Cp + min(cb, Cp - 1)) * len;
    for (int i = tid; i < Nf; i += DS_NT) {
        const int64_t t = (int64_t)p * B + i;
        const bool in = i < B && t < len;
        buf[lds_fft_ix<true>((int)bitrev((unsigned)i, log2n))] = in ? mk(wa[t], cb < Cp ? wb[t] : 0.0) : mk(0.0, 0.0);
    }
    __syncthreads();
    lds_fft_stages<false, true>(buf, tws, Nf, log2n, 1);
    cplx* oa = Wf + (((int64_t)e * P + p) * Cp + ca) * Pf;
    for (int k = tid; k < Pf; k += DS_NT) {
        cplx pa, pb;
        ds_unpack(buf[lds_fft_ix<true>(k)], conj(buf[lds_fft_ix<true>((Nf - k) & mask)]), pa, pb);
        oa[k] = pa;
        if (cb < Cp) oa[Pf + k] = pb;
    }
}

// One block into the ring.  xnew: the block, channel c at xnew + c ldx (double, or cplx when x_cplx); hist [C][B]: the previous
// block (cplx when planes2, else double).  planes2: 2C planes, pair p = complex channel p = planes (p, p + C); else pair p = the
// real channels (2p, 2p + 1).  KU: frequency bins per thread (B + 1 <= KU * DS_NT).  grid (P, 2)
// BANK: Wf holds S sets; set_p: this block's index (null: the previous block's, 0 on a fresh stream), clamped into [0, S - 1] before
// it forms an address; sel: the indices of the blocks t - 1 and t - 2 (-1: none yet, the block then does not fade).
// GROUP: grid (P, 2, L): listener l = blockIdx.z has its block at xnew + l lsx, its index at set_p + l lset, pos_p and sel at
// + l lpos, and its part of hist and ring by the shapes.
template <int KU, bool BANK, bool GROUP>
__global__ void __launch_bounds__(DS_NT) ds_forward_kernel(const void* __restrict__ xnew_, int x_cplx, int64_t ldx, const void* __restrict__ hist_,
                                                           int C, int planes2, const cplx* __restrict__ Wf, int B, int log2n, int P,
                                                           const int* __restrict__ pos_p_, cplx* __restrict__ ring_,
                                                           const int* __restrict__ set_p_, const int* __restrict__ sel_, int S,
                                                           DsStrides<GROUP> ls) {
    constexpr int NLD = DS_ELEMS / DS_NT;
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1, mask = Nf - 1;
    const double* xnew = reinterpret_cast<const double*>(xnew_);
    const double* hist = reinterpret_cast<const double*>(hist_);
    const int* pos_p = pos_p_;
    const int* sel = sel_;
    const int* set_p = set_p_;
    cplx* ring = ring_;
    if constexpr (GROUP) {
        const int64_t l = blockIdx.z;               // the listener
        xnew += l * ls.lsx * (x_cplx ? 2 : 1);      // (in doubles)
        hist += l * C * B * (planes2 ? 2 : 1);
        pos_p += l * ls.lpos;
        if (BANK) sel += l * ls.lpos;
        if (set_p) set_p += l * ls.lset;
        ring += l * 2 * P * Pf;
    }
    const int NTP = DS_ELEMS >> log2n;              // transforms per round
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [NTP][Nf], padded
    cplx* tws = buf + (DS_ELEMS + DS_ELEMS / 16);   // [Nf / 2]
    const int tid = threadIdx.x, part = blockIdx.x, e = blockIdx.y;
    const int Cp = planes2 ? 2 * C : C, npairs = planes2 ? C : (C + 1) / 2;
    ds_twiddles(tws, Nf);
    const int G = Pf <= DS_NT ? DS_NT / Pf : 1;     // groups of threads that share the pairs of a round (short transforms)
    cplx acc[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) acc[u] = mk(0, 0);
    const double* xr = xnew;
    const cplx* xc = reinterpret_cast<const cplx*>(xnew);
    const double* hr = hist;
    const cplx* hc = reinterpret_cast<const cplx*>(hist);
    // a round's samples travel global -> registers -> LDS; the loads of round r + 1 are issued before the transforms of round r
    cplx xv[NLD];
    auto fetch = [&](int p0) __attribute__((always_inline)) {
        const int np = min(NTP, npairs - p0);
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + DS_NT * j;
            const int t = idx >> log2n, i = idx & mask;
            cplx v = mk(0.0, 0.0);
            if (t < np) {
                const int pr = p0 + t;
                if (planes2) {
                    if (i < B) v = hc[(int64_t)pr * B + i];
                    else v = x_cplx ? xc[(int64_t)pr * ldx + (i - B)] : mk(xr[(int64_t)pr * ldx + (i - B)], 0.0);
                } else {
                    const int ca = 2 * pr, cb = min(ca + 1, C - 1);
                    if (i < B) v = mk(hr[(int64_t)ca * B + i], hr[(int64_t)cb * B + i]);
                    else v = mk(xr[(int64_t)ca * ldx + (i - B)], xr[(int64_t)cb * ldx + (i - B)]);
                    if (ca + 1 >= C) v.y = 0.0;
                }
            }
            xv[j] = v;
        }
    };
    fetch(0);   // (issued ahead of the selection's dependent loads: the samples do not depend on the sets)
    int s0 = 0, s1 = 0, s2 = 0;   // sigma_t, sigma_(t-1), sigma_(t-2)
    int nu = 1, u1 = 0, u2 = 0;   // the distinct sets of the window, oldest role first: s2, then u1, then u2
    if (BANK) {
        const int p1 = min(sel[0], S - 1), p2 = min(sel[1], S - 1);
        s0 = set_p ? min(max(*set_p, 0), S - 1) : max(p1, 0);
        s1 = p1 < 0 ? s0 : p1;
        s2 = p2 < 0 ? s1 : p2;
        if (s1 != s2) { u1 = s1; nu = 2; if (s0 != s1 && s0 != s2) { u2 = s0; nu = 3; } }
        else if (s0 != s1) { u1 = s0; nu = 2; }
    }
    const double invB = 1.0 / (double)B;
    const int nr = (npairs + NTP - 1) / NTP;   // rounds per set
    // one loop over (set, round): per set the plain stream's rounds, the sums carried from set to set
    int p0 = 0, q = 0;
#pragma unroll 1
    for (int it = 0; it < nu * nr; ++it) {
        const int np = min(NTP, npairs - p0);
        const int set = q == 0 ? s2 : q == 1 ? u1 : u2;
        // the gain shapes of the window's two halves under this set: its gains in block t - 1 and in block t
        const int ga = set == s1 ? (s1 == s2 ? DS_G_ONE : DS_G_R) : set == s2 ? DS_G_1MR : DS_G_ZERO;
        const int gb = set == s0 ? (s0 == s1 ? DS_G_ONE : DS_G_R) : set == s1 ? DS_G_1MR : DS_G_ZERO;
        const cplx* Wp = Wf + (((int64_t)set * 2 + e) * P + part) * Cp * Pf;
        __syncthreads();   // the previous round's spectra have been read (first round: the twiddles are written)
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int idx = tid + DS_NT * j;
            const int t = idx >> log2n, i = idx & mask;
            if (BANK) {   // the gains, on the way from the registers to LDS
                const int shape = i < B ? ga : gb;
                if (shape != DS_G_ONE) {   // (a gain of 1 is not multiplied: a constant index gives the plain stream's bits)
                    const double r = (double)((i & (B - 1)) + 1) * invB;   // exact: B is a power of two
                    const double g = shape == DS_G_R ? r : shape == DS_G_1MR ? 1.0 - r : 0.0;
                    xv[j].x *= g; xv[j].y *= g;
                }
            }
            if (t < np) buf[lds_fft_ix<true>((t << log2n) + (int)bitrev((unsigned)i, log2n))] = xv[j];
        }
        int p0n = p0 + NTP, qn = q;
        if (p0n >= npairs) { p0n = 0; ++qn; }
        if (qn < nu) fetch(p0n);
        __syncthreads();
        lds_fft_stages<false, true>(buf, tws, Nf, log2n, np);
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const int idx = tid + DS_NT * u;
            const int g = idx / Pf, k = idx - g * Pf;
            if (g < G) {
                const cplx* wk = Wp + k;
#pragma unroll 1
                for (int t = g; t < np; t += G) {   // (ascending pairs per group, the groups summed in order below: a fixed order)
                    const int pr = p0 + t;
                    const int ca = planes2 ? pr : 2 * pr, cb = planes2 ? pr + C : 2 * pr + 1;
                    cplx pa, pb;
                    ds_unpack(buf[lds_fft_ix<true>((t << log2n) + k)], conj(buf[lds_fft_ix<true>((t << log2n) + ((Nf - k) & mask))]), pa, pb);
                    cfma(acc[u], pa, wk[(int64_t)ca * Pf]);
                    if (cb < Cp) cfma(acc[u], pb, wk[(int64_t)cb * Pf]);
                }
            }
        }
        p0 = p0n; q = qn;
    }
    __syncthreads();
    if (G > 1) {   // the groups' partial sums meet in LDS; group 0 adds them in the order of the groups
        const int g = tid / Pf, k = tid - g * Pf;
        if (g > 0 && g < G) buf[g * Pf + k] = acc[0];
        __syncthreads();
        if (g == 0) {
            for (int o = 1; o < G; ++o) { const cplx x = buf[o * Pf + k]; acc[0].x += x.x; acc[0].y += x.y; }
        }
    }
    const int pos = *pos_p;
    int slot = pos + part;
    if (slot >= P) slot -= P;
    cplx* dst = ring + ((int64_t)e * P + slot) * Pf;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
        const int k = tid + DS_NT * u;
        if (k < Pf) {
            if (part == P - 1) dst[k] = acc[u];   // the slot the previous block gave up
            else { const cplx old = dst[k]; dst[k] = mk(old.x + acc[u].x, old.y + acc[u].y); }
        }
    }
}

// workgroup 0: out[i] (left), out[ldo + i] (right) = the last B samples of IFFT(ring slot `pos`) -- both ears in one packed
// transform, Y_L + i Y_R with Y_e[N - k] = conj(Y_e[k]) -- and pos <- (pos + 1) mod P; with a bank (sel not null) the same thread
// moves the selection on: sel <- (this block's index as the forward kernel took it, the previous block's).  The other workgroups:
// hist <- the block.  GROUP: grid (1 + ncopy, L): listener l = blockIdx.y, the pointers as in the forward kernel, out at + l lso
template <bool GROUP>
__global__ void __launch_bounds__(DS_NT) ds_inverse_kernel(const cplx* __restrict__ ring_, int B, int log2n, int P, int* __restrict__ pos_p_,
                                                           double* __restrict__ out_, int64_t ldo, const void* __restrict__ xnew_, int x_cplx,
                                                           int64_t ldx, void* __restrict__ hist_, int planes2, int C,
                                                           const int* __restrict__ set_p_, int* __restrict__ sel_, int S, DsStrides<GROUP> ls) {
    const int tid = threadIdx.x;
    int64_t l = 0;   // the listener
    if constexpr (GROUP) l = blockIdx.y;
    if (blockIdx.x > 0) {
        const int64_t total = (int64_t)C * B;
        const double* xr = reinterpret_cast<const double*>(xnew_);
        double* hist = reinterpret_cast<double*>(hist_);
        if constexpr (GROUP) { xr += l * ls.lsx * (x_cplx ? 2 : 1); hist += l * total * (planes2 ? 2 : 1); }
        const cplx* xc = reinterpret_cast<const cplx*>(xr);
        for (int64_t idx = (int64_t)(blockIdx.x - 1) * DS_NT + tid; idx < total; idx += (int64_t)(gridDim.x - 1) * DS_NT) {
            const int64_t c = idx >> (log2n - 1), i = idx & (B - 1);
            if (planes2) reinterpret_cast<cplx*>(hist)[idx] = x_cplx ? xc[c * ldx + i] : mk(xr[c * ldx + i], 0.0);
            else hist[idx] = xr[c * ldx + i];
        }
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const int Nf = 2 * B, Pf = B + 1;
    cplx* buf = reinterpret_cast<cplx*>(dyn);      // [Nf], padded
    cplx* tws = buf + (Nf + Nf / 16);               // [Nf / 2]
    const cplx* ring = ring_;
    int* pos_p = pos_p_;
    int* sel = sel_;
    const int* set_p = set_p_;
    double* out = out_;
    if constexpr (GROUP) {
        ring += l * 2 * P * Pf;
        pos_p += l * ls.lpos;
        if (sel) sel += l * ls.lpos;
        if (set_p) set_p += l * ls.lset;
        out += l * ls.lso;
    }
    const int pos = *pos_p;
    int sel_new0 = 0, sel_new1 = 0;   // the selection after this block, read ahead of the transform
    if (sel) {
        const int p1 = min(sel[0], S - 1);
        sel_new0 = set_p ? min(max(*set_p, 0), S - 1) : max(p1, 0);
        sel_new1 = p1 < 0 ? sel_new0 : p1;
    }
    ds_twiddles(tws, Nf);
    const cplx* yl = ring + (int64_t)pos * Pf;
    const cplx* yr = ring + ((int64_t)P + pos) * Pf;
    for (int k = tid; k < Pf; k += DS_NT) {
        const cplx l = yl[k], r = yr[k];
        buf[lds_fft_ix<true>((int)bitrev((unsigned)k, log2n))] = mk(l.x - r.y, l.y + r.x);
        if (k > 0 && k < B) buf[lds_fft_ix<true>((int)bitrev((unsigned)(Nf - k), log2n))] = mk(l.x + r.y, r.x - l.y);
    }
    __syncthreads();
    lds_fft_stages<true, true>(buf, tws, Nf, log2n, 1);
    const double scale = 1.0 / (double)Nf;
    for (int i = tid; i < B; i += DS_NT) {
        const cplx y = buf[lds_fft_ix<true>(B + i)];
        out[i] = y.x * scale;
        out[ldo + i] = y.y * scale;
    }
    if (tid == 0) {
        *pos_p = pos + 1 == P ? 0 : pos + 1;
        if (sel) { sel[1] = sel_new1; sel[0] = sel_new0; }
    }
}

void ds_attributes() {
    static PerDeviceOnce once;
    if (!once.first()) return;
#define EMAGLS_DS_ATTR(K) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024))
    EMAGLS_DS_ATTR(ds_filter_kernel);
    EMAGLS_DS_ATTR(ds_inverse_kernel<false>);
    EMAGLS_DS_ATTR(ds_inverse_kernel<true>);
#define EMAGLS_DS_ATTR_KU(KU) EMAGLS_DS_ATTR((ds_forward_kernel<KU, false, false>)); EMAGLS_DS_ATTR((ds_forward_kernel<KU, true, false>)); \
                              EMAGLS_DS_ATTR((ds_forward_kernel<KU, false, true>)); EMAGLS_DS_ATTR((ds_forward_kernel<KU, true, true>))
    EMAGLS_DS_ATTR_KU(1);
    EMAGLS_DS_ATTR_KU(2);
    EMAGLS_DS_ATTR_KU(3);
    EMAGLS_DS_ATTR_KU(5);
#undef EMAGLS_DS_ATTR_KU
#undef EMAGLS_DS_ATTR
}

}  // namespace

bool decode_stream_block_ok(int64_t B) { return B >= 64 && B <= 2048 && (B & (B - 1)) == 0; }

void launch_partition_spectra(const double* wpl, int Cp, int64_t len, int B, int P, int64_t Z, cplx* Wf, hipStream_t st) {
    ds_attributes();
    constexpr int64_t kPerLaunch = 32768;   // sets of planes per launch: grid.z stays below 65536
    for (int64_t z0 = 0; z0 < Z; z0 += kPerLaunch) {
        const dim3 grid((unsigned)((Cp + 1) / 2), (unsigned)P, (unsigned)std::min<int64_t>(kPerLaunch, Z - z0));
        ds_filter_kernel<<<grid, DS_NT, ds_single_lds(B), st>>>(wpl + z0 * Cp * len, Cp, len, B, ds_log2(2 * B), P,
                                                               Wf + z0 * P * Cp * (int64_t)(B + 1));
        KERNEL_CHECK();
    }
}

void launch_decode_stream_filters(const double* wpl, int Cp, int64_t len, int B, int P, int64_t S, cplx* Wf, hipStream_t st) {
    // the kernel's "ear" index runs over the 2 S (set, ear) pairs: wpl [S][2] and Wf [S][2] are both laid out that way
    launch_partition_spectra(wpl, Cp, len, B, P, 2 * S, Wf, st);
}

void launch_decode_stream_block(const DecodeStreamState& s, const void* x, bool x_cplx, int64_t ldx, const int* set, int standing, double* out,
                                int64_t ldo, hipStream_t st, int64_t lsx, int lset, int64_t lso) {
    ds_attributes();
    const int log2n = ds_log2(2 * s.B), Pf = s.B + 1, ku = (Pf + DS_NT - 1) / DS_NT;
    const bool group = s.L > 1;   // (a group of one listener is the single stream)
    const dim3 grid((unsigned)s.P, 2, (unsigned)s.L);
    const size_t dyn = ds_forward_lds(s.B);
    int* sel = s.S > 1 ? s.pos + 1 : nullptr;   // (a bank of one set has no selection to keep)
    const DsListeners ls{lsx, s.S > 1 ? 3 : 1 /* ints of a listener's position and selection */, lset, lso};
    // a window the host knows to meet one set alone runs the plain instance on that set's spectra: the same arithmetic, without
    // the selection's loads (the inverse kernel still moves the selection on)
    const cplx* Wf = s.Wf + (standing > 0 ? (int64_t)standing * 2 * s.P * (s.planes2 ? 2 * s.C : s.C) * Pf : 0);
#define EMAGLS_DS_GO(KU, BANK, GROUP, LS) ds_forward_kernel<KU, BANK, GROUP><<<grid, DS_NT, dyn, st>>>(x, x_cplx ? 1 : 0, ldx, s.hist, s.C, s.planes2 ? 1 : 0, Wf, s.B, log2n, s.P, s.pos, s.ring, set, sel, s.S, LS)
#define EMAGLS_DS_KU(BANK, GROUP, LS) if (ku == 1) EMAGLS_DS_GO(1, BANK, GROUP, LS); else if (ku == 2) EMAGLS_DS_GO(2, BANK, GROUP, LS); else if (ku == 3) EMAGLS_DS_GO(3, BANK, GROUP, LS); else EMAGLS_DS_GO(5, BANK, GROUP, LS)
    if (group) { if (sel) { EMAGLS_DS_KU(true, true, ls); } else { EMAGLS_DS_KU(false, true, ls); } }
    else if (sel && standing < 0) { EMAGLS_DS_KU(true, false, DsSingle{}); } else { EMAGLS_DS_KU(false, false, DsSingle{}); }
#undef EMAGLS_DS_KU
#undef EMAGLS_DS_GO
    KERNEL_CHECK();
    const unsigned ncopy = (unsigned)std::min<int64_t>(32, ceil_div((int64_t)s.C * s.B, 4 * DS_NT));
    if (group)
        ds_inverse_kernel<true><<<dim3(1 + ncopy, (unsigned)s.L), DS_NT, ds_single_lds(s.B), st>>>(s.ring, s.B, log2n, s.P, s.pos, out, ldo, x, x_cplx ? 1 : 0, ldx, s.hist,
                                                                                             s.planes2 ? 1 : 0, s.C, set, sel, s.S, ls);
    else
        ds_inverse_kernel<false><<<1 + ncopy, DS_NT, ds_single_lds(s.B), st>>>(s.ring, s.B, log2n, s.P, s.pos, out, ldo, x, x_cplx ? 1 : 0, ldx, s.hist,
                                                                         s.planes2 ? 1 : 0, s.C, set, sel, s.S, DsSingle{});
    KERNEL_CHECK();
}

}  // namespace emagls
