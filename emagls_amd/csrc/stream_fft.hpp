// What the block-streaming kernels share (decode_stream.hip, field_stream.hip): the workgroup size, the twiddles of a transform of
// Nf = 2B points, the split of a packed transform of two real signals, and the LDS sizes of a transform buffer.
#pragma once
#include "kernels.hpp"
#include "lds_fft.hpp"

namespace emagls {

constexpr int DS_NT = 512;     // threads of every kernel of the streams
constexpr int DS_ELEMS = 4096; // elements of the transform buffer: DS_ELEMS / Nf transforms per round, 8 loads per thread

__device__ __forceinline__ void ds_twiddles(cplx* tws, int Nf) {
    for (int j = threadIdx.x; j < Nf / 2; j += DS_NT) {
        double sn, cs;
        sincospi(-2.0 * (double)j / (double)Nf, &sn, &cs);   // (exact at the multiples of 1/4: Nf is a power of two)
        tws[j] = mk(cs, sn);
    }
}

// Z = FFT(a + i b) with real a, b:  A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2i)
__device__ __forceinline__ void ds_unpack(cplx z, cplx zr /* conj(Z[N-k]) */, cplx& pa, cplx& pb) {
    pa = mk(0.5 * (z.x + zr.x), 0.5 * (z.y + zr.y));
    pb = mk(0.5 * (z.y - zr.y), -0.5 * (z.x - zr.x));
}

// dynamic LDS of a round of DS_ELEMS / Nf transforms, and of a single one: the padded buffer and the twiddles
inline size_t ds_forward_lds(int B) { return sizeof(cplx) * ((size_t)DS_ELEMS + DS_ELEMS / 16 + (size_t)B); }
inline size_t ds_single_lds(int B) { const size_t Nf = 2 * (size_t)B; return sizeof(cplx) * (Nf + Nf / 16 + Nf / 2); }
inline int ds_log2(int Nf) { int l = 0; while ((1 << l) < Nf) ++l; return l; }

}  // namespace emagls
