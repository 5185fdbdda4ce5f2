// The array encoder inside the rotation launch of an encoded decode stream:
//     s_c[t] = sum_m enc[c][m] x[m][t],  accumulated from 0 with fma, m ascending, in FP64, real and imaginary part as separate chains
// (the arithmetic is part of the interface: an identity encoder gives the plain stream's bits).
// A workgroup of ENC_NT threads encodes a tile of ENC_T samples: thread = (sample t = tid % ENC_T, channel group g = tid / ENC_T),
// so a wave holds one g and 64 consecutive samples: its loads of the microphone block are contiguous and its reads of enc, staged
// once in LDS as [C][M], are broadcasts.  The thread keeps the sums of its channels g, g + ENC_G, ... (at most ENC_J of them, in
// registers) while m runs once over the microphones.
#pragma once
#include "common.hpp"

namespace emagls {

constexpr int ENC_T = 64;                   // samples of a tile (the smallest block of a decode stream)
constexpr int ENC_NT = 256;                 // threads of a workgroup
constexpr int ENC_G = ENC_NT / ENC_T;       // channel groups
constexpr int ENC_MAX = 64;                 // most microphones, most channels
constexpr int ENC_J = ENC_MAX / ENC_G;      // channels of a thread

// enc [C][M] device (interleaved complex when EC); x: the microphone block, microphone m at x + m ldx, n samples
struct EncIn { const double* enc; int M; const double* x; int64_t ldx; };

template <bool EC> using EncVal = std::conditional_t<EC, cplx, double>;

// bytes of LDS: enc, and behind it a tile [C][ENC_T] for the kernels that keep the encoded samples there
inline size_t enc_lds_bytes(int C, int M, bool ec, bool tile) {
    return esz(ec) * (size_t)C * M + (tile ? esz(ec) * (size_t)C * ENC_T : 0);
}

// every thread of the workgroup; st(c, t_local, value) for the channels of this thread, sample t0 + t_local < n
template <bool EC, typename St>
__device__ __forceinline__ void encode_tile(const EncIn& e, int C, int64_t t0, int64_t n, EncVal<EC>* __restrict__ enc_s, St st) {
    using V = EncVal<EC>;
    constexpr int SU = 4, MU = 8;   // loads in flight: of the staging, of the microphones
    const int tid = threadIdx.x, M = e.M, CM = C * M;
    {
        const V* __restrict__ src = reinterpret_cast<const V*>(e.enc);
        for (int i0 = tid; i0 < CM; i0 += SU * ENC_NT) {
            V v[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) v[u] = src[min(i0 + u * ENC_NT, CM - 1)];
#pragma unroll
            for (int u = 0; u < SU; ++u)
                if (i0 + u * ENC_NT < CM) enc_s[i0 + u * ENC_NT] = v[u];
        }
    }
    __syncthreads();
    const int t = tid & (ENC_T - 1);
    const int g = __builtin_amdgcn_readfirstlane(tid / ENC_T);   // uniform over the wave: the guards below are scalar branches
    const int nj = g < C ? (C - g + ENC_G - 1) / ENC_G : 0;      // channels g, g + ENC_G, ... < C
    const bool live = t0 + t < n;
    const double* __restrict__ xp = e.x + (live ? t0 + t : 0);
    V acc[ENC_J];
#pragma unroll
    for (int j = 0; j < ENC_J; ++j) acc[j] = V{};
    for (int m0 = 0; m0 < M; m0 += MU) {
        double xv[MU];   // MU microphones' samples are requested before the first is used (past M: the last one again, not used)
#pragma unroll
        for (int u = 0; u < MU; ++u) xv[u] = xp[(int64_t)min(m0 + u, M - 1) * e.ldx];
#pragma unroll
        for (int u = 0; u < MU; ++u) {
            if (m0 + u < M) {
#pragma unroll
                for (int j = 0; j < ENC_J; ++j)
                    if (j < nj) cfma(acc[j], enc_s[(g + ENC_G * j) * M + m0 + u], xv[u]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < ENC_J; ++j)
            if (j < nj) st(g + ENC_G * j, t, acc[j]);
    }
}

}  // namespace emagls
