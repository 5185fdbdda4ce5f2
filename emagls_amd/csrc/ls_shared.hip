// Least-squares rows of a geometry-sharing batch from ONE kept regularised inverse (lib/getEMagLsFilters.m:94):
//     W(k,:) = H(k,:) Y_reg_inv_k        for the bins 1 .. ls_end-1 below k_cut.
// A single design never forms Y_reg_inv_k of those bins: it carries its HRIR set through the factors (H conj(Y_c) -> R^-1 -> Z_k on
// the Householder route, u = H conj(g_k) -> (u Pm^T) conj(M_k) on the Gram route), which is the cheaper order for ONE set.  A batch
// of HRIR sets on one geometry repeats the geometry's share of that for every set and every execute; here the operand
//     Yls[k-1][c][d] = Y_reg_inv_k[d][c]
// is formed once per geometry (the cold run) and every set's rows are one D-long product per bin against it:
//   Householder-route bins:  conj(Y_c) (Z_k R^-H), by launch_zsolve_flagged / launch_yri_accurate on a copy of plan 0's Z
//   Gram-route bins (synthesising designs):  conj(g_k) Pm^T conj(M_k), g_k from the angles by the series of synth_ls_kernel
//   (yls_gram_kernel below)
// and ls_rows_kernel is the product for all lanes of a launch.
#include "kernels.hpp"
#include "persist_common.hpp"
#include "synth_common.hpp"

namespace emagls {

namespace {

// Yls of one Gram-route bin: thread = direction d.  t[c'] = sum_j conj(g_k[d][j]) Pm[c'][j] over the microphone rows j in the chain's
// row order (units: antipodal pairs first, g(x) = E + O and g(-x) = E - O, then single microphones -- as synth_ls_kernel), then
// Yls[c][d] = sum_c' t[c'] conj(M_k[c'][c]).
__global__ void __launch_bounds__(256) yls_gram_kernel(const cplx* __restrict__ bsc, int nord_pad, const double* __restrict__ dir_azi,
                                                       const double* __restrict__ dir_zen, const double* __restrict__ mic_azi,
                                                       const double* __restrict__ mic_zen, const int* __restrict__ smap, const double* __restrict__ Pm,
                                                       const cplx* __restrict__ Mw, int D, int nOut, int kb_lo, cplx* __restrict__ Yls, int64_t ldD) {
    __shared__ __attribute__((aligned(16))) cplx bs[SY_NORD];
    __shared__ double pm[PS_CMAX][PS_CMAX + 1];   // [c'][row], zero beyond nOut
    __shared__ cplx mks[PS_CMAX * PS_CMAX];       // conj(M_k)[c'][c]
    const int tid = threadIdx.x, kb = kb_lo + (int)blockIdx.y;
    const int npr = smap[32], nsg = smap[33];
    if (tid < nord_pad) bs[tid] = bsc[(int64_t)kb * nord_pad + tid];
    for (int idx = tid; idx < PS_CMAX * PS_CMAX; idx += 256) {
        const int c = idx / PS_CMAX, j = idx % PS_CMAX;
        pm[c][j] = c < nOut ? Pm[c * PS_CMAX + j] : 0.0;
    }
    const cplx* Mk = Mw + (int64_t)(kb - 1) * nOut * nOut;
    for (int idx = tid; idx < nOut * nOut; idx += 256) mks[idx] = conj(Mk[idx]);
    __syncthreads();
    const int d = (int)blockIdx.x * 256 + tid, dc = d < D ? d : D - 1;
    double sd, cd;
    synth_zen(dir_zen[dc], sd, cd);
    const double daz = dir_azi[dc];
    cplx t[PS_CMAX];
#pragma unroll
    for (int c = 0; c < PS_CMAX; ++c) t[c] = mk(0, 0);
    for (int u = 0; u < npr + nsg; ++u) {
        const bool paired = u < npr;
        const int row = paired ? 2 * u : 2 * npr + (u - npr);
        const int jm = smap[row];
        double sm, cm;
        synth_zen(mic_zen[jm], sm, cm);
        double x2[1];
        x2[0] = synth_x2(sd, cd, sm, cm, daz - mic_azi[jm]);
        cplx accE[1], accO[1];
        synth_group<1>(x2, accE, accO, bs, nord_pad);
        const cplx gA = conj(accE[0] + accO[0]), gB = conj(accE[0] - accO[0]);
#pragma unroll
        for (int c = 0; c < PS_CMAX; ++c) cfma(t[c], gA, pm[c][row]);
        if (paired) {
#pragma unroll
            for (int c = 0; c < PS_CMAX; ++c) cfma(t[c], gB, pm[c][row + 1]);
        }
    }
    if (d >= D) return;
    for (int c = 0; c < nOut; ++c) {
        cplx y = mk(0, 0);
#pragma unroll
        for (int cp = 0; cp < PS_CMAX; ++cp)
            if (cp < nOut) cfma(y, t[cp], mks[cp * nOut + c]);
        Yls[((int64_t)(kb - 1) * nOut + c) * ldD + d] = y;
    }
}

// W[lane][e][kb][c] = sum_d Hc[lane][e][kb][d] Yls[kb-1][c][d].  One workgroup = one bin x LR_ROWS rows (8 lanes x 2 ears), ALL
// directions: Yls_kb is read once for the rows a workgroup serves.  Tiles of LR_DT directions pass through LDS (the next tile is
// requested before the current one's arithmetic); thread = (channel c, slice ds of the tile), LR_DT / LR_NS directions per tile,
// LR_ROWS accumulators.  The order of addition of a row is fixed by D alone -- per slice the tiles in turn, then the slices 0 .. LR_NS-1 --
// whatever the number of lanes and wherever the row's lane sits (cold and warm runs, chunks of any size: the same bits).
constexpr int LR_NT = 512, LR_ROWS = 16, LR_DT = 64, LR_NS = LR_NT / 32, LR_DPT = LR_DT / LR_NS, LR_YLD = LR_DT + 1;
__global__ void __launch_bounds__(LR_NT) ls_rows_kernel(const cplx* __restrict__ Hc, int64_t ldH, int n_c, const cplx* __restrict__ Yls, int64_t ldD,
                                                        int D, int C, int P, cplx* __restrict__ W, int nlanes, size_t bstride) {
    __shared__ __attribute__((aligned(16))) cplx ys[32 * LR_YLD];          // [c][d]; afterwards the slices' sums [ds][4 rows][32]
    __shared__ __attribute__((aligned(16))) cplx hs[LR_ROWS * LR_DT];      // [row][d]
    static_assert(LR_NS * 4 * 32 <= 32 * LR_YLD, "the slices' sums of four rows fit the tile buffer");
    const int tid = threadIdx.x, kb = 1 + (int)blockIdx.x, lane0 = (int)blockIdx.y * (LR_ROWS / 2);
    const int c = tid & 31, ds = tid >> 5;
    const int lrow = tid >> 6, lcol = tid & 63;   // loads: 8 rows x 64 directions per pass
    const cplx* Yk = Yls + (int64_t)(kb - 1) * C * ldD;
    const cplx* hrow[2];
    bool hok[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int r = q * 8 + lrow, lane = lane0 + (r >> 1);
        hok[q] = lane < nlanes;
        hrow[q] = boffz(Hc, bstride, hok[q] ? (unsigned)lane : 0u) + ((int64_t)(r & 1) * n_c + kb) * ldH;
    }
    cplx yr[4], hr[2];
    auto load = [&](int d0) __attribute__((always_inline)) {
        const int d = d0 + lcol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = q * 8 + lrow;
            yr[q] = (row < C && d < D) ? Yk[(int64_t)row * ldD + d] : mk(0, 0);
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) hr[q] = (hok[q] && d < D) ? hrow[q][d] : mk(0, 0);
    };
    cplx acc[LR_ROWS];
#pragma unroll
    for (int r = 0; r < LR_ROWS; ++r) acc[r] = mk(0, 0);
    load(0);
    for (int d0 = 0; d0 < D; d0 += LR_DT) {
        __syncthreads();   // (the previous tile's readers are done)
#pragma unroll
        for (int q = 0; q < 4; ++q) ys[(q * 8 + lrow) * LR_YLD + lcol] = yr[q];
#pragma unroll
        for (int q = 0; q < 2; ++q) hs[(q * 8 + lrow) * LR_DT + lcol] = hr[q];
        __syncthreads();
        if (d0 + LR_DT < D) load(d0 + LR_DT);
#pragma unroll
        for (int i = 0; i < LR_DPT; ++i) {
            const int dl = ds * LR_DPT + i;
            const cplx y = ys[c * LR_YLD + dl];
#pragma unroll
            for (int r = 0; r < LR_ROWS; ++r) cfma(acc[r], hs[r * LR_DT + dl], y);
        }
    }
    cplx* red = ys;
#pragma unroll
    for (int part = 0; part < LR_ROWS / 4; ++part) {
        __syncthreads();   // (the tiles, or the previous part's sums, have been read)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) red[(ds * 4 + rr) * 32 + c] = acc[part * 4 + rr];
        __syncthreads();
        if (tid < 4 * 32) {
            const int rr = tid >> 5, r = part * 4 + rr, lane = lane0 + (r >> 1), e = r & 1;
            cplx w = mk(0, 0);
            for (int s = 0; s < LR_NS; ++s) w += red[(s * 4 + rr) * 32 + c];
            if (c < C && lane < nlanes) boffz(W, bstride, (unsigned)lane)[((int64_t)e * P + kb) * C + c] = w;
        }
    }
}

}  // namespace

void launch_yls_gram(const void* bsc, int nord_pad, const double* dir_azi, const double* dir_zen, const double* mic_azi, const double* mic_zen,
                     const int* smap, const double* Pm, const void* Mw, int D, int nOut, int kb_lo, int kb_hi, void* Yls, int64_t ldD, hipStream_t st) {
    if (kb_hi <= kb_lo) return;
    if (nOut > PS_CMAX || nord_pad > SY_NORD) throw Error(2, "ls_shared: more than 32 channels or 95 orders");
    yls_gram_kernel<<<dim3((unsigned)ceil_div(D, 256), (unsigned)(kb_hi - kb_lo)), 256, 0, st>>>((const cplx*)bsc, nord_pad, dir_azi, dir_zen, mic_azi, mic_zen, smap, Pm,
                                                                                               (const cplx*)Mw, D, nOut, kb_lo, (cplx*)Yls, ldD);
    KERNEL_CHECK();
}
// the rows of the bins 1 .. ls_end-1 for the lanes of the launch context (batch_ctx: Hc and W move by its stride, Yls is one for all)
void launch_ls_shared_rows(const void* Hc, int64_t ldH, int ls_end, const void* Yls, int64_t ldD, int D, int C, int P, void* W, hipStream_t st) {
    if (ls_end <= 1) return;
    if (C > 32) throw Error(2, "ls_shared: more than 32 channels");
    const int nlanes = batch_ctx().n;
    ls_rows_kernel<<<dim3((unsigned)(ls_end - 1), (unsigned)ceil_div(2 * nlanes, LR_ROWS)), LR_NT, 0, st>>>((const cplx*)Hc, ldH, ls_end, (const cplx*)Yls, ldD, D, C, P,
                                                                                                          (cplx*)W, nlanes, batch_ctx().stride);
    KERNEL_CHECK();
}

}  // namespace emagls
