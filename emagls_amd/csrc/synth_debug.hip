// Debug entries of the operand synthesis (emagls_debug_synth_operand, emagls_debug_synth_cosines): the Chebyshev evaluation of the resident sweeps -- synth_group<GS>
// of synth_common.hpp, the function sweep_synth.hip, sweep_reg.hip and synth_ls_kernel call -- on coefficient rows and arguments
// the caller supplies, so that a test can hold g(x) = E + O and g(-x) = E - O against a high-precision sum directly; and the argument
// 2 cos(direction, microphone) the sweeps form from the angles (synth_x2).
#include "device_mem.hpp"
#include "synth_common.hpp"

namespace emagls {

namespace {

constexpr int SD_NT = 256;

// One workgroup = one bin (blockIdx.y) x SD_NT groups of GS arguments.  The bin's row is staged in LDS as the sweeps stage theirs
// (16-byte aligned, one thread per coefficient); a thread's GS units are the arguments GS g .. GS g + GS - 1 (beyond nx: x = 0,
// evaluated and not stored).
template <int GS>
__global__ void __launch_bounds__(SD_NT) synth_operand_debug_kernel(const cplx* __restrict__ bsc, int nord_pad, const double* __restrict__ x, int64_t nx,
                                                                    cplx* __restrict__ gp, cplx* __restrict__ gm) {
    __shared__ __attribute__((aligned(16))) cplx bs[SY_NORD];
    const int tid = threadIdx.x;
    const int64_t kb = blockIdx.y;
    if (tid < nord_pad) bs[tid] = bsc[kb * nord_pad + tid];
    __syncthreads();
    const int64_t q0 = ((int64_t)blockIdx.x * SD_NT + tid) * GS;
    double x2[GS];
    cplx accE[GS], accO[GS];
#pragma unroll
    for (int i = 0; i < GS; ++i) x2[i] = q0 + i < nx ? 2.0 * x[q0 + i] : 0.0;   // (2x: the factor of the Chebyshev recurrence)
    synth_group<GS>(x2, accE, accO, bs, nord_pad);
#pragma unroll
    for (int i = 0; i < GS; ++i) {
        if (q0 + i < nx) {
            gp[kb * nx + q0 + i] = accE[i] + accO[i];
            gm[kb * nx + q0 + i] = accE[i] - accO[i];
        }
    }
}

// the sweeps' argument: x2[d][j] = synth_x2 of direction d and microphone j, from the angles as the sweeps form it
__global__ void __launch_bounds__(SD_NT) synth_cosines_debug_kernel(const double* __restrict__ dir_azi, const double* __restrict__ dir_zen, int64_t nd,
                                                                    const double* __restrict__ mic_azi, const double* __restrict__ mic_zen, int nm,
                                                                    double* __restrict__ x2) {
    const int64_t q = (int64_t)blockIdx.x * SD_NT + threadIdx.x;
    if (q >= nd * nm) return;
    const int64_t d = q / nm;
    const int j = (int)(q % nm);
    double sd, cd, sm, cm;
    synth_zen(dir_zen[d], sd, cd);
    synth_zen(mic_zen[j], sm, cm);
    x2[q] = synth_x2(sd, cd, sm, cm, dir_azi[d] - mic_azi[j]);
}

}  // namespace

void synth_cosines_debug(const double* dir_azi, const double* dir_zen, int64_t ndirs, const double* mic_azi, const double* mic_zen, int nmics, double* x2) {
    if (!dir_azi || !dir_zen || !mic_azi || !mic_zen || !x2) throw Error(1, "null pointer");
    if (ndirs < 1 || ndirs > ((int64_t)1 << 20) || nmics < 1 || nmics > 64) throw Error(1, "1 to 2^20 directions, 1 to 64 microphones");
    const size_t nb_d = sizeof(double) * (size_t)ndirs, nb_m = sizeof(double) * (size_t)nmics, nb_x = nb_d * (size_t)nmics;
    DevMem m_da(nb_d), m_dz(nb_d), m_ma(nb_m), m_mz(nb_m), m_x(nb_x);
    double *d_da = m_da.get<double>(), *d_dz = m_dz.get<double>(), *d_ma = m_ma.get<double>(), *d_mz = m_mz.get<double>(), *d_x = m_x.get<double>();
    HIP_CHECK(hipMemcpy(d_da, dir_azi, nb_d, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_dz, dir_zen, nb_d, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_ma, mic_azi, nb_m, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_mz, mic_zen, nb_m, hipMemcpyHostToDevice));
    synth_cosines_debug_kernel<<<(unsigned)ceil_div(ndirs * nmics, (int64_t)SD_NT), SD_NT>>>(d_da, d_dz, ndirs, d_ma, d_mz, nmics, d_x);
    KERNEL_CHECK();
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(x2, d_x, nb_x, hipMemcpyDeviceToHost));
}

void synth_operand_debug(const void* bsc, int nbins, int nord_pad, const double* x, int64_t nx, int gs, void* g_plus, void* g_minus) {
    if (!bsc || !x || !g_plus || !g_minus) throw Error(1, "null pointer");
    if (nord_pad < 2 || nord_pad > SY_NORD || (nord_pad & 1)) throw Error(1, "nord_pad must be even, at least 2 and at most 96");
    if (gs < 2 || gs > 4) throw Error(1, "the group size is 2, 3 or 4");
    if (nbins < 1 || nbins > 65535 || nx < 1 || nx > ((int64_t)1 << 24)) throw Error(1, "1 to 65535 bins, 1 to 2^24 arguments");
    const size_t nb_c = sizeof(cplx) * (size_t)nbins * nord_pad, nb_x = sizeof(double) * (size_t)nx, nb_g = sizeof(cplx) * (size_t)nbins * (size_t)nx;
    DevMem m_c(nb_c), m_x(nb_x), m_p(nb_g), m_m(nb_g);
    cplx *d_c = m_c.get<cplx>(), *d_p = m_p.get<cplx>(), *d_m = m_m.get<cplx>();
    double* d_x = m_x.get<double>();
    HIP_CHECK(hipMemcpy(d_c, bsc, nb_c, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_x, x, nb_x, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)ceil_div(ceil_div(nx, (int64_t)gs), (int64_t)SD_NT), (unsigned)nbins);
    if (gs == 2) synth_operand_debug_kernel<2><<<grid, SD_NT>>>(d_c, nord_pad, d_x, nx, d_p, d_m);
    else if (gs == 3) synth_operand_debug_kernel<3><<<grid, SD_NT>>>(d_c, nord_pad, d_x, nx, d_p, d_m);
    else synth_operand_debug_kernel<4><<<grid, SD_NT>>>(d_c, nord_pad, d_x, nx, d_p, d_m);
    KERNEL_CHECK();
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(g_plus, d_p, nb_g, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(g_minus, d_m, nb_g, hipMemcpyDeviceToHost));
}

}  // namespace emagls
