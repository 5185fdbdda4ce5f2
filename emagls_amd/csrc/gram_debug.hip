// Debug entries of the Gram route (emagls_debug_gram, emagls_debug_gram_assemble, emagls_debug_gram_from_g, emagls_debug_gram_solve): the
// product's own launchers -- launch_gram, launch_gram_kmat, launch_gram_gemm, launch_gram_from_g, launch_gram_solve, with their dispatch
// and their refusals -- on arrays the caller supplies, so that a test can hold Gy, K, the coefficients, A_k and the direct inverse against
// sums of higher precision step by step.  No kernel is launched from here and no dispatch is repeated here: an entry validates, allocates,
// copies, calls the launcher, synchronises, copies back and frees.  What a plan zero-fills once (the rows D ... gram_dpad of Yc, Kmat, Cf)
// is zero-filled here with the plan's padded leading dimensions; everything else a kernel writes starts as the sentinel.
#include "../../include/emagls.h"
#include "debug_common.hpp"
#include "kernels.hpp"

namespace emagls {

using debug::copy;
using debug::filled;
using debug::fill_sentinel;
using debug::sentinel;

namespace {
constexpr size_t GD_CAP = (size_t)1 << 30;
inline size_t up(size_t v, size_t m) { return (v + m - 1) / m * m; }
int* filled_minus_one(Scratch& b, size_t n) {
    int* p = b.get<int>(sizeof(int) * std::max<size_t>(n, 1));
    HIP_CHECK(hipMemset(p, 0xff, sizeof(int) * std::max<size_t>(n, 1)));
    return p;
}
}  // namespace

void gram_debug(const void* Yc, int64_t D, int S, int64_t ld, int is_cplx, int Sh, void* G, void* R) {
    if (!Yc || !G || !R) throw Error(1, "null pointer");
    if (is_cplx != 0 && is_cplx != 1) throw Error(1, "debug gram: is_cplx is 0 or 1");
    if (S < 1 || ld < S || ld > 8192 || Sh < 1 || Sh > S || D < 1 || D > 65536) throw Error(1, "debug gram: 1 <= Sh <= S <= ld <= 8192 and 1 <= D <= 65536");
    const size_t e = esz(is_cplx != 0), ss = (size_t)S * S, dpad = (size_t)gram_dpad(D, S), ks = (size_t)gram_ksplit(D, S);
    if ((dpad * (size_t)ld + ks * ss + ss + (size_t)Sh * Sh) * e > GD_CAP) throw Error(1, "debug gram: more than 1 GiB of device memory");
    const size_t w = e / sizeof(double);
    fill_sentinel(G, w * ss);
    fill_sentinel(R, w * (size_t)Sh * Sh);
    Scratch b;
    char* dY = filled<char>(b, dpad * (size_t)ld * e, 0.0);   // (rows D ... gram_dpad: zero, as the plan leaves them)
    HIP_CHECK(hipMemcpy(dY, Yc, (size_t)D * ld * e, hipMemcpyHostToDevice));
    char* dGp = filled<char>(b, ks * ss * e, sentinel());
    char* dG = filled<char>(b, ss * e, sentinel());
    char* dR = filled<char>(b, (size_t)Sh * Sh * e, sentinel());
    launch_gram(dY, D, S, ld, is_cplx != 0, dGp, dG, dR, Sh, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(G, dG, ss * e, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(R, dR, (size_t)Sh * Sh * e, hipMemcpyDeviceToHost));
}

void gram_assemble_debug(const void* Gy, const void* E, int ldE, const void* bn, int C, int nOrd, int P, int kb0, int nbins, int is_cplx,
                         const double* Kmat_in, void* F, double* Kmat, double* Cf, double* Apk) {
    const bool gemm_only = Kmat_in != nullptr;
    if (!bn || !Kmat || !Cf || !Apk) throw Error(1, "null pointer");
    if (gemm_only ? (Gy || E || F) : (!Gy || !E)) throw Error(1, "debug gram assemble: either Gy and E, or Kmat_in alone (no F then)");
    if (is_cplx != 0 && is_cplx != 1) throw Error(1, "debug gram assemble: is_cplx is 0 or 1");
    if (C < 1 || C > 32 || nOrd < 1 || nOrd > 96) throw Error(1, "debug gram assemble: 1 <= C <= 32 and 1 <= nOrd <= 96");
    if (nbins < 1 || kb0 < 0 || P < kb0 + nbins || P > 8192) throw Error(1, "debug gram assemble: 1 <= nbins, 0 <= kb0 and kb0 + nbins <= P <= 8192");
    const int S = nOrd * nOrd;
    if (!gemm_only && (ldE < S || ldE > 16384)) throw Error(1, "debug gram assemble: nOrd^2 <= ldE <= 16384");
    const size_t e = esz(is_cplx != 0), w = e / sizeof(double);
    const size_t Kp = up((size_t)S, 4), ldK = up((size_t)C * C, 64), ldC = up((size_t)P, 64);
    const size_t nF = gemm_only ? 0 : (size_t)nOrd * C * ldE, nGy = gemm_only ? 0 : (size_t)S * S, nE = gemm_only ? 0 : (size_t)C * ldE;
    if ((nF + nGy + nE) * e + (Kp * (ldK + ldC) + (size_t)nbins * ldK) * sizeof(double) + (size_t)P * nOrd * sizeof(cplx) > GD_CAP)
        throw Error(1, "debug gram assemble: more than 1 GiB of device memory");
    if (F) fill_sentinel(F, w * nF);
    fill_sentinel(Kmat, Kp * ldK);
    fill_sentinel(Cf, Kp * ldC);
    fill_sentinel(Apk, (size_t)nbins * ldK);
    Scratch b;
    const cplx* dbn = copy<cplx>(b, bn, (size_t)P * nOrd);
    double* dK = gemm_only ? copy<double>(b, Kmat_in, Kp * ldK) : filled<double>(b, Kp * ldK, 0.0);   // (rows beyond nOrd^2 stay zero)
    double* dCf = filled<double>(b, Kp * ldC, 0.0);
    double* dA = filled<double>(b, (size_t)nbins * ldK, sentinel());
    char* dF = nullptr;
    if (!gemm_only) {
        const char* dGy = copy<char>(b, Gy, nGy * e);
        const char* dE = copy<char>(b, E, nE * e);
        dF = filled<char>(b, nF * e, sentinel());
        launch_gram_kmat(dGy, dE, S, ldE, C, nOrd, is_cplx != 0, dF, ldE, dK, (int)ldK, nullptr);
    }
    launch_gram_gemm(dbn, nOrd, P, kb0, nbins, dCf, (int)ldC, dK, (int)ldK, C, dA, (int)ldK, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (F) HIP_CHECK(hipMemcpy(F, dF, nF * e, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(Kmat, dK, Kp * ldK * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(Cf, dCf, Kp * ldC * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(Apk, dA, (size_t)nbins * ldK * sizeof(double), hipMemcpyDeviceToHost));
}

void gram_from_g_debug(const void* G, int D, int C, int64_t ldD, int kb0, int g0, int nbins, double* Apk) {
    if (!G || !Apk) throw Error(1, "null pointer");
    if (C < 1 || C > 32 || D < 1 || ldD < D || ldD > 65536) throw Error(1, "debug gram from g: 1 <= C <= 32 and 1 <= D <= ldD <= 65536");
    if (g0 < 0 || kb0 < g0 || nbins < 1 || nbins > 8192 || kb0 > 8192) throw Error(1, "debug gram from g: 0 <= g0 <= kb0 <= 8192 and 1 <= nbins <= 8192");
    const size_t ldK = up((size_t)C * C, 64), g_stride = (size_t)C * ldD, slots = (size_t)(nbins + kb0 - g0);
    if (slots * g_stride * sizeof(cplx) + (size_t)nbins * ldK * sizeof(double) > GD_CAP) throw Error(1, "debug gram from g: more than 1 GiB of device memory");
    fill_sentinel(Apk, (size_t)nbins * ldK);
    Scratch b;
    const cplx* dG = copy<cplx>(b, G, slots * g_stride);
    double* dA = filled<double>(b, (size_t)nbins * ldK, sentinel());
    launch_gram_from_g(dG, (int64_t)g_stride, ldD, D, C, kb0, nbins, g0, dA, (int)ldK, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(Apk, dA, (size_t)nbins * ldK * sizeof(double), hipMemcpyDeviceToHost));
}

void gram_solve_debug(const double* Apk, int ldA, int C, int kb0, int nbins, double reg_c, void* Mw, void* R2w, double* sv, int* route, int* sweeps) {
    if (!Apk || !Mw || !R2w || !sv || !route || !sweeps) throw Error(1, "null pointer");
    if (C < 1 || C > 32 || ldA < C * C || ldA > 4096) throw Error(1, "debug gram solve: 1 <= C <= 32 and C^2 <= ldA <= 4096");
    if (kb0 < 1 || nbins < 1 || (int64_t)kb0 + nbins > 8192) throw Error(1, "debug gram solve: 1 <= kb0, 1 <= nbins and kb0 + nbins <= 8192");
    if (!(reg_c > 0.0) || !(reg_c <= 1.0)) throw Error(1, "debug gram solve: 0 < reg_c <= 1");
    const size_t P = (size_t)kb0 + nbins, cc = (size_t)C * C;
    fill_sentinel(Mw, 2 * P * cc);
    fill_sentinel(R2w, 2 * P * cc);
    fill_sentinel(sv, P * C);
    Scratch b;
    const double* dA = copy<double>(b, Apk, (size_t)nbins * ldA);
    cplx* dM = filled<cplx>(b, P * cc, sentinel());
    cplx* dR2 = filled<cplx>(b, P * cc, sentinel());
    double* dsv = filled<double>(b, P * C, sentinel());
    int* drt = filled_minus_one(b, P);
    int* dsw = filled_minus_one(b, P);
    launch_gram_solve(dA, ldA, C, kb0, nbins, reg_c, dM, dR2, dsv, drt, dsw, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(Mw, dM, P * cc * sizeof(cplx), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(R2w, dR2, P * cc * sizeof(cplx), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sv, dsv, P * C * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(route, drt, P * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sweeps, dsw, P * sizeof(int), hipMemcpyDeviceToHost));
}

}  // namespace emagls

extern "C" {

int emagls_debug_gram(const void* Yc, int64_t D, int S, int64_t ld, int is_cplx, int Sh, void* G, void* R) {
    return emagls::guarded_call([&] { emagls::gram_debug(Yc, D, S, ld, is_cplx, Sh, G, R); });
}

int emagls_debug_gram_assemble(const void* Gy, const void* E, int ldE, const void* bn, int C, int nOrd, int P, int kb0, int nbins, int is_cplx,
                               const double* Kmat_in, void* F, double* Kmat, double* Cf, double* Apk) {
    return emagls::guarded_call([&] { emagls::gram_assemble_debug(Gy, E, ldE, bn, C, nOrd, P, kb0, nbins, is_cplx, Kmat_in, F, Kmat, Cf, Apk); });
}

int emagls_debug_gram_from_g(const void* G, int D, int C, int64_t ldD, int kb0, int g0, int nbins, double* Apk) {
    return emagls::guarded_call([&] { emagls::gram_from_g_debug(G, D, C, ldD, kb0, g0, nbins, Apk); });
}

int emagls_debug_gram_solve(const double* Apk, int ldA, int C, int kb0, int nbins, double reg_c, void* Mw, void* R2w, double* sv, int* route,
                            int* sweeps) {
    return emagls::guarded_call([&] { emagls::gram_solve_debug(Apk, ldA, C, kb0, nbins, reg_c, Mw, R2w, sv, route, sweeps); });
}

}  // extern "C"
