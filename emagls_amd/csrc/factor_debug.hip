// Debug entries of the per-bin factor chain (emagls_debug_factor, emagls_debug_factor_gram, emagls_debug_wa_yri): the product's own
// launchers -- launch_factor, launch_wa_factor, launch_wa_factor_tiled (with launch_wa_ls behind them), launch_factor_jacobi_gram and
// launch_wa_yri, with their dispatch and their refusals -- on matrices the caller supplies, so that a test
// can hold Z_k, the singular values and M_k against a factorisation of higher precision shape by shape.  No kernel is launched from here
// and no dispatch is repeated here: an entry validates, allocates, copies, calls the launcher, synchronises, copies back and frees.
#include "../../include/emagls.h"
#include "args.hpp"
#include "debug_common.hpp"
#include "kernels.hpp"

namespace emagls {

using debug::copy;
using debug::filled;
using debug::fill_sentinel;
using debug::sentinel;

void factor_debug(const emagls_debug_factor_args& g) {
    const int S = g.S, C = g.C, ldS = g.ldS, nbins = g.nbins, kb0 = g.kb0, P = g.P;
    const bool dense = g.Xd != nullptr, tiled = g.path == 2, wide = g.path == 1 || tiled;
    if (!g.Z) throw Error(1, "debug factor: Z is required");
    if (dense == (g.Tn != nullptr)) throw Error(1, "debug factor: exactly one of Xd (dense) and Tn (assembled) is given");
    if (g.path < 0 || g.path > 2) throw Error(1, "debug factor: path is 0 (factor.hip), 1 (wide_array.hip) or 2 (wide_array.hip, tiled)");
    if (g.phases != 3 && g.phases != 12) throw Error(1, "debug factor: phases is 3 (one call) or 12 (phase 1, then phase 2)");
    if (tiled) {
        if (S < 1 || C < 1 || C > 32 || ldS < S || ldS > 16384 || nbins < 1 || nbins > 8)
            throw Error(1, "debug factor: the tiled path takes 1 <= S <= ldS <= 16384, 1 <= C <= 32 and 1 <= nbins <= 8");
    } else if (S < 1 || C < 1 || C > 64 || ldS < S || ldS > 4096) throw Error(1, "debug factor: 1 <= S <= ldS <= 4096 and 1 <= C <= 64");
    if (nbins < 1 || nbins > 4096 || kb0 < 0 || P < kb0 + nbins || P > 8192) throw Error(1, "debug factor: 1 <= nbins <= 4096 and kb0 + nbins <= P <= 8192");
    if (g.reg_mode != 0 && g.reg_mode != 1) throw Error(1, "debug factor: reg_mode is 0 (clip at reg_c s_max) or 1 (pinv tolerance)");
    if (!(g.reg_c >= 0.0) || !(g.reg_c <= 1.0) || !(g.tol_dim >= 0.0)) throw Error(1, "debug factor: 0 <= reg_c <= 1 and tol_dim >= 0");
    if (dense && (kb0 != 0 || (g.xd_stride != 0 && g.xd_stride != (int64_t)C * ldS))) throw Error(1, "debug factor: dense input has kb0 = 0 and xd_stride 0 or C ldS");
    if (!dense && (!g.bn || g.nOrders < 1 || g.nOrders > 1024)) throw Error(1, "debug factor: assembled input needs bn and 1 <= nOrders <= 1024");
    if (g.Hq && (!g.W || g.ldHq < S || g.ldHq > 16384 || g.ls_end < 0 || g.ls_end > P)) throw Error(1, "debug factor: Hq needs W, S <= ldHq <= 16384 and 0 <= ls_end <= P");
    if (wide && (!dense || g.reg_mode != 0 || g.phases != 3 || ldS % 64 != 0 || (g.Hq && g.hq_conj)))
        throw Error(1, "debug factor: the wide paths take dense input, reg_mode 0, phases 3, hq_conj 0, and ldS a multiple of 64");
    if (g.leaf_rows != 0 && (!tiled || g.leaf_rows < 1024 || g.leaf_rows > 4096)) throw Error(1, "debug factor: leaf_rows is 0, or 1024 ... 4096 on the tiled path");
    const WaTiling til = tiled ? wa_tiling(S, C, nbins, g.leaf_rows) : WaTiling{};   // (the cutting rule is the launcher's; it refuses a leaf shorter than C)
    const size_t csz = (size_t)C * ldS, cc = (size_t)C * C;
    const size_t nz = (wide ? (size_t)nbins : (size_t)P) * csz;
    if ((nz + 2 * (size_t)nbins * csz + (dense ? 0 : (size_t)g.nOrders * csz) + (g.Hq ? (size_t)2 * P * g.ldHq : 0)) * sizeof(cplx) + til.bytes > ((size_t)1 << 30))
        throw Error(1, "debug factor: more than 1 GiB of device memory");

    fill_sentinel(g.Z, 2 * (size_t)nbins * csz);
    if (g.W) fill_sentinel(g.W, 2 * (size_t)2 * P * C);
    Scratch b;
    cplx* dZ = filled<cplx>(b, nz, sentinel());
    cplx* dV = filled<cplx>(b, (size_t)nbins * csz, 0.0);
    double* dtau = filled<double>(b, (size_t)nbins * C, 0.0);
    cplx* dR2 = filled<cplx>(b, (size_t)nbins * cc, 0.0);
    cplx* dN = filled<cplx>(b, (size_t)nbins * cc, 0.0);
    double* dsv = filled<double>(b, (size_t)P * C, sentinel());
    int* dsw = b.get<int>(sizeof(int) * (size_t)P);
    HIP_CHECK(hipMemset(dsw, 0xff, sizeof(int) * (size_t)P));   // -1: no sweep count written
    cplx* Zout = dZ;
    double* svout = dsv;
    int* swout = dsw;
    if (wide) {
        // (the wide forms factor in place: every bin gets a copy of its own)
        cplx* dB = b.get<cplx>(sizeof(cplx) * (size_t)nbins * csz);
        for (int i = 0; i < nbins; ++i)
            HIP_CHECK(hipMemcpy(dB + (size_t)i * csz, static_cast<const cplx*>(g.Xd) + (size_t)i * g.xd_stride, csz * sizeof(cplx), hipMemcpyHostToDevice));
        if (tiled) {
            void* ws = filled<double>(b, til.bytes / sizeof(double), sentinel());
            launch_wa_factor_tiled(dB, dV, S, C, ldS, nbins, g.reg_c, dtau, dR2, dN, dsv, dsw, dZ, ws, nullptr, g.leaf_rows);
        } else {
            launch_wa_factor(dB, dV, S, C, ldS, nbins, g.reg_c, dtau, dR2, dN, dsv, dsw, dZ, nullptr);
        }
        if (g.Hq) {
            // the least-squares rows as the designs form them behind these factors: Hc [2][nbins][ldHq], Z in the place of Y_reg_inv
            cplx* dH = copy<cplx>(b, g.Hq, (size_t)2 * nbins * g.ldHq);
            cplx* dW = filled<cplx>(b, (size_t)2 * P * C, sentinel());
            launch_wa_ls(dH, g.ldHq, nbins, dZ, ldS, S, C, P, 0, std::min(g.ls_end, nbins), dW, nullptr);
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(g.W, dW, (size_t)2 * P * C * sizeof(cplx), hipMemcpyDeviceToHost));
        }
    } else {
        FactorArgs a{};
        a.S = S; a.C = C; a.ldS = ldS; a.kb0 = kb0; a.P = P;
        if (dense) {
            a.Xd = copy<cplx>(b, g.Xd, g.xd_stride == 0 ? csz : (size_t)nbins * csz);
            a.xd_stride = g.xd_stride;
        } else {
            a.Tn = g.tn_cplx ? (const void*)copy<cplx>(b, g.Tn, (size_t)g.nOrders * csz) : (const void*)copy<double>(b, g.Tn, (size_t)g.nOrders * csz);
            a.bn = copy<cplx>(b, g.bn, (size_t)P * g.nOrders);
            a.nOrders = g.nOrders;
        }
        a.reg_mode = g.reg_mode; a.reg_c = g.reg_c; a.tol_dim = g.tol_dim;
        a.Z = dZ; a.Vws = dV; a.sv = dsv; a.sweeps_out = dsw;
        a.tauw = dtau; a.R2w = dR2; a.Nw = dN;
        if (g.Hq) {
            cplx* dH = filled<cplx>(b, (size_t)2 * P * g.ldHq, 0.0);
            for (int e = 0; e < 2; ++e)
                HIP_CHECK(hipMemcpy(dH + ((size_t)e * P + kb0) * g.ldHq, static_cast<const cplx*>(g.Hq) + (size_t)e * nbins * g.ldHq,
                                    (size_t)nbins * g.ldHq * sizeof(cplx), hipMemcpyHostToDevice));
            a.Hq = dH; a.ldHq = g.ldHq; a.hq_estride = (int64_t)P * g.ldHq; a.ls_end = g.ls_end; a.hq_conj = g.hq_conj;
            a.W = filled<cplx>(b, (size_t)2 * P * C, sentinel());
        }
        if (g.phases == 3) launch_factor(a, nbins, g.tn_cplx != 0, nullptr, 3);
        else { launch_factor(a, nbins, g.tn_cplx != 0, nullptr, 1); launch_factor(a, nbins, g.tn_cplx != 0, nullptr, 2); }
        Zout = dZ + (size_t)kb0 * csz; svout = dsv + (size_t)kb0 * C; swout = dsw + kb0;
        HIP_CHECK(hipDeviceSynchronize());
        if (g.Hq) HIP_CHECK(hipMemcpy(g.W, a.W, (size_t)2 * P * C * sizeof(cplx), hipMemcpyDeviceToHost));
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(g.Z, Zout, (size_t)nbins * csz * sizeof(cplx), hipMemcpyDeviceToHost));
    if (g.sv) HIP_CHECK(hipMemcpy(g.sv, svout, (size_t)nbins * C * sizeof(double), hipMemcpyDeviceToHost));
    if (g.sweeps) HIP_CHECK(hipMemcpy(g.sweeps, swout, (size_t)nbins * sizeof(int), hipMemcpyDeviceToHost));
    if (g.N) HIP_CHECK(hipMemcpy(g.N, dN, (size_t)nbins * cc * sizeof(cplx), hipMemcpyDeviceToHost));
    if (g.R2) HIP_CHECK(hipMemcpy(g.R2, dR2, (size_t)nbins * cc * sizeof(cplx), hipMemcpyDeviceToHost));
    if (g.tau) HIP_CHECK(hipMemcpy(g.tau, dtau, (size_t)nbins * C * sizeof(double), hipMemcpyDeviceToHost));
}

void factor_gram_debug(const void* A, int nbins, int C, const int* route, int jrun, double reg_c, double cond_limit, void* M, double* sv, int* sweeps,
                       int* status) {
    if (!A || !route || !M || !sv || !sweeps || !status) throw Error(1, "null pointer");
    if (nbins < 1 || nbins > 4096 || C < 1 || C > 64) throw Error(1, "debug factor gram: 1 <= nbins <= 4096 and 1 <= C <= 64");
    if (jrun < 1 || jrun > 16) throw Error(1, "debug factor gram: 1 <= jrun <= 16");
    if (!(reg_c >= 0.0) || !(reg_c <= 1.0) || !(cond_limit >= 1.0)) throw Error(1, "debug factor gram: 0 <= reg_c <= 1 and cond_limit >= 1");
    for (int i = 0; i < nbins; ++i)
        if (route[i] != 1 && route[i] != 2) throw Error(1, "debug factor gram: route[bin] is 1 (Jacobi on A) or 2 (skipped)");
    const size_t cc = (size_t)C * C;
    fill_sentinel(M, 2 * (size_t)nbins * cc);
    Scratch b;
    FactorArgs fg{};
    fg.S = C; fg.C = C; fg.ldS = (int)(ceil_div(C, 64) * 64); fg.kb0 = 0; fg.P = nbins;
    fg.reg_mode = 0; fg.reg_c = reg_c;
    fg.sv = filled<double>(b, (size_t)nbins * C, sentinel());
    fg.route = copy<int>(b, route, (size_t)nbins);
    fg.status = b.get<int>(sizeof(int) * 4);
    HIP_CHECK(hipMemset(fg.status, 0, 4 * sizeof(int)));
    fg.cond_limit = cond_limit;
    fg.sweeps_out = b.get<int>(sizeof(int) * (size_t)nbins);
    HIP_CHECK(hipMemset(fg.sweeps_out, 0xff, sizeof(int) * (size_t)nbins));   // -1: skipped
    fg.tauw = filled<double>(b, (size_t)nbins * C, 0.0);
    fg.R2w = copy<cplx>(b, A, (size_t)nbins * cc);
    fg.Nw = filled<cplx>(b, (size_t)nbins * cc, 0.0);
    fg.Mw = filled<cplx>(b, (size_t)nbins * cc, sentinel());
    fg.jrun = jrun;
    launch_factor_jacobi_gram(fg, nbins, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(M, fg.Mw, (size_t)nbins * cc * sizeof(cplx), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sv, fg.sv, (size_t)nbins * C * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(sweeps, fg.sweeps_out, (size_t)nbins * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(status, fg.status, 4 * sizeof(int), hipMemcpyDeviceToHost));
}

void wa_yri_debug(const double* Q, int64_t ldQ, const void* Z, int S, int C, int ldS, int D, int64_t ldD, int nbins, void* Yri) {
    if (!Q || !Z || !Yri) throw Error(1, "null pointer");
    if (C < 1 || C > 64 || S < 1 || ldS < S || ldS > 16384 || ldQ < S || ldQ > 16384) throw Error(1, "debug wa_yri: 1 <= C <= 64, 1 <= S <= ldS <= 16384 and S <= ldQ <= 16384");
    if (D < 1 || ldD < D || ldD > 65536 || nbins < 1 || nbins > 4096) throw Error(1, "debug wa_yri: 1 <= D <= ldD <= 65536 and 1 <= nbins <= 4096");
    const size_t nq = (size_t)D * ldQ, nz = (size_t)nbins * C * ldS, ny = (size_t)nbins * C * ldD;
    if (nq * sizeof(double) + (nz + ny) * sizeof(cplx) > ((size_t)1 << 30)) throw Error(1, "debug wa_yri: more than 1 GiB of device memory");
    fill_sentinel(Yri, 2 * ny);
    Scratch b;
    const double* dQ = copy<double>(b, Q, nq);
    const cplx* dZ = copy<cplx>(b, Z, nz);
    cplx* dY = filled<cplx>(b, ny, sentinel());
    launch_wa_yri(dQ, ldQ, dZ, S, C, ldS, D, ldD, nbins, dY, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(Yri, dY, ny * sizeof(cplx), hipMemcpyDeviceToHost));
}

}  // namespace emagls

extern "C" {

int emagls_debug_wa_yri(const double* Q, int64_t ldQ, const void* Z, int S, int C, int ldS, int D, int64_t ldD, int nbins, void* Yri) {
    return emagls::guarded_call([&] { emagls::wa_yri_debug(Q, ldQ, Z, S, C, ldS, D, ldD, nbins, Yri); });
}

int emagls_debug_factor(const emagls_debug_factor_args* args) {
    return emagls::guarded_call([&] {
        if (!args) throw emagls::Error(1, "null pointer");
        emagls::factor_debug(*args);
    });
}

int emagls_debug_factor_gram(const void* A, int nbins, int C, const int* route, int jrun, double reg_c, double cond_limit, void* M, double* sv, int* sweeps,
                             int* status) {
    return emagls::guarded_call([&] { emagls::factor_gram_debug(A, nbins, C, route, jrun, reg_c, cond_limit, M, sv, sweeps, status); });
}

}  // extern "C"
