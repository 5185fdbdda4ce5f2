// The rigid-sphere array model of getSMAIRMatrix.m and of EMAinCH / EMAinSH, defined once for the design pipelines (plan_setup.hip,
// plan_run.hip) and the one-call entries (render_api.hip, response_api.hip, array_irs_api.hip): its scalars, MATLAB's pinv of one
// matrix, the encoder E, and the EMAinSH operands.  Plain functions that enqueue on the stream they are given -- no allocation and
// no synchronisation, so they run inside captured graphs and lane batches -- and small structs of the pointers they work on.  A
// plan fills those from its named buffers, a one-call entry from its Scratch.  No device code here.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_mem.hpp"
#include "kernels.hpp"

namespace emagls {

// ---- scalars
constexpr double C_SOUND = 343.0;   // dependencies/getSMAIRMatrix.m:86, getRadialFilter.m:31, lib/getMagLsSphericalHeadFilter.m:26

inline int round_up(int64_t v, int64_t m) { return (int)(ceil_div(v, m) * m); }

// simulation order of the array (getSMAIRMatrix.m:95); `order` is params.order, which eMagLS2 leaves at its default of 4
inline int smair_sim_order(int order, double fs, double radius) { return std::max(order, (int)std::ceil(fs * kPi * radius / C_SOUND)); }
// kr of bin 1 on f = linspace(0, fs/2, P)   (getSMAIRMatrix.m:90, :107)
inline double kr_bin_step(double fs, int P, double radius) { return 2.0 * kPi * ((fs / 2.0) / (double)(P - 1)) / C_SOUND * radius; }
// evaluation points of the EMAinSH rotation fit (emash.hip): enough to resolve order N exactly
inline int ema_sh_npts(int C) { return 4 * C + 8; }
// EMAinSH: one azimuth per SH channel at which its circular harmonic is 1 (or sqrt 2) -- where launch_ema_sh_e0 reads J
inline std::vector<double> ema_sh_channel_azimuths(int C, bool cb) {
    std::vector<double> na((size_t)C, 0.0);
    for (int c = 0; c < C; ++c) {
        int n = 0;
        while ((n + 1) * (n + 1) <= c) ++n;
        const int m = c - n * n - n;
        na[c] = (!cb && m < 0) ? kPi / (2.0 * -m) : 0.0;
    }
    return na;
}

// ---- pinv of one rows x cols matrix with MATLAB's tolerance tol_dim * eps(norm)
struct PinvWs {
    cplx *Xd, *Z, *Vws;   // [cols][ld]: the widened input (destroyed), pinv as [cols][ld], Householder vectors
    double* tauw;         // [cols]
    cplx *R2w, *Nw;       // [cols][cols]
};
inline PinvWs pinv_scratch(Scratch& s, int cols, int ld) {
    const size_t tall = sizeof(cplx) * (size_t)cols * ld, square = sizeof(cplx) * (size_t)cols * cols;   // (the tall ones zero-filled)
    return PinvWs{s.get<cplx>(tall, true), s.get<cplx>(tall, true), s.get<cplx>(tall, true), s.get<double>(sizeof(double) * cols),
                  s.get<cplx>(square), s.get<cplx>(square)};
}
inline void pinv_matrix(const PinvWs& w, int rows, int cols, int ld, double tol_dim, double* sv, hipStream_t st) {
    FactorArgs a{};
    a.S = rows; a.C = cols; a.ldS = ld; a.kb0 = 0; a.P = 2;   // P = 2: bin 0 is not a Nyquist bin
    a.Xd = w.Xd; a.xd_stride = 0;
    a.reg_mode = 1; a.tol_dim = tol_dim;
    a.Z = w.Z; a.Vws = w.Vws; a.sv = sv;
    a.tauw = w.tauw; a.R2w = w.R2w; a.Nw = w.Nw;
    launch_factor(a, 1, true, st);
}

// ---- the encoder: from the microphone SH matrix Ycm [S][M] to E [rows][ldS]   (getSMAIRMatrix.m:101-102, :119-121)
// RAW: E = Y_mic (M rows).  SH_PINV: E = pinv(Y_mic(:, 1:(order+1)^2)) Y_mic.  CH_PINV: E = pinv(getCH(order, micAzi)) Y_mic, 2 order + 1
// rows (EMAinCH.m:70, EMAinSH.m:66-75).  Yrm [M][ldS], the row-major Y_mic, is written when it is given (the pinv modes need it);
// RAW writes E unless E is Yrm itself.  lo: workspace of the pinv modes, [nOut][round_up(M, 64)]; lo.Z keeps pinv(Y_lo).
enum class Encoder { RAW, SH_PINV, CH_PINV };
inline void array_encoder(Encoder mode, const void* Ycm, int M, int S, int ldS, bool cb, int order, const double* mic_azi, void* Yrm,
                          const PinvWs& lo, void* E, hipStream_t st) {
    if (Yrm) launch_transpose_conj(Ycm, M, S, M, Yrm, M, ldS, cb, false, st);
    if (mode == Encoder::RAW) {
        if (E != Yrm) launch_transpose_conj(Ycm, M, S, M, E, M, ldS, cb, false, st);
        return;
    }
    const int ldM = round_up(M, 64), nOut = mode == Encoder::CH_PINV ? 2 * order + 1 : (order + 1) * (order + 1);
    if (mode == Encoder::CH_PINV) launch_ch_basis(order, M, mic_azi, cb, lo.Xd, ldM, st);
    else launch_widen(Ycm, M, cb, lo.Xd, ldM, nOut, M, false, false, st);
    pinv_matrix(lo, M, nOut, ldM, (double)std::max(M, nOut), nullptr, st);
    launch_small_gemm(lo.Z, ldM, true, Yrm, ldS, cb, E, ldS, cb, nOut, S, M, st);
}

// ---- EMAinSH operands (kernels and derivation: emash.hip)
// E0 = J Ech, circular -> spherical harmonics (EMAinSH.m:77-82): J from the order-N SHs at (nnm_azi, nnm_zen = pi/2) [C]
inline void ema_sh_e0(int N, int C, int S, int ldS, bool cb, const double* nnm_azi, const double* nnm_zen, double* tab_lo, void* Ypts,
                      const void* Ech, void* E0, hipStream_t st) {
    launch_sh_coeff(N, tab_lo, st);
    launch_sh_basis(N, C, nnm_azi, nnm_zen, tab_lo, cb, Ypts, C, st);
    launch_ema_sh_e0(Ech, ldS, Ypts, C, S, cb, E0, st);
}
// the per-direction SH rotations Rot [D][C][C] (EMAinSH.m:85-100), fitted on ema_sh_npts(C) points: their SHs at every rotated
// position and at the fixed one, Arot [C][ldA], ldA = round_up((D + 1) npts, 64), times the pinv of the fixed set's.
// ws: [C][round_up(npts, 64)].  sv [C] and sweeps [1] are written above 32 channels only.
struct EmaShRot {
    double *rot_azi, *rot_zen;   // [ldA]
    void* Arot;
    PinvWs ws;
    double* sv; int* sweeps;
    void* Rot;
};
inline void ema_sh_rotations(const EmaShRot& r, int N, int C, int D, bool cb, const double* azi, const double* zen, const double* tab_lo,
                             hipStream_t st) {
    const int npts = ema_sh_npts(C), ldP = round_up(npts, 64);
    const int64_t ldA = round_up((int64_t)(D + 1) * npts, 64);
    launch_rot_points(azi, zen, D, npts, r.rot_azi, r.rot_zen, st);
    launch_sh_basis(N, (int64_t)(D + 1) * npts, r.rot_azi, r.rot_zen, tab_lo, cb, r.Arot, ldA, st);
    const char* B = (const char*)r.Arot + esz(cb) * (size_t)D * npts;   // the unrotated point set: columns D*npts..
    launch_widen(B, ldA, cb, r.ws.Xd, ldP, C, npts, false, false, st);
    if (C > 32)   // orders 5..7: wide_array.hip's QR + one-sided Jacobi (no clipping: the point set resolves the order, nothing is
                  // dropped) -- Z comes out as pinv(B) [C][ldP] like the narrow factorisation's
        launch_wa_factor(r.ws.Xd, r.ws.Vws, npts, C, ldP, 1, 0.0, r.ws.tauw, r.ws.R2w, r.ws.Nw, r.sv, r.sweeps, r.ws.Z, st);
    else
        pinv_matrix(r.ws, npts, C, ldP, (double)std::max(npts, C), nullptr, st);
    launch_rot_from_points(r.Arot, ldA, r.ws.Z, ldP, C, npts, zen, D, cb, r.Rot, st);
}
// order terms of pwGrid.' on the horizontal projection of the grid (zen_eq = pi/2 [D]), every direction's row rotated:
// QT [simOrder + 1][C][ldY].  Ycm [S][ldY] and Yc [rowsYc][ldS] are the projected grid's SH matrix and its conjugate transpose.
inline void ema_sh_order_terms(int simOrder, int N, int D, int C, int S, int ldS, bool cb, const double* azi, const double* zen_eq,
                               const double* tab, void* Ycm, int64_t ldY, void* Yc, int64_t rowsYc, const void* E0, const void* Rot, void* QT,
                               hipStream_t st) {
    launch_sh_basis(simOrder, D, azi, zen_eq, tab, cb, Ycm, ldY, st);
    launch_transpose_conj(Ycm, D, S, ldY, Yc, rowsYc, ldS, cb, true, st);
    launch_qt(Yc, ldS, E0, ldS, D, S, C, simOrder + 1, cb, QT, ldY, st);
    launch_qt_rotate(QT, ldY, simOrder + 1, C, N, D, Rot, cb, st);
}

}  // namespace emagls
