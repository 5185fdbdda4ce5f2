// Stage pipelines of every design kind, the resident sweep and its gate, and the execute of a plan on its own (eager, captured,
// replayed), with the recovery from the device-side status words.  The array model's own sequences -- pinv of one matrix, the
// encoder E, the EMAinSH operands -- are calls into array_model.hpp, on the buffers the plan names.
#include "host_internal.hpp"

namespace {
// ---------------------------------------------------------------------------------------------
// pipelines
// ---------------------------------------------------------------------------------------------
// SH matrix on the HRIR grid, Cholesky-QR:  conj(Y) = Q R
void stage_hrir_basis(emagls_plan& p) {
    hipStream_t st = p.stream;
    const bool cb = p.cplx_basis;
    if (p.d.kind == EMAGLS_KIND_MAGLS_2D) {   // circular harmonics of the horizontal HRIR grid (getMagLsFilters2D.m:49)
        launch_ch_basis(p.d.order, (int)p.D, p.get<double>("hrir_azi"), cb, p.get("Ycm"), (int)p.ldD, st, !cb);
    } else if (!p.custom_basis) {
        launch_sh_coeff(p.simOrder, p.get<double>("sh_tab"), st);
        launch_sh_basis(p.simOrder, p.D, p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), p.get<double>("sh_tab"), cb,
                        p.get("Ycm"), p.ldD, st);
    }
    launch_transpose_conj(p.get("Ycm"), p.D, p.S, p.ldD, p.get("Yc"), p.Dpad, p.ldS, cb, true, st);
    p.mark("sh_basis");
    launch_gram(p.get("Yc"), p.D, p.S, p.ldS, cb, p.get("Gp"), nullptr, p.get("R"), p.S, st);
    p.mark("gram_mfma");
    launch_cholesky(p.get("R"), p.S, cb, p.get<int>("flag"), st);
    p.mark("cholesky");
    if (p.wide) return;   // (no orthonormal factor: pinv(Y_conj) = Y conj((Y^T conj(Y))^-1), run_pinv_of_R)
    launch_qform(p.get("Yc"), p.get("R"), p.get("Rinv"), p.S, p.D, p.ldS, cb, p.get("Q"), st);
    p.mark("qform");
}

void record_sweep_event(emagls_plan& p, size_t i) {
    if (p.sweep_events.size() <= i) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        p.sweep_events.push_back(e);
    }
    HIP_CHECK(hipEventRecord(p.sweep_events[i], p.stream));
}

// the workspace of array_model.hpp's pinv from a plan's buffers: the widened input, Z, Householder vectors, tau, R2, N
PinvWs plan_pinv_ws(emagls_plan& p, const char* Xd, const char* Z, const char* Vws, const char* tauw, const char* R2w, const char* Nw) {
    return PinvWs{p.get<cplx>(Xd), p.get<cplx>(Z), p.get<cplx>(Vws), p.get<double>(tauw), p.get<cplx>(R2w), p.get<cplx>(Nw)};
}
PinvWs plan_lo_ws(emagls_plan& p) { return plan_pinv_ws(p, "Ylo_c", "Zlo", "Vlo", "tau_lo", "R2_lo", "N_lo"); }   // pinv(Y_lo)

void run_pinv_of_R(emagls_plan& p) {
    // pinv(Y_conj) = conj(Q) Z_B, Z_B from the SVD of B = R with MATLAB's pinv tolerance
    hipStream_t st = p.stream;
    const bool cb = p.cplx_basis;
    if (p.wide) {   // 33..64 channels: the inverse of the Gram matrix, certified well conditioned on the device (wide.hip)
        launch_gram_inverse(p.get("R"), p.S, cb, p.get("Mg"), p.get<int>("flag"), st, p.has("Mgw") ? p.get("Mgw") : nullptr);
        launch_ypinv_gram(p.get("Ycm"), p.ldD, cb, p.get("Mg"), p.S, (int)p.D, p.get("Ypinv"), st);
        p.mark("pinv");
        return;
    }
    launch_widen(p.get("R"), p.S, cb, p.get("Rb"), p.ldS, p.C, p.S, /*transpose=*/true, /*upper_only=*/true, st);
    pinv_matrix(plan_pinv_ws(p, "Rb", "Zb", "Vws", "tauw", "R2w", "Nw"), p.S, p.C, p.ldS, (double)std::max<int64_t>(p.D, p.C), p.get<double>("sv"), st);
    launch_ypinv(p.get("Q"), p.ldS, cb, p.get("Zb"), p.ldS, (int)p.D, p.S, p.C, p.get("Ypinv"), p.ldD, st);
    p.mark("pinv");
}

// MagLS / MagLS-2D: everything before the sweep.  With the persistent sweep (the kernel of the array designs, one resident launch
// instead of one launch per bin) the operands are the same for every bin: G = Y_conj as complex [c][d] and
// M = (G^H G)^-1 = R^-1 R^-H from the Cholesky factor, since pinv(Y_conj) = conj(G) conj(M) for a full-rank basis.
void magls_pre_sweep(emagls_plan& p) {
    hipStream_t st = p.stream;
    const bool cb = p.cplx_basis;
    stage_hrir_basis(p);
    run_pinv_of_R(p);
    launch_conj_copy(p.get("Ycm"), p.get("Xc"), (int64_t)p.S * p.ldD, cb, st);  // Y_conj [c][d]
    stage_prologue(p, 0, nullptr, p.D);
    launch_ls_apply(p.get("Hc"), p.ldD, std::min(p.kcut0, p.P), p.get("Ypinv"), cb, p.ldD, (int)p.D, p.C, p.P, 0,
                    std::min(p.kcut0, p.P), p.get("W"), st);
    p.mark("ls_bins");
    if (p.sweep_persist) {
        launch_widen(p.get("Xc"), p.ldD, cb, p.get("Gm"), p.ldD, p.C, (int)p.D, false, false, st);
        launch_magls_m(p.get("R"), p.S, cb, p.P, p.get("Mw"), p.get<double>("cond_ok"), p.get<int>("flag"), st);
        p.mark("sweep_operands");
    }
}
void emagls_run_sweep(emagls_plan& p) {
    hipStream_t s0 = p.stream;
    const int k0 = std::max(p.kcut0, 1);
    HalfSweepMulti m{};
    m.n = 1;
    m.a[0] = emagls_half_args(p);
    p.sweep_launches = 0;
    if (k0 < p.P && p.sweep_persist) {
        emagls_plan* self = &p;
        p.reg_sweep = reg_sweep_wanted(&self, 1);
        SweepGate gate(s0, p.reg_sweep ? reg_sweep_gate_cost((int)p.D, 1) : 0);
        launch_zero(p.get("ll"), p.bufs["ll"].bytes, s0);
        if (p.reg_sweep) reg_args_upload(&m.a[0], 1, p.get("sweep_args"), p.sweep_args_last, s0);
        if (p.prof_level >= 2) record_sweep_event(p, 0);
        if (p.reg_sweep) launch_sweep_reg(p.get<HalfSweepArgs>("sweep_args"), m.a[0], 1, s0);
        else if (p.synth) launch_sweep_synth(m, s0); else launch_sweep_persist(m, s0);
        if (p.prof_level >= 2) record_sweep_event(p, 1);
        p.sweep_launches = 1;
    } else if (k0 < p.P) {
        for (int kb = k0; kb < p.P; ++kb) {
            if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches);
            launch_sweep_half(m, kb, s0);
            if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches + 1);
            ++p.sweep_launches;
        }
        launch_sweep_half_finalize(m, p.P - 1, s0);
    }
    p.mark("magls_sweep");
}
void execute_magls(emagls_plan& p) {
    hipStream_t st = p.stream;
    const bool cb = p.cplx_basis;
    magls_pre_sweep(p);
    if (p.sweep_persist) {   // (eager / profiled executes; plan_execute captures the two halves around the sweep otherwise)
        emagls_run_sweep(p);
        magls_post_sweep(p);
        return;
    }
    DenseSweepArgs a{};
    a.D = (int)p.D; a.C = p.C; a.ldD = (int)p.ldD; a.P = p.P;
    a.X = p.get("Xc"); a.x_stride = 0; a.Zd = p.get("Ypinv"); a.z_stride = 0;
    a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
    a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG; a.dpw = 0; a.kfirst = p.kcut0;
    p.sweep_launches = 0;
    for (int kb = p.kcut0; kb < p.P; ++kb) {
        if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches);
        if (p.wide) launch_sweep_wide(a, kb, cb, st); else launch_sweep_dense(a, kb, cb, st);
        if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches + 1);
        ++p.sweep_launches;
    }
    if (p.kcut0 < p.P) {
        if (p.wide) launch_sweep_wide_finalize(p.get("Wpart"), p.get("W"), p.nWG, p.C, p.P, p.P - 1, st);
        else launch_sweep_finalize(p.get("Wpart"), p.get("W"), p.nWG, p.C, p.P, p.P - 1, st);
    }
    p.mark("magls_sweep");
    magls_post_sweep(p);
}

// bins per Jacobi workgroup on the Gram route (warm start from the neighbouring bin: fewer rotations per bin, but the launch lasts as
// long as its longest run).  Round 5, config 3 through the job scheduler: a lone chunk of 20 designs on forked streams -- nothing else
// on the GPU, the launch on the critical path -- 2219 / 2231 sets/s with runs of 4, 2263 / 2301 with 2, 2277 / 2311 with single bins;
// chunks in flight next to each other (128 / 512 steps): 3474-3494 / 3537-3639 with 4, 3471-3497 / 3550-3597 with 2, 3375-3465 /
// 3544-3572 with 1.  So: single bins where the stages before the sweep are forked (latency mode), runs of 2 in lane groups.
int jacobi_run_length(const emagls_plan& p) {
    if (const int forced = sw_int<Sw::JACOBI_RUN>()) return forced;
    return (batch_ctx().n >= 2 && p.nstreams <= 1) ? 2 : 1;
}

// getEMagLsFiltersEMAinSH: the HRIR prologue, the array model, the per-direction rotations and G_k of every bin (kernels and derivation:
// emash.hip).  One stream.
void ema_sh_operands(emagls_plan& p) {
    const emagls_design_desc& d = p.d;
    const bool cb = p.cplx_basis;
    hipStream_t st = p.stream;
    const int M = (int)d.nmics, N = d.order, nOrd = p.simOrder + 1;
    const int ls_end = std::min(p.kcut0, p.P);
    p.sync_used = 0;
    // ---- HRIR prologue
    launch_twiddles(p.nfft, p.get("tw"), st);
    launch_hrir_grpdelay(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, d.ndirs, p.nfft, p.get("tw"), p.get<double>("dirsum"),
                         p.get<double>("grpd"), st);
    launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, p.D, nullptr, p.nfft, p.get("tw"), p.get<double>("grpd"), 0, ls_end,
                    p.kcut0, p.get("Hc"), p.get<double>("Habs"), p.ldD, st);
    if (p.diffuse)
        launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, p.D, nullptr, p.nfft, p.get("tw"), p.get<double>("grpd"), 0, p.P,
                        p.P, p.get("Hfull"), p.get<double>("Habs"), p.ldD, st);
    p.mark("hrir_prologue");
    // ---- array model: E0 = J pinv(CH(micAzi)) Y_mic   (EMAinSH.m:66-82), b_n(kr)
    launch_sh_coeff(p.simOrder, p.get<double>("sh_tab"), st);
    launch_sh_basis(p.simOrder, M, p.get<double>("mic_azi"), p.get<double>("mic_zen"), p.get<double>("sh_tab"), cb, p.get("Ymic_cm"), M, st);
    array_encoder(Encoder::CH_PINV, p.get("Ymic_cm"), M, p.S, p.ldS, cb, N, p.get<double>("mic_azi"), p.get("Ymic_rm"), plan_lo_ws(p), p.get("Ech"), st);
    ema_sh_e0(N, p.C, p.S, p.ldS, cb, p.get<double>("nnm_azi"), p.get<double>("nnm_zen"), p.get<double>("sh_tab_lo"), p.get("Ypts"), p.get("Ech"),
              p.get("E"), st);
    launch_modal_bn(p.simOrder, p.P, p.get<double>("kr"), 1.0, -1.0, p.get("bn"), nOrd, 1, st, p.get<int>("nvalid"));
    p.mark("array_model");
    // ---- per-direction SH rotations (EMAinSH.m:85-100)
    {
        EmaShRot r{p.get<double>("rot_azi"), p.get<double>("rot_zen"), p.get("Arot"), plan_pinv_ws(p, "Bc", "Zb", "Vb", "tau_b", "R2_b", "N_b"),
                   p.get<double>("sv"), p.get<int>("jsweeps"), p.get("Rot")};
        ema_sh_rotations(r, N, p.C, (int)p.D, cb, p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), p.get<double>("sh_tab_lo"), st);
    }
    p.mark("sh_rotations");
    // ---- order terms of pwGrid.' on the horizontal projection of the grid, rotated per direction; G_k of every bin
    ema_sh_order_terms(p.simOrder, N, (int)p.D, p.C, p.S, p.ldS, cb, p.get<double>("hrir_azi"), p.get<double>("hrir_zen_eq"), p.get<double>("sh_tab"),
                       p.get("Ycm"), p.ldD, p.get("Yc"), p.Dpad, p.get("E"), p.get("Rot"), p.get("QT"), st);
    launch_dspace_g(p.get("QT"), p.ldD, cb, p.get("bn"), nOrd, (int)p.D, p.C, p.P, p.g0, p.get("G"), st, 0, -1);
    p.mark("order_terms+G");
}
// everything before the sweep, up to order 4 (32 channels: the tuned Gram-route kernels and the resident sweep)
void ema_sh_pre_sweep(emagls_plan& p) {
    ema_sh_operands(p);
    const bool cb = p.cplx_basis;
    hipStream_t st = p.stream;
    const int ls_end = std::min(p.kcut0, p.P);
    const int64_t g_stride = (int64_t)p.C * p.ldD;
    (void)cb;
    // ---- per-bin C x C matrices: Gram route for every bin
    const int ldK = round_up(p.C * p.C, 64), gf = 1, nb = p.P - 1;
    launch_gram_from_g(p.get("G"), g_stride, p.ldD, (int)p.D, p.C, gf, nb, p.g0, p.get<double>("Apk"), ldK, st);
    launch_gram_solve(p.get<double>("Apk"), ldK, p.C, gf, nb, SVD_REGUL_CONST, p.get("Mw"), p.get("R2w"), p.get<double>("sv"),
                      p.get<int>("route"), p.get<int>("jsweeps"), st);
    {
        FactorArgs fg{};
        fg.S = p.C; fg.C = p.C; fg.ldS = round_up(p.C, 64); fg.kb0 = gf; fg.P = p.P;
        fg.reg_mode = 0; fg.reg_c = SVD_REGUL_CONST;
        fg.sv = p.get<double>("sv"); fg.route = p.get<int>("route"); fg.status = p.get<int>("flag");
        fg.cond_limit = 10.0 * GRAM_COND_EST;
        fg.sweeps_out = p.get<int>("jsweeps");
        fg.tauw = p.get<double>("tauw"); fg.R2w = p.get<cplx>("R2w"); fg.Nw = p.get<cplx>("Nw"); fg.Mw = p.get<cplx>("Mw");
        fg.jrun = jacobi_run_length(p);
        launch_factor_jacobi_gram(fg, nb, st);
    }
    launch_cond_flags(p.get<double>("sv"), p.C, p.P, 1, p.get<double>("cond_ok"), st);
    p.mark("gram_route");
    // ---- least-squares bins
    if (ls_end > 1)
        launch_ls_gram(p.get("Hc"), p.ldD, ls_end, (const cplx*)p.get("G") - (int64_t)p.g0 * g_stride, g_stride, p.ldD, p.get("Mw"), (int)p.D, p.C,
                       p.P, 1, ls_end, p.get("W"), st);
    p.mark("ls_bins");
}

// getEMagLsFiltersEMAinSH at orders 5..7 (36 / 49 / 64 channels; lib/getEMagLsFiltersEMAinSH.m:66-143): the per-direction rotations leave
// no common S-space, so pwGrid_k.' = G_k (D x C) is factored itself -- Householder QR, one-sided Jacobi on the triangular factor, 1 %
// clipping, back-transform: Y_reg_inv_k directly (wide_array.hip with Q = I, the form FromAtf takes above 32 microphones) --, then
// the least-squares bins and one sweep launch per bin.
void execute_ema_sh_wide(emagls_plan& p) {
    hipStream_t st = p.stream;
    const int nb = p.P - 1, ls_end = std::min(p.kcut0, p.P), k0 = std::max(p.kcut0, 1);
    const int64_t g_stride = (int64_t)p.C * p.ldD;
    ema_sh_operands(p);                                   // G_k of the bins 1 .. P-1 (g0 = 1)
    cplx* G = p.get<cplx>("G");
    cplx* Yri = p.get<cplx>("Yri");
    HIP_CHECK(hipMemcpyAsync(p.get("Bw"), G, sizeof(cplx) * (size_t)nb * g_stride, hipMemcpyDeviceToDevice, st));   // (the QR works in place)
    launch_wa_factor(p.get("Bw"), p.get("Vw"), (int)p.D, p.C, (int)p.ldD, nb, SVD_REGUL_CONST, p.get<double>("tauw"), p.get("R2w"), p.get("Nw"),
                     p.get<double>("sv") + p.C, p.get<int>("jsweeps") + 1, Yri, st);
    p.mark("factor_bins");
    launch_wa_ls(p.get("Hc"), p.ldD, ls_end, Yri, p.ldD, (int)p.D, p.C, p.P, 1, ls_end, p.get("W"), st);
    p.mark("ls_bins");
    DenseSweepArgs a{};
    a.D = (int)p.D; a.C = p.C; a.ldD = (int)p.ldD; a.P = p.P;
    a.X = G - g_stride; a.x_stride = g_stride;            // (indexed by kb: bin 1 at the buffer's start)
    a.Zd = Yri - g_stride; a.z_stride = g_stride;
    a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
    a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG; a.dpw = 0; a.kfirst = k0;
    p.sweep_launches = 0;
    for (int kb = k0; kb < p.P; ++kb) { launch_sweep_wide(a, kb, true, st); ++p.sweep_launches; }
    if (k0 < p.P) launch_sweep_wide_finalize(p.get("Wpart"), p.get("W"), p.nWG, p.C, p.P, p.P - 1, st);
    p.mark("magls_sweep");
    launch_filter_epilogue(p.get("W"), p.C, p.nfft, (int)p.d.len, p.get("tw"), p.get<double>("grpd"), p.req_cplx ? 1 : 0, 1, 0,
                           p.out_cplx ? 1 : 0, p.get("wL"), p.get("wR"), st);
    p.mark("epilogue");
}

// eMagLS / eMagLS2 with 33..64 channels: wide_array.hip.  One stream, every bin on the S-space route.
void execute_emagls_wide(emagls_plan& p) {
    if (p.d.kind == EMAGLS_KIND_EMA_SH) { execute_ema_sh_wide(p); return; }
    const emagls_design_desc& d = p.d;
    hipStream_t st = p.stream;
    const bool raw = d.kind == EMAGLS_KIND_EMAGLS2;
    const int M = (int)d.nmics, nOrd = p.simOrder + 1, nb = p.P - 1;
    const int ls_end = std::min(p.kcut0, p.P), k0 = std::max(p.kcut0, 1);
    const int64_t g_stride = (int64_t)p.C * p.ldD;
    // ---- SH matrices, array model, modal terms  (geo: skipped when the plan keeps them from its last run on these grids)
    const bool geo = !p.geo_skip;
    if (geo) {
    launch_sh_coeff(p.simOrder, p.get<double>("sh_tab"), st);
    launch_sh_basis(p.simOrder, p.D, p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), p.get<double>("sh_tab"), false, p.get("Ycm"), p.ldD, st);
    launch_transpose_conj(p.get("Ycm"), p.D, p.S, p.ldD, p.get("Yc"), p.Dpad, p.ldS, false, true, st);
    launch_sh_basis(p.simOrder, M, p.get<double>("mic_azi"), p.get<double>("mic_zen"), p.get<double>("sh_tab"), false, p.get("Ymic_cm"), M, st);
    if (raw) {
        array_encoder(Encoder::RAW, p.get("Ymic_cm"), M, p.S, p.ldS, false, 0, nullptr, nullptr, PinvWs{}, p.get("E"), st);   // E = Y_mic
    } else {
        // (eMagLS: nOut = C > 32 on this path, beyond the narrow pinv of array_model.hpp's encoder)
        // pinv(Y_lo) = (Y_lo^T Y_lo)^-1 Y_lo^T: the M x nOut SH matrix of the microphone grid has full column rank and is well
        // conditioned for any array that resolves the order (certified on the device like the SH Gram matrix of wide.hip)
        launch_wa_lo_gram(p.get("Ymic_cm"), M, p.nOut, p.get<double>("Ag"), st);
        launch_cholesky(p.get("Ag"), p.nOut, false, p.get<int>("flag"), st);
        launch_gram_inverse(p.get("Ag"), p.nOut, false, p.get("Minv"), p.get<int>("flag"), st);
        launch_wa_e(p.get("Ymic_cm"), M, p.nOut, p.S, p.get("Minv"), p.get("E"), (int)p.ldS, st);
    }
    launch_modal_bn(p.simOrder, p.P, p.get<double>("kr"), 1.0, -1.0, p.get("bn"), nOrd, 1, st, p.get<int>("nvalid"));
    }
    p.mark("array_model");
    // ---- HRIR prologue
    launch_twiddles(p.nfft, p.get("tw"), st);
    launch_hrir_grpdelay(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, d.ndirs, p.nfft, p.get("tw"), p.get<double>("dirsum"), p.get<double>("grpd"), st);
    launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, p.D, nullptr, p.nfft, p.get("tw"), p.get<double>("grpd"), 0, ls_end, p.kcut0,
                    p.get("Hc"), p.get<double>("Habs"), p.ldD, st);
    if (p.diffuse) {   // the covariance constraint's target: the time-aligned complex HRTFs of every bin; G starts at bin 1 here
        launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, p.D, nullptr, p.nfft, p.get("tw"), p.get<double>("grpd"), 0, p.P, p.P,
                        p.get("Hfull"), p.get<double>("Habs"), p.ldD, st);
        p.g0 = 1;
    }
    p.mark("hrir_prologue");
    // ---- conj(Y) = Q R, order terms T_n = R(:,blk_n) E(:,blk_n)^T and QT_n, G_k of every solved bin
    if (geo) {
    launch_gram(p.get("Yc"), p.D, p.S, p.ldS, false, p.get("Gp"), nullptr, p.get("R"), p.S, st);
    launch_cholesky(p.get("R"), p.S, false, p.get<int>("flag"), st);
    launch_qform(p.get("Yc"), p.get("R"), p.get("Rinv"), p.S, p.D, p.ldS, false, p.get("Q"), st);
    launch_tn(p.get("R"), p.get("E"), p.S, p.C, (int)p.ldS, nOrd, false, p.get("Tn"), p.ldS, st);
    launch_qt(p.get("Yc"), p.ldS, p.get("E"), p.ldS, (int)p.D, p.S, p.C, nOrd, false, p.get("QT"), p.ldD, st);
    launch_dspace_g(p.get("QT"), p.ldD, false, p.get("bn"), nOrd, (int)p.D, p.C, p.P, 1, p.get("G"), st, 0, raw ? -1 : (int)d.order);
    p.mark("order_terms+G");
    // ---- per-bin factors (bins 1 .. P-1) and Y_reg_inv
    launch_wa_assemble(p.get("Tn"), p.get("bn"), nOrd, p.S, p.C, (int)p.ldS, p.P, 1, nb, p.get("Bw"), st);
    launch_wa_factor(p.get("Bw"), p.get("Vw"), p.S, p.C, (int)p.ldS, nb, SVD_REGUL_CONST, p.get<double>("tauw"), p.get("R2w"), p.get("Nw"),
                     p.get<double>("sv") + p.C, p.get<int>("jsweeps") + 1, p.get("Zw"), st);
    launch_wa_yri(p.get("Q"), p.ldS, p.get("Zw"), p.S, p.C, (int)p.ldS, (int)p.D, p.ldD, nb, p.get("Yri"), st);
    }
    p.mark("factor_bins");
    // ---- least-squares bins, sweep (G and Yri start at bin 1)
    launch_wa_ls(p.get("Hc"), p.ldD, ls_end, p.get("Yri"), p.ldD, (int)p.D, p.C, p.P, 1, ls_end, p.get("W"), st);
    p.mark("ls_bins");
    DenseSweepArgs a{};
    a.D = (int)p.D; a.C = p.C; a.ldD = (int)p.ldD; a.P = p.P;
    a.X = p.get<cplx>("G") - g_stride; a.x_stride = g_stride;
    a.Zd = p.get<cplx>("Yri") - g_stride; a.z_stride = g_stride;
    a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
    a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG; a.dpw = 0; a.kfirst = k0;
    p.sweep_launches = 0;
    for (int kb = k0; kb < p.P; ++kb) { launch_sweep_wide(a, kb, true, st); ++p.sweep_launches; }
    if (k0 < p.P) launch_sweep_wide_finalize(p.get("Wpart"), p.get("W"), p.nWG, p.C, p.P, p.P - 1, st);
    p.mark("magls_sweep");
    emagls_post_sweep(p);
}

void execute_emagls(emagls_plan& p) {
    if (p.wide) { execute_emagls_wide(p); return; }
    emagls_pre_sweep(p);
    emagls_run_sweep(p);
    emagls_post_sweep(p);
}
constexpr int FROM_ATF_DENSE_REG = 8;   // microphones the dense route factors in factor.hip's register tiles (C 64 <= 512 threads)
constexpr int FROM_ATF_DENSE_ROWS = 4096;   // matched directions one workgroup factors; above: the tiled form at every width
bool from_atf_dense_tiled(const emagls_plan& p) { return !p.wide && p.Dm > FROM_ATF_DENSE_ROWS; }
// the dense route's copy of its bins' matrices at 9..32 microphones or more than 4096 matched directions, and the tiled form's
// workspace (the row blocks' triangles, the tree step's stack, reflectors and T_i): allocated when a conditioning flag first moves
// the route, for the dense bins only (a well-conditioned plan never holds them)
void from_atf_alloc_dense(emagls_plan& p) {
    const bool tiled = from_atf_dense_tiled(p);
    if (p.wide || (p.C <= FROM_ATF_DENSE_REG && !tiled) || p.gram_from == 1) return;
    const int dense_end = p.gram_from > 0 ? p.gram_from : p.P;
    p.alloc("Bd", sizeof(cplx) * (size_t)(dense_end - 1) * p.C * p.ldD, false);
    if (tiled) p.alloc("Td", wa_tiling((int)p.Dm, p.C, dense_end - 1).bytes, false);
}
void from_atf_shared_stage(emagls_plan& p) {    // ATF spectra on the matched directions and the per-bin factors
    hipStream_t st = p.stream;
    const emagls_design_desc& d = p.d;
    const int M = p.C, gf = p.gram_from, nb = gf > 0 ? p.P - gf : 0;
    const int64_t g_stride = (int64_t)M * p.ldD;
    const int ls_end = std::min(p.kcut0, p.P);
    launch_real_fft_gather(p.get<double>("atf"), d.atf_taps, (int64_t)M * p.Dm, p.get<int64_t>("colidx"), p.nfft, p.get("tw"),
                           p.get("X"), g_stride, p.Dm, p.ldD, st);
    p.mark("atf_fft");
    if (nb > 0) {
        const int ldK = round_up(M * M, 64);
        launch_gram_from_g(p.get("X"), g_stride, p.ldD, (int)p.Dm, M, gf, nb, 0, p.get<double>("Apk"), ldK, st);
        launch_gram_solve(p.get<double>("Apk"), ldK, M, gf, nb, SVD_REGUL_CONST, p.get("Mw"), p.get("R2w"), p.get<double>("sv"),
                          p.get<int>("route"), p.get<int>("jsweeps"), st);
        FactorArgs fg{};
        fg.S = M; fg.C = M; fg.ldS = round_up(M, 64); fg.kb0 = gf; fg.P = p.P;
        fg.reg_mode = 0; fg.reg_c = SVD_REGUL_CONST;
        fg.sv = p.get<double>("sv"); fg.route = p.get<int>("route"); fg.status = p.get<int>("flag");
        fg.cond_limit = 10.0 * GRAM_COND_EST;
        fg.sweeps_out = p.get<int>("jsweeps");
        const int64_t off = (int64_t)(gf - 1);   // (gram_solve stores bin kb at slot kb - 1; the Jacobi kernel indexes from its first bin)
        fg.tauw = p.get<double>("tauw") + off * M; fg.R2w = p.get<cplx>("R2w") + off * M * M; fg.Nw = p.get<cplx>("Nw") + off * M * M;
        fg.Mw = p.get<cplx>("Mw") + off * M * M;
        fg.jrun = 1;
        launch_factor_jacobi_gram(fg, nb, st);
    }
    launch_cond_flags(p.get<double>("sv"), M, p.P, 1, p.get<double>("cond_ok"), st);   // 1 for every bin ...
    const int dense_end = gf > 0 ? gf : p.P;   // bins [1, dense_end) on the dense route
    if (dense_end > 1) {
        FactorArgs a{};
        a.S = (int)p.Dm; a.C = M; a.ldS = (int)p.ldD; a.kb0 = 1; a.P = p.P;
        a.Xd = p.get<cplx>("X"); a.xd_stride = g_stride;
        a.reg_mode = 0; a.reg_c = SVD_REGUL_CONST;
        a.Z = p.get<cplx>("Z"); a.Vws = p.get<cplx>("Vws"); a.sv = p.get<double>("sv");
        a.Hq = p.get<cplx>("Hc"); a.ldHq = p.ldD; a.hq_estride = (int64_t)ls_end * p.ldD; a.ls_end = std::min(ls_end, dense_end);
        a.W = p.get<cplx>("W"); a.sweeps_out = p.get<int>("jsweeps");
        a.tauw = p.get<double>("tauw"); a.R2w = p.get<cplx>("R2w"); a.Nw = p.get<cplx>("Nw");
        const bool tiled = from_atf_dense_tiled(p);
        if (M <= FROM_ATF_DENSE_REG && !tiled) {
            launch_factor(a, dense_end - 1, true, st);
        } else {
            // 9..32 microphones: factor.hip's register tiles end at 8 columns of this height; wide_array.hip's tall forms factor a copy
            // of the dense bins' matrices (their QR works in place, the sweep still reads X) and write Y_reg_inv where the sweep
            // expects it.  Workspace slots 0 .. dense_end - 2: the Gram-route bins use the slots from gram_from - 1 on.
            // More than 4096 matched directions, 1..32 microphones: the same in row blocks (launch_wa_factor_tiled).
            cplx* X = p.get<cplx>("X");
            HIP_CHECK(hipMemcpyAsync(p.get("Bd"), X + g_stride, sizeof(cplx) * (size_t)(dense_end - 1) * g_stride, hipMemcpyDeviceToDevice, st));
            if (tiled)
                launch_wa_factor_tiled(p.get("Bd"), p.get("Vws"), (int)p.Dm, M, (int)p.ldD, dense_end - 1, SVD_REGUL_CONST, a.tauw, a.R2w, a.Nw,
                                       a.sv + M, a.sweeps_out + 1, a.Z + g_stride, p.get("Td"), st);
            else
            launch_wa_factor(p.get("Bd"), p.get("Vws"), (int)p.Dm, M, (int)p.ldD, dense_end - 1, SVD_REGUL_CONST, a.tauw, a.R2w, a.Nw, a.sv + M,
                             a.sweeps_out + 1, a.Z + g_stride, st);
            launch_wa_ls(p.get("Hc"), p.ldD, ls_end, a.Z + g_stride, p.ldD, (int)p.Dm, M, p.P, 1, a.ls_end, p.get("W"), st);
        }
        launch_zero(p.get<double>("cond_ok"), sizeof(double) * (size_t)dense_end, st);   // ... but the dense-route ones: the sweep reads their Y_reg_inv
    }
    p.mark("factor_bins");
}
void from_atf_pre_sweep(emagls_plan& p) {
    from_atf_subject_stage(p);
    from_atf_shared_stage(p);
    from_atf_ls_rows(p, p, p.stream);
    p.mark("ls_bins");
}

// FromAtf with 33..64 microphones: pwGrid_k.' = X_k.' (Dm x M) is its own "S-space" (Q = I), so wide_array.hip's per-bin kernels --
// Householder QR, one-sided Jacobi, back-transform -- give Y_reg_inv_k directly; one sweep launch per bin (lib/getEMagLsFiltersFromAtf.m:97-120).
void execute_from_atf_wide(emagls_plan& p) {
    hipStream_t st = p.stream;
    const emagls_design_desc& d = p.d;
    const int M = p.C, nb = p.P - 1;
    const int64_t g_stride = (int64_t)M * p.ldD;
    if (p.hrir_smaller)
        launch_grid_match(p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), d.ndirs, p.get<double>("atf_azi"),
                          p.get<double>("atf_zen"), d.natf, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    else
        launch_grid_match(p.get<double>("atf_azi"), p.get<double>("atf_zen"), d.natf, p.get<double>("hrir_azi"),
                          p.get<double>("hrir_zen"), d.ndirs, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    launch_atf_colidx(p.hrir_smaller ? p.get<int64_t>("match_idx") : nullptr, p.Dm, M, p.get<int64_t>("colidx"), st);
    p.mark("grid_match");
    stage_prologue(p, 1, p.hrir_smaller ? nullptr : p.get<int64_t>("match_idx"), p.Dm);
    launch_real_fft_gather(p.get<double>("atf"), d.atf_taps, (int64_t)M * p.Dm, p.get<int64_t>("colidx"), p.nfft, p.get("tw"),
                           p.get("X"), g_stride, p.Dm, p.ldD, st);
    p.mark("atf_fft");
    cplx* X = p.get<cplx>("X");
    cplx* Z = p.get<cplx>("Z");
    HIP_CHECK(hipMemcpyAsync(p.get("Bw"), X + g_stride, sizeof(cplx) * (size_t)nb * g_stride, hipMemcpyDeviceToDevice, st));
    launch_wa_factor(p.get("Bw"), p.get("Vws"), (int)p.Dm, M, (int)p.ldD, nb, SVD_REGUL_CONST, p.get<double>("tauw"), p.get("R2w"), p.get("Nw"),
                     p.get<double>("sv") + M, p.get<int>("jsweeps") + 1, Z + g_stride, st);
    p.mark("factor_bins");
    const int ls_end = std::min(p.kcut0, p.P);
    launch_wa_ls(p.get("Hc"), p.ldD, ls_end, Z + g_stride, p.ldD, (int)p.Dm, M, p.P, 1, ls_end, p.get("W"), st);
    p.mark("ls_bins");
    DenseSweepArgs a{};
    a.D = (int)p.Dm; a.C = M; a.ldD = (int)p.ldD; a.P = p.P;
    a.X = X; a.x_stride = g_stride; a.Zd = Z; a.z_stride = g_stride;
    a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
    a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG; a.dpw = 0;
    const int k0 = std::max(p.kcut0, 1);
    a.kfirst = k0;
    p.sweep_launches = 0;
    for (int kb = k0; kb < p.P; ++kb) { launch_sweep_wide(a, kb, true, st); ++p.sweep_launches; }
    if (k0 < p.P) launch_sweep_wide_finalize(p.get("Wpart"), p.get("W"), p.nWG, M, p.P, p.P - 1, st);
    p.mark("magls_sweep");
    launch_filter_epilogue(p.get("W"), M, p.nfft, (int)d.len, p.get("tw"), p.get<double>("grpd"), 0, 1, 1, 0, p.get("wL"), p.get("wR"), st);
    p.mark("epilogue");
}

void execute_from_atf(emagls_plan& p) {
    if (p.wide) { execute_from_atf_wide(p); return; }
    // (eager / profiled executes; plan_execute captures the stages around the sweep otherwise.  More than 4096 matched directions:
    // the Gram route first as well, emagls_run_sweep then launches bin by bin; flagged bins take the dense route's tiled form)
    // (9..32 microphones without the resident sweep on more rows than factor.hip's 32-column tiles hold, e.g. more than 3072 matched
    // directions: the Gram route first as well, the flagged bins on the dense route of that width)
    if (p.sweep_persist || p.Dm > 4096 || (p.C > FROM_ATF_DENSE_REG && p.Dm > 768)) {
        from_atf_pre_sweep(p);
        emagls_run_sweep(p);
        from_atf_post_sweep(p);
        return;
    }
    hipStream_t st = p.stream;
    const emagls_design_desc& d = p.d;
    const int M = p.C;
    // ---- grid matching (FromAtf.m:56-95)
    if (p.hrir_smaller)
        launch_grid_match(p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), d.ndirs, p.get<double>("atf_azi"),
                          p.get<double>("atf_zen"), d.natf, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    else
        launch_grid_match(p.get<double>("atf_azi"), p.get<double>("atf_zen"), d.natf, p.get<double>("hrir_azi"),
                          p.get<double>("hrir_zen"), d.ndirs, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    launch_atf_colidx(p.hrir_smaller ? p.get<int64_t>("match_idx") : nullptr, p.Dm, M, p.get<int64_t>("colidx"), st);
    p.mark("grid_match");
    stage_prologue(p, 1, p.hrir_smaller ? nullptr : p.get<int64_t>("match_idx"), p.Dm);
    // atfs = fft(atfIrs, nfft) on the matched directions only: X[kb][m][d]
    launch_real_fft_gather(p.get<double>("atf"), d.atf_taps, (int64_t)M * p.Dm, p.get<int64_t>("colidx"), p.nfft, p.get("tw"),
                           p.get("X"), (int64_t)M * p.ldD, p.Dm, p.ldD, st);
    p.mark("atf_fft");
    const int ls_end = std::min(p.kcut0, p.P);
    {
        FactorArgs a{};
        a.S = (int)p.Dm; a.C = M; a.ldS = (int)p.ldD; a.kb0 = 1; a.P = p.P;
        a.Xd = p.get<cplx>("X"); a.xd_stride = (int64_t)M * p.ldD;
        a.reg_mode = 0; a.reg_c = SVD_REGUL_CONST;
        a.Z = p.get<cplx>("Z"); a.Vws = p.get<cplx>("Vws"); a.sv = p.get<double>("sv");
        a.Hq = p.get<cplx>("Hc"); a.ldHq = p.ldD; a.hq_estride = (int64_t)ls_end * p.ldD; a.ls_end = ls_end;
        a.W = p.get<cplx>("W"); a.sweeps_out = p.get<int>("jsweeps");
        a.tauw = p.get<double>("tauw"); a.R2w = p.get<cplx>("R2w"); a.Nw = p.get<cplx>("Nw");
        launch_factor(a, p.P - 1, true, st);
    }
    p.mark("factor_bins");
    {
        DenseSweepArgs a{};
        a.D = (int)p.Dm; a.C = M; a.ldD = (int)p.ldD; a.P = p.P;
        a.X = p.get("X"); a.x_stride = (int64_t)M * p.ldD; a.Zd = p.get("Z"); a.z_stride = (int64_t)M * p.ldD;
        a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
        a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG;
        const int k0 = std::max(p.kcut0, 1);
        a.kfirst = k0;
        p.sweep_launches = 0;
        for (int kb = k0; kb < p.P; ++kb) {
            if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches);
            launch_sweep_dense(a, kb, true, st);
            if (p.prof_level >= 2) record_sweep_event(p, 2 * (size_t)p.sweep_launches + 1);
            ++p.sweep_launches;
        }
        if (k0 < p.P) launch_sweep_finalize(p.get("Wpart"), p.get("W"), p.nWG, M, p.P, p.P - 1, st);
    }
    p.mark("magls_sweep");
    launch_filter_epilogue(p.get("W"), M, p.nfft, (int)d.len, p.get("tw"), p.get<double>("grpd"), 0, 1, 1, 0, p.get("wL"),
                           p.get("wR"), st);
    p.mark("epilogue");
}

void run_pipeline(emagls_plan& p) {
    const emagls_design_desc& d = p.d;
    p.stage_names.clear();
    launch_zero(p.get("flag"), sizeof(int) * NFLAG, p.stream);
    if (p.has("route")) launch_zero(p.get("route"), p.bufs["route"].bytes, p.stream);
    if (p.has("W")) launch_zero(p.get("W"), p.bufs["W"].bytes, p.stream);
    p.mark("begin");
    switch (d.kind) {
        case EMAGLS_KIND_LS: execute_ls(p); break;
        case EMAGLS_KIND_MAGLS:
        case EMAGLS_KIND_MAGLS_2D: execute_magls(p); break;
        case EMAGLS_KIND_EMAGLS:
        case EMAGLS_KIND_EMAGLS2:
        case EMAGLS_KIND_EMA_CH:
        case EMAGLS_KIND_EMA_SH: execute_emagls(p); break;
        default: execute_from_atf(p); break;
    }
}
}  // namespace

namespace emagls {
void stage_prologue(emagls_plan& p, int mode, const int64_t* didx, int64_t Dh) {
    hipStream_t st = p.stream;
    const emagls_design_desc& d = p.d;
    launch_twiddles(p.nfft, p.get("tw"), st);
    // group delay from the sum over ALL HRIR directions (lib/getEMagLsFilters.m:74-75)
    launch_hrir_grpdelay(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, d.ndirs, p.nfft, p.get("tw"),
                         p.get<double>("dirsum"), p.get<double>("grpd"), st);
    launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, Dh, didx, p.nfft, p.get("tw"), p.get<double>("grpd"),
                    mode, std::min(p.kcut0, p.P), p.kcut0, p.get("Hc"), p.get<double>("Habs"), p.ldD, st);
    if (p.diffuse && mode == 0)
        launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, Dh, didx, p.nfft, p.get("tw"), p.get<double>("grpd"),
                        0, p.P, p.P, p.get("Hfull"), p.get<double>("Habs"), p.ldD, st);
    p.mark("hrir_prologue");
}

void execute_ls(emagls_plan& p) {
    stage_hrir_basis(p);
    run_pinv_of_R(p);
    launch_ls_filters(p.get<double>("hL"), p.get<double>("hR"), p.d.nsamp, (int)p.D, p.get("Ypinv"), p.cplx_basis, p.ldD,
                      p.C, p.get("wL"), p.get("wR"), p.stream);
    p.mark("ls_filters");
}
void magls_post_sweep(emagls_plan& p) {
    hipStream_t st = p.stream;
    const bool cb = p.cplx_basis;
    if (p.diffuse)   // pwGrid is Y_conj for every bin
        launch_diffuse_constraint(p.get("W"), p.get("Xc"), cb, 0, 1, p.get("Hfull"), (int)p.D, p.C, p.ldD, p.P, st);
    // complex basis: getShFreqDomainConjugate (getMagLsFilters.m) / getChFreqDomainConjugate (getMagLsFilters2D.m:82-83)
    launch_filter_epilogue(p.get("W"), p.C, p.nfft, (int)p.d.len, p.get("tw"), p.get<double>("grpd"),
                           cb ? (p.d.kind == EMAGLS_KIND_MAGLS_2D ? 2 : 1) : 0, 0, 0,
                           p.out_cplx ? 1 : 0, p.get("wL"), p.get("wR"), st);
    p.mark("epilogue");
}

// The synthesising sweep needs the Gram-route bins only: M~_k of the swept bins, the start value W(k_cut-1,:) (a least-squares bin of the
// Gram route), |H|, the Chebyshev coefficients.  The Cholesky factor of the grid's SH Gram matrix and the whole orthonormal route of
// the ill-conditioned low bins (T_n, Householder QR, Jacobi, back-transform, their least-squares rows: bins 1 .. hh_end-1) feed the
// filters' rows, i.e. the epilogue AFTER the sweep -- 0.9 ms of the 3 ms a lone 20-design chunk spent before its sweep.  A batch
// therefore runs them next to the sweep on a stream of their own (batch_execute_lanes).  EMAGLS_DEFER_HH=0: everything before the sweep.
bool plan_defers_hh_route(const emagls_plan& p) {
    const int k0 = std::max(p.kcut0, 1);
    return sw_int<Sw::DEFER_HH>() != 0 && p.synth && !p.diffuse && p.prof_level == 0 && p.d.kind != EMAGLS_KIND_EMA_SH && p.gram_from > 0 && p.hh_end > 1 && p.hh_end <= k0 - 1;
}
// ---- The HRIR-side stages of an array design (lib/getEMagLsFilters.m:72-81, :94), for the plan h that owns the HRIR set on the
// geometry of plan g.  emagls_pre_sweep calls them with g = h; a geometry-sharing batch (batch_geo_stage) with plan 0 as g, or, in
// lane mode, with the lanes' own copies of plan 0's operands.  Both forms CALL these functions: that is what gives plan 0's filters
// the same bits in a cold, a warm and a single-plan execute.
// the spectra: H of the least-squares bins (and its transpose HcT for the rows below), |H| of the swept bins, the group delays
void hrir_spectra(emagls_plan& h, const emagls_plan& g, hipStream_t st, bool transposed) {
    const emagls_design_desc& d = h.d;
    const int ls_end = std::min(g.kcut0, g.P);
    launch_twiddles(h.nfft, h.get("tw"), st);
    launch_hrir_grpdelay(h.get<double>("hL"), h.get<double>("hR"), d.nsamp, d.ndirs, h.nfft, h.get("tw"), h.get<double>("dirsum"),
                         h.get<double>("grpd"), st);
    launch_hrir_fft(h.get<double>("hL"), h.get<double>("hR"), d.nsamp, h.D, nullptr, h.nfft, h.get("tw"), h.get<double>("grpd"), 0, ls_end,
                    h.kcut0, h.get("Hc"), h.get<double>("Habs"), h.ldD, st, (transposed && ls_end > 0) ? h.get<double>("HcT") : nullptr,
                    round_up(4 * std::max(ls_end, 1), 64));
}
// arguments of the Householder route's launches (factor.hip): Z, Hq, W and the status words are the HRIR set's, everything else the
// geometry's.  sweeps_out: jsweeps in a plan's own pipeline, null for a subject; cond_ok: null until launch_cond_flags has written it
FactorArgs hh_factor_args(emagls_plan& h, emagls_plan& g, int* sweeps_out, double* cond_ok) {
    const int ls_end = std::min(g.kcut0, g.P);
    FactorArgs fa{};
    fa.S = g.S_h; fa.C = g.C; fa.ldS = g.ldS_h; fa.kb0 = 1; fa.P = g.P;
    fa.Tn = g.get("Tn"); fa.bn = g.get<cplx>("bn"); fa.nOrders = g.n_h + 1; fa.bn_stride = g.simOrder + 1;
    fa.reg_mode = 0; fa.reg_c = SVD_REGUL_CONST;
    fa.Z = h.get<cplx>("Z");
    fa.Mw = g.get<cplx>("Mw");
    fa.Vws = g.get<cplx>("Vws"); fa.sv = g.get<double>("sv");
    fa.Hq = h.get<cplx>("Hq"); fa.ldHq = g.ldS_h; fa.hq_estride = (int64_t)ls_end * g.ldS_h; fa.ls_end = std::min(ls_end, g.hh_end);
    fa.hq_conj = 1;
    fa.route = g.get<int>("route"); fa.status = h.get<int>("flag");
    fa.cond_limit = 10.0 * GRAM_COND_EST;   // (not the env override: the forced-estimate test must trip this check)
    fa.W = h.get<cplx>("W"); fa.sweeps_out = sweeps_out;
    fa.tauw = g.get<double>("tauw"); fa.R2w = g.get<cplx>("R2w"); fa.Nw = g.get<cplx>("Nw");
    fa.cond_ok = cond_ok;
    return fa;
}
// the least-squares right-hand sides H conj(Q) of the Householder-route bins.  Q itself is never formed: H conj(Q) is
// conj( conj(H conj(Yc)) R^-1 ), one D-long product and a row solve for the least-squares rows
void hrir_hh_rows(emagls_plan& h, emagls_plan& g, hipStream_t st) {
    const bool cb = g.cplx_basis;
    const int ls_end = std::min(g.kcut0, g.P);
    launch_hy_conj_mfma(h.get<double>("HcT"), round_up(4 * std::max(ls_end, 1), 64), ls_end, g.get("Yc"), g.ldS, cb, (int)g.D, g.S_h,
                        h.get<double>("Hyp"), h.get("Hq"), g.ldS_h, st);
    // (also forms the inverses of R's diagonal blocks, which the ill-conditioned swept bins need: at least one row)
    launch_qform(h.get("Hq"), g.get(cb ? "R" : "Rc"), h.get(cb ? "Rinv" : "Rinvc"), g.S_h, 2 * (int64_t)std::max(ls_end, 1), g.ldS_h, true, h.get("Hq"), st);
}
// back-transform + least-squares bins of the Householder route (into the HRIR set's own Z and W)
void hrir_hh_back(const FactorArgs& fa, const emagls_plan& g, hipStream_t st) { launch_factor(fa, g.hh_end - 1, g.cplx_basis, st, 2); }
// least-squares bins on the Gram route.  Synthesising designs: u(k) = H(k,:) conj(g_k) from the angles (the HRIR set's own copies of
// the grids and of the row order), then W(k,:) = (u Pm^T) conj(M_k) like the swept bins' rows, on the coefficients, Pm and M_k of
// `src`; lanes_share: `src` is ONE design's for every lane of the launch.  Otherwise on g's G_k and M_k.
void hrir_gram_ls_rows(emagls_plan& h, emagls_plan& g, const emagls_plan& src, bool lanes_share, hipStream_t st) {
    const int gf = g.gram_from, ls_end = std::min(g.kcut0, g.P), M = (int)g.d.nmics;
    if (!(gf > 0 && gf < ls_end)) return;
    if (g.synth) {
        launch_synth_ls(h.get("Hc"), h.ldD, ls_end, src.bufs.at("bsc").p, synth_nord_pad(g.simOrder + 1), h.get<double>("hrir_azi"), h.get<double>("hrir_zen"),
                        h.get<double>("mic_azi"), h.get<double>("mic_zen"), h.get<int>("smap"), (int)g.D, M, g.P, gf, ls_end, h.get("Usw"), st, lanes_share);
        launch_synth_rows(h.get("Usw"), synth_ls_chunks((int)g.D), src.bufs.at("Pm").p, src.bufs.at("Mw").p, g.C, M, gf, ls_end, g.P, h.get("W"), st, lanes_share);
    } else {
        const int64_t g_stride = (int64_t)g.C * g.ldD;
        launch_ls_gram(h.get("Hc"), h.ldD, ls_end, g.get<cplx>("G") - (int64_t)g.g0 * g_stride, g_stride, g.ldD, g.get("Mw"), (int)g.D, g.C, g.P, gf,
                       ls_end, h.get("W"), st);
    }
}
// what every execute of a design begins with: no stage marks, clean status words, zero filters' rows
void subject_reset(emagls_plan& p, hipStream_t st) {
    p.stage_names.clear();
    launch_zero(p.get("flag"), sizeof(int) * NFLAG, st);
    launch_zero(p.get("W"), p.bufs["W"].bytes, st);
}

void emagls_pre_sweep(emagls_plan& p) {
    if (p.d.kind == EMAGLS_KIND_EMA_SH) { ema_sh_pre_sweep(p); return; }
    const emagls_design_desc& d = p.d;
    const bool cb = p.cplx_basis;
    const bool raw = d.kind == EMAGLS_KIND_EMAGLS2;
    const int M = (int)d.nmics;
    const int ldM = round_up(M, 64);
    // side streams shorten one design's critical path; with several designs in flight they only add queue
    // contention, so a plan can be restricted to its main stream (emagls_plan_set_streams / EMAGLS_STREAMS=1)
    if (p.nstreams >= 2) p.need_sides(p.nstreams);   // (no-op for a lane group: batch_lanes_part lends the batch's streams)
    hipStream_t s0 = p.stream, s1 = p.nstreams >= 2 ? p.side[0] : s0, s2 = p.nstreams >= 3 ? p.side[1] : s0;
    hipStream_t s3 = p.nstreams >= 4 ? p.side[2] : s0;   // the Gram route of the per-bin factors (needs Gy, E, b_n; not the Cholesky factor)
    const int nOrd = p.simOrder + 1;
    const int k0 = std::max(p.kcut0, 1);
    // routes (plan_routes): Householder bins [1, hh_end) on the orders 0..n_h, Gram-route bins [gf, P) on all orders
    // (the least-squares bins among them: below min(k_cut, hh_end) on the Householder route, the others on the Gram route)
    const int gf = p.gram_from, hh_end = p.hh_end, Sh = p.S_h, ldSh = p.ldS_h, nOrdH = p.n_h + 1;
    const int phase = plan_defers_hh_route(p) ? p.pre_phase : 0;
    if (phase != 2) p.sync_used = 0;

    // The stages before the sweep as blocks.  Their data dependencies: array (mic SH matrix, E, b_n) <- nothing; prologue (HRIR
    // spectra) <- nothing; basis (Yc) <- nothing; gram (Gy, R) <- basis; chol <- gram; gterms (QT_n, G_k) <- basis, array;
    // rows (H conj(Q)) <- prologue, chol; gram_route (M_k of the Gram-route bins) <- gram, array; hh_route (QR + Jacobi of the
    // Householder-route bins) <- chol, array; flags <- gram_route, hh_route; back (Z_k, least-squares rows) <- flags, rows;
    // tail (least-squares rows of the Gram route, accurate Y_reg_inv) <- gterms, back.
    // order 0 issues them as three or four branches on the plan's streams (one design: shortest critical path).  Orders 1 and 2
    // are single-stream sequences for lane groups that run side by side (batch_execute_lanes): order 1 issues the kernels that
    // fill the chip first (HRIR transform, Gram matrix, G_k) and the latency-bound chains after them (Cholesky, per-bin
    // factors), order 2 the other way round -- two groups in the SAME order meet at the same kernels and add up their times,
    // two groups in complementary orders hide one's chains behind the other's bandwidth-bound kernels.
    const int order = (s1 == s0 && s2 == s0 && s3 == s0) ? p.stage_order : 0;
    hipEvent_t e_E = nullptr, e_Yc = nullptr, e_Gy = nullptr, e_R = nullptr;

    auto blk_array = [&] {
    // s1: array model  E = Y_mic (raw) or pinv(Y_mic(:,1:nOut)) Y_mic   (getSMAIRMatrix.m:101-102,119-121), b_n(kr)
    if (!p.custom_basis)
        launch_sh_basis(p.simOrder, M, p.get<double>("mic_azi"), p.get<double>("mic_zen"), p.get<double>("sh_tab"), cb,
                        p.get("Ymic_cm"), M, s1);
    // (raw: both Ymic_rm and E are written; EMAinCH: pinv(chFunction(order, micGridAziRad)), getEMagLsFiltersEMAinCH.m:70)
    array_encoder(raw ? Encoder::RAW : d.kind == EMAGLS_KIND_EMA_CH ? Encoder::CH_PINV : Encoder::SH_PINV, p.get("Ymic_cm"), M, p.S, p.ldS, cb, d.order,
                  p.get<double>("mic_azi"), p.get("Ymic_rm"), raw ? PinvWs{} : plan_lo_ws(p), p.get("E"), s1);
    // bnAll = -sphModalCoeffs(simOrder, kr, 'rigid')   (getSMAIRMatrix.m:107)
    launch_modal_bn(p.simOrder, p.P, p.get<double>("kr"), 1.0, -1.0, p.get("bn"), nOrd, 1, s1, p.get<int>("nvalid"));
    if (p.synth)   // scaled modal terms of the Legendre series and pinv(Y_lo) as the real matrix Pm (identity: raw microphones)
        launch_synth_prepare(p.get("bn"), nOrd, p.P, p.get("bsc"), raw ? nullptr : p.get("Zlo"), ldM, p.C, M, p.get<int>("smap"), p.get<double>("Pm"), s1);
    e_E = p.next_sync_event();
    if (s1 != s0) HIP_CHECK(hipEventRecord(e_E, s1));
    };

    auto blk_prologue = [&] {
    // s2: HRIR prologue
        hrir_spectra(p, p, s2);
        if (p.diffuse)   // the target covariance needs the complex HRTFs of all bins (the sweep only keeps |H| above k_cut)
            launch_hrir_fft(p.get<double>("hL"), p.get<double>("hR"), d.nsamp, p.D, nullptr, p.nfft, p.get("tw"),
                            p.get<double>("grpd"), 0, p.P, p.P, p.get("Hfull"), p.get<double>("Habs"), p.ldD, s2);
    };

    auto blk_basis = [&] {
    // s0: SH matrix of the HRIR grid
    if (!p.custom_basis)
        launch_sh_basis(p.simOrder, p.D, p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), p.get<double>("sh_tab"), cb,
                        p.get("Ycm"), p.ldD, s0);
    launch_transpose_conj(p.get("Ycm"), p.D, p.S, p.ldD, p.get("Yc"), p.Dpad, p.ldS, cb, true, s0);
    p.mark("sh_basis");
    e_Yc = p.next_sync_event();
    if (s1 != s0) HIP_CHECK(hipEventRecord(e_Yc, s0));
    };
    auto blk_gram = [&] {
    // s0: Gram matrix Gy of conj(Y); its leading block (Householder-route orders) goes to R
    launch_gram(p.get("Yc"), p.D, p.S, p.ldS, cb, p.get("Gp"), p.get("Gy"), p.get("R"), Sh, s0);
    p.mark("gram_mfma");
    e_Gy = p.next_sync_event();
    if (s3 != s0) HIP_CHECK(hipEventRecord(e_Gy, s0));
    };
    auto blk_chol = [&] {
    launch_cholesky(p.get("R"), Sh, cb, p.get<int>("flag"), s0);
    p.mark("cholesky");
    e_R = p.next_sync_event();
    if (s2 != s0) HIP_CHECK(hipEventRecord(e_R, s0));
    };

    auto blk_gterms = [&] {
    // s1 (after the array model): order terms of pwGrid.' and G_k of every bin from g0 on -- needs only conj(Y) and E
    if (s1 != s0) HIP_CHECK(hipStreamWaitEvent(s1, e_Yc, 0));
    // (the synthesising sweep and its least-squares bins evaluate their operands themselves: neither order terms nor G_k)
    const int g_end = p.synth ? p.g0 : p.P;
    if (g_end > p.g0) {
    launch_qt(p.get("Yc"), p.ldS, p.get("E"), p.ldS, (int)p.D, p.S, p.C, nOrd, cb, p.get("QT"), p.ldD, s1);
    // (complex-arithmetic pipeline: G_k is still evaluated on the real order terms; circular-harmonic
    // channels would need their own channel transform and take the complex kernel)
    launch_dspace_g(p.get("QT"), p.ldD, cb, p.get("bn"), nOrd, (int)p.D, p.C, p.P, p.g0, p.get("G"), s1,
                    (cb && d.kind != EMAGLS_KIND_EMA_CH && !p.custom_basis) ? 1 : 0, raw ? -1 : (int)d.order, g_end);
    }
    };
    auto blk_rows = [&] {
    // s2 (after the prologue): the least-squares right-hand sides H conj(Q) of the Householder-route bins
    if (s2 != s0) HIP_CHECK(hipStreamWaitEvent(s2, e_R, 0));
    if (hh_end > 1) {
        // (real basis: the rows are complex all the same, so R is widened to a complex copy for the row solves)
        if (!cb) launch_widen(p.get("R"), Sh, false, p.get("Rc"), Sh, Sh, Sh, false, /*upper_only=*/true, s2);
        hrir_hh_rows(p, p, s2);
    }
    };

    // s0: per-bin factors.  Gram route first (needs E, b_n, Gy): K matrices, one GEMM over the bins, direct inverses
    // (on a stream of its own with four streams: it does not need the Cholesky factor, the Householder route does)
    FactorArgs fa = hh_factor_args(p, p, p.get<int>("jsweeps"), nullptr);   // (cond_ok: blk_flags)
    auto blk_gram_route = [&] {
    if (s1 != s0) HIP_CHECK(hipStreamWaitEvent(s0, e_E, 0));
    if (s3 != s0) { HIP_CHECK(hipStreamWaitEvent(s3, e_Gy, 0)); HIP_CHECK(hipStreamWaitEvent(s3, e_E, 0)); }
    if (p.nb_gram > 0) {
        const int ldK = round_up(p.C * p.C, 64), ldCf = round_up(p.P, 64);
        launch_gram_kmat(p.get("Gy"), p.get("E"), p.S, p.ldS, p.C, nOrd, cb, p.get("Fg"), p.ldS, p.get<double>("Kmat"), ldK, s3);
        launch_gram_gemm(p.get("bn"), nOrd, p.P, gf, p.nb_gram, p.get<double>("Cf"), ldCf, p.get<double>("Kmat"), ldK, p.C,
                         p.get<double>("Apk"), ldK, s3);
        launch_gram_solve(p.get<double>("Apk"), ldK, p.C, gf, p.nb_gram, SVD_REGUL_CONST, p.get("Mw"), p.get("R2w"), p.get<double>("sv"),
                          p.get<int>("route"), p.get<int>("jsweeps"), s3);
        // bins in which the 1 % clipping is active (cond > 100) or the certificate failed: Jacobi SVD of the Gram matrix
        FactorArgs fg = fa;
        fg.kb0 = gf;
        const int64_t off = (int64_t)(gf - 1);
        fg.R2w = fa.R2w + off * p.C * p.C; fg.Mw = fa.Mw + off * p.C * p.C; fg.Nw = fa.Nw + off * p.C * p.C; fg.tauw = fa.tauw + off * p.C;
        // batches have workgroups to spare: a Jacobi workgroup walks a run of neighbouring bins, each warm-started from the
        // previous one (a third of the sweeps); a single design keeps one bin per workgroup (shortest critical path)
        fg.jrun = jacobi_run_length(p);
        launch_factor_jacobi_gram(fg, p.nb_gram, s3);
        p.mark("gram_route");
    }
    };
    auto blk_hh_route = [&] {
    // Householder route: T_n of the orders 0..n_h, per-bin QR + Jacobi
    if (hh_end > 1) {
        launch_tn(p.get("R"), p.get("E"), Sh, p.C, p.ldS, nOrdH, cb, p.get("Tn"), ldSh, s0);
        p.mark("array_model+tn");
        launch_factor(fa, hh_end - 1, cb, s0, 1);
    }
    };
    auto blk_flags = [&] {
    // cond_ok[kb]: the cheap direction-space identity is accurate for this bin.  Only the other swept bins (and the
    // least-squares bins) need Z_k, i.e. the back-transform
    p.depend(s0, s3);   // (singular-value bounds of the Gram-route bins)
    launch_cond_flags(p.get<double>("sv"), p.C, p.P, hh_end, p.get<double>("cond_ok"), s0);
    fa.cond_ok = p.get<double>("cond_ok");
    p.mark("factor_qr_jacobi");
    };
    auto blk_back = [&] {
    // join s2 (Hq, spectra, group delays): back-transform + least-squares bins of the Householder route
    p.depend(s0, s2);
    if (hh_end > 1) hrir_hh_back(fa, p, s0);
    p.mark("factor_back+ls_bins");
    };
    auto blk_tail = [&] {
    // join s1 (G)
    p.depend(s0, s1);
    hrir_gram_ls_rows(p, p, p, false, s0);   // least-squares bins on the Gram route
    // ill-conditioned swept bins (Householder route only): Y_reg_inv_k = conj(Q) Z_k = conj(Yc) (Z_k R^-H); the flagged bins'
    // Z rows are solved in place first
    if (hh_end > k0) {
        launch_zsolve_flagged(p.get("Z"), ldSh, p.get(cb ? "R" : "Rc"), p.get(cb ? "Rinv" : "Rinvc"), p.get<double>("cond_ok"), Sh, p.C,
                              hh_end, k0, s0);
        launch_yri_accurate(p.get("Yc"), p.ldS, cb, p.get("Z"), ldSh, p.get<double>("cond_ok"), (int)p.D, Sh, p.C, hh_end, k0,
                            p.get("Yri"), p.ldD, s0, p.custom_basis ? nullptr : p.get("Ycm"), p.ldD);
    }
    // synthesising sweep: the chain runs in the microphone domain on Mt_k = Pm^T M_k Pm, from the start value W(k0-1,:) Pm
    if (p.synth) launch_synth_mt(p.get("Mw"), p.get<double>("Pm"), p.C, M, k0, p.P, p.get("W"), p.get("Mt"), p.get("Winit"), s0);
    };

    if (phase == 2) {   // what the sweep did not need, on one stream: Cholesky factor, orthonormal route of the low bins, their rows
        blk_chol(); blk_rows(); blk_hh_route(); blk_flags(); blk_back();
        return;
    }
    launch_sh_coeff(p.simOrder, p.get<double>("sh_tab"), s0);
    if (phase == 1) {   // only what the sweep needs (forked like order 0 when the plan has side streams)
        if (s1 != s0) p.depend(s1, s0);
        if (s2 != s0) p.depend(s2, s0);
        // (tried: the least-squares bins' partial sums u(k) = H(k,:) conj(g_k) on the prologue's stream, off this path -- 2755-2813 against
        // 2802-2855 sets/s at 20 steps: the Gram route then queued behind the HRIR transform in one hardware queue)
        blk_array(); blk_prologue(); blk_basis(); blk_gram(); blk_gterms(); blk_gram_route();
        p.depend(s0, s2);   // (spectra of the least-squares bins, |H|)
        p.depend(s0, s3);   // (M_k of the Gram-route bins when that route has a stream of its own)
        blk_tail();
        p.mark("yri_operands");
        return;
    }
    if (order == 1) {          // bandwidth-bound kernels first
        blk_array(); blk_prologue(); blk_basis(); blk_gram(); blk_gterms();
        blk_chol(); blk_rows(); blk_gram_route(); blk_hh_route(); blk_flags(); blk_back(); blk_tail();
    } else if (order == 2) {   // latency-bound chains first
        blk_array(); blk_basis(); blk_gram(); blk_chol(); blk_gram_route(); blk_hh_route(); blk_flags();
        blk_prologue(); blk_rows(); blk_gterms(); blk_back(); blk_tail();
    } else {
        // ---- fork: three independent branches
        p.depend(s1, s0);
        p.depend(s2, s0);
        blk_array(); blk_prologue(); blk_basis(); blk_gram(); blk_chol(); blk_gterms(); blk_rows();
        blk_gram_route(); blk_hh_route(); blk_flags(); blk_back(); blk_tail();
    }
    p.mark("yri_operands");
}

HalfSweepArgs emagls_half_args(emagls_plan& p) {
    const int k0 = std::max(p.kcut0, 1);
    HalfSweepArgs a{};
    a.D = (int)p.D; a.C = p.C; a.ldD = (int)p.ldD; a.P = p.P;
    a.g_stride = (int64_t)p.C * p.ldD;
    if (p.d.kind == EMAGLS_KIND_FROM_ATF) {   // G_k = the matched ATF spectra of bin k, [kb][m][ldD]; bins below the Gram route: Y_reg_inv in Z
        a.D = (int)p.Dm;
        a.G = p.get<cplx>("X");
        a.Yri = p.get<cplx>("Z");
    } else if (magls_kind(p.d.kind)) {   // one operand for every bin (magls_pre_sweep)
        a.g_stride = 0;
        a.G = p.get<cplx>("Gm");
        a.Yri = a.G;             // (never read: every bin is well conditioned)
    } else {
    a.G = p.get<cplx>("G") - (int64_t)p.g0 * a.g_stride;    // indexed by kb (G starts at bin g0 <= k0)
    a.Yri = p.get<cplx>("Yri") - (int64_t)k0 * a.g_stride;
    }
    a.Mw = p.get<cplx>("Mw") - (int64_t)1 * p.C * p.C;      // factor stage stores bin kb at slot kb-1
    a.cond_ok = p.get<double>("cond_ok");
    a.Habs = p.get<double>("Habs"); a.ldH = p.ldD; a.kabs0 = p.kcut0;
    a.Wpart = p.get<cplx>("Wpart"); a.W = p.get<cplx>("W"); a.nWG = p.nWG_dense; a.kfirst = k0;
    a.ll = p.get<unsigned long long>("ll");
    a.abort_flag = p.get<int>("flag") + 1;
    a.skip_flag = magls_kind(p.d.kind) ? p.get<int>("flag") + 4 : nullptr;
    a.timing = p.has("sweep_timing") ? p.get<long long>("sweep_timing") : nullptr;
    a.force_global = sw_on<Sw::PERSIST_GLOBAL>() ? 1 : 0;
    a.fetch_mode = sw_int<Sw::SWEEP_FETCH>();
    a.wait_ticks = (long long)sw_int<Sw::SWEEP_WAIT_MS>() * 100000ll;
    if (p.synth) {   // the chain's channels are the microphones (sweep_synth.hip)
        const int M = (int)p.d.nmics;
        a.C = M;
        a.G = nullptr; a.Yri = nullptr;
        a.Mw = p.get<cplx>("Mt") - (int64_t)M * M;
        a.dir_azi = p.get<double>("hrir_azi"); a.dir_zen = p.get<double>("hrir_zen");
        a.mic_azi = p.get<double>("mic_azi"); a.mic_zen = p.get<double>("mic_zen");
        a.smap = p.get<int>("smap");
        a.bsc = p.get<cplx>("bsc"); a.nord_pad = synth_nord_pad(p.simOrder + 1);
        a.synth_split = sw_int<Sw::SYNTH_SPLIT>();
        a.synth_prio = sw_int<Sw::SYNTH_PRIO>();
        a.Winit = p.get<cplx>("Winit"); a.U = p.get<cplx>("Usw");
    }
    return a;
}

// A persistent sweep needs all of its workgroups resident.  Two sweeps launched from different streams could each get a
// part of the CUs and wait for the rest forever (the kernels would give up after their time-out and report an error), so the
// sweeps of a device pass through one gate that counts workgroup slots per XCD: a sweep is launched behind as many of the
// earlier ones (oldest first, by their completion events) as it takes for everything that may still be running next to it to
// fit.  The register-resident form (sweep_reg.hip) takes ceil(n / 8) x nWG of the 96 slots of its kind an XCD has (3 workgroups
// per CU), so several of its launches run side by side; the slab forms (sweep_persist.hip, sweep_synth.hip) fill every CU's LDS
// and take the whole gate.  The sweep is therefore never part of a captured graph (plans and batches capture the stages before
// it).  The gate's state is per device and guarded by a mutex: plans of different host threads may sweep on the same GPU.
std::mutex& SweepGate::mutex() { static std::mutex m; return m; }
SweepGate::State& SweepGate::state() {   // (call with the mutex held)
    static std::map<int, State> per_device;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    State& st = per_device[dev];
    if (st.capacity == 0) st.capacity = std::max(1, reg_sweep_slots_per_xcd());
    return st;
}
SweepGate::SweepGate(hipStream_t s, int slots_per_xcd) : lock(mutex()), st(s), slots(0) {
    State& g = state();
    slots = slots_per_xcd <= 0 ? g.capacity : std::min(slots_per_xcd, g.capacity);
    // finished launches no longer hold slots (anywhere in the queue: launches of different sizes finish out of order)
    for (auto it = g.inflight.begin(); it != g.inflight.end();) {
        if (hipEventQuery(it->ev) == hipSuccess) { g.pool.push_back(it->ev); it = g.inflight.erase(it); }
        else ++it;
    }
    (void)hipGetLastError();   // (hipErrorNotReady of the query is not an error)
    // Everything that has not FINISHED may still run next to this launch unless this launch waits for it -- also a launch that
    // an earlier one already waits for (it may not even have started: sweeps are enqueued behind the stages before them).  So
    // an entry stays in the queue, and counts for every later launch, until its event reports completion; this launch waits
    // for the oldest entries, as many as it takes for the rest to fit next to it.
    int held = 0;
    for (const Entry& e : g.inflight) held += e.slots;
    for (const Entry& e : g.inflight) {
        if (held + slots <= g.capacity) break;
        HIP_CHECK(hipStreamWaitEvent(st, e.ev, 0));
        held -= e.slots;
    }
}
SweepGate::~SweepGate() {   // (the lock is held from the waits to the record: no other sweep can slip in between)
    try {
        State& g = state();
        hipEvent_t ev = nullptr;
        if (!g.pool.empty()) { ev = g.pool.back(); g.pool.pop_back(); }
        else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        const hipError_t e = ev ? hipEventRecord(ev, st) : hipErrorUnknown;
        if (e == hipSuccess) g.inflight.push_back(Entry{ev, slots});
        else {   // (e.g. the stream belongs to another device than the calling thread's current one: the next sweep would not
                 // be ordered behind this one -- never silently)
            (void)hipGetLastError();
            fprintf(stderr, "emagls: the sweep gate's event could not be recorded (%s): persistent sweeps are no longer ordered\n",
                    hipGetErrorString(e));
        }
    } catch (...) {}
}
// does the register-resident form serve these `n` designs (all synthesising, of one shape) in one launch?  Up to 8 designs (one per
// XCD) the slab form is the faster one -- 5.4 us per bin on 29 CUs per design against 7.0 us on 22 -- and a launch of its own has the
// device to itself anyway; from 9 designs on the register-resident form wins (16 designs: 3.8 against 3.4 ms next to each other, but
// 32 designs in 5.2 ms and room for other kernels).
bool reg_sweep_wanted(emagls_plan* const* plans, int n) {
    const int mode = sw_int<Sw::SWEEP_REG>();
    if (mode == 0 || n < 1 || (mode == 1 && n < 9)) return false;
    const emagls_plan& q = *plans[0];
    for (int j = 0; j < n; ++j) {
        const emagls_plan& p = *plans[j];
        if (!p.synth || p.synth_units < 1 || p.synth_units > reg_sweep_max_units() || p.D != q.D || !p.has("sweep_args")) return false;
    }
    return reg_sweep_fits((int)q.D, (int)q.d.nmics, q.synth_units, q.simOrder + 1, n);
}
// the argument blocks of a launch in device memory (stored again only when one of them changed)
void reg_args_upload(const HalfSweepArgs* host, int n, void* dev, std::vector<char>& last, hipStream_t st) {
    const size_t bytes = sizeof(HalfSweepArgs) * (size_t)n;
    if (last.size() == bytes && memcmp(last.data(), host, bytes) == 0) return;
    store_sweep_args(host, n, static_cast<HalfSweepArgs*>(dev), st);
    last.assign(reinterpret_cast<const char*>(host), reinterpret_cast<const char*>(host) + bytes);
}

void emagls_post_sweep(emagls_plan& p) {
    const bool raw = p.d.kind == EMAGLS_KIND_EMAGLS2;
    const int conj_mode = !p.req_cplx || raw ? 0 : (p.d.kind == EMAGLS_KIND_EMA_CH ? 2 : 1);   // Hermitian mirror / SH rule / CH rule
    if (p.synth) {   // the chain stored the microphone-domain totals u(k): W(k,:) = (u(k) Pm^T) conj(M_k) for the swept bins
        const emagls_plan& g = p.geo_from ? *p.geo_from : p;   // (geometry-sharing batches: plan 0's Pm and M_k)
        launch_synth_rows(p.get("Usw"), 1, g.bufs.at("Pm").p, g.bufs.at("Mw").p, p.C, (int)p.d.nmics, std::max(p.kcut0, 1), p.P, p.P, p.get("W"), p.stream,
                          p.geo_from != nullptr);
    }
    if (p.diffuse)   // (in the real-arithmetic pipeline W is still W_r here: the rendered HRTFs W G are the same in either basis)
        launch_diffuse_constraint(p.get("W"), p.get("G"), true, (int64_t)p.C * p.ldD, p.g0, p.get("Hfull"), (int)p.D, p.C, p.ldD, p.P,
                                  p.stream);
    if (p.real_internal && !raw) launch_sh_rows_to_complex(p.get("W"), p.C, 2 * p.P, (int)p.d.order, p.stream);   // W_c = W_r T_N
    launch_filter_epilogue(p.get("W"), p.C, p.nfft, (int)p.d.len, p.get("tw"), p.get<double>("grpd"), conj_mode, 1, 0,
                           p.out_cplx ? 1 : 0, p.get("wL"), p.get("wR"), p.stream);
    p.mark("epilogue");
}

// ---- getEMagLsFiltersFromAtf on the persistent sweep --------------------------------------------------------------------------
// pwGrid_k = atfsMatched(k,:,:) (M x Dm) is given, not modelled (FromAtf.m:100-104): G_k = X_k, its M x M Gram matrix from G_k
// itself (the EMAinSH route), M_k by the direct inverse / the Jacobi SVD of the Gram matrix.  Measured ATFs can be arbitrarily
// ill-conditioned at low frequencies: the device check of the Gram route (cond < 3e4) raises the status flag with the highest
// offending bin, the host moves the route's start behind it (plan_recover) and the bins below take the dense route
// (Householder QR + Jacobi SVD of X_k itself), whose Y_reg_inv the sweep reads directly (cond_ok = 0).
// What depends on the HRIR set of the subject, and what only on the grids and the ATFs (shared by a batch of subjects):
void from_atf_subject_stage(emagls_plan& p) {   // grid matching (cheap; the prologue needs the match) + HRIR prologue
    hipStream_t st = p.stream;
    const emagls_design_desc& d = p.d;
    if (p.hrir_smaller)
        launch_grid_match(p.get<double>("hrir_azi"), p.get<double>("hrir_zen"), d.ndirs, p.get<double>("atf_azi"),
                          p.get<double>("atf_zen"), d.natf, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    else
        launch_grid_match(p.get<double>("atf_azi"), p.get<double>("atf_zen"), d.natf, p.get<double>("hrir_azi"),
                          p.get<double>("hrir_zen"), d.ndirs, p.get<double>("cartB"), p.get<int64_t>("match_idx"),
                          p.get<double>("match_dev"), p.get<double>("mean_dev"), st);
    launch_atf_colidx(p.hrir_smaller ? p.get<int64_t>("match_idx") : nullptr, p.Dm, p.C, p.get<int64_t>("colidx"), st);
    p.mark("grid_match");
    stage_prologue(p, 1, p.hrir_smaller ? nullptr : p.get<int64_t>("match_idx"), p.Dm);
}
// least-squares bins on the Gram route with the operands of `sh` (the plan itself, or the plan whose ATF side a batch shares)
void from_atf_ls_rows(emagls_plan& p, emagls_plan& sh, hipStream_t st) {
    const int ls_end = std::min(p.kcut0, p.P), gf = sh.gram_from;
    if (gf > 0 && gf < ls_end)
        launch_ls_gram(p.get("Hc"), p.ldD, ls_end, sh.get("X"), (int64_t)p.C * p.ldD, p.ldD, sh.get("Mw"), (int)p.Dm, p.C, p.P, gf, ls_end,
                       p.get("W"), st);
}
void from_atf_post_sweep(emagls_plan& p) {
    launch_filter_epilogue(p.get("W"), p.C, p.nfft, (int)p.d.len, p.get("tw"), p.get<double>("grpd"), 0, 1, 1, 0, p.get("wL"),
                           p.get("wR"), p.stream);
    p.mark("epilogue");
}

void plan_execute(emagls_plan& p) {
    const emagls_design_desc& d = p.d;
    if (p.custom_basis) {
        if (!p.have_basis || !p.have_hrirs) throw Error(EMAGLS_ERR_ARG, "HRIRs and the SH matrices must be set before execute");
    } else {
        if (!p.have_hrir_grid || !p.have_hrirs) throw Error(EMAGLS_ERR_ARG, "HRIRs and their grid must be set before execute");
        if (array_kind(d.kind) && !p.have_mic_grid)
            throw Error(EMAGLS_ERR_ARG, "microphone grid must be set before execute");
    }
    if (d.kind == EMAGLS_KIND_FROM_ATF && !p.have_atfs) throw Error(EMAGLS_ERR_ARG, "ATFs must be set before execute");
    ++p.solo_runs;
    if (p.nstreams >= 2) p.need_sides(p.nstreams);   // (before any capture begins)
    const bool persist = d.kind != EMAGLS_KIND_LS && p.sweep_persist;
    if (p.prof_level == 0 && p.use_graph && persist) {
        // the persistent sweep is launched directly (SweepGate); the stages before it are captured from the second
        // execute on (the first runs eagerly: one-time function attributes, lazy module load)
        // a design with forked stages (it has the device to itself) runs what its sweep does not need -- Cholesky factor, orthonormal
        // route of the low bins: plan_defers_hh_route -- NEXT to the sweep, eagerly on a stream of its own (a dozen launches)
        if (!p.pre) p.defer_hh = (p.nstreams >= 2 || p.alone) && array_kind(d.kind) && plan_defers_hh_route(p);
        {
            Scoped phase(p.pre_phase, p.defer_hh ? 1 : 0);
            if (!p.pre && p.eager_runs >= 1 && !forks_streams(p)) p.pre.capture(p.stream, [&] { plan_pre_stage(p); });
            if (p.pre) p.pre.launch(p.stream); else plan_pre_stage(p);
        }
        if (p.defer_hh) {
            if (!p.hh_stream) p.hh_stream = StreamPool::get().take();
            p.depend(p.hh_stream, p.stream);   // (behind the stages the sweep needs, before the sweep is enqueued)
        }
        emagls_run_sweep(p);
        if (p.defer_hh) {
            {
                Scoped st(p.stream, p.hh_stream);
                Scoped one(p.nstreams, 1);
                Scoped phase(p.pre_phase, 2);
                emagls_pre_sweep(p);
            }
            p.depend(p.stream, p.hh_stream);   // (the epilogue reads the rows of every bin)
        }
        if (d.kind == EMAGLS_KIND_FROM_ATF) from_atf_post_sweep(p);
        else if (magls_kind(d.kind)) magls_post_sweep(p);
        else emagls_post_sweep(p);
        if (!p.pre) ++p.eager_runs;
        p.executed = true;
        return;
    }
    // sets of one geometry through a plan of the 33..64-channel path: the stages that depend on the grids alone are kept from the last clean run
    // on these grids; such an execute runs eagerly (a thousand launches of 12 us each: the host stays ahead)
    if (p.geo_keep && p.wide && p.prof_level == 0 && (d.kind == EMAGLS_KIND_EMAGLS || d.kind == EMAGLS_KIND_EMAGLS2) &&
        p.geo_done_version == p.atf_side_version) {
        {
            Scoped skip(p.geo_skip, true);
            run_pipeline(p);
        }
        p.executed = true;
        return;
    }
    p.geo_run_version = p.atf_side_version;
    if (p.prof_level == 0 && p.use_graph && !forks_streams(p)) {
        // first execute runs eagerly (one-time function attributes, lazy module load), the second is captured
        if (!p.graph && p.eager_runs >= 1) p.graph.capture(p.stream, [&] { run_pipeline(p); });
        if (p.graph) {
            p.graph.launch(p.stream);
            p.executed = true;
            return;
        }
    }
    run_pipeline(p);
    ++p.eager_runs;
    p.executed = true;
}

// the stages before the sweep of a plan on its own stream (its own executes and every batch form that runs them per plan)
void plan_pre_stage(emagls_plan& p) {
    subject_reset(p, p.stream);
    if (p.has("route")) launch_zero(p.get("route"), p.bufs["route"].bytes, p.stream);
    if (p.d.kind == EMAGLS_KIND_FROM_ATF) from_atf_pre_sweep(p);
    else if (magls_kind(p.d.kind)) magls_pre_sweep(p);
    else emagls_pre_sweep(p);
}

void drop_plan_graphs(emagls_plan& p) {
    p.graph.reset();
    p.pre.reset();
    p.eager_runs = 0;
}
// Device-side status words of a design: [0] Cholesky pivot, [1] persistent sweep gave up waiting, [2] a Gram-route bin was
// worse conditioned than the kr estimate promised ([3] = the highest such bin), [4] MagLS: the SH basis is too ill-conditioned
// for the inverse form M = R^-1 R^-H of the persistent sweep (the reference's pinv would drop singular values), [5] LS / MagLS
// above 32 channels: basis too ill-conditioned for the Gram-inverse form of pinv (fatal: no SVD route at that width).
// [1], [2] and [4] are recoverable: the design is re-run without the feature.  [1] and [2] stick to the plan (a residency or
// conditioning property of the shape); [4] is a property of THIS call's grid, so the launch-per-bin sweep only serves the
// re-run and a cached plan tries the persistent form again on its next call.
// Returns true when the design has to be executed again; throws when a flag cannot be recovered from.
bool plan_recover(emagls_plan& p, const int* flag, bool apply) {
    bool redo = false;
    if (flag[2]) {
        // flag[3] = the highest Gram-route bin whose condition number exceeded the limit: the route restarts behind it (the
        // Householder route then covers more bins and, at their higher kr, more orders: plan_routes refuses beyond its tile)
        if (p.gram_from == 0 || flag[3] < p.gram_from)
            throw Error(EMAGLS_ERR_NUMERIC, "internal: Gram-route conditioning flag outside the route (stale graph)");
        if (apply && p.d.kind == EMAGLS_KIND_FROM_ATF) {
            // measured ATFs: the bins up to the offending one take the dense route (QR + Jacobi of the matched ATF matrix itself)
            p.gram_from = flag[3] + 1 < p.P ? flag[3] + 1 : 0;
            from_atf_alloc_dense(p);
            HIP_CHECK(hipStreamSynchronize(p.stream));
        } else if (apply) {
            p.gram_floor = std::max(p.gram_floor, flag[3] + 1);
            plan_routes(p);
            plan_alloc_routes(p);
            HIP_CHECK(hipStreamSynchronize(p.stream));
        }
        redo = true;
    }
    if (flag[4]) {
        if (!p.sweep_persist) throw Error(EMAGLS_ERR_NUMERIC, "internal: MagLS conditioning flag without the persistent sweep");
        if (apply) { p.sweep_persist = false; p.persist_suspended = true; if (p.synth_want) { plan_alloc_routes(p); HIP_CHECK(hipStreamSynchronize(p.stream)); } }
        redo = true;
    }
    if (flag[1]) {
        // not every workgroup of the persistent sweep became resident (CUs held by another process, partitioned device):
        // the launch-per-bin sweep needs no co-residency
        if (!p.sweep_persist) throw Error(EMAGLS_ERR_HIP, "phase sweep: a workgroup timed out waiting for its peers' partial sums");
        if (apply) { p.sweep_persist = false; if (p.synth_want) { plan_alloc_routes(p); HIP_CHECK(hipStreamSynchronize(p.stream)); } }
        redo = true;
    }
    return redo;
}
void throw_fatal_flags(const int* flag) {
    if (flag[1]) throw Error(EMAGLS_ERR_HIP, "phase sweep: a workgroup timed out waiting for its peers' partial sums");
    if (flag[2]) throw Error(EMAGLS_ERR_NUMERIC, "per-bin factorisation: ill-conditioned bin on the Gram route after the re-run");
    if (flag[5])
        throw Error(EMAGLS_ERR_UNSUPPORTED, "the SH basis of this order is too ill-conditioned on the HRIR grid for the 33..64-channel path "
                                            "(cond > 1e4: pinv would need the SVD route, which stops at 32 channels in this build)");
    if (flag[0])
        throw Error(EMAGLS_ERR_NUMERIC,
                    "SH Gram matrix of the HRIR grid is not positive definite (the grid cannot resolve the required SH order)");
}
}  // namespace emagls
