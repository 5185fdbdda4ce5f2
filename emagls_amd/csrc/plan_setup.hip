// Plan set-up: derive the constants of a design (nfft, k_cut, simulation order: lib/getEMagLsFilters.m:44-48,
// dependencies/getSMAIRMatrix.m:95), decide the routes of its per-bin factorisation and allocate every device buffer once.
#include "host_internal.hpp"

namespace {
// compute units of the current device (cached per device id)
int device_cu_count() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    int n = 0;
    HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    cache[dev] = n;
    return n;
}

// (power-of-two FFT lengths run on the LDS FFTs of fft.hip, any other even length on its direct-DFT kernels)
void check_nfft(int nfft) {
    if (nfft < 8) throw Error(EMAGLS_ERR_UNSUPPORTED, "filter length below 4 is not supported");
}

// ---------------------------------------------------------------------------------------------
// plan construction: derive constants, allocate every device buffer once
// ---------------------------------------------------------------------------------------------

// Smallest order n such that every order above it contributes less than 1e-20 of the strongest mode to pwGrid at kr = x:
// |b_n(x)| (2n+1) / |b_0| <= x^n / (2n-1)!! (2n+1) for the rigid sphere (|j_n(x)| <= x^n / (2n+1)!!; the Wronskian form of b_n
// divides by x^2 |h_n'(x)| >= (n+1) (2n-1)!! / x^n).  Dropping those orders perturbs the bin's matrix by 1/200 of its own
// FP64 rounding error: the reference's LAPACK SVD cannot tell the difference.
constexpr double ORDER_NOISE = 1e-18;
int orders_above_noise(double x, int nmax) {
    double term = 1.0;   // x^n / (2n-1)!!
    for (int n = 1; n <= nmax; ++n) {
        term *= x / (double)(2 * n - 1);
        if ((double)n > x && term * (2 * n + 1) < ORDER_NOISE) return n - 1;
    }
    return nmax;
}
static bool plan_persist_possible(const emagls_plan& p) {
    const int64_t Dh = (p.d.kind == EMAGLS_KIND_FROM_ATF) ? p.Dm : p.D;
    return sw_on<Sw::SWEEP_PERSIST>() && !p.wide && persist_sweep_fits((int)Dh, p.C, 1);
}
// Is the synthesising sweep in effect?  Needs the persistent form (all workgroups resident) and every swept bin on the Gram
// route (the ill-conditioned swept bins of tiny arrays read Y_reg_inv_k from memory: they keep the materialised operands).
void plan_update_synth(emagls_plan& p) {
    const int k0 = std::max(p.kcut0, 1);
    p.synth = p.synth_want && !p.synth_block && p.sweep_persist && p.hh_end <= k0 && p.gram_from > 0 && k0 < p.P &&
              synth_sweep_fits((int)p.D, (int)p.d.nmics, p.simOrder + 1, 1);
}
// first bin of the Gram route (GRAM_COND_EST and what it stands for: host_internal.hpp)
static_assert(GRAM_COND_EST == 3.0e3, "the default of EMAGLS_GRAM_COND_EST in switches.hpp");
int emagls_gram_from(const emagls_plan& p) {
    if (!p.gram_route || p.d.mic_radius <= 0.0 || !sw_on<Sw::GRAM_ROUTE>()) return 0;
    int n = 0;
    if (p.d.kind == EMAGLS_KIND_EMA_CH) n = p.d.order;   // 2N+1 circular harmonics reach order N
    else while ((n + 1) * (n + 1) < p.C) ++n;
    if (n < 1) return 0;
    double dfact = 1.0;
    for (int i = 3; i <= 2 * n + 1; i += 2) dfact *= i;
    const double est_limit = sw_real<Sw::GRAM_COND_EST>();   // (tests force the re-run path with a huge limit)
    const double kr_min = std::pow(dfact / est_limit, 1.0 / n);
    const double df = p.d.fs / p.nfft;
    const int kb = (int)std::ceil(kr_min * C_SOUND / (2.0 * kPi * p.d.mic_radius) / df);
    // (least-squares bins above the estimate take the route as well: W(k,:) = (H conj(G_k)) conj(M_k), gramroute.hip)
    const int from = std::max(kb, 1);
    return from < p.P ? from : 0;
}
}  // namespace

namespace emagls {
// routes of the per-bin factorisation (see emagls_plan): derived from kr only, so that every rank / replay takes the same
void plan_routes(emagls_plan& p) {
    const emagls_design_desc& d = p.d;
    const int k0 = std::max(p.kcut0, 1);
    p.gram_from = emagls_gram_from(p);
    // EMAinSH has no radial terms in its model: pwGrid_k is well conditioned at every bin (emash.hip) and all bins take the Gram route
    if (d.kind == EMAGLS_KIND_EMA_SH) p.gram_from = 1;
    else if (p.gram_from > 0 && p.gram_from < p.gram_floor) p.gram_from = p.gram_floor < p.P ? p.gram_floor : 0;
    p.hh_end = p.gram_from > 0 ? p.gram_from : p.P;
    const double f_h = (double)(p.hh_end - 1) * (d.fs / 2.0) / (double)(p.P - 1);
    int n_min = 0;   // the S-space factor needs at least as many rows as channels
    while ((n_min + 1) * (n_min + 1) < p.C) ++n_min;
    p.n_h = std::min(p.simOrder, std::max({orders_above_noise(2.0 * kPi * f_h / C_SOUND * d.mic_radius, p.simOrder), n_min, p.nh_floor}));
    p.S_h = (p.n_h + 1) * (p.n_h + 1);
    p.ldS_h = round_up(p.S_h, 64);
    if (p.S_h > 768)
        throw Error(EMAGLS_ERR_UNSUPPORTED, "the ill-conditioned low bins of this design need more than 27 orders on the orthonormal route "
                                            "(Gram route off or moved up by a conditioning check): not supported in this build");
    if (d.kind == EMAGLS_KIND_EMA_SH) { p.hh_end = 1; p.n_h = n_min; p.S_h = (n_min + 1) * (n_min + 1); p.ldS_h = round_up(p.S_h, 64); }
    // the orthonormal route factors the first S_h columns of the grid's SH matrix (Cholesky of their Gram block): they must be
    // independent.  The columns beyond S_h only enter through products (Gram matrix, order terms), so D < S is no obstacle.
    if (p.D < p.S_h)
        throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer HRIR directions than the SH channels of the orthonormal route (the low bins need "
                                            "(n_h + 1)^2 independent columns of the grid's SH matrix)");
    p.g0 = (p.gram_from > 0 && p.gram_from < k0) ? p.gram_from : k0;
    if (p.diffuse) p.g0 = 1;   // the constraint renders the HRTFs of every solved bin: G_k from the first one
    p.nb_gram = p.gram_from > 0 ? p.P - p.gram_from : 0;
}
// Row order of the microphones in the synthesising sweep: smap[0..M) = microphone of row r, smap[32] = antipodal pairs (rows 2u,
// 2u + 1), smap[33] = single microphones after them.  Two microphones are a pair when their unit vectors cancel to a few ulps:
// cos(d, j') = -cos(d, j) then holds to the rounding error of either cosine, and one polynomial evaluation serves both.
// EMAGLS_SYNTH_PAIRS=0: no pairing.
void synth_pairing(const double* azi, const double* zen, int M, int* smap) {
    std::vector<double> u((size_t)3 * M);
    for (int j = 0; j < M; ++j) {
        u[3 * j] = std::sin(zen[j]) * std::cos(azi[j]); u[3 * j + 1] = std::sin(zen[j]) * std::sin(azi[j]); u[3 * j + 2] = std::cos(zen[j]);
    }
    std::vector<int> partner((size_t)M, -1);
    const double tol = 8.0 * 2.220446049250313e-16;
    if (sw_on<Sw::SYNTH_PAIRS>() && M <= 32)
        for (int j = 0; j < M; ++j) {
            if (partner[j] >= 0) continue;
            for (int k = j + 1; k < M; ++k) {
                if (partner[k] >= 0) continue;
                if (std::fabs(u[3 * j] + u[3 * k]) <= tol && std::fabs(u[3 * j + 1] + u[3 * k + 1]) <= tol && std::fabs(u[3 * j + 2] + u[3 * k + 2]) <= tol) {
                    partner[j] = k; partner[k] = j;
                    break;
                }
            }
        }
    for (int i = 0; i < 34; ++i) smap[i] = 0;
    int row = 0, npr = 0, nsg = 0;
    for (int j = 0; j < M && j < 32; ++j) if (partner[j] > j) { smap[row++] = j; smap[row++] = partner[j]; ++npr; }
    for (int j = 0; j < M && j < 32; ++j) if (partner[j] < 0) { smap[row++] = j; ++nsg; }
    smap[32] = npr; smap[33] = nsg;
}
// buffers whose size depends on the routes (re-entered when a conditioning check moves the routes: alloc keeps what is large enough)
void plan_alloc_routes(emagls_plan& p) {
    const bool cb = p.cplx_basis;
    const int k0 = std::max(p.kcut0, 1);
    const int ls_end = std::max(std::min(p.kcut0, p.P), 1);
    const int nOrd = p.simOrder + 1;
    p.alloc("R", esz(cb) * (size_t)p.S_h * p.S_h);                     // Cholesky factor of the leading block of Gy
    p.alloc("Rinv", esz(cb) * (size_t)ceil_div(p.S_h, 32) * 32 * 32);
    if (!cb) {   // complex copies of R and of its diagonal-block inverses (row solves of complex rows in the real basis)
        p.alloc("Rc", sizeof(cplx) * (size_t)p.S_h * p.S_h);
        p.alloc("Rinvc", sizeof(cplx) * (size_t)ceil_div(p.S_h, 32) * 32 * 32);
    }
    p.alloc("Tn", esz(cb) * (size_t)(p.n_h + 1) * p.C * p.ldS_h);
    p.alloc("Hq", sizeof(cplx) * (size_t)2 * ls_end * p.ldS_h);
    p.alloc("Hyp", sizeof(double) * hy_mfma_workspace_doubles(ls_end, p.S_h, cb));
    p.alloc("HcT", sizeof(double) * (size_t)hy_mfma_kpad((int)p.D) * round_up(4 * ls_end, 64));   // (rows >= D stay zero)
    p.alloc("Z", sizeof(cplx) * (size_t)p.hh_end * p.C * p.ldS_h);
    p.alloc("Vws", sizeof(cplx) * (size_t)p.hh_end * p.C * p.ldS_h);
    plan_update_synth(p);
    // (the synthesising sweep and its least-squares bins evaluate their operands themselves: no G_k in memory)
    const int g_end = p.synth ? p.g0 : p.P;
    p.alloc("G", sizeof(cplx) * ((size_t)std::max(g_end - p.g0, 1) * p.C + 32) * p.ldD, false);  // + 32 rows: the persistent sweep loads all 32 slab rows of a bin unconditionally
    if (p.synth_want) {
        const int M = (int)p.d.nmics;
        p.alloc("bsc", sizeof(cplx) * (size_t)p.P * synth_nord_pad(nOrd));
        p.alloc("Pm", sizeof(double) * 32 * 32);
        if (!p.has("smap")) {   // (identity order until the microphone grid arrives)
            int smap[34] = {0};
            for (int j = 0; j < 32; ++j) smap[j] = j < M ? j : 0;
            smap[33] = M;
            p.alloc("smap", sizeof smap);
            p.upload("smap", smap, sizeof smap);
            p.synth_units = M;
            HIP_CHECK(hipStreamSynchronize(p.stream));
        }
        p.alloc("Mt", sizeof(cplx) * ((size_t)p.P * M * M + 1024));
        p.alloc("Winit", sizeof(cplx) * 64);
        p.alloc("Usw", sizeof(cplx) * (size_t)synth_ls_chunks((int)p.D) * 2 * p.P * 32);   // [chunk][e][bin][32]: the chain's totals use chunk 0
    }
    p.alloc("Yri", sizeof(cplx) * (size_t)std::max(p.hh_end - k0, 1) * p.C * p.ldD, false);    // only Householder-route bins can be flagged ill-conditioned
    if (p.nb_gram > 0) {
        const int ldK = round_up(p.C * p.C, 64), Kp = round_up(nOrd * nOrd, 4);
        p.alloc("Fg", esz(cb) * (size_t)nOrd * p.C * p.ldS);
        p.alloc("Kmat", sizeof(double) * (size_t)Kp * ldK);                                   // (rows beyond nOrd^2 stay zero)
        p.alloc("Cf", sizeof(double) * (size_t)Kp * round_up(p.P, 64));                       // (sized for every bin: the routes may move)
        p.alloc("Apk", sizeof(double) * (size_t)p.P * ldK);
    }
}

thread_local hipStream_t g_plan_stream_shared = nullptr;   // set by the job scheduler around the creation of a chunk's plans
void plan_setup(emagls_plan& p) {
    const emagls_design_desc& d = p.d;
    if (d.kind < EMAGLS_KIND_LS || d.kind > EMAGLS_KIND_EMA_SH) throw Error(EMAGLS_ERR_ARG, "unknown design kind");
    if (d.basis != EMAGLS_BASIS_REAL && d.basis != EMAGLS_BASIS_COMPLEX) throw Error(EMAGLS_ERR_ARG, "shDefinition must be 'real' or 'complex'");
    if (d.ndirs < 1 || d.nsamp < 1) throw Error(EMAGLS_ERR_ARG, "empty HRIR set");
    if (d.kind != EMAGLS_KIND_FROM_ATF && d.order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
    HIP_CHECK(hipGetDevice(&p.device));
    const auto t_setup0 = std::chrono::steady_clock::now();
    // (the plans of a job chunk share the slot's stream -- hipStreamCreate was 3 ms of a plan's set-up, four streams each --; the side
    // streams of a multi-stream execute are taken when one first asks for them)
    if (g_plan_stream_shared) { p.stream = g_plan_stream_shared; p.owns_stream = false; }
    else p.stream = StreamPool::get().take();
    p.use_graph = !sw_on<Sw::NO_GRAPH>();
    const auto t_setup1 = std::chrono::steady_clock::now();
    if (const int ns = sw_int<Sw::STREAMS>()) p.nstreams = ns;
    p.req_cplx = d.basis == EMAGLS_BASIS_COMPLEX;
    // Complex-basis eMagLS / eMagLS2 designs run in real arithmetic.  With Y_c = Y_r T (T unitary, block diagonal per order)
    // smair_c = T_N^H smair_r T and pwGrid_c = T_N^H pwGrid_r, hence Y_reg_inv_c = Y_reg_inv_r T_N, the angles
    // W(k-1,:) pwGrid are the same and W_c(k,:) = W_r(k,:) T_N for every solved bin (lib/getEMagLsFilters.m:87-103); the DC
    // rule and the SH conjugate rule (:109-118) act on W_c and stay in the epilogue.  eMagLS2 is basis free (T cancels).
    // The real pipeline has a 3x cheaper Gram and half the bytes in T_n and QT: 1460 vs 1295 sets/s at config 3.
    p.custom_basis = d.custom_basis != 0;
    p.diffuse = d.diffuseness != 0;
    if (p.diffuse && (d.kind == EMAGLS_KIND_LS || d.kind == EMAGLS_KIND_FROM_ATF))
        throw Error(EMAGLS_ERR_ARG, "the diffuseness constraint applies to MagLS, eMagLS, eMagLS2 and the EMA variant");
    if (p.custom_basis && (d.kind == EMAGLS_KIND_FROM_ATF || d.kind == EMAGLS_KIND_EMA_CH || d.kind == EMAGLS_KIND_MAGLS_2D))
        throw Error(EMAGLS_ERR_UNSUPPORTED, "caller-supplied SH matrices are available for LS, MagLS, eMagLS and eMagLS2 designs");
    // (a caller-supplied complex basis need not be ours rotated by T: it takes the complex-arithmetic pipeline)
    p.real_internal = p.req_cplx && !p.custom_basis && (d.kind == EMAGLS_KIND_EMAGLS || d.kind == EMAGLS_KIND_EMAGLS2);
    if (!sw_on<Sw::REAL_INTERNAL>()) p.real_internal = false;
    p.cplx_basis = p.req_cplx && !p.real_internal;
    p.D = d.ndirs;
    p.ldD = round_up(p.D, 64);
    const bool cb = p.cplx_basis;

    p.alloc("hL", sizeof(double) * d.nsamp * d.ndirs, false);
    p.alloc("hR", sizeof(double) * d.nsamp * d.ndirs, false);
    p.alloc("hrir_azi", sizeof(double) * p.D, false);
    p.alloc("hrir_zen", sizeof(double) * p.D, false);
    p.alloc("flag", sizeof(int) * NFLAG);

    if (d.kind == EMAGLS_KIND_LS) p.alloc("grpd", sizeof(double) * 2);
    if (d.kind != EMAGLS_KIND_LS) {
        if (d.len < d.nsamp)
            throw Error(EMAGLS_ERR_ARG, magls_kind(d.kind) ? "HRIR len too short" : "len too short");
        if (!(d.fs > 0)) throw Error(EMAGLS_ERR_ARG, "fs must be positive");
        p.nfft = (int)std::min<int64_t>(NFFT_MAX_LEN, 2 * d.len);
        check_nfft(p.nfft);
        if (d.len % 2) throw Error(EMAGLS_ERR_ARG, "filter length must be even");
        // nfft is capped at NFFT_MAX_LEN: a longer filter makes the reference index wMlsL(n_shift-len/2+1 : n_shift+len/2) with a
        // non-positive start (lib/getEMagLsFilters.m:135-136) and fail; the kernels would read outside their LDS buffers.
        if (d.len > p.nfft)
            throw Error(EMAGLS_ERR_ARG, "len exceeds the oversampled FFT length min(2048, 2*len): the reference fails with an index error");
        p.P = p.nfft / 2 + 1;
        const double f2 = (d.fs / 2.0) / (double)(p.P - 1);  // f(2) of linspace(0, fs/2, P)
        const double f_cut = (d.kind == EMAGLS_KIND_FROM_ATF) ? d.f_trans : std::max(F_CUT_MIN_FREQ, 500.0 * d.order);
        p.k_cut = (int)std::ceil(f_cut / f2);
        if (p.k_cut < 1) p.k_cut = 1;
        p.kcut0 = std::min(p.k_cut - 1, p.P);  // 0-based index of the first magnitude-least-squares bin
        if (magls_kind(d.kind) && p.kcut0 < 1) throw Error(EMAGLS_ERR_ARG, "k_cut must be at least 2");
        p.alloc("tw", sizeof(cplx) * p.nfft);
        p.alloc("grpd", sizeof(double) * (2 + 4 * (size_t)p.P));   // the two delays, then the delay phases [2][P] (grpdelay_median_kernel)
        if (p.diffuse) p.alloc("Hfull", sizeof(cplx) * (size_t)2 * p.P * p.ldD);   // time-aligned complex HRTFs of every bin
        p.alloc("dirsum", sizeof(double) * 2 * d.nsamp * hrir_dirsum_chunks(d.ndirs));
    }

    const int N = d.order;
    if (d.kind == EMAGLS_KIND_LS || magls_kind(d.kind)) {
        p.simOrder = N;
        // getMagLsFilters2D.m:49: Y_conj = getCH(order, azi)' has 2*order+1 rows (the numHarmonics of :47 is never used)
        p.S = d.kind == EMAGLS_KIND_MAGLS_2D ? 2 * N + 1 : (N + 1) * (N + 1);
        p.C = p.S;
        p.nOut = p.S;
        // up to 32 channels: the tuned kernels (register tiles, the persistent sweep); 33..256 (SH orders 5..15, CH orders 16..127): the
        // plain path of wide.hip -- pinv(Y_conj) from the inverse of the Gram matrix, one sweep launch per bin (above 64 channels its
        // loop forms)
        p.wide = p.S > 32;
        if (p.S > 256) throw Error(EMAGLS_ERR_UNSUPPORTED, d.kind == EMAGLS_KIND_MAGLS_2D ? "CH order above 127 is not supported in this build"
                                                                                            : "SH order above 15 is not supported for LS/MagLS in this build");
        if (p.S > 64 && p.diffuse) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 channels: no covariance constraint in this build");
        if (p.D < p.S) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer HRIR directions than SH channels");
    } else if (array_kind(d.kind)) {
        if (!(d.mic_radius > 0) || d.nmics < 1) throw Error(EMAGLS_ERR_ARG, "invalid array geometry");
        // getSMAIRMatrix.m:95: max(params.order, ceil(fs*pi*r/C)).  lib/getEMagLs2Filters.m:51-63 leaves params.order unset, so
        // getSMAIRMatrix.m:39-41 defaults it to 4 there: for eMagLS2 `order` only sets f_cut (:47), never the simulation order.
        const int smair_order = d.kind == EMAGLS_KIND_EMAGLS2 ? SMAIR_DEFAULT_ORDER : N;
        p.simOrderOwn = smair_sim_order(smair_order, d.fs, d.mic_radius);
        // sim_order_pad: simulate on more orders than the design's own, with b_n = 0 above its own order -- the same sum, so
        // the same filters; array radii of neighbouring simulation-order classes then have one shape and share a lane batch
        if (d.sim_order_pad < 0) throw Error(EMAGLS_ERR_ARG, "negative sim_order_pad");
        if (d.sim_order_pad > 0 && (p.custom_basis || d.kind == EMAGLS_KIND_EMA_SH))
            throw Error(EMAGLS_ERR_UNSUPPORTED, "sim_order_pad is available for eMagLS / eMagLS2 / EMAinCH designs on the built-in SH basis");
        p.simOrder = std::max(p.simOrderOwn, d.sim_order_pad);
        p.S = (p.simOrder + 1) * (p.simOrder + 1);
        p.nOut = d.kind == EMAGLS_KIND_EMA_CH ? 2 * N + 1 : (N + 1) * (N + 1);   // EMAinCH.m:66: numHarmonics = 2*order+1
        if (d.kind == EMAGLS_KIND_EMA_SH && d.nmics < 2 * N + 1)
            throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer microphones than circular harmonics (2*order+1)");
        p.C = d.kind == EMAGLS_KIND_EMAGLS2 ? (int)d.nmics : p.nOut;
        // up to 32 channels / microphones: the tuned per-bin kernels.  33..64 (a 64-capsule array; SH orders 5..7 in the SH domain):
        // the plain S-space path of wide_array.hip -- real-arithmetic pipeline, one design at a time (any simulation order the
        // narrow path takes: 64 microphones at 7 / 8 / 10 cm agree with the oracle to 1e-10, tools/experiments/wide_radius.py)
        if (p.C > 32) {
            if (p.C > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 output channels is not supported in this build");
            if (d.kind != EMAGLS_KIND_EMAGLS && d.kind != EMAGLS_KIND_EMAGLS2 && d.kind != EMAGLS_KIND_EMA_SH)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 32 output channels: eMagLS / eMagLS2 / EMAinSH only");
            if (p.custom_basis || d.sim_order_pad > 0)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 32 output channels: built-in SH basis, no padding");
            // (EMAinSH orders 5..7 factor the direction-space operands themselves -- execute_ema_sh_wide -- in either basis)
            if (d.kind != EMAGLS_KIND_EMA_SH && p.req_cplx && !p.real_internal)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 32 output channels: the real-arithmetic pipeline only");
            if (d.kind == EMAGLS_KIND_EMA_SH && p.diffuse) throw Error(EMAGLS_ERR_UNSUPPORTED, "EMAinSH above order 4: no covariance constraint in this build");
            p.wide = true;
        }
        if (p.simOrder > 85) throw Error(EMAGLS_ERR_UNSUPPORTED, "simulation order above 85 (array radius > ~19.3 cm at 48 kHz) is not supported: the reference's own getSH overflows there (factorials beyond 170!)");
        // (fewer directions than simulated SH channels are fine as long as the orders of the orthonormal route are covered:
        // plan_routes checks D >= S_h.  The wide path orthogonalises all S columns.)
        if (p.D < p.S && (p.wide || d.kind == EMAGLS_KIND_EMA_SH)) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer HRIR directions than simulated SH channels");
        // (rank-deficient array model on the 33..64-channel path, e.g. 49 microphones on a 2 cm sphere at 16 kHz -- 25 simulated SH channels: the
        // reference's clipped inverse is then 100 / s_max times singular vectors of rounding noise; launch_wa_factor)
        if (p.wide && d.kind != EMAGLS_KIND_EMA_SH && p.S < p.C)
            throw Error(EMAGLS_ERR_UNSUPPORTED, "33..64 channels with fewer simulated SH channels than channels (rank-deficient array model: the reference's clipped inverse is rounding noise there) is not supported");
        if (p.D < p.C) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer HRIR directions than channels");
        if (d.kind != EMAGLS_KIND_EMAGLS2 && d.kind != EMAGLS_KIND_EMA_SH && d.nmics < p.nOut)
            throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer microphones than output channels");
    } else {
        if (d.nmics < 1 || d.natf < 1 || d.atf_taps < 1) throw Error(EMAGLS_ERR_ARG, "invalid ATF set");
        p.C = (int)d.nmics;
        // up to 32 microphones on the Gram route (the M x M factors of the persistent sweep's form); the dense route behind its
        // conditioning flag -- QR + Jacobi of the Dm x M matrix itself -- in factor.hip's register tiles up to 8 columns at this row
        // count, in wide_array.hip's tall forms from 9 on, and in its tiled form (row blocks + a tree step) at every width above 4096
        // matched directions (from_atf_shared_stage)
        // (33..64 microphones: the plain per-bin path of wide_array.hip on the matched ATF matrices themselves, one subject at a time)
        if (p.C > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 ATF microphones is not supported in this build");
        p.wide = p.C > 32;
        p.hrir_smaller = d.ndirs <= d.natf;  // min([a b]) returns the first index on ties (FromAtf.m:62)
        p.Dm = p.hrir_smaller ? d.ndirs : d.natf;
        // (up to 3072 matched directions: resident sweep; above: the Gram route with one launch per bin, sweep_half_kernel walking
        // several slabs per workgroup; the dense route -- QR of the Dm x M matrix itself -- in one workgroup per bin up to 4096 rows and
        // in row blocks above)
        if (p.Dm > 65536) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 65536 matched directions is not supported in this build");
        if (p.Dm < p.C) throw Error(EMAGLS_ERR_UNSUPPORTED, "fewer directions than microphones");
    }
    p.ldS = round_up(std::max(p.S, 1), 64);

    if (d.kind != EMAGLS_KIND_FROM_ATF) {
        // ---- SH machinery on the HRIR grid
        p.Dpad = std::max<int64_t>(gram_dpad(p.D, p.S), hy_mfma_kpad((int)p.D));   // (rows D..Dpad of Yc are zero)
        p.alloc("sh_tab", sizeof(double) * sh_coeff_count(p.simOrder));
        p.alloc("Ycm", esz(cb) * (size_t)p.S * p.ldD);                 // [S][ldD] column-major SH matrix
        p.alloc("Yc", esz(cb) * (size_t)p.Dpad * p.ldS);               // [Dpad][ldS] conj(Y), direction-major
        p.alloc("Gp", esz(cb) * (size_t)gram_ksplit(p.D, p.S) * p.S * p.S);
        if (!array_kind(d.kind)) {   // (array designs: R covers the Householder-route orders only, plan_alloc_routes; Q is never formed)
            p.alloc("R", esz(cb) * (size_t)p.S * p.S);
            p.alloc("Q", esz(cb) * (size_t)p.D * p.ldS);
            p.alloc("Rinv", esz(cb) * (size_t)ceil_div(p.S, 32) * 32 * 32);
        }
    }
    if (d.kind == EMAGLS_KIND_LS || magls_kind(d.kind)) {
        p.alloc("Rb", sizeof(cplx) * (size_t)p.C * p.ldS);             // R as [c][s] complex
        p.alloc("Zb", sizeof(cplx) * (size_t)p.C * p.ldS);
        p.alloc("Vws", sizeof(cplx) * (size_t)p.C * p.ldS);
        p.alloc("sv", sizeof(double) * p.C);
        p.alloc("tauw", sizeof(double) * p.C);
        p.alloc("R2w", sizeof(cplx) * (size_t)p.C * p.C);
        p.alloc("Nw", sizeof(cplx) * (size_t)p.C * p.C);
        p.alloc("Ypinv", esz(cb) * (size_t)p.C * p.ldD);
        if (p.wide) p.alloc("Mg", sizeof(cplx) * (size_t)p.S * p.S);   // (Y^T conj(Y))^-1
        if (p.S > 64) p.alloc("Mgw", sizeof(cplx) * (size_t)p.S * p.S + 2 * sizeof(double));   // R^-1 and the certificate's norms (wide.hip: 65..256 channels)
        if (d.kind == EMAGLS_KIND_LS) {
            p.out_rows = d.nsamp;
        } else {
            p.alloc("Xc", esz(cb) * (size_t)p.S * p.ldD);              // Y_conj as [c][d]
        }
    }
    if (array_kind(d.kind)) {
        const int M = (int)d.nmics;
        const int ldM = round_up(M, 64);
        p.alloc("mic_azi", sizeof(double) * M, false);
        p.alloc("mic_zen", sizeof(double) * M, false);
        p.alloc("Ymic_cm", esz(cb) * (size_t)p.S * M);                 // [S][M]
        p.alloc("Ymic_rm", esz(cb) * (size_t)ldM * p.ldS);             // [M][ldS]
        p.alloc("E", esz(cb) * (size_t)p.C * p.ldS);                   // [C][ldS]
        if (d.kind == EMAGLS_KIND_EMA_SH || (d.kind != EMAGLS_KIND_EMAGLS2 && p.nOut <= 32)) {   // (EMAinSH: pinv of the 2N+1 circular harmonics, any order)
            p.alloc("Ylo_c", sizeof(cplx) * (size_t)p.nOut * ldM);     // [nOut][ldM] complex copy of Y_Lo^T
            p.alloc("Zlo", sizeof(cplx) * (size_t)p.nOut * ldM);
            p.alloc("Vlo", sizeof(cplx) * (size_t)p.nOut * ldM);
            p.alloc("tau_lo", sizeof(double) * p.nOut);
            p.alloc("R2_lo", sizeof(cplx) * (size_t)p.nOut * p.nOut);
            p.alloc("N_lo", sizeof(cplx) * (size_t)p.nOut * p.nOut);
        }
        if (d.kind == EMAGLS_KIND_EMA_SH) {
            const int npts = ema_sh_npts(p.C), ldP = round_up(npts, 64);   // (C <= 64: orders up to 7, checked above)
            const int64_t ldA = round_up((int64_t)(p.D + 1) * npts, 64);
            p.alloc("Ech", esz(cb) * (size_t)(2 * N + 1) * p.ldS);          // pinv(CH(micAzi)) Y_mic
            p.alloc("sh_tab_lo", sizeof(double) * sh_coeff_count(N));      // recurrence table of the output order (its layout depends on the order)
            p.alloc("hrir_zen_eq", sizeof(double) * p.D, false);           // pi/2: the horizontal projection of the HRIR grid
            p.alloc("nnm_azi", sizeof(double) * p.C, false);
            p.alloc("nnm_zen", sizeof(double) * p.C, false);
            p.alloc("Ypts", esz(cb) * (size_t)p.C * p.C);
            p.alloc("rot_azi", sizeof(double) * (size_t)ldA, false);
            p.alloc("rot_zen", sizeof(double) * (size_t)ldA, false);
            p.alloc("Arot", esz(cb) * (size_t)p.C * ldA, false);           // SHs of order N at all rotated points (and the fixed set)
            p.alloc("Bc", sizeof(cplx) * (size_t)p.C * ldP);
            p.alloc("Zb", sizeof(cplx) * (size_t)p.C * ldP);
            p.alloc("Vb", sizeof(cplx) * (size_t)p.C * ldP);
            p.alloc("tau_b", sizeof(double) * p.C);
            p.alloc("R2_b", sizeof(cplx) * (size_t)p.C * p.C);
            p.alloc("N_b", sizeof(cplx) * (size_t)p.C * p.C);
            p.alloc("Rot", esz(cb) * (size_t)p.D * p.C * p.C, false);
            const std::vector<double> eq((size_t)p.D, kPi / 2.0), na = ema_sh_channel_azimuths(p.C, cb), nz((size_t)p.C, kPi / 2.0);
            p.upload("hrir_zen_eq", eq.data(), sizeof(double) * p.D);
            p.upload("nnm_azi", na.data(), sizeof(double) * p.C);
            p.upload("nnm_zen", nz.data(), sizeof(double) * p.C);
            HIP_CHECK(hipStreamSynchronize(p.stream));   // (the host vectors go out of scope)
        }
        p.alloc("kr", sizeof(double) * p.P, false);
        p.alloc("nvalid", sizeof(int) * 4);
        p.upload("nvalid", &p.simOrderOwn, sizeof(int));
        p.alloc("bn", sizeof(cplx) * (size_t)p.P * (p.simOrder + 1));
        if (p.wide && d.kind == EMAGLS_KIND_EMA_SH) {
            // EMAinSH orders 5..7 (36..64 channels): G_k of every bin materialised, factored in place of a common S-space
            // (wide_array.hip on the D x C operand itself, like FromAtf above 32 microphones), one sweep launch per bin
            const size_t nb = (size_t)p.P - 1, nOrdW = (size_t)p.simOrder + 1;
            p.alloc("QT", esz(cb) * nOrdW * p.C * p.ldD);
            p.alloc("G", sizeof(cplx) * (nb * p.C + 32) * p.ldD, false);
            p.alloc("Yri", sizeof(cplx) * (nb * p.C + 32) * p.ldD, false);
            p.alloc("Bw", sizeof(cplx) * nb * p.C * p.ldD, false);
            p.alloc("Vw", sizeof(cplx) * nb * p.C * p.ldD, false);
            p.alloc("tauw", sizeof(double) * nb * p.C);
            p.alloc("R2w", sizeof(cplx) * nb * p.C * p.C);
            p.alloc("Nw", sizeof(cplx) * nb * p.C * p.C);
            p.alloc("sv", sizeof(double) * (size_t)p.P * p.C);
            p.alloc("jsweeps", sizeof(int) * (size_t)p.P);
            p.g0 = 1;
        } else if (p.wide) {   // wide_array.hip: every bin on the S-space route in global memory, Y_reg_inv of every bin materialised
            const size_t nb = (size_t)p.P - 1, nOrdW = (size_t)p.simOrder + 1;
            p.alloc("R", sizeof(double) * (size_t)p.S * p.S);
            p.alloc("Rinv", sizeof(double) * (size_t)ceil_div(p.S, 32) * 32 * 32);
            p.alloc("Q", sizeof(double) * (size_t)p.D * p.ldS);
            p.alloc("Tn", sizeof(double) * nOrdW * p.C * p.ldS);
            p.alloc("QT", sizeof(double) * nOrdW * p.C * p.ldD);
            p.alloc("G", sizeof(cplx) * (nb * p.C + 32) * p.ldD, false);
            p.alloc("Yri", sizeof(cplx) * (nb * p.C + 32) * p.ldD, false);
            p.alloc("Bw", sizeof(cplx) * nb * p.C * p.ldS, false);
            p.alloc("Vw", sizeof(cplx) * nb * p.C * p.ldS, false);
            p.alloc("Zw", sizeof(cplx) * nb * p.C * p.ldS, false);
            p.alloc("tauw", sizeof(double) * nb * p.C);
            p.alloc("R2w", sizeof(cplx) * nb * p.C * p.C);
            p.alloc("Nw", sizeof(cplx) * nb * p.C * p.C);
            p.alloc("sv", sizeof(double) * (size_t)p.P * p.C);
            p.alloc("jsweeps", sizeof(int) * (size_t)p.P);
            if (d.kind == EMAGLS_KIND_EMAGLS && p.nOut > 32) {
                p.alloc("Ag", sizeof(double) * (size_t)p.nOut * p.nOut);
                p.alloc("Minv", sizeof(cplx) * (size_t)p.nOut * p.nOut);
            }
        } else {
        p.alloc("route", sizeof(int) * (size_t)p.P);
        p.alloc("Gy", esz(cb) * (size_t)p.S * p.S);                    // Gram matrix of conj(Y) (upper block triangle)
        p.sweep_persist = plan_persist_possible(p);
        p.synth_want = sw_on<Sw::SWEEP_SYNTH>() && !cb && !p.custom_basis && !p.diffuse && d.kind != EMAGLS_KIND_EMA_SH &&
                       synth_sweep_supported((int)p.D, (int)d.nmics, p.simOrder + 1) && persist_sweep_supported((int)p.D, (int)d.nmics);
        plan_routes(p);
        plan_alloc_routes(p);
        p.alloc("sv", sizeof(double) * (size_t)p.P * p.C);
        p.alloc("jsweeps", sizeof(int) * (size_t)p.P);
        p.alloc("tauw", sizeof(double) * (size_t)p.P * p.C);
        p.alloc("R2w", sizeof(cplx) * (size_t)p.P * p.C * p.C);
        p.alloc("Nw", sizeof(cplx) * (size_t)p.P * p.C * p.C);
        p.alloc("Mw", sizeof(cplx) * ((size_t)p.P * p.C * p.C + 1024));
        p.alloc("cond_ok", sizeof(double) * (size_t)p.P);
        p.alloc("QT", esz(cb) * (size_t)(p.simOrder + 1) * p.C * p.ldD);
        if (sw_on<Sw::SWEEP_TIMING>()) p.alloc("sweep_timing", sizeof(long long) * 16 * (size_t)p.P);
        }
    }
    if (d.kind == EMAGLS_KIND_FROM_ATF) {
        const int M = p.C;
        p.alloc("atf", sizeof(double) * (size_t)d.atf_taps * M * d.natf, false);
        p.alloc("atf_azi", sizeof(double) * d.natf, false);
        p.alloc("atf_zen", sizeof(double) * d.natf, false);
        p.alloc("cartB", sizeof(double) * 3 * std::max(d.natf, d.ndirs));
        p.alloc("match_idx", sizeof(int64_t) * p.Dm);
        p.alloc("match_dev", sizeof(double) * p.Dm);
        p.alloc("mean_dev", sizeof(double));
        p.alloc("colidx", sizeof(int64_t) * (size_t)p.Dm * M);
        p.ldD = round_up(p.Dm, 64);
        p.alloc("X", sizeof(cplx) * ((size_t)p.P * M + 32) * p.ldD);   // (+ 32 rows: the persistent sweep loads whole 32-row slabs)
        p.alloc("Z", sizeof(cplx) * ((size_t)p.P * M + 32) * p.ldD);
        // the per-bin M x M factors of the persistent sweep's form (Gram route, gramroute.hip): A_k = X_k X_k^H from the matched
        // ATF spectra themselves, M_k = V diag(s_reg / s) V^H
        p.alloc("Apk", sizeof(double) * (size_t)p.P * round_up(M * M, 64));
        p.alloc("Mw", sizeof(cplx) * ((size_t)p.P * M * M + 1024));
        p.alloc("cond_ok", sizeof(double) * (size_t)p.P);
        p.alloc("route", sizeof(int) * (size_t)p.P);
        p.gram_from = 1;   // every bin starts on the Gram route; a device-side conditioning flag moves the start up (plan_recover)
        p.alloc("Vws", sizeof(cplx) * (size_t)p.P * M * p.ldD);
        if (p.wide) p.alloc("Bw", sizeof(cplx) * (size_t)p.P * M * p.ldD);   // the matched ATF matrices again: the QR works in place
        p.alloc("sv", sizeof(double) * (size_t)p.P * M);
        p.alloc("jsweeps", sizeof(int) * (size_t)p.P);
        p.alloc("tauw", sizeof(double) * (size_t)p.P * M);
        p.alloc("R2w", sizeof(cplx) * (size_t)p.P * M * M);
        p.alloc("Nw", sizeof(cplx) * (size_t)p.P * M * M);
    }
    if (d.kind != EMAGLS_KIND_LS) {
        const int64_t Dh = (d.kind == EMAGLS_KIND_FROM_ATF) ? p.Dm : p.D;
        const int n_c = std::max(std::min(p.kcut0, p.P), 1);
        p.alloc("Hc", sizeof(cplx) * (size_t)2 * n_c * p.ldD);
        p.alloc("Habs", sizeof(double) * (size_t)2 * std::max(p.P - p.kcut0, 1) * p.ldD);
        p.alloc("W", sizeof(cplx) * (size_t)2 * p.P * p.C);
        if (magls_kind(d.kind) || d.kind == EMAGLS_KIND_FROM_ATF || p.wide) p.nWG = dense_sweep_nwg((int)Dh, p.C);
        p.nWG_dense = dense_sweep_nwg((int)Dh, p.C);
        // the persistent sweep keeps one workgroup per CU resident (142 KB of LDS each): it needs the shape to fit one XCD's
        // 32 CUs per design AND that many CUs on this device (a partitioned or CU-masked GPU takes the launch-per-bin form)
        p.sweep_persist = plan_persist_possible(p);
        if (magls_kind(d.kind) && p.sweep_persist) {
            p.alloc("Gm", sizeof(cplx) * ((size_t)p.C + 32) * p.ldD);      // Y_conj as complex [c][d] (+ 32 rows: whole-slab loads)
            p.alloc("Mw", sizeof(cplx) * ((size_t)p.P * p.C * p.C + 1024));
            p.alloc("cond_ok", sizeof(double) * (size_t)p.P);
        }
        p.alloc("ll", std::max(persist_sweep_ll_bytes((int)Dh, p.synth_want ? std::max(p.C, (int)d.nmics) : p.C),
                               p.synth_want ? reg_sweep_ll_bytes((int)Dh, (int)d.nmics) : (size_t)0));
        if (p.synth_want) p.alloc("sweep_args", sizeof(HalfSweepArgs));
        p.alloc("Wpart", sizeof(cplx) * (size_t)2 * std::max(p.nWG, p.nWG_dense) * 2 * p.C);
        p.out_rows = d.len;
    }
    p.out_cols = p.C;
    p.out_cplx = p.req_cplx && d.kind != EMAGLS_KIND_FROM_ATF;
    p.alloc("wL", (p.out_cplx ? sizeof(cplx) : sizeof(double)) * (size_t)p.out_rows * p.out_cols);
    p.alloc("wR", (p.out_cplx ? sizeof(cplx) : sizeof(double)) * (size_t)p.out_rows * p.out_cols);
    const auto t_setup2 = std::chrono::steady_clock::now();
    HIP_CHECK(hipStreamSynchronize(p.stream));
    if (sw_on<Sw::JOBS_TRACE>()) {
        const auto t_setup3 = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "emagls trace: plan setup: streams %.3f ms, %zu buffers in %zu slabs %.3f ms, final sync %.3f ms\n", ms(t_setup0, t_setup1), p.bufs.size(),
                p.slabs.size(), ms(t_setup1, t_setup2), ms(t_setup2, t_setup3));
        static std::atomic<int> shown{0};
        if (shown.fetch_add(1) % 64 == 0) {   // (every 64th plan: its largest buffers)
            std::vector<std::pair<size_t, std::string>> big;
            for (auto& kv : p.bufs) big.emplace_back(kv.second.bytes, kv.first);
            std::sort(big.rbegin(), big.rend());
            std::string line;
            for (size_t i = 0; i < big.size() && i < 12; ++i) line += " " + big[i].second + "=" + std::to_string(big[i].first >> 20);
            fprintf(stderr, "emagls trace: plan of %lld MB (sim order %d, S_h %d, hh_end %d); largest buffers (MB):%s\n", (long long)(p.total_bytes >> 20), p.simOrder, p.S_h, p.hh_end, line.c_str());
        }
    }
}
}  // namespace emagls
