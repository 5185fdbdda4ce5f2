// C ABI (include/emagls.h) for device, basis, plan, batch and one-shot calls, with the one-shot plan cache.  The entries check
// their arguments and call down into batch_run.hip, plan_run.hip and plan_setup.hip; nothing here sequences launches.
// There is no CPU fallback: without a GPU every entry point returns an error.
#include "host_internal.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// One-shot entry points (what the MEX shim binds: lib/get*Filters.m signatures, host arrays in, filters out).
// A shape-keyed cache keeps the plans of recent calls alive -- device buffers, captured graphs, the routes a
// conditioning check may have moved -- so that a repeated design costs the uploads, one replay and the download instead
// of ~1.5 GB of hipMalloc and an eager first execute.  emagls_cache_clear() (mexAtExit) releases everything.
// ---------------------------------------------------------------------------------------------
struct CachedPlan {
    std::unique_ptr<emagls_plan> plan;
    emagls_design_desc desc{};
    int device = 0;
    bool busy = false;
    uint64_t last_use = 0;
};
std::mutex g_cache_mu;
std::vector<CachedPlan> g_cache;
uint64_t g_cache_tick = 0;

int one_shot(const emagls_design_desc& desc, const double* hL, const double* hR, const double* azi, const double* zen,
             const double* mic_azi, const double* mic_zen, const double* atf, const double* atf_azi, const double* atf_zen,
             void* wL, void* wR, double* mean_dev, const void* Y_hrir = nullptr, const void* Y_mic = nullptr) {
    return guarded([&] {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        emagls_plan* p = nullptr;
        std::unique_ptr<emagls_plan> fresh;
        bool cached = false;
        {
            std::lock_guard<std::mutex> lk(g_cache_mu);
            for (auto& c : g_cache)
                if (!c.busy && c.device == dev && same_desc(c.desc, desc)) { c.busy = true; p = c.plan.get(); cached = true; break; }
        }
        if (!p) {
            fresh.reset(new emagls_plan);
            fresh->d = desc;
            plan_setup(*fresh);
            if (array_kind(desc.kind)) {
                // One stream: the independent branches of a single design could fork onto side streams (3 streams: 3.55 instead of
                // ~4 ms in a plan), but a MULTI-stream capture is what both hipGraphLaunch crashes of this round had in common
                // (StreamPool above; again with the pool in place after a lane batch of the same shape) and a cached one-shot plan
                // is captured and replayed inside whatever session the caller runs.  EMAGLS_ONESHOT_STREAMS=3 restores the forks.
                fresh->nstreams = sw_int<Sw::ONESHOT_STREAMS>();
                fresh->alone = true;   // (a one-shot call has the device to itself: the orthonormal route of the low bins runs next to the sweep)
            }
            p = fresh.get();
        }
        auto release = [&](bool ok) {
            std::lock_guard<std::mutex> lk(g_cache_mu);
            if (cached) {
                for (size_t i = 0; i < g_cache.size(); ++i)
                    if (g_cache[i].plan.get() == p) {
                        if (ok) { g_cache[i].busy = false; g_cache[i].last_use = ++g_cache_tick; }
                        else g_cache.erase(g_cache.begin() + i);   // a failed call leaves the plan in an unknown state: drop it
                        break;
                    }
            } else if (ok && sw_int<Sw::PLAN_CACHE>() > 0) {
                if (g_cache.size() >= (size_t)sw_int<Sw::PLAN_CACHE>()) {   // evict the least recently used idle plan
                    size_t victim = g_cache.size();
                    for (size_t i = 0; i < g_cache.size(); ++i)
                        if (!g_cache[i].busy && (victim == g_cache.size() || g_cache[i].last_use < g_cache[victim].last_use)) victim = i;
                    if (victim < g_cache.size()) g_cache.erase(g_cache.begin() + victim);
                }
                if (g_cache.size() < (size_t)sw_int<Sw::PLAN_CACHE>()) {
                    CachedPlan c;
                    c.plan = std::move(fresh);
                    c.desc = desc; c.device = dev; c.busy = false; c.last_use = ++g_cache_tick;
                    g_cache.push_back(std::move(c));
                }
            }
        };
        try {
            auto req = [](int rc) { if (rc != EMAGLS_OK) throw Error(rc, g_last_error); };
            if (desc.custom_basis) {
                req(emagls_plan_set_basis(p, Y_hrir, Y_mic));
            } else {
                req(emagls_plan_set_hrir_grid(p, azi, zen));
                if (mic_azi) req(emagls_plan_set_mic_grid(p, mic_azi, mic_zen));
            }
            req(emagls_plan_set_hrirs(p, hL, hR));
            if (atf) req(emagls_plan_set_atfs(p, atf, atf_azi, atf_zen));
            plan_execute(*p);
            req(emagls_plan_get_filters(p, wL, wR));
            if (mean_dev) {
                emagls_plan_info info;
                req(emagls_plan_get_info(p, &info));
                *mean_dev = info.mean_grid_dev_deg;
            }
        } catch (...) {
            release(false);
            throw;
        }
        release(true);
    });
}

// designs per batch: 8 by default (one per XCD in the resident sweep), up to 16 (two per XCD) after emagls_set_batch_max / EMAGLS_BATCH_MAX
static_assert(REG_SWEEP_MAX == 32, "the clamp of EMAGLS_BATCH_MAX in switches.hpp");
std::atomic<int> g_batch_max{sw_int<Sw::BATCH_MAX>()};   // (initialised at load time: the switch table is usable then, see switches.hpp)
}  // namespace

namespace emagls {
bool same_desc(const emagls_design_desc& a, const emagls_design_desc& b) {
    return a.kind == b.kind && a.basis == b.basis && a.order == b.order && a.fs == b.fs && a.len == b.len && a.nsamp == b.nsamp &&
           a.ndirs == b.ndirs && a.mic_radius == b.mic_radius && a.nmics == b.nmics && a.f_trans == b.f_trans &&
           a.atf_taps == b.atf_taps && a.natf == b.natf && a.custom_basis == b.custom_basis && a.diffuseness == b.diffuseness &&
           a.sim_order_pad == b.sim_order_pad;
}
thread_local int g_batch_max_override = 0;   // emagls_design_hrir_sets builds batches of 16 of its own whatever the caller's limit is
}  // namespace emagls

// =============================================================================================
extern "C" {

const char* emagls_last_error(void) { return g_last_error.c_str(); }
int emagls_version(void) { return 100; }

int emagls_device_count(int* count) {
    return guarded([&] {
        if (!count) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipGetDeviceCount(count));
    });
}
int emagls_set_device(int device) {
    return guarded([&] { HIP_CHECK(hipSetDevice(device)); });
}

void emagls_sets_cache_clear_internal();
void emagls_atfsets_cache_clear_internal();
void emagls_jobs_cache_clear_internal();
int emagls_cache_release_designs(void) {
    return guarded([&] {
        {
            std::lock_guard<std::mutex> lk(g_cache_mu);
            for (size_t i = g_cache.size(); i-- > 0;)
                if (!g_cache[i].busy) g_cache.erase(g_cache.begin() + i);
        }
        emagls_sets_cache_clear_internal();
        emagls_atfsets_cache_clear_internal();
        emagls_jobs_cache_clear_internal();
    });
}
int emagls_cache_clear(void) {
    return guarded([&] {
        {
            std::lock_guard<std::mutex> lk(g_cache_mu);
            for (size_t i = g_cache.size(); i-- > 0;)
                if (!g_cache[i].busy) g_cache.erase(g_cache.begin() + i);
        }
        decode_family_cache_clear();
        emagls_sets_cache_clear_internal();
        emagls_atfsets_cache_clear_internal();
        emagls_jobs_cache_clear_internal();
        BlockPool::get().clear();
    });
}

int emagls_fp64_peak_tflops(int which, double* tflops) {
    return guarded([&] {
        if (!tflops || which < 0 || which > 2) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        *tflops = measure_fp64_peak(which, 3);
    });
}

int emagls_self_test(int which, double* max_err) {
    return guarded([&] {
        if (!max_err || which < 0 || which > 2) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        *max_err = which == 0 ? reg_contract_selftest() : gram_tile_selftest(which == 2);
    });
}

int emagls_debug_synth_operand(const void* bsc, int nbins, int nord_pad, const double* x, int64_t nx, int gs, void* g_plus, void* g_minus) {
    return guarded([&] { synth_operand_debug(bsc, nbins, nord_pad, x, nx, gs, g_plus, g_minus); });
}

int emagls_debug_synth_cosines(const double* dir_azi, const double* dir_zen, int64_t ndirs, const double* mic_azi, const double* mic_zen, int nmics, double* x2) {
    return guarded([&] { synth_cosines_debug(dir_azi, dir_zen, ndirs, mic_azi, mic_zen, nmics, x2); });
}

int emagls_debug_twiddles(int nfft, void* tw) {
    return guarded([&] { twiddles_debug(nfft, tw); });
}

int emagls_debug_filter_epilogue(const void* W, int C, int nfft, int len, const double* grpd, int conj_mode, int dc_rule, int shift_mode, int out_cplx,
                                 int n_ears, double fade_rel, void* outL, void* outR) {
    return guarded([&] { filter_epilogue_debug(W, C, nfft, len, grpd, conj_mode, dc_rule, shift_mode, out_cplx, n_ears, fade_rel, outL, outR); });
}

int emagls_debug_hrir_spectra(const double* hL, const double* hR, int64_t L, int64_t D_src, int64_t D, const int64_t* didx, int nfft, int mode, int n_c,
                              int kabs0, const double* grpd_in, int64_t ldD, int ldT, double* grpd_out, void* phs, void* Hc, double* Habs, double* HcT) {
    return guarded([&] { hrir_spectra_debug(hL, hR, L, D_src, D, didx, nfft, mode, n_c, kabs0, grpd_in, ldD, ldT, grpd_out, phs, Hc, Habs, HcT); });
}

int emagls_debug_real_spectra(const double* x, int64_t L, int64_t ncols_src, int64_t ncols, const int64_t* colidx, int nfft, int64_t ldo, int64_t inner,
                              int64_t ld_inner, void* out) {
    return guarded([&] { real_spectra_debug(x, L, ncols_src, ncols, colidx, nfft, ldo, inner, ld_inner, out); });
}

int emagls_fp64_peak_tflops_ex(int which, int burst, double* tflops, double* shader_mhz) {
    return guarded([&] {
        if (!tflops || which < 0 || which > 2) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        *tflops = measure_fp64_peak(which, 3, burst != 0, shader_mhz);
    });
}

int emagls_sh_basis(int order, int64_t ndirs, const double* azi, const double* zen, int basis, void* Y) {
    return guarded([&] {
        if (order < 0 || ndirs < 0 || !azi || !zen || !Y) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        if (ndirs == 0) return;
        const bool cb = basis == EMAGLS_BASIS_COMPLEX;
        const size_t S = (size_t)(order + 1) * (order + 1);
        DevMem d_azi(sizeof(double) * ndirs), d_zen(sizeof(double) * ndirs), d_tab(sizeof(double) * sh_coeff_count(order)), d_Y(esz(cb) * S * ndirs);
        HIP_CHECK(hipMemcpy(d_azi.get(), azi, sizeof(double) * ndirs, hipMemcpyDefault));
        HIP_CHECK(hipMemcpy(d_zen.get(), zen, sizeof(double) * ndirs, hipMemcpyDefault));
        launch_sh_coeff(order, d_tab.get<double>(), nullptr);
        launch_sh_basis(order, ndirs, d_azi.get<double>(), d_zen.get<double>(), d_tab.get<double>(), cb, d_Y.get(), ndirs, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(Y, d_Y.get(), esz(cb) * S * ndirs, hipMemcpyDefault));
    });
}

int emagls_sh_basis_device(int order, int64_t ndirs, const double* d_azi, const double* d_zen, int basis, void* d_Y,
                           void* stream) {
    return guarded([&] {
        if (order < 0 || ndirs < 0 || !d_azi || !d_zen || !d_Y) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        if (ndirs == 0) return;
        // the recurrence table is tiny and depends only on the order: cached per (thread, order).  A raw pointer on purpose, not a
        // DevMem: nothing may free device memory while a thread's storage is destroyed (device_mem.hpp)
        thread_local int tab_order = -1;
        thread_local double* tab = nullptr;
        hipStream_t st = (hipStream_t)stream;
        if (tab_order != order) {
            if (tab) { HIP_CHECK(hipFree(tab)); tab = nullptr; }
            HIP_CHECK(hipMalloc(&tab, sizeof(double) * sh_coeff_count(order)));
            tab_order = order;
            launch_sh_coeff(order, tab, st);
        }
        launch_sh_basis(order, ndirs, d_azi, d_zen, tab, basis == EMAGLS_BASIS_COMPLEX, d_Y, ndirs, st);
    });
}

int emagls_modal_bn(int order, int64_t nfreq, const double* kr, void* bn) {
    return guarded([&] {
        if (order < 0 || nfreq < 0 || !kr || !bn) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        if (nfreq == 0) return;
        DevMem d_kr(sizeof(double) * nfreq), d_bn(sizeof(cplx) * nfreq * (order + 1));
        HIP_CHECK(hipMemcpy(d_kr.get(), kr, sizeof(double) * nfreq, hipMemcpyDefault));
        launch_modal_bn(order, nfreq, d_kr.get<double>(), 1.0, 1.0, d_bn.get(), 1, nfreq, nullptr);  // column-major [nfreq x (order+1)]
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(bn, d_bn.get(), sizeof(cplx) * nfreq * (order + 1), hipMemcpyDefault));
    });
}

// ---------------------------------------------------------------------------------------------
int emagls_plan_create(const emagls_design_desc* desc, emagls_plan** plan) {
    return guarded([&] {
        if (!desc || !plan) throw Error(EMAGLS_ERR_ARG, "null pointer");
        std::unique_ptr<emagls_plan> p(new emagls_plan);
        p->d = *desc;
        plan_setup(*p);
        *plan = p.release();
    });
}
int emagls_plan_destroy(emagls_plan* plan) {
    return guarded([&] {
        DeviceGuard dg(plan ? plan->device : -1);
        delete plan;
    });
}
int emagls_plan_set_hrir_grid(emagls_plan* p, const double* azi, const double* zen) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !azi) throw Error(EMAGLS_ERR_ARG, "null pointer");
        // a horizontal HRIR set (getMagLsFilters2D) has no zenith argument: pi/2 for every direction
        std::vector<double> equator;
        if (p->d.kind == EMAGLS_KIND_MAGLS_2D) { equator.assign((size_t)p->d.ndirs, kPi / 2.0); zen = equator.data(); }
        if (!zen) throw Error(EMAGLS_ERR_ARG, "null pointer");
        p->upload("hrir_azi", azi, sizeof(double) * p->d.ndirs);
        p->upload("hrir_zen", zen, sizeof(double) * p->d.ndirs);
        HIP_CHECK(hipStreamSynchronize(p->stream));
        p->have_hrir_grid = true;
        ++p->atf_side_version;
    });
}
int emagls_plan_set_mic_grid(emagls_plan* p, const double* azi, const double* zen) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !azi) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (!p->has("mic_azi")) throw Error(EMAGLS_ERR_ARG, "this design kind has no microphone grid");
        // an equatorial array (EMAinCH) has no zenith argument: pi/2 for every microphone (getEMagLsFiltersEMAinCH.m:60)
        std::vector<double> equator;
        if (p->d.kind == EMAGLS_KIND_EMA_CH || p->d.kind == EMAGLS_KIND_EMA_SH) { equator.assign((size_t)p->d.nmics, kPi / 2.0); zen = equator.data(); }
        if (!zen) throw Error(EMAGLS_ERR_ARG, "null pointer");
        p->upload("mic_azi", azi, sizeof(double) * p->d.nmics);
        p->upload("mic_zen", zen, sizeof(double) * p->d.nmics);
        if (p->has("smap")) {   // the synthesising sweep's row order of the microphones: antipodal pairs first (sweep_synth.hip)
            int smap[34];
            synth_pairing(azi, zen, (int)p->d.nmics, smap);
            p->upload("smap", smap, sizeof smap);
            p->synth_units = smap[32] + smap[33];
            HIP_CHECK(hipStreamSynchronize(p->stream));   // (the host array goes out of scope)
        }
        // kr = 2*pi*f/C * smaRadius on f = linspace(0, fs/2, P)   (getSMAIRMatrix.m:90,107)
        std::vector<double> kr(p->P);
        for (int k = 0; k < p->P; ++k) {
            const double f = (double)k * (p->d.fs / 2.0) / (double)(p->P - 1);
            kr[k] = 2.0 * kPi * f / C_SOUND * p->d.mic_radius;
        }
        p->upload("kr", kr.data(), sizeof(double) * p->P);
        HIP_CHECK(hipStreamSynchronize(p->stream));
        p->have_mic_grid = true;
        ++p->atf_side_version;   // (a geometry-sharing batch compares the grids again)
    });
}
int emagls_plan_set_basis(emagls_plan* p, const void* Y_hrir, const void* Y_mic) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !Y_hrir) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (!p->custom_basis) throw Error(EMAGLS_ERR_ARG, "the plan was not created with custom_basis = 1");
        const size_t es = esz(p->cplx_basis);
        // MATLAB layout [ndirs x S] column-major -> Ycm [S][ldD]
        HIP_CHECK(hipMemcpy2DAsync(p->get("Ycm"), (size_t)p->ldD * es, Y_hrir, (size_t)p->D * es, (size_t)p->D * es, (size_t)p->S, hipMemcpyDefault,
                                   p->stream));
        if (array_kind(p->d.kind)) {
            if (!Y_mic) throw Error(EMAGLS_ERR_ARG, "the array designs need the SH matrix of the microphone grid too");
            p->upload("Ymic_cm", Y_mic, es * (size_t)p->S * p->d.nmics);   // [nmics x S] column-major == [S][M]
            std::vector<double> kr(p->P);
            for (int k = 0; k < p->P; ++k) kr[k] = 2.0 * kPi * ((double)k * (p->d.fs / 2.0) / (double)(p->P - 1)) / C_SOUND * p->d.mic_radius;
            p->upload("kr", kr.data(), sizeof(double) * p->P);
        }
        HIP_CHECK(hipStreamSynchronize(p->stream));
        p->have_basis = true;
    });
}
int emagls_plan_set_hrirs(emagls_plan* p, const double* hL, const double* hR) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !hL || !hR) throw Error(EMAGLS_ERR_ARG, "null pointer");
        p->upload("hL", hL, sizeof(double) * p->d.nsamp * p->d.ndirs);
        p->upload("hR", hR, sizeof(double) * p->d.nsamp * p->d.ndirs);
        HIP_CHECK(hipStreamSynchronize(p->stream));
        p->have_hrirs = true;
    });
}
int emagls_plan_set_atfs(emagls_plan* p, const double* atf, const double* azi, const double* zen) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !atf || !azi || !zen) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (!p->has("atf")) throw Error(EMAGLS_ERR_ARG, "this design kind has no ATFs");
        p->upload("atf", atf, sizeof(double) * p->d.atf_taps * p->d.nmics * p->d.natf);
        p->upload("atf_azi", azi, sizeof(double) * p->d.natf);
        p->upload("atf_zen", zen, sizeof(double) * p->d.natf);
        HIP_CHECK(hipStreamSynchronize(p->stream));
        p->have_atfs = true;
        ++p->atf_side_version;
    });
}
int emagls_plan_execute(emagls_plan* p) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p) throw Error(EMAGLS_ERR_ARG, "null pointer");
        plan_execute(*p);
    });
}
int emagls_plan_synchronize(emagls_plan* p) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(p->sync_stream ? p->sync_stream : p->stream));
    });
}
int emagls_plan_get_filters(emagls_plan* p, void* wL, void* wR) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !wL || !wR) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (!p->executed) throw Error(EMAGLS_ERR_ARG, "plan has not been executed");
        HIP_CHECK(hipStreamSynchronize(p->sync_stream ? p->sync_stream : p->stream));
        plan_check_flags(*p);
        const size_t bytes = (p->out_cplx ? sizeof(cplx) : sizeof(double)) * (size_t)p->out_rows * p->out_cols;
        HIP_CHECK(hipMemcpy(wL, p->get("wL"), bytes, hipMemcpyDefault));
        HIP_CHECK(hipMemcpy(wR, p->get("wR"), bytes, hipMemcpyDefault));
    });
}
int emagls_plan_sweep_form_in_batch(emagls_plan* p, int designs, int* form) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !form || designs < 1 || designs > REG_SWEEP_MAX) throw Error(EMAGLS_ERR_ARG, "emagls_plan_sweep_form_in_batch: null pointer or designs outside 1..32");
        std::vector<emagls_plan*> same((size_t)designs, p);
        const bool reg = p->synth && reg_sweep_wanted(same.data(), designs);
        *form = p->d.kind == EMAGLS_KIND_LS ? 0 : (p->synth ? (reg ? 3 : 2) : (p->sweep_persist ? 1 : 0));
    });
}
int emagls_plan_get_info(emagls_plan* p, emagls_plan_info* info) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !info) throw Error(EMAGLS_ERR_ARG, "null pointer");
        std::memset(info, 0, sizeof *info);
        info->nfft = p->nfft; info->num_pos_freqs = p->P; info->k_cut = p->k_cut; info->sim_order = p->simOrder;
        info->num_sh_sim = p->S; info->num_channels = p->C; info->out_is_complex = p->out_cplx;
        info->out_rows = p->out_rows; info->out_cols = p->out_cols; info->num_sweep_launches = p->sweep_launches;
        info->device_bytes = p->total_bytes;
        info->gram_from = p->gram_from; info->hh_end = p->hh_end; info->hh_orders = p->n_h + 1; info->g_first = p->g0;
        info->sim_order_own = array_kind(p->d.kind) ? p->simOrderOwn : p->simOrder;
        bool reg = false;   // the form the next sweep takes (decided per launch: a batch's for its members)
        if (p->synth) {
            bool whole = p->owner != nullptr;
            if (whole) for (auto* q : p->owner->plans) whole = whole && q != nullptr;
            reg = whole ? reg_sweep_wanted(p->owner->plans.data(), (int)p->owner->plans.size()) : reg_sweep_wanted(&p, 1);
        }
        info->sweep_form = p->d.kind == EMAGLS_KIND_LS ? 0 : (p->synth ? (reg ? 3 : 2) : (p->sweep_persist ? 1 : 0));
        info->sweep_units = p->synth ? p->synth_units : 0;
        if (p->executed) {
            HIP_CHECK(hipStreamSynchronize(p->stream));
            double g[2];
            HIP_CHECK(hipMemcpy(g, p->get("grpd"), sizeof g, hipMemcpyDeviceToHost));
            info->grp_delay_l = g[0]; info->grp_delay_r = g[1];
            if (p->has("mean_dev")) HIP_CHECK(hipMemcpy(&info->mean_grid_dev_deg, p->get("mean_dev"), sizeof(double), hipMemcpyDeviceToHost));
        }
    });
}
int emagls_plan_set_profiling(emagls_plan* p, int level) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p) throw Error(EMAGLS_ERR_ARG, "null pointer");
        p->prof_level = level;
    });
}
int emagls_plan_set_streams(emagls_plan* p, int nstreams) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nstreams < 1 || nstreams > 4) throw Error(EMAGLS_ERR_ARG, "nstreams must be 1..4");
        HIP_CHECK(hipStreamSynchronize(p->stream));
        drop_plan_graphs(*p);   // (the next execute runs eagerly again, the one after it captures with the new stream count)
        p->nstreams = nstreams;
    });
}
int emagls_plan_num_stages(emagls_plan* p) { return p ? (int)p->stage_names.size() : 0; }
const char* emagls_plan_stage_name(emagls_plan* p, int i) {
    if (!p || i < 0 || i >= (int)p->stage_names.size()) return "";
    return p->stage_names[i].c_str();
}
int emagls_plan_stage_times(emagls_plan* p, double* ms, int n) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !ms) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(p->stream));
        const int ns = (int)p->stage_names.size();
        for (int i = 0; i < n; ++i) {
            ms[i] = 0.0;
            if (i >= 1 && i < ns) {
                float t = 0.f;
                HIP_CHECK(hipEventElapsedTime(&t, p->stage_events[i - 1], p->stage_events[i]));
                ms[i] = t;
            }
        }
    });
}
int emagls_plan_sweep_kernel_time(emagls_plan* p, double* total_ms, int* launches) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !total_ms || !launches) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(p->stream));
        double tot = 0.0;
        int n = 0;
        if (p->prof_level >= 2) {
            for (int i = 0; i < p->sweep_launches && 2 * (size_t)i + 1 < p->sweep_events.size(); ++i) {
                float t = 0.f;
                HIP_CHECK(hipEventElapsedTime(&t, p->sweep_events[2 * i], p->sweep_events[2 * i + 1]));
                tot += t;
                ++n;
            }
        }
        *total_ms = tot;
        *launches = n;
    });
}
int emagls_plan_debug_buffer(emagls_plan* p, const char* name, void* dst, size_t* nbytes) {
    return guarded([&] {
        DeviceGuard dg(p ? p->device : -1);
        if (!p || !name || !nbytes) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (std::string(name) == "Yls") {   // the kept operand of a sharing batch's least-squares rows: the batch owns it, its plans show it
            emagls_batch* b = p->owner;
            if (!b || !b->geo_share || !b->geo_ls_shared || !b->yls.get()) throw Error(EMAGLS_ERR_ARG, "Yls: the plan's batch keeps no such operand");
            const emagls_plan& p0 = *b->plans[0];
            const size_t bytes = sizeof(cplx) * (size_t)(std::min(p0.kcut0, p0.P) - 1) * p0.C * p0.ldD;
            if (!dst) { *nbytes = bytes; return; }
            HIP_CHECK(hipStreamSynchronize(b->stream));
            const size_t n = std::min(*nbytes, bytes);
            HIP_CHECK(hipMemcpy(dst, b->yls.get(), n, hipMemcpyDeviceToHost));
            *nbytes = n;
            return;
        }
        auto it = p->bufs.find(name);
        if (it == p->bufs.end()) throw Error(EMAGLS_ERR_ARG, std::string("unknown buffer ") + name);
        if (!dst) { *nbytes = it->second.bytes; return; }
        HIP_CHECK(hipStreamSynchronize(p->stream));
        const size_t n = std::min(*nbytes, it->second.bytes);
        HIP_CHECK(hipMemcpy(dst, it->second.p, n, hipMemcpyDeviceToHost));
        *nbytes = n;
    });
}
void* emagls_plan_stream(emagls_plan* p) { return p ? (void*)p->stream : nullptr; }

int emagls_batch_create(emagls_plan** plans, int nplans, emagls_batch** batch) {
    return guarded([&] {
        if (!plans || !batch || nplans < 1) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        // Up to 8 designs per batch by default.  9 to 16 share one sweep launch with two workgroups per CU, which covers EVERY
        // CU: safe and fastest when nothing else runs on the device, but another stream's kernel that needs a whole CU
        // (e.g. factor_qr: 1024 threads x 128 registers) makes the dispatcher hold back the sweep's remaining workgroups
        // while the resident ones wait for them -- observed as a 0.4 s stall until the sweep's own time-out falls back to the
        // launch-per-bin form.  Hence opt-in: EMAGLS_BATCH_MAX=16.
        const int batch_max = std::max(g_batch_max.load(), g_batch_max_override);
        if (nplans > batch_max)
            throw Error(EMAGLS_ERR_UNSUPPORTED, batch_max >= REG_SWEEP_MAX ? "at most 32 designs per batch"
                                                                             : "at most 8 designs per batch (emagls_set_batch_max(16) / EMAGLS_BATCH_MAX=16 allows 16)");
        std::unique_ptr<emagls_batch> b(new emagls_batch);
        for (int j = 0; j < nplans; ++j) {
            emagls_plan* p = plans[j];
            if (!p) throw Error(EMAGLS_ERR_ARG, "null plan");
            if (!array_kind(p->d.kind) && p->d.kind != EMAGLS_KIND_FROM_ATF && !magls_kind(p->d.kind) && p->d.kind != EMAGLS_KIND_LS)
                throw Error(EMAGLS_ERR_UNSUPPORTED, "batches take eMagLS / eMagLS2 / EMAinCH / EMAinSH plans, LS / MagLS / MagLS-2D plans, or FromAtf plans "
                                                    "(subjects of one ATF set)");
            if ((p->d.kind == EMAGLS_KIND_LS) != (plans[0]->d.kind == EMAGLS_KIND_LS) ||
                (p->d.kind == EMAGLS_KIND_LS && (p->cplx_basis != plans[0]->cplx_basis || p->d.order != plans[0]->d.order || p->d.nsamp != plans[0]->d.nsamp)))
                throw Error(EMAGLS_ERR_ARG, "LS plans share a batch only with LS plans of the same order, basis and HRIR length");
            if ((p->d.kind == EMAGLS_KIND_FROM_ATF) != (plans[0]->d.kind == EMAGLS_KIND_FROM_ATF))
                throw Error(EMAGLS_ERR_ARG, "FromAtf plans cannot share a batch with array designs");
            if (magls_kind(p->d.kind) != magls_kind(plans[0]->d.kind) || (magls_kind(p->d.kind) && p->d.kind != plans[0]->d.kind))
                throw Error(EMAGLS_ERR_ARG, "MagLS plans share a batch only with MagLS plans of the same kind");
            if (magls_kind(p->d.kind) && (p->diffuse != plans[0]->diffuse || p->cplx_basis != plans[0]->cplx_basis || p->d.order != plans[0]->d.order))
                throw Error(EMAGLS_ERR_ARG, "all designs of a batch must have the same shape (order, basis, constraint)");
            if (p->wide) throw Error(EMAGLS_ERR_UNSUPPORTED, "designs with more than 32 channels run one at a time");
            if (p->owner) throw Error(EMAGLS_ERR_ARG, "a plan belongs to another batch (destroy that batch first)");
            if (p->device != plans[0]->device) throw Error(EMAGLS_ERR_ARG, "the plans of a batch must live on one device");
            for (int i = 0; i < j; ++i) if (plans[i] == p) throw Error(EMAGLS_ERR_ARG, "the same plan appears twice in the batch");
            const emagls_plan* q = plans[0];
            if (p->P != q->P || p->kcut0 != q->kcut0 || p->C != q->C || p->nWG_dense != q->nWG_dense || p->D != q->D || p->sweep_persist != q->sweep_persist ||
                p->Dm != q->Dm || p->d.natf != q->d.natf || p->d.atf_taps != q->d.atf_taps || p->d.len != q->d.len)
                throw Error(EMAGLS_ERR_ARG, "all designs of a batch must have the same shape (directions, channels, bins, k_cut)");
            b->plans.push_back(p);
        }
        b->device = b->plans[0]->device;
        DeviceGuard dg(b->device);
        b->stream = StreamPool::get().take();
        b->use_graph = !sw_on<Sw::NO_GRAPH>();
        // one persistent sweep launch keeps designs x nWG workgroups resident: one per CU up to 8 designs (one design per XCD),
        // two per CU beyond (77 KB of LDS and 5 waves per workgroup)
        // (up to 8 designs: 16 CUs stay free of sweep workgroups, so that kernels of other batches which need a whole CU keep
        // making progress and the dispatcher never has a reason to hold the sweep's own workgroups back)
        // (decided here, before any launch, from the runtime's occupancy of the kernel variant: persist_sweep_fits)
        const bool array_batch = b->plans[0]->d.kind != EMAGLS_KIND_FROM_ATF && !magls_kind(b->plans[0]->d.kind) && b->plans[0]->d.kind != EMAGLS_KIND_LS;
        for (auto* p : b->plans) HIP_CHECK(hipStreamSynchronize(p->stream));
        // (the sweep's form first -- one launch serves every design: the synthesising forms only when all qualify --, then its residency)
        trace_mark("batch create: plans synchronised");
        if (array_batch) batch_unify_synth(*b);
        trace_mark("batch create: sweep form unified");
        batch_decide_residency(*b);
        trace_mark("batch create: residency decided");
        if (nplans > SWEEP_MULTI_MAX && !(b->plans[0]->synth && b->plans[0]->sweep_persist && reg_sweep_wanted(b->plans.data(), nplans)))
            throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 16 designs per batch: only array designs that take the register-resident sweep (built-in SH basis, "
                                                "microphone grids set, at most 18 antipodal pairs + single microphones, a launch the device can hold)");
        for (auto* p : b->plans) {
            p->nstreams = 1;
            p->prof_level = 0;
            p->sync_stream = b->stream;
            p->owner = b.get();
        }
        b->atf = b->plans[0]->d.kind == EMAGLS_KIND_FROM_ATF;
        b->magls = magls_kind(b->plans[0]->d.kind) || b->plans[0]->d.kind == EMAGLS_KIND_LS;
        if (!b->atf && !b->magls) { batch_unify_synth(*b); batch_try_lanes(*b); }
        trace_mark("batch create: lanes tried");
        *batch = b.release();
    });
}
int emagls_batch_execute(emagls_batch* b) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        batch_execute(*b);
    });
}
int emagls_batch_synchronize(emagls_batch* b) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(b->stream));
    });
}
int emagls_batch_get_filters(emagls_batch* b, void* const* wL, void* const* wR) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b || !wL || !wR) throw Error(EMAGLS_ERR_ARG, "null pointer");
        const size_t n = b->plans.size();
        for (size_t j = 0; j < n; ++j) {
            if (!wL[j] || !wR[j]) throw Error(EMAGLS_ERR_ARG, "null pointer");
            if (!b->plans[j]) throw Error(EMAGLS_ERR_ARG, "a plan of this batch has been destroyed");
            if (!b->plans[j]->executed) throw Error(EMAGLS_ERR_ARG, "batch has not been executed");
        }
        emagls_plan& p0 = *b->plans[0];
        const size_t bytes = (p0.out_cplx ? sizeof(cplx) : sizeof(double)) * (size_t)p0.out_rows * p0.out_cols;
        // the copies are ordered behind the batch on its stream; one synchronisation for everything
        std::vector<int> flags(NFLAG * n, 0);
        for (int attempt = 0; attempt < 3; ++attempt) {
            if (b->lanes)
                HIP_CHECK(hipMemcpy2DAsync(flags.data(), NFLAG * sizeof(int), p0.get("flag"), b->stride, NFLAG * sizeof(int), n,
                                           hipMemcpyDeviceToHost, b->stream));
            else
                for (size_t j = 0; j < n; ++j)
                    HIP_CHECK(hipMemcpyAsync(&flags[NFLAG * j], b->plans[j]->get("flag"), NFLAG * sizeof(int), hipMemcpyDeviceToHost, b->stream));
            // lane batch into device buffers of this GPU: one scatter launch instead of 2 n copies (0.25 ms on the stream for 16
            // designs -- the tail of a short run's timed region)
            bool scattered = false;
            if (b->lanes && n <= 32 && bytes % 16 == 0) {
                bool dev_dst = true;
                for (size_t j = 0; j < n && dev_dst; ++j)
                    for (void* q : {wL[j], wR[j]}) {
                        hipPointerAttribute_t at{};
                        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); dev_dst = false; break; }
                        if (at.type != hipMemoryTypeDevice || at.device != b->device || ((uintptr_t)q & 15)) { dev_dst = false; break; }
                    }
                if (dev_dst) {
                    LanePtrs lp{};
                    for (size_t j = 0; j < n; ++j) { lp.p[2 * j] = wL[j]; lp.p[2 * j + 1] = wR[j]; }
                    launch_scatter_lanes(p0.get("wL"), p0.get("wR"), b->stride, bytes, (int)n, lp, b->stream);
                    scattered = true;
                }
            }
            if (!scattered)
                for (size_t j = 0; j < n; ++j) {
                    HIP_CHECK(hipMemcpyAsync(wL[j], b->plans[j]->get("wL"), bytes, hipMemcpyDefault, b->stream));
                    HIP_CHECK(hipMemcpyAsync(wR[j], b->plans[j]->get("wR"), bytes, hipMemcpyDefault, b->stream));
                }
            HIP_CHECK(hipStreamSynchronize(b->stream));
            bool redo = false;
            for (size_t j = 0; j < n; ++j) redo = plan_recover(*b->plans[j], &flags[NFLAG * j], false) || redo;
            if (!redo) break;
            // recoverable: a Gram-route bin worse conditioned than estimated, or a persistent sweep that did not become resident
            batch_redo(*b, flags);
        }
        for (auto* q : b->plans)   // (a MagLS re-run on the launch-per-bin sweeps is done: the next execute starts on the persistent form again)
            if (q->persist_suspended) { q->persist_suspended = false; q->sweep_persist = true; }
        for (size_t j = 0; j < n; ++j) throw_fatal_flags(&flags[NFLAG * j]);
        // clean: the geometry state of a sharing batch's cold run serves its next executes (batch_execute_geo)
        if (b->geo_cold_pending) { b->geo_kept_version = b->geo_ran_version; b->geo_cold_pending = false; }
    });
}
int emagls_batch_geometry_runs(emagls_batch* b, long long* cold, long long* warm) {
    return guarded([&] {
        if (!b || !cold || !warm) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *cold = b->geo_cold_runs;
        *warm = b->geo_warm_runs;
    });
}
int emagls_batch_lane_mode(emagls_batch* b, int* lanes) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b || !lanes) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *lanes = b->lanes ? 1 : 0;
    });
}
int emagls_set_batch_max(int max_designs, int* previous) {
    return guarded([&] {
        if (max_designs < 1 || max_designs > REG_SWEEP_MAX) throw Error(EMAGLS_ERR_ARG, "a batch holds 1..32 designs (more than 16: array designs on the register-resident sweep)");
        const int prev = g_batch_max.exchange(max_designs);
        if (previous) *previous = prev;
    });
}
int emagls_batch_set_geometry_sharing(emagls_batch* b, int enable) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        b->geo_want = enable != 0;
        b->geo_checked_version = ~0ull;
        batch_geo_forget(*b);   // (the next sharing execute runs the geometry stages)
    });
}
int emagls_batch_shares_geometry(emagls_batch* b, int* shared) {
    return guarded([&] {
        if (!b || !shared) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *shared = b->geo_share ? 1 : 0;
    });
}
int emagls_batch_shares_atf_side(emagls_batch* b, int* shared) {
    return guarded([&] {
        if (!b || !shared) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *shared = b->atf_share ? 1 : 0;
    });
}
int emagls_batch_set_stream(emagls_batch* b, void* stream) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b || !stream) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        if (b->own_stream) emagls::pool_stream_give(b->stream);
        b->stream = (hipStream_t)stream;      // (captured graphs are not tied to a stream: they replay on the new one)
        b->own_stream = false;
        for (auto* p : b->plans) if (p) p->sync_stream = b->stream;
    });
}
int emagls_batch_set_streams(emagls_batch* b, int nstreams) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (nstreams < 1 || nstreams > 4) throw Error(EMAGLS_ERR_ARG, "nstreams must be 1..4");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        for (int i = 0; i < nstreams - 1; ++i) if (!b->side[i]) b->side[i] = emagls::pool_stream_take();
        if (nstreams != b->nstreams) drop_batch_graphs(*b);   // (forked stages run eagerly; back on one stream, the execute after the next captures)
        b->nstreams = nstreams;
    });
}
int emagls_batch_set_stage_order(emagls_batch* b, int order) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (order < 0 || order > 2) throw Error(EMAGLS_ERR_ARG, "stage order must be 0, 1 or 2");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        if (order != b->order_hint) drop_batch_graphs(*b);
        b->order_hint = order;
    });
}
int emagls_batch_set_side_stream(emagls_batch* b, void* stream) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b || !stream) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        if (b->side[0] && !b->side0_external) { HIP_CHECK(hipStreamSynchronize(b->side[0])); emagls::pool_stream_give(b->side[0]); }
        b->side[0] = (hipStream_t)stream;
        b->side0_external = true;
    });
}
int emagls_batch_set_profiling(emagls_batch* b, int level) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b) throw Error(EMAGLS_ERR_ARG, "null pointer");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        if (level >= 1)
            for (auto& e : b->sweep_ev) if (!e) HIP_CHECK(hipEventCreate(&e));
        b->prof_level = level;
    });
}
int emagls_batch_sweep_time(emagls_batch* b, double* ms) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        if (!b || !ms) throw Error(EMAGLS_ERR_ARG, "null pointer");
        if (b->prof_level < 1 || !b->sweep_ev[0]) throw Error(EMAGLS_ERR_ARG, "batch profiling is off");
        HIP_CHECK(hipStreamSynchronize(b->stream));
        float t = 0.f;
        HIP_CHECK(hipEventElapsedTime(&t, b->sweep_ev[0], b->sweep_ev[1]));
        *ms = t;
    });
}
int emagls_batch_destroy(emagls_batch* b) {
    return guarded([&] {
        DeviceGuard dg(b ? b->device : -1);
        delete b;
    });
}

// ---------------------------------------------------------------------------------------------
int emagls_get_ls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                          const double* zen, int order, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_LS; d.basis = basis; d.order = order; d.nsamp = nsamp; d.ndirs = ndirs;
    return one_shot(d, hL, hR, azi, zen, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_magls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                             const double* zen, int order, double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_MAGLS; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    return one_shot(d, hL, hR, azi, zen, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                              const double* zen, double mic_radius, const double* mic_azi, const double* mic_zen,
                              int64_t nmics, int order, double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMAGLS; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics;
    if (!mic_azi || !mic_zen) { g_last_error = "null microphone grid"; return EMAGLS_ERR_ARG; }
    return one_shot(d, hL, hR, azi, zen, mic_azi, mic_zen, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls2_filters(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                               const double* zen, double mic_radius, const double* mic_azi, const double* mic_zen,
                               int64_t nmics, int order, double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMAGLS2; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics;
    if (!mic_azi || !mic_zen) { g_last_error = "null microphone grid"; return EMAGLS_ERR_ARG; }
    return one_shot(d, hL, hR, azi, zen, mic_azi, mic_zen, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls_filters_ema_in_ch(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                                        const double* zen, double mic_radius, const double* mic_azi, int64_t nmics, int order,
                                        double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMA_CH; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics;
    if (!mic_azi || nmics < 1) { g_last_error = "invalid array geometry"; return EMAGLS_ERR_ARG; }
    std::vector<double> mic_zen((size_t)nmics, kPi / 2.0);   // getEMagLsFiltersEMAinCH.m:60: equatorial array
    return one_shot(d, hL, hR, azi, zen, mic_azi, mic_zen.data(), nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls_filters_ema_in_sh(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi,
                                        const double* zen, double mic_radius, const double* mic_azi, int64_t nmics, int order,
                                        double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMA_SH; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics;
    if (!mic_azi || nmics < 1) { g_last_error = "invalid array geometry"; return EMAGLS_ERR_ARG; }
    std::vector<double> mic_zen((size_t)nmics, kPi / 2.0);   // getEMagLsFiltersEMAinSH.m:58: equatorial array
    return one_shot(d, hL, hR, azi, zen, mic_azi, mic_zen.data(), nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls_filters_from_atf(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs,
                                       const double* azi, const double* zen, const double* atf_irs, int64_t atf_taps,
                                       int64_t nmics, int64_t natf, const double* atf_azi, const double* atf_zen, double fs,
                                       int64_t filter_len, double f_trans, double* wL, double* wR, double* mean_dev) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_FROM_ATF; d.basis = EMAGLS_BASIS_REAL; d.fs = fs; d.len = filter_len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.nmics = nmics; d.f_trans = f_trans; d.atf_taps = atf_taps; d.natf = natf;
    if (!atf_irs || !atf_azi || !atf_zen) { g_last_error = "null ATF set"; return EMAGLS_ERR_ARG; }
    return one_shot(d, hL, hR, azi, zen, nullptr, nullptr, atf_irs, atf_azi, atf_zen, wL, wR, mean_dev);
}

int emagls_get_magls_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                int order, double fs, int64_t len, int apply_dc, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_MAGLS; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.diffuseness = apply_dc != 0;
    return one_shot(d, hL, hR, azi, zen, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
static int emagls_array_dc(int kind, const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                           double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs, int64_t len,
                           int apply_dc, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = kind; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics; d.diffuseness = apply_dc != 0;
    return one_shot(d, hL, hR, azi, zen, mic_azi, mic_zen, nullptr, nullptr, nullptr, wL, wR, nullptr);
}
int emagls_get_emagls_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                 double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                                 int64_t len, int apply_dc, int basis, void* wL, void* wR) {
    return emagls_array_dc(EMAGLS_KIND_EMAGLS, hL, hR, nsamp, ndirs, azi, zen, mic_radius, mic_azi, mic_zen, nmics, order, fs, len, apply_dc,
                           basis, wL, wR);
}
int emagls_get_emagls2_filters_dc(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, const double* zen,
                                  double mic_radius, const double* mic_azi, const double* mic_zen, int64_t nmics, int order, double fs,
                                  int64_t len, int apply_dc, int basis, void* wL, void* wR) {
    return emagls_array_dc(EMAGLS_KIND_EMAGLS2, hL, hR, nsamp, ndirs, azi, zen, mic_radius, mic_azi, mic_zen, nmics, order, fs, len, apply_dc,
                           basis, wL, wR);
}
int emagls_get_magls_filters_2d(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const double* azi, int order, double fs,
                                int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_MAGLS_2D; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    return one_shot(d, hL, hR, azi, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr);
}

int emagls_simulation_order(int kind, int order, double fs, double mic_radius) {
    switch (kind) {
        case EMAGLS_KIND_EMAGLS: case EMAGLS_KIND_EMA_CH: case EMAGLS_KIND_EMA_SH:
            return smair_sim_order(order, fs, mic_radius);
        case EMAGLS_KIND_EMAGLS2:
            return smair_sim_order(SMAIR_DEFAULT_ORDER, fs, mic_radius);     // params.order unset -> 4
        default: return order;
    }
}
int emagls_design_out_shape(const emagls_design_desc* desc, int64_t* rows, int64_t* cols, int* is_complex) {
    return guarded([&] {
        if (!desc || !rows || !cols || !is_complex) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        const emagls_design_desc& d = *desc;
        if (d.kind < EMAGLS_KIND_LS || d.kind > EMAGLS_KIND_EMA_SH || d.order < 0) throw Error(EMAGLS_ERR_ARG, "invalid design kind or order");
        switch (d.kind) {
            case EMAGLS_KIND_EMAGLS2: case EMAGLS_KIND_FROM_ATF: *cols = d.nmics; break;                       // one filter per microphone
            case EMAGLS_KIND_MAGLS_2D: case EMAGLS_KIND_EMA_CH: *cols = 2 * (int64_t)d.order + 1; break;       // circular harmonics
            default: *cols = ((int64_t)d.order + 1) * (d.order + 1);
        }
        *rows = d.kind == EMAGLS_KIND_LS ? d.nsamp : d.len;                                                    // lib/getLsFilters.m:33: h * Y_pinv
        *is_complex = d.basis == EMAGLS_BASIS_COMPLEX && d.kind != EMAGLS_KIND_FROM_ATF;
    });
}
int emagls_get_ls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir, int order,
                                     int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_LS; d.basis = basis; d.order = order; d.nsamp = nsamp; d.ndirs = ndirs; d.custom_basis = 1;
    return one_shot(d, hL, hR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr, Y_hrir, nullptr);
}
int emagls_get_magls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir, int order,
                                        double fs, int64_t len, int basis, void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_MAGLS; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs; d.custom_basis = 1;
    return one_shot(d, hL, hR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr, Y_hrir, nullptr);
}
int emagls_get_emagls_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir,
                                         double mic_radius, const void* Y_mic, int64_t nmics, int order, double fs, int64_t len, int basis,
                                         void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMAGLS; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics; d.custom_basis = 1;
    if (!Y_mic) { g_last_error = "null microphone SH matrix"; return EMAGLS_ERR_ARG; }
    return one_shot(d, hL, hR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr, Y_hrir, Y_mic);
}
int emagls_get_emagls2_filters_with_basis(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, const void* Y_hrir,
                                          double mic_radius, const void* Y_mic, int64_t nmics, int order, double fs, int64_t len, int basis,
                                          void* wL, void* wR) {
    emagls_design_desc d{};
    d.kind = EMAGLS_KIND_EMAGLS2; d.basis = basis; d.order = order; d.fs = fs; d.len = len; d.nsamp = nsamp; d.ndirs = ndirs;
    d.mic_radius = mic_radius; d.nmics = nmics; d.custom_basis = 1;
    if (!Y_mic) { g_last_error = "null microphone SH matrix"; return EMAGLS_ERR_ARG; }
    return one_shot(d, hL, hR, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, wL, wR, nullptr, Y_hrir, Y_mic);
}

}  // extern "C"
