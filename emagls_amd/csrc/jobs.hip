// C ABI, continued: HRIR sets and ATF subjects in one call, job lists with their resident slots, and the multi-GPU shard planner.
#include "host_internal.hpp"

extern "C" {

// ---------------------------------------------------------------------------------------------
// HRIR sets on one geometry in ONE call (what a loop over subjects around lib/get*Filters.m does): plans + a geometry-sharing
// batch per chunk of up to 16 sets, kept for the next call of the same shape (emagls_cache_clear releases them).
// ---------------------------------------------------------------------------------------------
namespace {
struct SetsCache {
    emagls_design_desc desc{};
    int device = -1, n = 0;
    std::vector<emagls_plan*> plans;
    emagls_batch* batch = nullptr;
    std::vector<double> grid[4];      // the grids the plans hold (hrir azi / zen, mic azi / zen): unchanged grids are not uploaded again
    void release() {
        for (auto& g : grid) g.clear();
        if (batch) { emagls_batch_destroy(batch); batch = nullptr; }
        for (auto* p : plans) emagls_plan_destroy(p);
        plans.clear();
        n = 0; device = -1;
    }
};
std::mutex g_sets_mu;
SetsCache g_sets[3];   // (two sets of plans for the full chunks, which alternate, and one for the tail chunk)
}  // namespace
void emagls_sets_cache_clear_internal() {
    std::lock_guard<std::mutex> lk(g_sets_mu);
    for (auto& c : g_sets) c.release();
}

int emagls_design_hrir_sets(int kind, const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, int64_t nsets,
                            const double* hrir_azi, const double* hrir_zen, double mic_radius, const double* mic_azi, const double* mic_zen,
                            int64_t nmics, int order, double fs, int64_t len, int basis, void* wL, void* wR) {
    return guarded([&] {
        if (!hL || !hR || !hrir_azi || !wL || !wR || nsets < 1) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        const bool arr = array_kind(kind);
        if (!arr && kind != EMAGLS_KIND_LS && kind != EMAGLS_KIND_MAGLS && kind != EMAGLS_KIND_MAGLS_2D)
            throw Error(EMAGLS_ERR_UNSUPPORTED, "HRIR-set job lists: LS, MagLS, MagLS-2D, eMagLS, eMagLS2, EMAinCH, EMAinSH");
        emagls_design_desc d{};
        d.kind = kind; d.basis = basis; d.order = order; d.fs = fs; d.len = kind == EMAGLS_KIND_LS ? nsamp : len; d.nsamp = nsamp; d.ndirs = ndirs;
        d.mic_radius = arr ? mic_radius : 0.0; d.nmics = arr ? nmics : 0;
        auto req = [](int r) { if (r != EMAGLS_OK) throw Error(r, g_last_error); };
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_sets_mu);
        // Full chunks alternate between two plan sets: while one computes, the next chunk's HRIRs are uploaded into the other
        // (5.5 MB per set from pageable memory: as long as the chunk's compute).  The tail chunk has a set of its own.
        struct Pending { SetsCache* c = nullptr; int64_t first = 0; };
        Pending pend[3];
        size_t out_bytes = 0;
        auto collect = [&](Pending& q) {
            if (!q.c) return;
            SetsCache* c = q.c;
            q.c = nullptr;
            const int n = c->n;
            if (n == 1 || !c->batch) {   // (no batch: designs with more than 32 channels run one at a time)
                for (int j = 0; j < n; ++j)
                    req(emagls_plan_get_filters(c->plans[(size_t)j], (char*)wL + (q.first + j) * out_bytes, (char*)wR + (q.first + j) * out_bytes));
            } else {
                std::vector<void*> pl((size_t)n), pr((size_t)n);
                for (int j = 0; j < n; ++j) { pl[(size_t)j] = (char*)wL + (q.first + j) * out_bytes; pr[(size_t)j] = (char*)wR + (q.first + j) * out_bytes; }
                req(emagls_batch_get_filters(c->batch, pl.data(), pr.data()));
            }
        };
        try {
            int64_t k = 0;
            for (int64_t first = 0; first < nsets; ++k) {
                // (chunks of designs with more than 32 channels run plan by plan and hold gigabytes per plan: four at a time)
                const bool wide_kind = ((kind == EMAGLS_KIND_MAGLS_2D || kind == EMAGLS_KIND_EMA_CH) ? 2 * order + 1 : kind == EMAGLS_KIND_EMAGLS2 ? (int)nmics : (order + 1) * (order + 1)) > 32;
                // (eMagLS / eMagLS2 there: one plan per chunk -- two plans alternate and keep their geometry stages, plan_execute -- instead of four)
                const int chunk_max = wide_kind ? ((kind == EMAGLS_KIND_EMAGLS || kind == EMAGLS_KIND_EMAGLS2) ? 1 : 4) : kind == EMAGLS_KIND_EMA_SH ? 4 : SWEEP_MULTI_MAX;
                const int n = (int)std::min<int64_t>(chunk_max, nsets - first);
                const int slot = n == chunk_max ? (int)(k % 2) : 2;
                SetsCache* c = &g_sets[slot];
                collect(pend[slot]);      // (the chunk this plan set computed two chunks ago)
                if (!(c->n == n && c->device == dev && same_desc(c->desc, d))) {
                    c->release();
                    try {
                        for (int j = 0; j < n; ++j) {
                            emagls_plan* p = nullptr;
                            req(emagls_plan_create(&d, &p));
                            p->geo_keep = true;   // (one geometry for every set by this entry point's contract: plans of the 33..64-channel path keep their geometry stages)
                            c->plans.push_back(p);
                        }
                        // designs with more than 32 channels (LS / MagLS orders 5..7, arrays of 33..64 channels) do not enter
                        // batches (emagls_batch_create): their chunk runs plan by plan, same filters as nsets single calls
                        // (EMAinSH -- lib/getEMagLsFiltersEMAinSH.m:32 -- has no lane batches either: plan by plan)
                        if (n > 1 && !c->plans[0]->wide && kind != EMAGLS_KIND_EMA_SH) {
                            int r;
                            { Scoped limit(g_batch_max_override, SWEEP_MULTI_MAX); r = emagls_batch_create(c->plans.data(), n, &c->batch); }
                            req(r);
                            req(emagls_batch_set_geometry_sharing(c->batch, 1));
                        }
                    } catch (...) { c->release(); throw; }
                    c->desc = d; c->device = dev; c->n = n;
                }
                auto same = [](const std::vector<double>& have, const double* now, size_t cnt) {
                    return now ? (have.size() == cnt && std::memcmp(have.data(), now, cnt * sizeof(double)) == 0) : have.empty();
                };
                const bool hgrid_same = same(c->grid[0], hrir_azi, (size_t)ndirs) && same(c->grid[1], hrir_zen, (size_t)ndirs) && !c->grid[0].empty();
                const bool mgrid_same = !arr || (same(c->grid[2], mic_azi, (size_t)nmics) && same(c->grid[3], mic_zen, (size_t)nmics) && !c->grid[2].empty());
                for (int j = 0; j < n; ++j) {
                    emagls_plan* p = c->plans[(size_t)j];
                    if (!hgrid_same) req(emagls_plan_set_hrir_grid(p, hrir_azi, hrir_zen));
                    if (arr && !mgrid_same) req(emagls_plan_set_mic_grid(p, mic_azi, mic_zen));
                    req(emagls_plan_set_hrirs(p, hL + (first + j) * nsamp * ndirs, hR + (first + j) * nsamp * ndirs));
                }
                auto keep = [](std::vector<double>& dst, const double* src, size_t cnt) { if (src) dst.assign(src, src + cnt); else dst.clear(); };
                keep(c->grid[0], hrir_azi, (size_t)ndirs); keep(c->grid[1], hrir_zen, (size_t)ndirs);
                if (arr) { keep(c->grid[2], mic_azi, (size_t)nmics); keep(c->grid[3], mic_zen, (size_t)nmics); }
                emagls_plan_info info;
                req(emagls_plan_get_info(c->plans[0], &info));
                out_bytes = (info.out_is_complex ? sizeof(cplx) : sizeof(double)) * (size_t)info.out_rows * info.out_cols;
                if (n > 1 && c->batch) req(emagls_batch_execute(c->batch));   // (asynchronous)
                else for (int j = 0; j < n; ++j) req(emagls_plan_execute(c->plans[(size_t)j]));
                pend[slot].c = c;
                pend[slot].first = first;
                first += n;
            }
            for (auto& q : pend) collect(q);
        } catch (...) {   // (a failed call leaves the plans in an unknown state)
            for (auto& c : g_sets) c.release();
            throw;
        }
    });
}

// The HRTF subjects of ONE ATF set in one call (BASELINE config 5; lib/getEMagLsFiltersFromAtf.m:1 in a loop over subjects).  The
// ATF set is uploaded once (plan 0) and handed to the other plans device to device; the batch then finds equal ATF sides and
// computes that side once (batch_atf_decide_sharing).
namespace {
std::mutex g_atfsets_mu;
SetsCache g_atfsets[2];
}  // namespace
void emagls_atfsets_cache_clear_internal() {
    std::lock_guard<std::mutex> lk(g_atfsets_mu);
    for (auto& c : g_atfsets) c.release();
}

// ---------------------------------------------------------------------------------------------
// Job lists (independent designs are the unit of parallelism -- the loop over array radii / HRIR sets / subjects that
// a user of the reference writes around one of its functions, testEMagLs.m:75-95).  emagls_jobs_run takes the list, cuts it into
// chunks of consecutive jobs of one shape, and keeps up to `in_flight` chunks between input upload and result collection: every
// chunk in flight has a worker thread of the library (uploads, the batch's graph launches, the wait for its filters), so that one
// chunk's inputs travel and another's results are collected while the GPU works on the others.  The plans and lane batches of a
// chunk shape stay resident between calls (released by emagls_cache_clear) whenever the chunk's designs can be re-used as they are
// (same descriptors); array radii that change from chunk to chunk get plans of their own and release them.
// ---------------------------------------------------------------------------------------------
namespace {
struct JobSlot {
    std::string key;                  // the descriptors of the slot's designs, byte for byte
    std::string shape;                // what makes designs share a lane batch (job_shape), job by job: a slot of another key but this shape hands its memory on
    int device = -1;
    std::vector<emagls_plan*> plans;
    emagls_batch* batch = nullptr;
    std::vector<std::vector<double>> grids;   // per plan: hrir azi | zen | mic azi | zen as last uploaded (unchanged grids are not uploaded again)
    uint64_t last_use = 0, last_call = 0;     // (last_call: the emagls_jobs_run call that used the slot last)
    int runs = 0;                             // executes so far (the first two are the eager run and the graph capture)
    hipStream_t stream = nullptr;             // the plans' common stream (uploads, and the executes of designs that run plan by plan)
    ~JobSlot() {
        if (batch) emagls_batch_destroy(batch);
        for (auto* p : plans) emagls_plan_destroy(p);
        if (stream) emagls::pool_stream_give(stream);   // (synchronised there)
    }
};
std::mutex g_jobs_mu;
std::vector<std::unique_ptr<JobSlot>> g_jobs_free;   // resident slots nobody uses at the moment
std::atomic<int> g_jobs_prof{0};                     // emagls_jobs_set_profiling: the chunks' batches time their sweep launches
// A resident chunk's second run (the hipGraph capture of the stages around the sweep) has the job lists' share of the device to itself:
// captures next to other threads' uploads or launches ended in hipErrorStreamCaptureInvalidated ("operation failed due to a previous
// error during capture").  Every other run shares the lock.
std::shared_timed_mutex g_jobs_warm_mu;
uint64_t g_jobs_tick = 0;
std::atomic<size_t> g_jobs_resident_max{8 * REG_SWEEP_MAX};   // designs kept resident between calls (0.19 GB each at config 3); at least one call's chunks in flight

void check_rc(int rc) { if (rc != EMAGLS_OK) throw Error(rc, g_last_error); }
bool is_device_pointer(const void* p) {
    hipPointerAttribute_t at{};
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (plain host memory: not registered)
    return at.type == hipMemoryTypeDevice;
}
// what makes two designs share a lane batch: everything but the array radius inside one (padded) simulation-order class
void job_shape(const emagls_design_desc& d, std::string& out) {
    emagls_design_desc k = d;
    if (array_kind(d.kind) && d.sim_order_pad > 0) {
        const int own = smair_sim_order(d.kind == EMAGLS_KIND_EMAGLS2 ? SMAIR_DEFAULT_ORDER : d.order, d.fs, d.mic_radius);
        if (own <= d.sim_order_pad) k.mic_radius = 0.0;   // (laid out for sim_order_pad whatever the radius)
    }
    out.assign(reinterpret_cast<const char*>(&k), sizeof k);
}
// will the slot's next execute capture hipGraphs?  (the batch forms and plan_execute capture on the run after an eager one)
bool slot_will_capture(const JobSlot& s) {
    if (s.batch) {
        const emagls_batch& b = *s.batch;
        if (!b.use_graph || b.eager_runs < 1) return false;
        // a sharing batch of array designs captures each of its two forms the first time that form runs (batch_execute_geo)
        if (b.geo_share && !b.atf && !b.magls) return !b.post || !(batch_geo_next_is_warm(b) ? b.warm : b.group[0]);
        return !b.group[0] && !(b.plans.size() && b.plans[0]->pre);
    }
    for (const emagls_plan* p : s.plans)
        if (p->use_graph && p->prof_level == 0 && p->eager_runs >= 1 && !p->pre && !p->graph) return true;
    return false;
}
std::atomic<long long> g_jobs_geo_runs[3];   // chunk executes since emagls_cache_clear: independent designs, cold, warm (emagls_jobs_geometry_runs)
// The scheduler's own rule for sharing geometry (needs no device: descriptors and host grids alone): every job of the chunk has the same
// descriptor, byte for byte, of a kind batch_geo_decide_sharing accepts -- eMagLS / eMagLS2 / EMAinCH, at most 32 channels, no
// covariance constraint, built-in basis -- and the same grids.  The batch's comparison on the device stays the final word.
bool jobs_chunk_shares_geometry(const emagls_job* jobs, int n) {
    if (!jobs || n < 2) return false;
    const emagls_design_desc& d0 = jobs[0].desc;
    if (d0.kind != EMAGLS_KIND_EMAGLS && d0.kind != EMAGLS_KIND_EMAGLS2 && d0.kind != EMAGLS_KIND_EMA_CH) return false;
    if (d0.custom_basis || d0.diffuseness || d0.ndirs <= 0 || d0.nmics <= 0) return false;
    const int64_t ch = d0.kind == EMAGLS_KIND_EMAGLS2 ? d0.nmics : d0.kind == EMAGLS_KIND_EMA_CH ? 2 * (int64_t)d0.order + 1 : (int64_t)(d0.order + 1) * (d0.order + 1);
    if (ch > 32) return false;   // (the 33..64-channel path runs plan by plan: geo_keep)
    auto same = [](const double* a, const double* b, int64_t m) {
        if (a == b) return true;   // (also: both absent)
        return a && b && memcmp(a, b, sizeof(double) * (size_t)m) == 0;
    };
    if (!jobs[0].hrir_azi || !jobs[0].mic_azi) return false;
    for (int j = 1; j < n; ++j) {
        const emagls_job& x = jobs[j];
        if (memcmp(&x.desc, &d0, sizeof d0) != 0) return false;
        if (!same(x.hrir_azi, jobs[0].hrir_azi, d0.ndirs) || !same(x.hrir_zen, jobs[0].hrir_zen, d0.ndirs) ||
            !same(x.mic_azi, jobs[0].mic_azi, d0.nmics) || !same(x.mic_zen, jobs[0].mic_zen, d0.nmics)) return false;
    }
    return true;
}
void jobs_run_chunk(const emagls_job* jobs, int n, int device, int flags, bool solo, uint64_t call) {
    DeviceGuard dg(device);
    const bool trace = sw_on<Sw::JOBS_TRACE>();
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace) fprintf(stderr, "emagls jobs: chunk of %d, %s at %.3f ms\n", n, what,
                           std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    // (a list of ONE chunk has the device to itself: its batch runs the stages before the sweep as one lane group forked onto three
    // streams -- the independent branches of the pipeline side by side: 2160 against 2070 sets/s for a list of 20 config-3 designs --,
    // chunks that share the device with others as two single-stream lane groups: 3300 against 3140 sets/s at 512 designs)
    std::string key(solo ? "S" : "P"), shape(solo ? "S" : "P"), one;
    for (int j = 0; j < n; ++j) {
        key.append(reinterpret_cast<const char*>(&jobs[j].desc), sizeof(emagls_design_desc));
        job_shape(jobs[j].desc, one);
        shape.append(one);
    }
    std::unique_ptr<JobSlot> slot, recycled;
    {
        std::lock_guard<std::mutex> lk(g_jobs_mu);
        for (size_t i = 0; i < g_jobs_free.size(); ++i)
            if (g_jobs_free[i]->device == device && g_jobs_free[i]->key == key) { slot = std::move(g_jobs_free[i]); g_jobs_free.erase(g_jobs_free.begin() + i); break; }
        // no resident slot of these designs, but an idle one of the same SHAPE (other array radii of the same padded classes: the next
        // list of a radius study): its memory serves the new slot -- slabs and arena go back to the block pool and come out again at
        // exactly the sizes asked for.  Fresh device memory is what a new slot must not need: hipMalloc of a 4 GB arena took 0.3 ms on
        // some boxes and 0.5 s on others (the driver clears VRAM it hands out for the first time), 1 s per call of 28 new radii.
        if (!slot)
            for (size_t i = 0; i < g_jobs_free.size(); ++i)
                if (g_jobs_free[i]->device == device && g_jobs_free[i]->shape == shape && g_jobs_free[i]->last_call != call) {   // (not a chunk of THIS list: a repeat of the list finds all its chunks resident)
                    recycled = std::move(g_jobs_free[i]); g_jobs_free.erase(g_jobs_free.begin() + i); break;
                }
    }
    recycled.reset();   // (outside the lock: the destructor waits for the slot's streams)
    // a chunk shares the device with the other chunks in flight, except on its slot's SECOND run: that one captures the hipGraphs of the
    // stages around the sweep, and a capture next to another thread's uploads or launches is invalidated (hipErrorStreamCaptureInvalidated)
    // (decided from the objects' own state, not from the slot's run count: a batch whose graphs were dropped by a recovery --
    // drop_batch_graphs after a flagged bin or a lanes rebuild -- captures again on a later run)
    const bool was_resident = slot != nullptr;
    std::shared_lock<std::shared_timed_mutex> shared(g_jobs_warm_mu, std::defer_lock);
    std::unique_lock<std::shared_timed_mutex> alone(g_jobs_warm_mu, std::defer_lock);
    // (the exclusive lock only around the execute that captures: the uploads before it and the wait for the filters after it run next to
    // the other chunks -- a first call with host arrays spent 40 ... 140 ms per chunk uploading under the exclusive lock)
    shared.lock();
    if (!slot) {
        slot.reset(new JobSlot);
        slot->key = key; slot->shape = shape; slot->device = device;
        slot->grids.resize((size_t)n);
        slot->stream = emagls::pool_stream_take();
        struct SharedStream { SharedStream(hipStream_t st) { g_plan_stream_shared = st; } ~SharedStream() { g_plan_stream_shared = nullptr; } } shared_stream(slot->stream);
        for (int j = 0; j < n; ++j) {
            emagls_plan* p = nullptr;
            check_rc(emagls_plan_create(&jobs[j].desc, &p));
            slot->plans.push_back(p);
            if (j == 0) lap("first plan created");
        }
        lap("plans created");
    }
    for (int j = 0; j < n; ++j) {
        const emagls_job& jb = jobs[j];
        emagls_plan* p = slot->plans[(size_t)j];
        const emagls_design_desc& d = jb.desc;
        // grids (host arrays): uploaded when they differ from what the plan holds
        std::vector<double> g;
        auto app = [&](const double* a, int64_t m) { if (a) g.insert(g.end(), a, a + m); else g.push_back(-1e300); };
        const bool has_mics = array_kind(d.kind);
        app(jb.hrir_azi, d.ndirs); app(jb.hrir_zen, d.ndirs);
        if (has_mics) { app(jb.mic_azi, d.nmics); app(jb.mic_zen, d.nmics); }
        if (g != slot->grids[(size_t)j]) {
            if (!jb.hrir_azi) throw Error(EMAGLS_ERR_ARG, "job without an HRIR grid");
            check_rc(emagls_plan_set_hrir_grid(p, jb.hrir_azi, jb.hrir_zen));
            if (has_mics) {
                if (!jb.mic_azi) throw Error(EMAGLS_ERR_ARG, "array design without a microphone grid");
                check_rc(emagls_plan_set_mic_grid(p, jb.mic_azi, jb.mic_zen));
            }
            slot->grids[(size_t)j] = std::move(g);
        }
        if (d.kind == EMAGLS_KIND_FROM_ATF) {
            if (!jb.atf || !jb.atf_azi || !jb.atf_zen) throw Error(EMAGLS_ERR_ARG, "FromAtf job without its ATF set");
            check_rc(emagls_plan_set_atfs(p, jb.atf, jb.atf_azi, jb.atf_zen));
        }
        if (!jb.hL || !jb.hR || !jb.wL || !jb.wR) throw Error(EMAGLS_ERR_ARG, "job without HRIRs or without room for its filters");
        if (!slot->batch && n > 1 && !slot->runs) check_rc(emagls_plan_set_hrirs(p, jb.hL, jb.hR));   // (before the batch exists: plan by plan)
    }
    lap("inputs set");
    if (n > 1 && !slot->batch && !slot->runs) {
        int rc;
        { Scoped limit(g_batch_max_override, REG_SWEEP_MAX); rc = emagls_batch_create(slot->plans.data(), n, &slot->batch); }
        if (rc != EMAGLS_OK && rc != EMAGLS_ERR_UNSUPPORTED) check_rc(rc);   // (unsupported as a batch -- e.g. more than 32 channels: plan by plan)
        if (rc != EMAGLS_OK) slot->batch = nullptr;
        if (slot->batch && solo && slot->batch->lanes) {
            if (const int fork = sw_int<Sw::JOBS_FORK>(); fork >= 2) {
                if (slot->batch->groups != 1) { HIP_CHECK(hipStreamSynchronize(slot->batch->stream)); drop_batch_graphs(*slot->batch); slot->batch->groups = 1; }
                check_rc(emagls_batch_set_streams(slot->batch, fork));
            }
        }
        if (slot->batch) {
            slot->batch->alone = solo;   // (chunks in flight next to each other keep the orthonormal route before their sweeps: batch_defers_hh)
            if (!solo && slot->batch->group[0]) { HIP_CHECK(hipStreamSynchronize(slot->batch->stream)); drop_batch_graphs(*slot->batch); }
        }
        lap("batch created");
    } else if (slot->batch) {
        // the HRIRs of every design on the batch's stream, ordered before its execute: no host synchronisation per plan
        // (jobs that name the SAME HRIR arrays -- one HRIR set for every radius of an array sweep -- are served device to device from
        // the first plan that received them: 5.5 MB over PCIe instead of 5.5 MB per design from pageable memory)
        // inputs that already lie in device memory: ONE gather launch for the whole chunk (hipMemcpyAsync per buffer otherwise)
        bool gathered = false;
        if (2 * n <= 64) {
            bool all_dev = true;
            for (int j = 0; j < n && all_dev; ++j) all_dev = is_device_pointer(jobs[j].hL) && is_device_pointer(jobs[j].hR);
            if (all_dev) {
                LanePtrs src{}, dst{};
                const emagls_plan& q0 = *slot->plans[0];
                const size_t bytes = sizeof(double) * (size_t)q0.d.nsamp * (size_t)q0.d.ndirs;
                for (int j = 0; j < n; ++j) {
                    emagls_plan& q = *slot->plans[(size_t)j];
                    src.p[2 * j] = const_cast<double*>(jobs[j].hL); src.p[2 * j + 1] = const_cast<double*>(jobs[j].hR);
                    dst.p[2 * j] = q.get("hL"); dst.p[2 * j + 1] = q.get("hR");
                    q.have_hrirs = true;
                }
                launch_gather_buffers(src, dst, 2 * n, bytes, slot->batch->stream);
                gathered = true;
            }
        }
        for (int j = 0; j < n && !gathered; ++j) {
            emagls_plan& q = *slot->plans[(size_t)j];
            const size_t bytes = sizeof(double) * (size_t)q.d.nsamp * (size_t)q.d.ndirs;
            int src = -1;
            for (int i = 0; i < j && src < 0; ++i)
                if (jobs[i].hL == jobs[j].hL && jobs[i].hR == jobs[j].hR && slot->plans[(size_t)i]->d.nsamp == q.d.nsamp && slot->plans[(size_t)i]->d.ndirs == q.d.ndirs) src = i;
            const void* sl = src >= 0 ? slot->plans[(size_t)src]->get("hL") : jobs[j].hL;
            const void* sr = src >= 0 ? slot->plans[(size_t)src]->get("hR") : jobs[j].hR;
            HIP_CHECK(hipMemcpyAsync(q.get("hL"), sl, bytes, hipMemcpyDefault, slot->batch->stream));
            HIP_CHECK(hipMemcpyAsync(q.get("hR"), sr, bytes, hipMemcpyDefault, slot->batch->stream));
            q.have_hrirs = true;
        }
    } else {
        for (int j = 0; j < n; ++j) check_rc(emagls_plan_set_hrirs(slot->plans[(size_t)j], jobs[j].hL, jobs[j].hR));
    }
    if (slot->batch) {
        // HRIR sets on one geometry: the geometry stages once per chunk, and kept by the chunk's batch between runs (batch_execute_geo).
        // Decided here without being asked (jobs_chunk_shares_geometry: EMAGLS_JOBS_INDEPENDENT / EMAGLS_JOBS_AUTO_SHARE=0 switch that
        // off); with EMAGLS_JOBS_SHARE_GEOMETRY the batch is asked whatever the rule says (MagLS / LS sets on one grid).  Either way the
        // library compares the grids on the device, and a chunk whose designs do not agree runs them as independent designs.
        const int kind = jobs[0].desc.kind;
        bool want = false;
        if (flags & EMAGLS_JOBS_SHARE_GEOMETRY) want = kind != EMAGLS_KIND_FROM_ATF && kind != EMAGLS_KIND_EMA_SH;
        else if (sw_on<Sw::JOBS_AUTO_SHARE>() && !(flags & EMAGLS_JOBS_INDEPENDENT)) want = jobs_chunk_shares_geometry(jobs, n);
        // (only when it changes: the call makes the batch compare its grids again and run its geometry stages again)
        if (want != slot->batch->geo_want) check_rc(emagls_batch_set_geometry_sharing(slot->batch, want ? 1 : 0));
    }
    // (designs of the 33..64-channel path run plan by plan: with the flag a plan keeps its geometry stages from its last clean run while
    // its own grids stay the same -- plan_execute)
    if (!slot->batch) for (auto* q : slot->plans) q->geo_keep = (flags & EMAGLS_JOBS_SHARE_GEOMETRY) != 0;
    // (decided here, from the objects' state AFTER this run's grids and sharing switch are in: a replaced grid takes a sharing batch back
    // to its cold form, whose graph may not exist yet)
    const bool capturing = was_resident && slot_will_capture(*slot);
    {
        if (slot->batch) {
            std::vector<void*> wl((size_t)n), wr((size_t)n);
            for (int j = 0; j < n; ++j) { wl[(size_t)j] = jobs[j].wL; wr[(size_t)j] = jobs[j].wR; }
            if (slot->batch->prof_level != g_jobs_prof.load()) check_rc(emagls_batch_set_profiling(slot->batch, g_jobs_prof.load()));
            if (capturing) { shared.unlock(); alone.lock(); }
            check_rc(emagls_batch_execute(slot->batch));
            if (capturing) { alone.unlock(); shared.lock(); }
            ++g_jobs_geo_runs[slot->batch->last_form];
            check_rc(emagls_batch_get_filters(slot->batch, wl.data(), wr.data()));
        } else {
            ++g_jobs_geo_runs[0];
            if (capturing) { shared.unlock(); alone.lock(); }
            for (int j = 0; j < n; ++j) check_rc(emagls_plan_execute(slot->plans[(size_t)j]));
            if (capturing) { alone.unlock(); shared.lock(); }
            for (int j = 0; j < n; ++j) check_rc(emagls_plan_get_filters(slot->plans[(size_t)j], jobs[j].wL, jobs[j].wR));
        }
        ++slot->runs;
    }
    lap("executed and collected");
    // keep the slot when its designs can serve another chunk as they are
    std::lock_guard<std::mutex> lk(g_jobs_mu);
    slot->last_use = ++g_jobs_tick;
    slot->last_call = call;
    g_jobs_free.push_back(std::move(slot));
    size_t resident = 0;
    for (auto& f : g_jobs_free) resident += f->plans.size();
    while (resident > g_jobs_resident_max.load() && g_jobs_free.size() > 1) {   // least recently used first
        size_t old = 0;
        for (size_t i = 1; i < g_jobs_free.size(); ++i) if (g_jobs_free[i]->last_use < g_jobs_free[old]->last_use) old = i;
        resident -= g_jobs_free[old]->plans.size();
        g_jobs_free.erase(g_jobs_free.begin() + old);
    }
}
}  // namespace
void emagls_jobs_cache_clear_internal() {
    std::lock_guard<std::mutex> lk(g_jobs_mu);
    g_jobs_free.clear();
    for (auto& c : g_jobs_geo_runs) c.store(0);
}
int emagls_jobs_geometry_runs(long long* independent, long long* cold, long long* warm) {
    return guarded([&] {
        if (!independent || !cold || !warm) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *independent = g_jobs_geo_runs[0].load(); *cold = g_jobs_geo_runs[1].load(); *warm = g_jobs_geo_runs[2].load();
    });
}
int emagls_jobs_would_share_geometry(const emagls_job* jobs, int njobs, int* share) {
    return guarded([&] {
        if (!jobs || !share || njobs < 0) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        *share = jobs_chunk_shares_geometry(jobs, njobs) ? 1 : 0;
    });
}

int emagls_jobs_set_profiling(int level) {
    return guarded([&] { g_jobs_prof.store(level > 0 ? 1 : 0); });
}
int emagls_jobs_sweep_times(double* ms, int* designs, int capacity, int* count) {
    return guarded([&] {
        if (!count || capacity < 0 || (capacity > 0 && (!ms || !designs))) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        std::lock_guard<std::mutex> lk(g_jobs_mu);
        int n = 0;
        for (auto& f : g_jobs_free) {
            if (!f->batch || f->batch->prof_level < 1 || !f->batch->sweep_ev[0] || f->batch->eager_runs < 1) continue;
            if (n < capacity) {
                DeviceGuard dg(f->device);
                float t = 0.f;
                if (hipEventElapsedTime(&t, f->batch->sweep_ev[0], f->batch->sweep_ev[1]) != hipSuccess) { (void)hipGetLastError(); continue; }
                ms[n] = t; designs[n] = (int)f->plans.size();
            }
            ++n;
        }
        *count = n;
    });
}

int emagls_jobs_run(const emagls_job* jobs, int64_t njobs, int batch_size, int in_flight, int flags) {
    return guarded([&] {
        if (!jobs || njobs < 0) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        if (njobs == 0) return;
        if (batch_size <= 0) batch_size = REG_SWEEP_MAX;
        if (in_flight <= 0) in_flight = 4;
        batch_size = std::min(batch_size, REG_SWEEP_MAX);
        g_jobs_resident_max.store(std::max((size_t)8 * REG_SWEEP_MAX, (size_t)2 * batch_size * (size_t)in_flight));   // (EMAGLS_JOBS_RESIDENT overrides)
        if (const int v = sw_int<Sw::JOBS_RESIDENT>(); v > 0) g_jobs_resident_max.store((size_t)v);
        int device = 0;
        HIP_CHECK(hipGetDevice(&device));
        // chunks: consecutive jobs of one shape; more than 16 designs per chunk only where the register-resident sweep takes them
        // (array designs on the built-in basis; decided when the batch is created: a refused batch of 17 ... 32 is an error the caller
        // avoids by asking for batches of 16)
        std::vector<std::pair<int64_t, int>> chunks;
        for (int64_t first = 0; first < njobs;) {
            std::string shape, other;
            job_shape(jobs[first].desc, shape);
            int cap = array_kind(jobs[first].desc.kind) && !jobs[first].desc.custom_basis && !jobs[first].desc.diffuseness ? batch_size
                                                                                                                            : std::min(batch_size, SWEEP_MULTI_MAX);
            // HRIR sets on one geometry on the 33..64-channel path (plan by plan, gigabytes per plan): one design per chunk, so that the sets
            // pass through `in_flight` plans which keep their geometry stages (plan_execute) instead of one plan per set
            {
                const emagls_design_desc& d0 = jobs[first].desc;
                const int64_t ch = d0.kind == EMAGLS_KIND_EMAGLS2 ? d0.nmics : (int64_t)(d0.order + 1) * (d0.order + 1);
                if ((flags & EMAGLS_JOBS_SHARE_GEOMETRY) && (d0.kind == EMAGLS_KIND_EMAGLS || d0.kind == EMAGLS_KIND_EMAGLS2) && ch > 32) cap = 1;
            }
            int n = 1;
            while (first + n < njobs && n < cap && (job_shape(jobs[first + n].desc, other), other == shape)) ++n;
            chunks.emplace_back(first, n);
            first += n;
        }
        static std::atomic<uint64_t> g_jobs_call{0};
        const uint64_t call = ++g_jobs_call;
        // workers: each takes the next chunk until none is left; the first error stops the hand-out and is reported
        std::atomic<size_t> next{0};
        std::mutex err_mu;
        int err_code = EMAGLS_OK;
        std::string err_msg;
        auto work = [&] {
            for (;;) {
                const size_t c = next.fetch_add(1);
                if (c >= chunks.size()) return;
                {
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (err_code != EMAGLS_OK) return;
                }
                try {
                    try {
                        jobs_run_chunk(jobs + chunks[c].first, chunks[c].second, device, flags, chunks.size() == 1, call);
                    } catch (const Error& e) {
                        // a chunk of 17 ... 32 designs whose sweep stopped being the register-resident form (a recovery moved it to
                        // the slab or launch-per-bin forms, which hold 16 designs): the same designs as two chunks of at most 16
                        if (chunks[c].second <= SWEEP_MULTI_MAX || e.code != EMAGLS_ERR_UNSUPPORTED || !strstr(e.what(), "more than 16 designs")) throw;
                        const int h = (chunks[c].second + 1) / 2;
                        jobs_run_chunk(jobs + chunks[c].first, h, device, flags, false, call);
                        jobs_run_chunk(jobs + chunks[c].first + h, chunks[c].second - h, device, flags, false, call);
                    }
                } catch (const Error& e) {
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (err_code == EMAGLS_OK) { err_code = e.code; err_msg = e.what(); }
                } catch (const std::exception& e) {
                    std::lock_guard<std::mutex> lk(err_mu);
                    if (err_code == EMAGLS_OK) { err_code = EMAGLS_ERR_HIP; err_msg = e.what(); }
                }
            }
        };
        const int nthreads = (int)std::min<size_t>((size_t)in_flight, chunks.size());
        std::vector<std::thread> th;
        for (int t = 1; t < nthreads; ++t) th.emplace_back(work);
        work();
        for (auto& t : th) t.join();
        if (err_code != EMAGLS_OK) throw Error(err_code, err_msg);
    });
}
// ---------------------------------------------------------------------------------------------
// Job lists over several GPUs at the C boundary: the split of emagls_amd/batch.py restated in C, and a runner that
// drives the devices of ONE process from a thread each -- what a MEX caller (one MATLAB process) or any C host has without
// torch.distributed.  One process per GPU with an RCCL gather is the other form (emagls_amd/batch.py; INTEGRATION.md shows both).
// ---------------------------------------------------------------------------------------------
namespace {
// run time model of one lane batch of n designs laid out for sim_order (emagls_amd/batch.py: batch_cost, measured in round 4)
double shard_batch_cost(int n, int sim_order) {
    const double S = (double)(sim_order + 1) * (sim_order + 1), g = n / 8.0;
    if (sim_order < 19) return 5.6 + 7.2 * g;
    return (6.4 + 2.4 * g) + (1.67 + 1.93 * g) * 1e-3 * S;
}
// emagls_amd/batch.py: padded_lane_batches(sim_orders, max_batch, balance=True) -- consecutive chunks of the jobs sorted by simulation
// order, cut at equal COST; returns (first, size) into `order`
std::vector<std::pair<int, int>> shard_padded_batches(const std::vector<int>& so_sorted, int max_batch) {
    const int n = (int)so_sorted.size();
    const int nb = (n + max_batch - 1) / max_batch;
    std::vector<std::pair<int, int>> out;
    if (nb <= 1) { out.emplace_back(0, n); return out; }
    auto cut = [&](double T, std::vector<std::pair<int, int>>& chunks) {
        chunks.clear();
        int pos = 0;
        while (pos < n) {
            if (shard_batch_cost(1, so_sorted[pos]) > T) return false;
            int size = 1;
            while (pos + size < n && size < 32 && shard_batch_cost(size + 1, so_sorted[pos + size]) <= T) ++size;
            chunks.emplace_back(pos, size);
            pos += size;
        }
        return true;
    };
    double lo = 0.0, hi = shard_batch_cost(32, so_sorted.back()) + 1.0;
    std::vector<std::pair<int, int>> c;
    for (int it = 0; it < 40; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (cut(mid, c) && (int)c.size() <= nb) hi = mid; else lo = mid;
    }
    cut(hi, out);
    return out;
}
struct ShardUnit { std::vector<int> jobs; int pad = 0; double cost = 1.0; };
// the units of a list (lane batches of array-radius families, single jobs otherwise) in list order of their first job
void shard_units(const emagls_job* jobs, int64_t njobs, int max_batch, std::vector<ShardUnit>& units) {
    // families: everything but the array radius (and the padding) equal
    std::map<std::string, std::vector<int>> fam;
    std::vector<std::string> fam_order;
    for (int64_t j = 0; j < njobs; ++j) {
        emagls_design_desc k = jobs[j].desc;
        const bool radius_family = (k.kind == EMAGLS_KIND_EMAGLS || k.kind == EMAGLS_KIND_EMAGLS2 || k.kind == EMAGLS_KIND_EMA_CH) && !k.custom_basis && k.nmics <= 32;
        if (radius_family) { k.mic_radius = 0.0; k.sim_order_pad = 0; }
        std::string key(reinterpret_cast<const char*>(&k), sizeof k);
        key.push_back(radius_family ? 'R' : 'E');
        if (!fam.count(key)) fam_order.push_back(key);
        fam[key].push_back((int)j);
    }
    for (const std::string& key : fam_order) {
        const std::vector<int>& idx = fam[key];
        if (key.back() == 'R' && idx.size() > 1) {
            std::vector<int> order(idx.size());
            for (size_t i = 0; i < idx.size(); ++i) order[i] = (int)i;
            auto so_of = [&](int i) { const emagls_design_desc& d = jobs[idx[(size_t)i]].desc; return emagls_simulation_order(d.kind, d.order, d.fs, d.mic_radius); };
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return so_of(a) < so_of(b); });
            std::vector<int> so_sorted(order.size());
            for (size_t i = 0; i < order.size(); ++i) so_sorted[i] = so_of(order[i]);
            if (so_sorted.front() == so_sorted.back()) {   // one simulation-order class: equal jobs, a unit each (the library cuts a rank's share into chunks)
                for (int j : idx) { ShardUnit u; u.jobs.push_back(j); u.cost = 1.0; units.push_back(std::move(u)); }
                continue;
            }
            for (auto& fs : shard_padded_batches(so_sorted, max_batch)) {
                ShardUnit u;
                for (int i = fs.first; i < fs.first + fs.second; ++i) { u.jobs.push_back(idx[(size_t)order[(size_t)i]]); u.pad = std::max(u.pad, so_sorted[(size_t)i]); }
                u.cost = shard_batch_cost((int)u.jobs.size(), u.pad);
                units.push_back(std::move(u));
            }
        } else {
            for (int j : idx) { ShardUnit u; u.jobs.push_back(j); u.cost = 1.0; units.push_back(std::move(u)); }
        }
    }
}
}  // namespace

int emagls_jobs_shard(const emagls_job* jobs, int64_t njobs, int world, int max_batch, int* rank_of_job, int* order_in_rank, int* sim_order_pad) {
    return guarded([&] {
        if (!jobs || njobs < 0 || world < 1 || !rank_of_job) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        if (max_batch <= 0) max_batch = 16;
        if (max_batch > 32) throw Error(EMAGLS_ERR_ARG, "a batch holds 1..32 designs");
        std::vector<ShardUnit> units;
        shard_units(jobs, njobs, max_batch, units);
        // whole units to ranks by longest processing time (ties: the earlier unit, the lower rank), cheapest first inside a rank
        std::vector<int> by_cost(units.size());
        for (size_t i = 0; i < units.size(); ++i) by_cost[i] = (int)i;
        std::stable_sort(by_cost.begin(), by_cost.end(), [&](int a, int b) { return units[(size_t)a].cost > units[(size_t)b].cost; });
        std::vector<double> load((size_t)world, 0.0);
        std::vector<std::vector<int>> mine((size_t)world);
        for (int u : by_cost) {
            int r = 0;
            for (int q = 1; q < world; ++q) if (load[(size_t)q] < load[(size_t)r]) r = q;
            mine[(size_t)r].push_back(u);
            load[(size_t)r] += units[(size_t)u].cost;
        }
        for (int r = 0; r < world; ++r) {
            std::stable_sort(mine[(size_t)r].begin(), mine[(size_t)r].end(), [&](int a, int b) {
                return units[(size_t)a].cost < units[(size_t)b].cost || (units[(size_t)a].cost == units[(size_t)b].cost && a < b); });
            int pos = 0;
            for (int u : mine[(size_t)r])
                for (int j : units[(size_t)u].jobs) {
                    rank_of_job[j] = r;
                    if (order_in_rank) order_in_rank[j] = pos;
                    if (sim_order_pad) sim_order_pad[j] = units[(size_t)u].pad;
                    ++pos;
                }
        }
    });
}

int emagls_jobs_run_devices(const emagls_job* jobs, int64_t njobs, const int* devices, int ndevices, int batch_size, int in_flight, int flags) {
    return guarded([&] {
        if (!jobs || njobs < 0 || !devices || ndevices < 1) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        int avail = 0;
        HIP_CHECK(hipGetDeviceCount(&avail));
        for (int i = 0; i < ndevices; ++i) if (devices[i] < 0 || devices[i] >= avail) throw Error(EMAGLS_ERR_ARG, "no such device");
        if (njobs == 0) return;
        std::vector<int> rank((size_t)njobs), pos((size_t)njobs), pad((size_t)njobs);
        check_rc(emagls_jobs_shard(jobs, njobs, ndevices, std::min(batch_size > 0 ? batch_size : 16, 16), rank.data(), pos.data(), pad.data()));
        // every device's share as a list of its own (jobs of one lane batch adjacent, laid out for the batch's simulation order)
        std::vector<std::vector<emagls_job>> share((size_t)ndevices);
        for (int r = 0; r < ndevices; ++r) {
            int64_t cnt = 0;
            for (int64_t j = 0; j < njobs; ++j) cnt += rank[(size_t)j] == r;
            share[(size_t)r].resize((size_t)cnt);
        }
        for (int64_t j = 0; j < njobs; ++j) {
            emagls_job jb = jobs[j];
            if (pad[(size_t)j] > 0 && jb.desc.sim_order_pad == 0) jb.desc.sim_order_pad = pad[(size_t)j];
            share[(size_t)rank[(size_t)j]][(size_t)pos[(size_t)j]] = jb;
        }
        std::vector<int> rc((size_t)ndevices, EMAGLS_OK);
        std::vector<std::string> msg((size_t)ndevices);
        auto work = [&](int r) {
            if (share[(size_t)r].empty()) return;
            if (hipSetDevice(devices[r]) != hipSuccess) { rc[(size_t)r] = EMAGLS_ERR_HIP; msg[(size_t)r] = "hipSetDevice failed"; return; }
            rc[(size_t)r] = emagls_jobs_run(share[(size_t)r].data(), (int64_t)share[(size_t)r].size(), batch_size > 0 ? batch_size : 32, in_flight, flags);
            if (rc[(size_t)r] != EMAGLS_OK) msg[(size_t)r] = g_last_error;   // (thread-local: this thread's)
        };
        std::vector<std::thread> th;
        for (int r = 1; r < ndevices; ++r) th.emplace_back(work, r);
        int keep = 0;
        HIP_CHECK(hipGetDevice(&keep));
        work(0);
        for (auto& t : th) t.join();
        HIP_CHECK(hipSetDevice(keep));
        for (int r = 0; r < ndevices; ++r)
            if (rc[(size_t)r] != EMAGLS_OK) throw Error(rc[(size_t)r], "device " + std::to_string(devices[r]) + ": " + msg[(size_t)r]);
    });
}

int emagls_from_atf_hrir_sets(const double* hL, const double* hR, int64_t nsamp, int64_t ndirs, int64_t nsets, const double* hrir_azi,
                              const double* hrir_zen, const double* atf_irs, int64_t atf_taps, int64_t nmics, int64_t natf, const double* atf_azi,
                              const double* atf_zen, double fs, int64_t filter_len, double f_trans, double* wL, double* wR, double* mean_dev) {
    return guarded([&] {
        if (!hL || !hR || !hrir_azi || !hrir_zen || !atf_irs || !atf_azi || !atf_zen || !wL || !wR || nsets < 1) throw Error(EMAGLS_ERR_ARG, "invalid argument");
        emagls_design_desc d{};
        d.kind = EMAGLS_KIND_FROM_ATF; d.basis = EMAGLS_BASIS_REAL; d.fs = fs; d.len = filter_len; d.nsamp = nsamp; d.ndirs = ndirs;
        d.nmics = nmics; d.f_trans = f_trans; d.atf_taps = atf_taps; d.natf = natf;
        auto req = [](int r) { if (r != EMAGLS_OK) throw Error(r, g_last_error); };
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(g_atfsets_mu);
        const size_t out_bytes = sizeof(double) * (size_t)filter_len * (size_t)nmics;
        for (int64_t first = 0; first < nsets;) {
            const int n = (int)std::min<int64_t>(SWEEP_MULTI_MAX, nsets - first);
            const int slot = n == SWEEP_MULTI_MAX ? 0 : 1;
            SetsCache* c = &g_atfsets[slot];
            if (!(c->n == n && c->device == dev && same_desc(c->desc, d))) {
                c->release();
                try {
                    for (int j = 0; j < n; ++j) {
                        emagls_plan* p = nullptr;
                        req(emagls_plan_create(&d, &p));
                        c->plans.push_back(p);
                    }
                    if (n > 1) {
                        int r;
                        { Scoped limit(g_batch_max_override, SWEEP_MULTI_MAX); r = emagls_batch_create(c->plans.data(), n, &c->batch); }
                        req(r);
                    }
                } catch (...) { c->release(); throw; }
                c->desc = d; c->device = dev; c->n = n;
            }
            try {
                // the ATF set and the grids: host -> plan 0, plan 0 -> the others on the device (the set is 268 MB at config 5)
                emagls_plan* p0 = c->plans[0];
                req(emagls_plan_set_hrir_grid(p0, hrir_azi, hrir_zen));
                req(emagls_plan_set_atfs(p0, atf_irs, atf_azi, atf_zen));
                for (int j = 1; j < n; ++j) {
                    emagls_plan* p = c->plans[(size_t)j];
                    for (const char* name : {"atf", "atf_azi", "atf_zen", "hrir_azi", "hrir_zen"})
                        HIP_CHECK(hipMemcpyAsync(p->get(name), p0->get(name), p0->bufs[name].bytes, hipMemcpyDeviceToDevice, p0->stream));
                    p->have_atfs = true; p->have_hrir_grid = true;
                    ++p->atf_side_version;
                }
                HIP_CHECK(hipStreamSynchronize(p0->stream));
                for (int j = 0; j < n; ++j)
                    req(emagls_plan_set_hrirs(c->plans[(size_t)j], hL + (first + j) * nsamp * ndirs, hR + (first + j) * nsamp * ndirs));
                if (n == 1) {
                    req(emagls_plan_execute(p0));
                    req(emagls_plan_get_filters(p0, (char*)wL + first * out_bytes, (char*)wR + first * out_bytes));
                } else {
                    std::vector<void*> pl((size_t)n), pr((size_t)n);
                    for (int j = 0; j < n; ++j) { pl[(size_t)j] = (char*)wL + (first + j) * out_bytes; pr[(size_t)j] = (char*)wR + (first + j) * out_bytes; }
                    req(emagls_batch_execute(c->batch));
                    req(emagls_batch_get_filters(c->batch, pl.data(), pr.data()));
                }
                if (mean_dev) {
                    emagls_plan_info info;
                    req(emagls_plan_get_info(p0, &info));
                    *mean_dev = info.mean_grid_dev_deg;
                }
            } catch (...) { c->release(); throw; }
            first += n;
        }
    });
}

}  // extern "C"
