// Internal header of the host translation units (host_pools.hip, plan_setup.hip, plan_run.hip, batch_run.hip, capi.hip, jobs.hip): the
// plan and batch structs, the pools they draw from, and the declarations of what one of these files calls in another.  The array
// model's scalars and shared host sequences come with array_model.hpp.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/emagls.h"
#include "array_model.hpp"
#include "device_mem.hpp"
#include "kernels.hpp"

using namespace emagls;

struct emagls_batch;
void emagls_batch_forget(emagls_batch* b, emagls_plan* p);

namespace emagls {

constexpr int NFFT_MAX_LEN = 2048;      // lib/getEMagLsFilters.m:35
constexpr double F_CUT_MIN_FREQ = 1e3;  // :36
constexpr double SVD_REGUL_CONST = 0.01;  // :39
constexpr int NFLAG = 8;                   // device-side status words of a design (plan_recover)
constexpr int SMAIR_DEFAULT_ORDER = 4;    // dependencies/getSMAIRMatrix.m:39-41 (params.order when the caller leaves it unset)

// ---- defined in host_pools.hip
extern thread_local std::string g_last_error;   // what emagls_last_error() returns: written by guarded_call only
void trace_mark(const char* what);

// Streams are recycled through a process-wide pool and never destroyed.  A design plan owns three and a long session creates
// and drops hundreds of plans (one-shot cache evictions, radius sweeps).  Under the HIP 7.0 runtime that torch bundles, a
// multi-stream graph capture on stream handles the runtime had recycled after many hipStreamDestroy calls produced a graph
// whose hipGraphLaunch dereferenced a null pointer (reproduced: tests/test_gpu_config4.py followed by test_gpu_parity.py, crash
// in the third custom-basis one-shot call; gone with the pool, and gone with single-stream capture).
struct StreamPool {
    std::mutex mu;
    std::map<int, std::vector<hipStream_t>> idle;   // per device
    static StreamPool& get() { static StreamPool* p = new StreamPool; return *p; }   // (never destroyed: outlives every plan)
    hipStream_t take() {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        {   // The first streams a process creates each open a hardware queue of their own (GPU_MAX_HW_QUEUES = 4), later ones share
            // those queues.  Since round 6 a job chunk's plans no longer take four streams each (hipStreamCreate was 3 ms of a plan's
            // set-up), so a lone chunk's batch would fork its stages onto exactly those first streams -- and ran 8 % slower that way
            // (2400-2470 against 2590-2670 sets/s at 20 steps, A/B on one box, profiles/r06_stream_warm.md; any number of parked streams
            // from 4 to 80 restores it).  So the pool parks 8 streams before it hands the first one out (EMAGLS_STREAM_WARM=n; 0: none).
            const int warm = sw_int<Sw::STREAM_WARM>();
            static std::once_flag once;
            if (warm > 0) std::call_once(once, [&] {
                std::lock_guard<std::mutex> lk(mu);
                for (int i = 0; i < warm; ++i) { hipStream_t st = nullptr; if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess) idle[dev].push_back(st); }
            });
        }
        if (sw_on<Sw::STREAM_POOL>()) {
            std::lock_guard<std::mutex> lk(mu);
            auto& v = idle[dev];
            if (!v.empty()) { hipStream_t st = v.back(); v.pop_back(); return st; }
        }
        hipStream_t st = nullptr;
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return st;
    }
    void give(hipStream_t st) {
        if (!st) return;
        if (!sw_on<Sw::STREAM_POOL>()) { hipStreamDestroy(st); return; }
        hipStreamSynchronize(st);
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) { hipStreamDestroy(st); return; }
        std::lock_guard<std::mutex> lk(mu);
        idle[dev].push_back(st);
    }
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool owned = false;   // allocated on its own (hipFree when dropped); false once a batch moved it into its arena
};
// Device memory of plans (slabs) and batches (arenas) comes from a process-wide pool of blocks that are handed back instead of freed:
// a job list whose plans live for one chunk each otherwise pays hipMalloc / hipFree of ~0.35 GB per design again and again (and
// the calls were erratic next to running kernels: 30 ms ... 1.6 s for the plans of one chunk).  emagls_cache_clear() frees the pool;
// EMAGLS_POOL_GB (default 128) bounds what it keeps.
struct BlockPool {
    std::mutex mu;
    std::map<int, std::multimap<size_t, void*>> free_;   // device -> size -> block
    size_t held = 0;
    static BlockPool& get() { static BlockPool* p = new BlockPool; return *p; }   // (never destroyed: plans of static caches hand their blocks back at exit)
    static size_t cap() {
        // (128 GB of the 288: a rank's share of BASELINE config 4 holds two arenas of 21 GB -- the small radii keep materialised
        // operands, 1.5 GB per design -- plus as much again in released plan slabs while the next chunks are being built; with 64 GB the
        // arenas were freed and every list of new radii allocated them afresh, 0.3 ms ... 5 s per hipMalloc)
        return (size_t)sw_int<Sw::POOL_GB>() << 30;
    }
    // Sizes of large blocks (batch arenas: gigabytes) come in classes -- multiples of an eighth of the power of two below them -- so that
    // the arenas of similar chunks (other array radii: routes, hence buffer sizes, a few per cent apart) are the SAME size and one
    // chunk's released arena serves the next exactly.  Fresh device memory is what a new chunk must not need: hipMalloc of a 4 GB arena
    // took 0.3 ms on one box and 0.5 ... 2.9 s next to running kernels on others (profiles/r06_cold_path.md).
    static size_t size_class(size_t bytes) {
        size_t step = (size_t)64 << 20;
        while (step * 16 <= bytes) step *= 2;
        return (bytes + step - 1) / step * step;
    }
    // a block of at least `bytes` (exactly `bytes` when it has to be allocated); *got = its size
    // (alloc_bytes: what a miss allocates -- an arena asks for a block that holds its need and, when there is none, allocates the size
    // class of an eighth more: the next list's need, a few per cent larger, then fits the block this one hands back)
    void* take(size_t bytes, size_t* got, size_t alloc_bytes = 0) {
        if (alloc_bytes < bytes) alloc_bytes = bytes;
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        {
            std::lock_guard<std::mutex> lk(mu);
            auto& fl = free_[dev];
            auto it = fl.lower_bound(bytes);
            // (the smallest block that is large enough, up to a quarter larger -- half larger for the gigabyte-sized arenas, whose need
            // moves by a few per cent from one list of array radii to the next: fresh device memory for 2 x 4.5 GB took 3.6 s there)
            if (it != fl.end() && it->first <= bytes + (bytes >= ((size_t)1 << 30) ? bytes / 2 : bytes / 4)) {
                void* p = it->second;
                *got = it->first;
                held -= it->first;
                fl.erase(it);
                return p;
            }
        }
        void* p = nullptr;
        const auto t_alloc0 = std::chrono::steady_clock::now();
        hipError_t e = hipMalloc(&p, alloc_bytes);
        if (sw_on<Sw::JOBS_TRACE>() && alloc_bytes >= ((size_t)256 << 20)) {
            std::lock_guard<std::mutex> lk(mu);
            std::string have;
            for (auto& kv : free_[dev]) if (kv.first >= ((size_t)256 << 20)) have += " " + std::to_string(kv.first >> 20);
            fprintf(stderr, "emagls trace: block pool miss: need %zu MB, hipMalloc of %zu MB took %.1f ms; large blocks in the pool (MB):%s\n", bytes >> 20, alloc_bytes >> 20,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_alloc0).count(), have.c_str());
        }
        if (e == hipErrorOutOfMemory) {   // the pool may hold gigabytes of blocks of other sizes: return them to the runtime and try once more
            (void)hipGetLastError();
            clear();
            e = hipMalloc(&p, alloc_bytes);
        }
        HIP_CHECK(e);
        *got = alloc_bytes;
        return p;
    }
    void give(void* p, size_t bytes) {
        if (!p) return;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); hipFree(p); return; }
        std::lock_guard<std::mutex> lk(mu);
        if (held + bytes > cap()) { hipFree(p); return; }
        free_[dev].emplace(bytes, p);
        held += bytes;
    }
    void clear() {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& d : free_) for (auto& kv : d.second) hipFree(kv.second);
        free_.clear();
        held = 0;
    }
};

// one allocation that holds the buffers of all plans of a batch at a constant stride (see emagls_batch)
struct Arena {
    void* base = nullptr;
    size_t bytes = 0;
    ~Arena() { if (base) BlockPool::get().give(base, bytes); }
};

// kinds that run the array-model pipeline (simulated array -> per-bin factor -> sweep)
static inline bool magls_kind(int k) { return k == EMAGLS_KIND_MAGLS || k == EMAGLS_KIND_MAGLS_2D; }
static inline bool array_kind(int k) { return k == EMAGLS_KIND_EMAGLS || k == EMAGLS_KIND_EMAGLS2 || k == EMAGLS_KIND_EMA_CH || k == EMAGLS_KIND_EMA_SH; }

// A captured graph and its executable instance, owned together (non-copyable).  The only place on the host side that begins a
// capture, instantiates a graph or destroys one: a struct that holds such a member needs no line of its own for it.
struct CapturedGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    CapturedGraph() = default;
    CapturedGraph(const CapturedGraph&) = delete;
    CapturedGraph& operator=(const CapturedGraph&) = delete;
    ~CapturedGraph() { if (exec) hipGraphExecDestroy(exec); if (graph) hipGraphDestroy(graph); }   // (never throws)
    explicit operator bool() const { return exec != nullptr; }
    // what `body` enqueues on `st`, captured and instantiated; a body that throws ends the capture and leaves nothing behind
    template <typename F> void capture(hipStream_t st, F&& body) {
        HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        try {
            body();
        } catch (...) {
            hipGraph_t tmp = nullptr;
            hipStreamEndCapture(st, &tmp);
            if (tmp) hipGraphDestroy(tmp);
            throw;
        }
        HIP_CHECK(hipStreamEndCapture(st, &graph));
        HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    }
    void launch(hipStream_t st) const { HIP_CHECK(hipGraphLaunch(exec, st)); }
    void reset() {
        if (exec) { HIP_CHECK(hipGraphExecDestroy(exec)); exec = nullptr; }
        if (graph) { HIP_CHECK(hipGraphDestroy(graph)); graph = nullptr; }
    }
};

// A value lent to a variable for one scope (non-copyable): the old one comes back when the scope ends, by return or by exception.
// Every temporary override of plan or batch state is one of these (a batch lending its stream to all its plans: StreamLoan below).
template <typename T> struct Scoped {
    T& var;
    T old;
    template <typename U> Scoped(T& v, U&& value) : var(v), old(v) { var = std::forward<U>(value); }
    Scoped(const Scoped&) = delete;
    Scoped& operator=(const Scoped&) = delete;
    ~Scoped() { var = old; }
};
template <typename T, typename U> Scoped(T&, U&&) -> Scoped<T>;

}  // namespace emagls

struct emagls_plan {
    emagls_design_desc d{};
    int device = -1;              // the HIP device the plan was created on: every C entry point runs on it (DeviceGuard)
    hipStream_t stream = nullptr;
    std::map<std::string, DevBuf> bufs;
    std::shared_ptr<Arena> arena;  // set when a batch moved the buffers into its arena (they are not freed one by one then)
    // The plan's ~75 buffers are carved out of a few slabs (one hipMalloc / hipFree per 32 MB instead of one per buffer: a job list
    // whose array radii change from chunk to chunk creates and releases its plans inside the call, and 1200 hipFree calls per chunk
    // of 16 plans were 0.28 s of its 0.39 s).  A buffer that grows takes a new region; the slabs go when the plan goes, or when a
    // batch has moved every buffer into its arena.
    struct Slab { char* base; size_t size, used; };
    std::vector<Slab> slabs;
    bool slab_zeroed = false;      // the newest slab was zero-filled when it was taken
    static constexpr size_t SLAB_BYTES = (size_t)32 << 20;
    void* slab_take(size_t bytes) {
        bytes = (bytes + 255) / 256 * 256;
        if (slabs.empty() || slabs.back().used + bytes > slabs.back().size) {
            Slab sl{nullptr, (std::max(bytes, SLAB_BYTES) + SLAB_BYTES - 1) / SLAB_BYTES * SLAB_BYTES, 0};
            sl.base = static_cast<char*>(BlockPool::get().take(sl.size, &sl.size));
            // (one fill per slab instead of one per buffer: 66 hipMemsetAsync calls were 1.9 ms of a plan's set-up)
            if (hipMemsetAsync(sl.base, 0, sl.size, stream) != hipSuccess) { (void)hipGetLastError(); slab_zeroed = false; } else slab_zeroed = true;
            slabs.push_back(sl);
        }
        void* p = slabs.back().base + slabs.back().used;
        slabs.back().used += bytes;
        return p;
    }
    void release_slabs() {
        for (auto& sl : slabs) BlockPool::get().give(sl.base, sl.size);
        slabs.clear();
    }
    int64_t total_bytes = 0;
    // derived constants
    bool cplx_basis = false;      // element type of the internal SH machinery
    bool req_cplx = false;        // shDefinition == 'complex' was requested
    bool real_internal = false;   // complex request served by the real-arithmetic pipeline + a unitary channel transform
    int nfft = 0, P = 0, k_cut = 0, kcut0 = 0;
    int simOrder = 0, S = 0, C = 0, ldS = 0, nOut = 0;
    int simOrderOwn = 0;          // the design's own simulation order (getSMAIRMatrix.m:95); simOrder may be padded above it
    int64_t D = 0, ldD = 0, Dpad = 0, Dm = 0;  // Dm: matched direction count (FROM_ATF)
    bool hrir_smaller = true;
    bool out_cplx = false;
    int64_t out_rows = 0, out_cols = 0;
    int nWG = 0, nWG_dense = 0;   // workgroups of the launch-per-bin sweeps (MagLS / FromAtf: nWG; array designs: nWG_dense)
    // Gram route of the per-bin factorisation for the well-conditioned swept bins (factor.hip); switched off for good
    // when a run reports that the kr-based conditioning estimate was too optimistic (the plan is then re-executed)
    bool gram_route = true;
    // Routes of the per-bin factorisation (plan_routes): bins [1, hh_end) take the orthonormal S-space route (Householder QR +
    // Jacobi SVD) on the orders 0..n_h whose modal strength is above 1e-20 of the strongest there (S_h = (n_h+1)^2 rows); bins
    // [gram_from, P) take the Gram route (gramroute.hip) on all orders.  gram_floor: lower bound of gram_from that a device-side
    // conditioning check imposed (recovery).  g0: first bin whose direction-space operand G_k exists.
    int gram_from = 0, gram_floor = 0, hh_end = 0, n_h = 0, S_h = 0, ldS_h = 0, g0 = 0, nb_gram = 0;
    int nh_floor = 0;   // least number of orders on the Householder route (a lane batch gives all its designs the same routes)
    bool persist_suspended = false;   // sweep_persist switched off for ONE re-run (status word 4), restored afterwards
    bool sweep_persist = true;  // (EMAGLS_SWEEP_PERSIST=0 disables) one resident launch for all swept bins (sweep_persist.hip)
    // Operand synthesis (sweep_synth.hip): the resident sweep evaluates the slab of pwGrid_k.' of every bin itself from the angles
    // between HRIR directions and microphones instead of reading a materialised G_k (540 MB per design at config 3).  synth_want:
    // the design qualifies (built-in real SH machinery, <= 32 microphones, no covariance constraint); synth: it is in effect
    // (persistent sweep, no swept bin on the Householder route) -- plan_update_synth
    bool synth_want = false, synth = false;
    int synth_units = 0;          // antipodal microphone pairs + single microphones (set with the microphone grid)
    // the register-resident form of the synthesising sweep (sweep_reg.hip) took the last sweep of this plan (decided per launch:
    // reg_sweep_wanted); its argument block lies in device memory ("sweep_args"; the host copy tells when it has to be stored again)
    bool reg_sweep = false;
    std::vector<char> sweep_args_last;
    bool synth_block = false;     // a batch whose designs do not all qualify keeps every one of them on the materialised operands
    const emagls_plan* geo_from = nullptr;   // set while a geometry-sharing batch runs this plan's stages on plan 0's geometry
    emagls_batch* owner = nullptr;  // the batch this plan currently belongs to (cleared by either destructor)
    bool have_hrir_grid = false, have_mic_grid = false, have_hrirs = false, have_atfs = false, have_basis = false;
    uint64_t atf_side_version = 0;   // bumped when the grids or the ATF set are replaced (a FromAtf batch re-checks that its plans agree)
    bool diffuse = false;         // diffuseness (covariance) constraint after the sweep (render.hip: diffuse_constraint_kernel)
    bool custom_basis = false;    // the SH matrices come from the caller (a custom shFunction evaluated on the MATLAB side)
    bool wide = false;            // LS / MagLS with 33..64 channels (SH orders 5..7): the plain path of wide.hip
    // profiling
    int prof_level = 0;
    std::vector<std::string> stage_names;
    std::vector<hipEvent_t> stage_events;
    std::vector<double> stage_ms;
    std::vector<hipEvent_t> sweep_events;
    int sweep_launches = 0;
    bool executed = false;
    // hipGraph replay of the whole design (launch-bound: ~520 small kernels per execute)
    CapturedGraph graph;
    int eager_runs = 0;
    bool use_graph = true;
    CapturedGraph pre;                       // stages before the sweep, captured on the plan's own stream (its own executes and stream-mode batches)
    int nstreams = 1;
    int stage_order = 0;          // order of the stages before the sweep (emagls_pre_sweep): 0 branches, 1 / 2 the complementary single-stream orders of lane groups
    int pre_phase = 0;            // emagls_pre_sweep: 0 everything, 1 only what the sweep needs, 2 the rest (plan_defers_hh_route)
    // HRIR sets on ONE geometry through a plan of the 33..64-channel path (emagls_design_hrir_sets): what depends on the grids and the array only
    // -- G_k, the per-bin factors, Y_reg_inv_k: 19 of the 31 ms of a 64-capsule design -- is kept from the last clean run on the same grids
    bool geo_keep = false;                   // the caller runs sets of one geometry through this plan
    bool geo_skip = false;                   // (this execute: the geometry stages are skipped)
    uint64_t geo_done_version = ~0ull;       // atf_side_version of the last run whose flags came back clean
    uint64_t geo_run_version = ~0ull;        // ... of the last full run (promoted by plan_check_flags)
    uint64_t solo_runs = 0;                  // executes of the plan on its own (they rewrite the geometry state a sharing batch keeps: batch_geo_version)
    bool defer_hh = false;       // plan_execute: what the captured stages before the sweep were captured with
    bool alone = false;           // the plan of a one-shot call (the device to itself, like a plan with forked stages)
    hipStream_t hh_stream = nullptr;   // the stream of the stages that run next to the sweep
    hipStream_t sync_stream = nullptr;  // stream whose completion means this plan's results are ready
    // fork/join inside one design: independent branches run on side streams (such a plan runs eagerly: forks_streams)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};   // taken from the pool when a multi-stream execute first needs them (need_sides)
    bool owns_stream = true;      // false: `stream` belongs to the job slot that created the plan (one stream for all plans of a chunk)
    void need_sides(int n) { for (int i = 0; i < n - 1 && i < 3; ++i) if (!side[i]) side[i] = StreamPool::get().take(); }
    std::vector<hipEvent_t> sync_events;
    size_t sync_used = 0;
    hipEvent_t next_sync_event() {
        if (sync_used == sync_events.size()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sync_events.push_back(e);
        }
        return sync_events[sync_used++];
    }
    // make `waiter` wait for everything enqueued so far on `signaller`
    void depend(hipStream_t waiter, hipStream_t signaller) {
        if (waiter == signaller) return;  // same stream: already ordered
        hipEvent_t e = next_sync_event();
        HIP_CHECK(hipEventRecord(e, signaller));
        HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
    }

    ~emagls_plan() {
        if (owner) emagls_batch_forget(owner, this);
        // the slabs go back to a pool that other threads take from at once (no hipFree that would wait for pending work): nothing
        // enqueued by this plan may still be running on them
        if (stream) hipStreamSynchronize(stream);
        for (auto st : side) if (st) hipStreamSynchronize(st);
        if (hh_stream) hipStreamSynchronize(hh_stream);
        (void)hipGetLastError();
        for (auto& kv : bufs) if (kv.second.p && kv.second.owned) hipFree(kv.second.p);
        release_slabs();
        for (auto e : stage_events) hipEventDestroy(e);
        for (auto e : sweep_events) hipEventDestroy(e);
        for (auto e : sync_events) hipEventDestroy(e);
        for (auto st : side) StreamPool::get().give(st);
        StreamPool::get().give(hh_stream);
        if (owns_stream) StreamPool::get().give(stream);
    }
    void* alloc(const std::string& name, size_t bytes, bool zero = true) {
        if (bytes == 0) bytes = 16;
        auto it = bufs.find(name);
        if (it != bufs.end()) {   // re-allocation (a design's routes changed): keep what is large enough
            if (it->second.bytes >= bytes) {   // (the recorded size follows the request: lane batches compare and copy by it)
                total_bytes -= (int64_t)(it->second.bytes - bytes);
                it->second.bytes = bytes;
                return it->second.p;
            }
            if (it->second.owned) HIP_CHECK(hipFree(it->second.p));
            total_bytes -= (int64_t)it->second.bytes;
        }
        DevBuf b;
        b.p = slab_take((bytes + 15) / 16 * 16);  // (launch_zero works on whole 8-byte words)
        b.bytes = bytes;
        b.owned = false;   // (part of a slab, zero-filled when the slab was taken)
        if (zero && !slab_zeroed) HIP_CHECK(hipMemsetAsync(b.p, 0, bytes, stream));
        bufs[name] = b;
        total_bytes += (int64_t)bytes;
        return b.p;
    }
    template <typename T = void> T* get(const std::string& name) {
        auto it = bufs.find(name);
        if (it == bufs.end()) throw Error(EMAGLS_ERR_ARG, "internal: unknown buffer " + name);
        return reinterpret_cast<T*>(it->second.p);
    }
    bool has(const std::string& name) const { return bufs.count(name) != 0; }
    void upload(const std::string& name, const void* src, size_t bytes) {
        auto it = bufs.find(name);
        if (it == bufs.end() || it->second.bytes < bytes) throw Error(EMAGLS_ERR_ARG, "internal: upload size mismatch for " + name);
        HIP_CHECK(hipMemcpyAsync(it->second.p, src, bytes, hipMemcpyDefault, stream));
    }
    void mark(const char* name) {
        if (prof_level < 1) return;
        const size_t i = stage_names.size();
        stage_names.push_back(name);
        if (stage_events.size() <= i) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            stage_events.push_back(e);
        }
        HIP_CHECK(hipEventRecord(stage_events[i], stream));
    }
};

struct emagls_batch {
    std::vector<emagls_plan*> plans;
    int device = -1;              // device of its plans
    // lanes: all plans have the same shape and their buffers sit `stride` bytes apart in one arena, so every
    // launch of the design pipeline covers the whole batch (grid.z = design)
    bool lanes = false;
    size_t stride = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;                    // false once the caller supplied the stream (emagls_batch_set_stream)
    // FromAtf subjects: the ATF side (spectra of the matched ATFs, per-bin factors) is computed by plan 0 and read by all plans when
    // they hold the same grids and ATF set (checked on the device whenever one of them was replaced)
    bool atf = false, atf_share = false, atf_inputs_same = false;
    uint64_t atf_checked_version = ~0ull;
    // array designs that differ only in their HRIR sets (same grids, array, orders): the geometry stages run once (opt-in,
    // emagls_batch_set_geometry_sharing; checked on the device whenever a grid was replaced)
    bool magls = false;     // MagLS / MagLS-2D plans (HRIR sets on one or several grids): batch_execute_magls
    bool geo_want = false, geo_share = false, geo_inputs_same = false;
    uint64_t geo_checked_version = ~0ull;
    // a sharing batch of array designs keeps its geometry stages between executes (batch_execute_geo): the "cold" form runs plan 0's
    // whole pipeline and hands its factors to the subjects, the "warm" form only what an HRIR set enters, for every plan
    uint64_t geo_kept_version = ~0ull;         // batch_geo_version of the last cold run whose status flags came back clean
    uint64_t geo_ran_version = ~0ull;          // ... of the last cold run enqueued (promoted by emagls_batch_get_filters)
    bool geo_cold_pending = false;             // that run's flags have not been read yet
    CapturedGraph warm;                        // the warm form's stages before the sweep (the stages after it are the same in both forms)
    int last_form = 0;                         // the last execute: 0 independent designs (or another kind of batch), 1 cold, 2 warm
    long long geo_cold_runs = 0, geo_warm_runs = 0;
    // the kept operand of the least-squares rows: Yls [bin 1 .. ls_end-1][C][ldD] = Y_reg_inv_k of plan 0's geometry, written by the
    // cold run only (zls: its copy of plan 0's Z of those bins, solved against R^H in place); geo_ls_shared: this batch takes that form
    // (batch_geo_decide_sharing)
    bool geo_ls_shared = false;
    emagls::DevMem yls, zls;
    emagls::DevMem cmp_flag;
    int nstreams = 1;                          // lane mode: streams the stages before the sweep fork onto (emagls_batch_set_streams)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    // the stages before the sweep, one graph per lane group (on `stream`, side[0], side[1], side[2]: batch_execute_lanes); [0] is also
    // those stages of the atf / magls / geo-cold forms and the captured launch-per-bin sweep of a batch without lanes
    CapturedGraph group[4];
    int prof_level = 0;
    hipEvent_t sweep_ev[2] = {nullptr, nullptr};
    CapturedGraph post;                        // lane mode: the stages after the sweep (the sweep is launched directly)
    bool side0_external = false;               // side[0] belongs to the caller (emagls_batch_set_side_stream)
    int order_hint = 0;                        // single-group batches: 1 / 2 = stage order of emagls_pre_sweep the caller asks for (emagls_batch_set_stage_order)
    int groups = 1;                            // lane groups before the sweep (ceil(designs / 8), up to 4: batch_execute_lanes)
    CapturedGraph group_hh[4];                 // per lane group: the stages the sweep does not need (plan_defers_hh_route), next to the sweep
    hipStream_t hh_stream[4] = {nullptr, nullptr, nullptr, nullptr};
    bool defer_hh = false;                     // what the captured graphs were captured with (batch_execute_lanes)
    bool alone = true;                         // the batch has the device to itself: the default of emagls_batch_create; the job scheduler clears it for the chunks of a list that keeps several in flight
    int eager_runs = 0;
    bool use_graph = true;
    emagls::DevMem sweep_args_dev;             // argument blocks of the register-resident sweep, one per plan (sweep_reg.hip)
    std::vector<char> sweep_args_last;
    std::vector<hipEvent_t> events;
    size_t used = 0;
    hipEvent_t next_event() {
        if (used == events.size()) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            events.push_back(e);
        }
        return events[used++];
    }
    void depend(hipStream_t waiter, hipStream_t signaller) {
        hipEvent_t e = next_event();
        HIP_CHECK(hipEventRecord(e, signaller));
        HIP_CHECK(hipStreamWaitEvent(waiter, e, 0));
    }
    ~emagls_batch() {
        // a batch may still be in flight on a caller-owned stream (emagls_batch_set_stream): its graph execs and events must
        // outlive it (pool-owned streams are synchronised again when they are handed back).  The graphs are members: they are
        // destroyed after this body, hence after the synchronisation of `stream` here and of the hh_streams below.
        if (stream) hipStreamSynchronize(stream);
        for (auto e : events) hipEventDestroy(e);
        for (int i = 0; i < 4; ++i)
            if (hh_stream[i]) { hipStreamSynchronize(hh_stream[i]); emagls::pool_stream_give(hh_stream[i]); }
        for (auto e : sweep_ev) if (e) hipEventDestroy(e);
        if (stream && own_stream) emagls::pool_stream_give(stream);
        for (int i = 0; i < 3; ++i) if (side[i] && !(i == 0 && side0_external)) { hipStreamSynchronize(side[i]); emagls::pool_stream_give(side[i]); }
        for (auto* p : plans) if (p) { p->sync_stream = nullptr; p->owner = nullptr; }
    }
};

namespace emagls {

// one stream lent to every plan of a batch for a scope (the single-stream forms enqueue all their plans' stages on the batch's stream)
struct StreamLoan {
    const std::vector<emagls_plan*>& plans;
    std::vector<hipStream_t> keep;
    StreamLoan(const std::vector<emagls_plan*>& ps, hipStream_t st) : plans(ps) {
        keep.reserve(ps.size());
        for (auto* p : ps) { keep.push_back(p->stream); p->stream = st; }
    }
    StreamLoan(const StreamLoan&) = delete;
    StreamLoan& operator=(const StreamLoan&) = delete;
    ~StreamLoan() { for (size_t j = 0; j < keep.size(); ++j) plans[j]->stream = keep[j]; }
};

// guarded_call for a callable of any type (the lambdas of the C entry points)
template <typename F> int guarded(F&& f) {
    return guarded_call([&] { f(); });
}

// First bin of the Gram route: cond(B_k) is governed by the ratio of the lowest to the highest modal coefficient the C
// output channels can carry, |b_0 / b_n| ~ (2n+1)!! / (kr)^n with n = ceil(sqrt(C)) - 1; the route starts where that
// estimate falls below GRAM_COND_EST (the Jacobi kernel verifies cond < 10x that and asks for a re-run otherwise).  The
// route's error is eps cond^2 <= 2e-7 eps-relative at the verification limit 3e4, i.e. 2e-8 on M_k: two orders inside the
// 1e-6 parity tolerance.  With 3e3 the Householder route of the em32 design ends at 1 kHz (bin 21 of 513), where 16 orders are
// above the noise floor: 256 rows, the register tile with which its kernels fit next to a resident sweep workgroup.
constexpr double GRAM_COND_EST = 3.0e3;

// Graphs are captured from ONE stream only.  A capture whose stages fork onto side streams yields a graph with parallel branches,
// and hipGraphLaunch of such graphs faults inside the HIP 7.0 runtime bundled with torch (hip::Graph::UpdateStreams): in long
// sessions (StreamPool above), and on the first replay of a lone job chunk's forked lane batch when the process has two hardware
// queues.  Forked stages therefore run eagerly on their streams; everything on one stream keeps its graphs.
inline bool forks_streams(const emagls_plan& p) { return p.nstreams >= 2; }

// ---- defined in plan_setup.hip
extern thread_local hipStream_t g_plan_stream_shared;   // set by the job scheduler around the creation of a chunk's plans
void plan_routes(emagls_plan& p);
void synth_pairing(const double* azi, const double* zen, int M, int* smap);
void plan_alloc_routes(emagls_plan& p);
void plan_setup(emagls_plan& p);

// ---- defined in plan_run.hip
void stage_prologue(emagls_plan& p, int mode, const int64_t* didx, int64_t Dh);
void execute_ls(emagls_plan& p);
void magls_post_sweep(emagls_plan& p);
bool plan_defers_hh_route(const emagls_plan& p);
// the HRIR-side stages of an array design, for the plan h that owns the HRIR set on the geometry of plan g (h itself inside its own
// pipeline): the ONE definition that emagls_pre_sweep and the geometry-sharing batch form (batch_geo_stage) both call
// (transposed: also HcT, the direction-major copy of the least-squares bins' spectra that hrir_hh_rows reads)
void hrir_spectra(emagls_plan& h, const emagls_plan& g, hipStream_t st, bool transposed = true);
FactorArgs hh_factor_args(emagls_plan& h, emagls_plan& g, int* sweeps_out, double* cond_ok);
void hrir_hh_rows(emagls_plan& h, emagls_plan& g, hipStream_t st);
void hrir_hh_back(const FactorArgs& fa, const emagls_plan& g, hipStream_t st);
void hrir_gram_ls_rows(emagls_plan& h, emagls_plan& g, const emagls_plan& src, bool lanes_share, hipStream_t st);
void subject_reset(emagls_plan& p, hipStream_t st);
void emagls_pre_sweep(emagls_plan& p);
HalfSweepArgs emagls_half_args(emagls_plan& p);
// the gate every resident sweep of a device passes through (one per process and device: mutex() and state() are defined once)
struct SweepGate {
    struct Entry { hipEvent_t ev; int slots; };
    struct State { std::deque<Entry> inflight; std::vector<hipEvent_t> pool; int capacity = 0; };
    static std::mutex& mutex();
    static State& state();   // (call with the mutex held)
    std::unique_lock<std::mutex> lock;
    hipStream_t st;
    int slots;
    SweepGate(hipStream_t s, int slots_per_xcd);   // slots_per_xcd <= 0: the whole device
    ~SweepGate();
};
bool reg_sweep_wanted(emagls_plan* const* plans, int n);
void reg_args_upload(const HalfSweepArgs* host, int n, void* dev, std::vector<char>& last, hipStream_t st);
void emagls_post_sweep(emagls_plan& p);
void from_atf_subject_stage(emagls_plan& p);
void from_atf_ls_rows(emagls_plan& p, emagls_plan& sh, hipStream_t st);
void from_atf_post_sweep(emagls_plan& p);
void plan_pre_stage(emagls_plan& p);
void plan_execute(emagls_plan& p);
void drop_plan_graphs(emagls_plan& p);
bool plan_recover(emagls_plan& p, const int* flag, bool apply);
void throw_fatal_flags(const int* flag);

// ---- defined in batch_run.hip
void batch_geo_forget(emagls_batch& b);
bool batch_geo_next_is_warm(const emagls_batch& b);
void batch_execute(emagls_batch& b);
void drop_batch_graphs(emagls_batch& b);
void batch_unify_synth(emagls_batch& b);
void batch_decide_residency(emagls_batch& b);
void batch_try_lanes(emagls_batch& b);
void batch_redo(emagls_batch& b, const std::vector<int>& flags);
void plan_check_flags(emagls_plan& p);

// ---- defined in capi.hip, called by jobs.hip
bool same_desc(const emagls_design_desc& a, const emagls_design_desc& b);
extern thread_local int g_batch_max_override;   // emagls_design_hrir_sets builds batches of 16 of its own whatever the caller's limit is

}  // namespace emagls
