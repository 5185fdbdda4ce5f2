// Batches: lane groups, the ATF / geometry / MagLS sharing forms, the shared sweep launch, and the re-run of a batch whose
// designs raised a recoverable flag.
#include "host_internal.hpp"

// a plan of the batch is being destroyed before the batch: the batch must not touch it again
void emagls_batch_forget(emagls_batch* b, emagls_plan* p) {
    for (auto& q : b->plans) if (q == p) q = nullptr;
}

namespace {
void batch_sweep_stage(emagls_batch& b) {
    const int nb = (int)b.plans.size();
    std::vector<HalfSweepArgs> ha((size_t)nb);
    for (int j = 0; j < nb; ++j) ha[j] = emagls_half_args(*b.plans[j]);
    if (b.atf_share || b.geo_share)   // one ATF side / one geometry for every subject
        for (int j = 1; j < nb; ++j) {
            ha[j].G = ha[0].G; ha[j].Yri = ha[0].Yri; ha[j].Mw = ha[0].Mw; ha[j].cond_ok = ha[0].cond_ok;
            ha[j].bsc = ha[0].bsc; ha[j].smap = ha[0].smap;   // (synthesising sweep: plan 0's scaled modal terms and Mt; the grids are the same by the sharing check)
            ha[j].skip_flag = ha[0].skip_flag;   // (MagLS: plan 0 judged the basis for everybody)
        }
    const bool reg = b.plans[0]->sweep_persist && reg_sweep_wanted(b.plans.data(), nb);
    for (auto* q : b.plans) q->reg_sweep = reg;
    if (!reg && nb > SWEEP_MULTI_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "internal: more than 16 designs in a batch need the register-resident sweep");
    HalfSweepMulti h{};
    h.n = std::min(nb, SWEEP_MULTI_MAX);
    for (int j = 0; j < h.n; ++j) h.a[j] = ha[j];
    emagls_plan& q0 = *b.plans[0];
    const int kk0 = std::max(q0.kcut0, 1);
    if (kk0 >= q0.P) return;
    if (q0.sweep_persist) {
        // (tried in round 4: the launch on a stream of the highest priority, so that the dispatcher places the sweep's workgroups
        // before other batches' refilling kernels -- per batch, or one per device: 1744 against 1646 sets/s at 20 steps in one
        // session, nothing in the next, and with six / eight batches in flight the extra streams, multiplexed onto hardware
        // queues that held each other's waits, stalled runs for seconds (28-880 sets/s): rejected)
        hipStream_t ss = b.stream;
        {
            SweepGate gate(ss, reg ? reg_sweep_gate_cost((int)q0.D, nb) : 0);
            if (b.lanes) { BatchScope sc(nb, b.stride); launch_zero(q0.get("ll"), q0.bufs["ll"].bytes, ss); }   // (one launch for every lane)
            else for (auto* q : b.plans) launch_zero(q->get("ll"), q->bufs["ll"].bytes, ss);
            if (reg) {
                if (!b.sweep_args_dev.get()) b.sweep_args_dev.alloc(sizeof(HalfSweepArgs) * (size_t)REG_SWEEP_MAX);
                reg_args_upload(ha.data(), nb, b.sweep_args_dev.get(), b.sweep_args_last, ss);
            }
            if (b.prof_level >= 1) HIP_CHECK(hipEventRecord(b.sweep_ev[0], ss));
            if (reg) launch_sweep_reg(b.sweep_args_dev.get<const HalfSweepArgs>(), ha[0], nb, ss);
            else if (q0.synth) launch_sweep_synth(h, ss); else launch_sweep_persist(h, ss);
            if (b.prof_level >= 1) HIP_CHECK(hipEventRecord(b.sweep_ev[1], ss));
        }
        if (ss != b.stream) b.depend(b.stream, ss);
        return;
    }
    for (int kb = kk0; kb < q0.P; ++kb) launch_sweep_half(h, kb, b.stream);
    launch_sweep_half_finalize(h, q0.P - 1, b.stream);
}

// a lane batch whose designs all keep the orthonormal route of their low bins off the path to the sweep (plan_defers_hh_route)
bool batch_defers_hh(const emagls_batch& b) {
    // Only a batch that has the device to itself (a job list of ONE chunk: b.alone, set with its forked streams): there the stages are
    // the path to the sweep -- 2570-2620 -> 2810-2880 sets/s at 20 steps although the sweep itself runs 10 % longer next to them.  With
    // four chunks in flight the same work only moves, and the slower sweeps cost 6 % (3470 -> 3270 at 128 steps).
    if (!b.lanes || !(b.alone || sw_int<Sw::DEFER_HH>() == 2) || b.geo_share || b.atf_share) return false;
    for (const emagls_plan* p : b.plans) if (!p || !plan_defers_hh_route(*p)) return false;
    return true;
}
// lane mode: the pipeline of plan `first` is enqueued once on `st` with grid.z = `count` designs (plans first .. first + count - 1)
// part 0: stages before the sweep, part 2: stages after it
void batch_lanes_part(emagls_batch& b, int part, int first, int count, hipStream_t st, int group = 0) {
    emagls_plan& p0 = *b.plans[first];
    const int ns = (part == 0 && b.groups == 1) ? b.nstreams : 1;
    int order = 0;
    // the two lane groups of a batch issue the stages before the sweep in complementary orders (emagls_pre_sweep, orders 1 and 2);
    // EMAGLS_STAGGER=0: both in the order of a single design
    if (part == 0 && ns == 1 && sw_on<Sw::STAGGER>()) order = b.groups > 1 ? 1 + group % 2 : (b.order_hint ? 1 + (b.order_hint - 1) % 2 : 0);
    // plan `first` stands for its lanes: on the group's stream, with the batch's side streams when the stages fork
    Scoped stream(p0.stream, st);
    Scoped nstreams(p0.nstreams, ns);
    Scoped stage_order(p0.stage_order, order);
    Scoped side0(p0.side[0], ns > 1 ? b.side[0] : p0.side[0]), side1(p0.side[1], ns > 1 ? b.side[1] : p0.side[1]),
        side2(p0.side[2], ns > 1 ? b.side[2] : p0.side[2]);
    // part 0 of a batch that runs the orthonormal route next to its sweep: only what the sweep needs; part 3: the rest
    Scoped pre_phase(p0.pre_phase, part == 3 ? 2 : (part == 0 && b.defer_hh) ? 1 : 0);
    BatchScope sc(count, b.stride);
    if (part == 0) plan_pre_stage(p0); else if (part == 3) emagls_pre_sweep(p0); else emagls_post_sweep(p0);
}
// what an execute leaves in its plans: `launches` sweep launches each
void mark_executed(emagls_batch& b, int launches) {
    for (auto* p : b.plans) { p->executed = true; p->sweep_launches = launches; }
}
int sweep_launch_count(const emagls_plan& p0) { return p0.sweep_persist ? 1 : p0.P - std::max(p0.kcut0, 1); }
// Lane GROUPS: a batch of more than 8 designs runs the stages before its sweep as two half-batches on two streams (each one
// launch of every kernel for its lanes, each a captured single-stream graph) and then ONE resident sweep launch for all designs.
// Sixteen lanes in one launch sequence take about twice as long per kernel as eight (the bandwidth-bound kernels scale with
// the lanes, and the latency-bound ones get 2x the workgroups), and that sequence is the path to the sweep; two half-batches
// next to each other overlap their latency-bound kernels (measured at --steps 20: the 16-lane sequence 8.6 ms).
int batch_group_first(const emagls_batch& b, int g) { const int n = (int)b.plans.size(), h = (n + b.groups - 1) / b.groups; return std::min(n, g * h); }
void batch_execute_lanes(emagls_batch& b) {
    // (one lane group with more than one stream forks its stages: never captured, see forks_streams)
    const bool replay = b.use_graph && b.eager_runs >= 1 && !(b.groups == 1 && b.nstreams > 1);
    const int n = (int)b.plans.size();
    const int ng = b.groups;
    for (int g = 1; g < ng; ++g) if (!b.side[g - 1]) b.side[g - 1] = emagls::pool_stream_take();
    hipStream_t gs[4] = {b.stream, b.stream, b.stream, b.stream};
    for (int g = 1; g < ng; ++g) gs[g] = b.side[g - 1];
    // the stages the sweep does not need (Cholesky factor, orthonormal route of the low bins) run NEXT to it, one stream per lane group
    // (decided on the eager run and when the graphs are captured; a replay keeps what its graphs were captured with)
    if (!replay || !b.group[0]) b.defer_hh = batch_defers_hh(b);
    const bool defer = b.defer_hh;
    if (defer) for (int g = 0; g < ng; ++g) if (!b.hh_stream[g]) b.hh_stream[g] = emagls::pool_stream_take();
    if (replay && !b.group[0]) {
        for (int g = 0; g < ng; ++g) {
            const int f = batch_group_first(b, g), c = batch_group_first(b, g + 1) - f;
            b.group[g].capture(gs[g], [&] { batch_lanes_part(b, 0, f, c, gs[g], g); });
            if (defer) b.group_hh[g].capture(b.hh_stream[g], [&] { batch_lanes_part(b, 3, f, c, b.hh_stream[g], g); });
        }
        b.post.capture(b.stream, [&] { batch_lanes_part(b, 2, 0, n, b.stream); });
    }
    b.used = 0;
    for (int g = 1; g < ng; ++g) b.depend(gs[g], b.stream);   // (the previous execute of this batch is done with the buffers)
    if (replay && ng > 1) {
        // a graph launch of ~60 kernel nodes costs ~1 ms of host time: the other groups' launches go out from threads of their
        // own, or their stages would start a millisecond (three under a profiler) behind the first group's
        hipError_t err[4] = {hipSuccess, hipSuccess, hipSuccess, hipSuccess};
        const int dev = b.device;
        std::vector<std::thread> th;
        for (int g = 1; g < ng; ++g)
            th.emplace_back([&, g] { err[g] = hipSetDevice(dev); if (err[g] == hipSuccess) err[g] = hipGraphLaunch(b.group[g].exec, gs[g]); });
        err[0] = hipGraphLaunch(b.group[0].exec, gs[0]);
        for (auto& t : th) t.join();
        for (int g = 0; g < ng; ++g) HIP_CHECK(err[g]);
    } else {
        for (int g = 0; g < ng; ++g) {
            const int f = batch_group_first(b, g), c = batch_group_first(b, g + 1) - f;
            if (replay) b.group[g].launch(gs[g]); else batch_lanes_part(b, 0, f, c, gs[g], g);
        }
    }
    if (defer) for (int g = 0; g < ng; ++g) b.depend(b.hh_stream[g], gs[g]);   // (behind the group's stages, before the sweep is enqueued)
    for (int g = 1; g < ng; ++g) b.depend(b.stream, gs[g]);
    batch_sweep_stage(b);   // (never captured: see SweepGate)
    if (defer) {
        for (int g = 0; g < ng; ++g) {
            const int f = batch_group_first(b, g), c = batch_group_first(b, g + 1) - f;
            if (replay) b.group_hh[g].launch(b.hh_stream[g]); else batch_lanes_part(b, 3, f, c, b.hh_stream[g], g);
            b.depend(b.stream, b.hh_stream[g]);   // (the epilogue reads the rows of every bin)
        }
    }
    if (replay) b.post.launch(b.stream); else batch_lanes_part(b, 2, 0, n, b.stream);
    mark_executed(b, sweep_launch_count(*b.plans[0]));
    if (!replay) ++b.eager_runs;
}

// ---- what the sharing forms and the per-plan form have in common
// Do the buffers `names` of every plan hold the same words as plan 0's?  Compared on the device, and only when a plan's grids or ATF
// set were replaced since the last comparison (atf_side_version); `same` keeps the answer in between.
bool batch_inputs_same(emagls_batch& b, std::initializer_list<const char*> names, uint64_t& checked_version, bool& same) {
    uint64_t ver = 0;
    for (auto* p : b.plans) ver = ver * 1000003ull + p->atf_side_version;
    if (ver == checked_version) return same;
    if (!b.cmp_flag.get()) b.cmp_flag.alloc(16);
    HIP_CHECK(hipStreamSynchronize(b.stream));
    HIP_CHECK(hipMemsetAsync(b.cmp_flag.get(), 0, 16, b.stream));
    emagls_plan& p0 = *b.plans[0];
    for (size_t j = 1; j < b.plans.size(); ++j)
        for (const char* name : names) launch_compare_words(p0.get(name), b.plans[j]->get(name), p0.bufs[name].bytes, b.cmp_flag.get<int>(), b.stream);
    int differ = 0;
    HIP_CHECK(hipMemcpyAsync(&differ, b.cmp_flag.get(), sizeof differ, hipMemcpyDeviceToHost, b.stream));
    HIP_CHECK(hipStreamSynchronize(b.stream));
    checked_version = ver;
    return same = differ == 0;
}
// the two modes enqueue different stages: nothing captured for the other one may be replayed (and a batch that shares its geometry,
// or stops doing so, runs its geometry stages again)
void batch_set_sharing(emagls_batch& b, bool& field, bool share) {
    if (share == field) return;
    for (auto* p : b.plans) drop_plan_graphs(*p);
    drop_batch_graphs(b);
    if (&field == &b.geo_share || &field == &b.geo_ls_shared) batch_geo_forget(b);
    field = share;
}
// The whole batch as two single-stream graphs around the resident sweep: `stage(b, pre_part)` before it and `stage(b, 2)` after it on
// the batch's stream, eagerly on the first execute, captured (`pre`, b.post) when first needed afterwards; the sweep between them is
// never captured (SweepGate).
void batch_run_two_graphs(emagls_batch& b, CapturedGraph& pre, void (*stage)(emagls_batch&, int), int pre_part, int launches) {
    const bool replay = b.use_graph && b.eager_runs >= 1;
    if (replay && !pre) pre.capture(b.stream, [&] { stage(b, pre_part); });
    if (replay && !b.post) b.post.capture(b.stream, [&] { stage(b, 2); });
    b.used = 0;
    if (replay) pre.launch(b.stream); else stage(b, pre_part);
    batch_sweep_stage(b);
    if (replay) b.post.launch(b.stream); else stage(b, 2);
    mark_executed(b, launches);
    if (!replay) ++b.eager_runs;
}
// A batch as separate graphs on separate streams (one hipGraph executes its nodes in order, so parallel branches inside ONE graph
// would serialize): per-plan `pre` stages (graphs, on replays) on the plans' own streams, the shared sweep on the batch's stream
// (captured only in its launch-per-bin form), per-plan `post` stages, ordered by events outside the graphs.
template <typename Pre> void batch_run_per_plan(emagls_batch& b, bool replay, Pre pre, void (*post)(emagls_plan&), int launches) {
    emagls_plan& p0 = *b.plans[0];
    if (replay && !p0.pre) {
        for (auto* p : b.plans) p->pre.capture(p->stream, [&] { pre(*p); });
        if (!p0.sweep_persist) b.group[0].capture(b.stream, [&] { batch_sweep_stage(b); });
    }
    b.used = 0;
    for (auto* p : b.plans) b.depend(p->stream, b.stream);   // (the previous sweep of this batch is done with the plans' buffers)
    for (auto* p : b.plans) {
        if (replay) p->pre.launch(p->stream); else pre(*p);
        b.depend(b.stream, p->stream);
    }
    if (b.atf_share)   // (FromAtf subjects only) least-squares bins of the other subjects on plan 0's operands
        for (size_t j = 1; j < b.plans.size(); ++j) from_atf_ls_rows(*b.plans[j], p0, b.stream);
    if (p0.sweep_persist) batch_sweep_stage(b);   // (never captured: see SweepGate)
    else if (replay) b.group[0].launch(b.stream); else batch_sweep_stage(b);
    for (auto* p : b.plans) {
        b.depend(p->stream, b.stream);
        post(*p);
        b.depend(b.stream, p->stream);  // batch stream completion == all results ready
    }
    mark_executed(b, launches);
    if (!replay) ++b.eager_runs;
}

// FromAtf subjects share their ATF side when every plan holds the same grids and ATF set and no bin needs the dense route
void batch_atf_decide_sharing(emagls_batch& b) {
    const bool same = batch_inputs_same(b, {"atf", "atf_azi", "atf_zen", "hrir_azi", "hrir_zen"}, b.atf_checked_version, b.atf_inputs_same);
    bool routes_ok = true;
    for (auto* p : b.plans) routes_ok = routes_ok && p->gram_from == 1 && p->sweep_persist == b.plans[0]->sweep_persist;
    batch_set_sharing(b, b.atf_share, same && routes_ok && b.plans.size() > 1);
}
void from_atf_subject_pre_stage(emagls_plan& p) {   // a subject of a sharing batch: everything but the ATF side
    subject_reset(p, p.stream);
    from_atf_subject_stage(p);
}
// Subjects of ONE ATF set on ONE HRIR grid (checked on the device): the whole batch as two single-stream graphs around the
// resident sweep -- plan 0's full stage (grid match, ATF spectra, per-bin factors), then per subject only the HRIR prologue
// (plan 0's grid match serves every subject) and the least-squares rows; afterwards every subject's epilogue.  Eight graphs
// on eight streams with an event pair each (the earlier form) cost more host time than the stages take on the GPU: 10.2 ms
// per batch of BASELINE config 5, of which 3.3 ms are the sweep and ~4 ms kernels that could overlap.
void batch_atf_shared_stage(emagls_batch& b, int part) {
    emagls_plan& p0 = *b.plans[0];
    StreamLoan loan(b.plans, b.stream);
    if (part == 2) {
        for (auto* p : b.plans) from_atf_post_sweep(*p);
        return;
    }
    plan_pre_stage(p0);
    for (size_t j = 1; j < b.plans.size(); ++j) {
        emagls_plan& p = *b.plans[j];
        subject_reset(p, b.stream);
        // (the subject keeps its own copy of the match: emagls_plan_get_info and the debug buffers read it per plan)
        // (plain device-to-device copies: match_idx holds 64-bit integers)
        HIP_CHECK(hipMemcpyAsync(p.get("match_idx"), p0.get("match_idx"), sizeof(int64_t) * (size_t)p.Dm, hipMemcpyDeviceToDevice, b.stream));
        HIP_CHECK(hipMemcpyAsync(p.get("match_dev"), p0.get("match_dev"), sizeof(double) * (size_t)p.Dm, hipMemcpyDeviceToDevice, b.stream));
        HIP_CHECK(hipMemcpyAsync(p.get("mean_dev"), p0.get("mean_dev"), sizeof(double), hipMemcpyDeviceToDevice, b.stream));
        stage_prologue(p, 1, p.hrir_smaller ? nullptr : p.get<int64_t>("match_idx"), p.Dm);
        from_atf_ls_rows(p, p0, b.stream);
    }
}
void batch_execute_atf(emagls_batch& b) {
    for (auto* p : b.plans)
        if (!p->have_hrirs || !p->have_hrir_grid || !p->have_atfs)
            throw Error(EMAGLS_ERR_ARG, "every plan of the batch needs its HRIRs, its grid and the ATFs");
    batch_atf_decide_sharing(b);
    emagls_plan& p0 = *b.plans[0];
    if (b.atf_share && p0.sweep_persist) { batch_run_two_graphs(b, b.group[0], batch_atf_shared_stage, 0, 1); return; }
    batch_run_per_plan(b, b.use_graph && b.eager_runs >= 1,
                       [&](emagls_plan& p) { if (b.atf_share && &p != &p0) from_atf_subject_pre_stage(p); else plan_pre_stage(p); },
                       from_atf_post_sweep, sweep_launch_count(p0));
}

// ---------------------------------------------------------------------------------------------
// Batches of HRIR sets on ONE geometry (north_star: independent jobs "per HRTF set"): same HRIR grid, same array, same
// orders and lengths.  Everything of lib/getEMagLsFilters.m:44-70,85-93 -- the SH matrices, the array model, pwGrid_k and its
// regularised inverse of every bin -- depends on the geometry only; the HRIR set enters through the spectra (:72-81), the
// least-squares rows (:94) and the sweep's magnitudes (:99-102).  Plan 0 runs the whole pipeline; the other plans run their
// HRIR prologue, their least-squares rows on plan 0's factors, and sweep on plan 0's G_k / M_k (batch_sweep_stage).
// ---------------------------------------------------------------------------------------------
// A sharing batch KEEPS its geometry state between executes (the <= 32-channel counterpart of a wide plan's geo_keep): after one clean
// "cold" run -- plan 0's whole pipeline, its factors handed to the subjects -- the "warm" form enqueues only what an HRIR set enters,
// for every plan of the batch, plan 0 included (batch_geo_stage).  What the kept state was computed from: every plan's grids
// (atf_side_version) and the plans' own executes in between (plan_execute rewrites a plan's copies of the factors).
// EMAGLS_GEO_KEEP=0: every sharing execute is a cold one.
uint64_t batch_geo_version(const emagls_batch& b) {
    uint64_t ver = 0;
    for (const emagls_plan* p : b.plans) ver = (ver * 1000003ull + p->atf_side_version) * 1000003ull + p->solo_runs;
    return ver;
}
// The least-squares rows of a sharing batch come from ONE kept operand Yls = Y_reg_inv_k of the bins below k_cut (ls_shared.hip;
// geo_yls_stage forms it in the cold run) when every such bin has a route to it: the Householder-route bins from plan 0's Z, the
// Gram-route bins of a SYNTHESISING design from the angles.  A design whose Gram-route bins read the materialised G_k
// (launch_ls_gram) keeps the stages that carry every HRIR set through the factors, and so does EMAGLS_GEO_LS_SHARED=0.  So do the
// raw-microphone designs (eMagLS2): their explicit operand gives filters 2.5e-12 away from the single designs' (6 sets, em32, 901
// directions; 3.6e-14 for eMagLS), and a sharing batch of them is held to 1e-12 of its single designs
// (test_hrir_sets_on_one_geometry_share_it).  Decided here, once per batch and again whenever its plans' routes may have moved; a
// change of the answer drops the graphs and the kept state.
static bool batch_geo_ls_shared_wanted(const emagls_plan& p0) {
    const int ls_end = std::min(p0.kcut0, p0.P);
    const bool gram_ls = p0.gram_from > 0 && p0.gram_from < ls_end;
    return sw_on<Sw::GEO_LS_SHARED>() && p0.d.kind != EMAGLS_KIND_EMAGLS2 && ls_end > 1 && p0.C <= 32 && (!gram_ls || p0.synth) &&
           (p0.hh_end <= 1 || p0.has("Z"));
}
void batch_geo_decide_sharing(emagls_batch& b) {
    bool share = false;
    if (b.geo_want && b.plans.size() > 1) {
        emagls_plan& p0 = *b.plans[0];
        bool eligible = (p0.d.kind == EMAGLS_KIND_EMAGLS || p0.d.kind == EMAGLS_KIND_EMAGLS2 || p0.d.kind == EMAGLS_KIND_EMA_CH) && !p0.wide &&
                        !p0.diffuse && !p0.custom_basis;
        for (auto* p : b.plans) {
            const emagls_design_desc &x = p->d, &y = p0.d;
            eligible = eligible && x.kind == y.kind && x.order == y.order && x.fs == y.fs && x.len == y.len && x.nsamp == y.nsamp &&
                       x.ndirs == y.ndirs && x.mic_radius == y.mic_radius && x.nmics == y.nmics && x.basis == y.basis &&
                       x.sim_order_pad == y.sim_order_pad && p->wide == p0.wide && p->diffuse == p0.diffuse && p->custom_basis == p0.custom_basis &&
                       p->real_internal == p0.real_internal && p->gram_from == p0.gram_from && p->hh_end == p0.hh_end && p->n_h == p0.n_h &&
                       p->g0 == p0.g0 && p->sweep_persist == p0.sweep_persist;
        }
        share = eligible && batch_inputs_same(b, {"hrir_azi", "hrir_zen", "mic_azi", "mic_zen"}, b.geo_checked_version, b.geo_inputs_same);
    }
    batch_set_sharing(b, b.geo_share, share);
    batch_set_sharing(b, b.geo_ls_shared, share && batch_geo_ls_shared_wanted(*b.plans[0]));
}
// What the HRIR set of plan h enters, on plan 0's geometry (lib/getEMagLsFilters.m:72-81, :94): its spectra; behind plan 0's stages
// the least-squares bins -- H conj(Q) R^-1 rows and the back-transform of the Householder-route bins (into h's own Z), G_k / M_k for the
// Gram-route bins --; a synthesising design's start value of the microphone-domain chain.  g: where the launches read the
// geometry's operands -- plan 0, or in a lane launch the lanes' own copies (then every pointer of a launch moves by the same stride);
// plan 0's coefficients, Pm and M_k serve every lane of a synthesising design.
void geo_hrir_side(emagls_plan& h, emagls_plan& g, emagls_plan& p0, hipStream_t st) {
    subject_reset(h, st);
    h.sync_used = 0;
    hrir_spectra(h, p0, st);
    if (g.hh_end > 1) {
        hrir_hh_rows(h, g, st);
        hrir_hh_back(hh_factor_args(h, g, nullptr, g.get<double>("cond_ok")), g, st);
    }
    hrir_gram_ls_rows(h, g, p0, true, st);
    if (p0.synth) launch_synth_winit(h.get("W"), p0.get("Pm"), p0.C, (int)p0.d.nmics, std::max(p0.kcut0, 1), p0.P, h.get("Winit"), st, true);
}
// The same with the kept operand (b.geo_ls_shared), in two steps.  The spectra of plan h -- without HcT: nothing reads HcT, Hyp, Hq,
// Rinv or Z in this form --, then the least-squares rows W(k,:) = H(k,:) Yls_k of every lane of the launch context in one launch and the
// start value of the chain from them.
void geo_spectra_side(emagls_plan& h, emagls_plan& p0, hipStream_t st) {
    subject_reset(h, st);
    h.sync_used = 0;
    hrir_spectra(h, p0, st, false);
}
void geo_ls_shared_rows(emagls_plan& h, emagls_plan& p0, const void* yls, hipStream_t st) {
    launch_ls_shared_rows(h.get("Hc"), h.ldD, std::min(p0.kcut0, p0.P), yls, p0.ldD, (int)p0.D, p0.C, p0.P, h.get("W"), st);
    if (p0.synth) launch_synth_winit(h.get("W"), p0.get("Pm"), p0.C, (int)p0.d.nmics, std::max(p0.kcut0, 1), p0.P, h.get("Winit"), st, true);
}
// Yls of plan 0's geometry, behind plan 0's whole pipeline (cold run; outside any lane scope: ONE design's operands).  Every bin from
// the route it takes in hrir_hh_back / hrir_gram_ls_rows: [1, min(hh_end, ls_end)) Householder, [gram_from, ls_end) Gram.
//   Householder route: Y_reg_inv_k = conj(Q) Z_k = conj(Yc) (Z_k R^-H), the form launch_yri_accurate gives the flagged swept bins, here
//   for EVERY such bin (cond_ok null) and on a copy of Z: plan 0's own Z stays what its pipeline wrote.  R's diagonal-block inverses
//   are plan 0's (hrir_hh_rows has just written them).
//   Gram route: conj(g_k) Pm^T conj(M_k) from the angles (launch_yls_gram).
void geo_yls_stage(emagls_batch& b, hipStream_t st) {
    emagls_plan& g = *b.plans[0];
    const bool cb = g.cplx_basis;
    const int ls_end = std::min(g.kcut0, g.P), hh_ls = std::min(g.hh_end, ls_end), gf = g.gram_from;
    cplx* yls = b.yls.get<cplx>();
    if (hh_ls > 1) {
        HIP_CHECK(hipMemcpyAsync(b.zls.get(), g.get("Z"), sizeof(cplx) * (size_t)hh_ls * g.C * g.ldS_h, hipMemcpyDeviceToDevice, st));
        launch_zsolve_flagged(b.zls.get(), g.ldS_h, g.get(cb ? "R" : "Rc"), g.get(cb ? "Rinv" : "Rinvc"), nullptr, g.S_h, g.C, hh_ls, 1, st);
        launch_yri_accurate(g.get("Yc"), g.ldS, cb, b.zls.get(), g.ldS_h, nullptr, (int)g.D, g.S_h, g.C, hh_ls, 1, yls, g.ldD, st,
                            g.custom_basis ? nullptr : g.get("Ycm"), g.ldD);
    }
    if (gf > 0 && gf < ls_end)
        launch_yls_gram(g.get("bsc"), synth_nord_pad(g.simOrder + 1), g.get<double>("hrir_azi"), g.get<double>("hrir_zen"), g.get<double>("mic_azi"),
                        g.get<double>("mic_zen"), g.get<int>("smap"), g.get<double>("Pm"), g.get("Mw"), (int)g.D, g.C, gf, ls_end,
                        yls, g.ldD, st);
}
// One stream for the whole batch (the subjects' stages are short and the sweep chain is what bounds a batch of HRIR sets), so
// that the stages before and after the sweep are two single-stream graphs: issued eagerly, the ~250 launches of a 16-set batch
// cost 11 ms of host time (measured: 1380 sets/s whatever the number of batches in flight).
// part 0: the cold form's stages before the sweep, 1: the warm form's, 2: the stages after the sweep (the same in both forms)
//
// What a warm run relies on (DESIGN.md section 6 has the audit): it reads plan 0's route, sv, cond_ok, Tn, bn, bsc, Pm, Mw / Mt, smap, G
// and Yri, and every plan's own copies of Yc, R / Rc, Vws, Nw, tauw, cond_ok, G and Mw of the least-squares bins -- all written by plan
// 0's geometry stages and broadcast_lanes only.  The HRIR-dependent stages write flag, W, tw, dirsum, grpd, Hc, HcT, Habs, Hyp, Hq,
// Rinv / Rinvc (from R: the same values every time), Z (from Vws, Nw, tauw: the same values every time; read by nobody afterwards),
// Usw and Winit; the sweep writes ll, Wpart, W and Usw; the stages after it W, wL and wR.  Every plan buffer is a range of its own
// in the arena (batch_try_lanes), so none of these aliases a kept one.  A warm run does NOT pass through plan_pre_stage, which would
// zero plan 0's route.
//
// With the kept operand (b.geo_ls_shared, the default for synthesising designs) the warm run is shorter: it reads plan 0's Pm, bsc, Mt,
// smap (the sweep and synth_winit) and the batch's Yls, written by the cold run's geo_yls_stage only; the HRIR-dependent stages write
// flag, W, tw, dirsum, grpd, Hc, Habs and Winit.  Nothing reads or writes HcT, Hyp, Hq, Rinv, Z or the subjects' copies of Yc, R, Vws, Nw,
// tauw, G, Mw.  In the cold run plan 0's own pipeline still writes its least-squares rows and Winit through the factors; the row
// launch for all lanes, plan 0 included, overwrites them before the sweep is enqueued, so plan 0 returns the same bits cold and warm.
// Plan 0's status words are those of its pipeline (it is not reset again); a subject's stages raise none in either form
// (factor_back writes no status word), so batch_redo sees the geometry's flags through plan 0 as before.
void batch_geo_stage(emagls_batch& b, int part) {
    emagls_plan& p0 = *b.plans[0];
    StreamLoan loan(b.plans, b.stream);
    const int n = (int)b.plans.size();
    // what an HRIR set enters, for the plans first .. n-1 on plan 0's geometry: the subjects of a cold run (plan 0 has just run its
    // whole pipeline), every plan of a warm run.  Plan 0 CALLS the same functions here as inside its own pipeline (plan_run.hip:
    // hrir_spectra, hrir_hh_rows, hh_factor_args, hrir_hh_back, hrir_gram_ls_rows from emagls_pre_sweep's blk_prologue, blk_rows,
    // blk_back, blk_tail; synth_winit_kernel is block 0 of synth_mt_kernel), so its filters have the same bits in both forms.
    // f(h, g) for the plans first .. n-1: one call with the lanes' launch context, or one call per plan (g: geo_hrir_side)
    auto each = [&](int first, auto f) {
        if (first >= n) return;
        if (b.lanes) {
            BatchScope sc(n - first, b.stride);
            f(*b.plans[first], *b.plans[first]);
        } else {
            for (int j = first; j < n; ++j) f(*b.plans[j], p0);
        }
    };
    auto hrir_side = [&](int first) {
        if (b.geo_ls_shared) {   // spectra of the plans that have not run theirs; rows and start value of EVERY plan from the kept operand
            each(first, [&](emagls_plan& h, emagls_plan&) { geo_spectra_side(h, p0, b.stream); });
            each(0, [&](emagls_plan& h, emagls_plan&) { geo_ls_shared_rows(h, p0, b.yls.get(), b.stream); });
        } else {
            each(first, [&](emagls_plan& h, emagls_plan& g) { geo_hrir_side(h, g, p0, b.stream); });
        }
    };
    if (part == 1) {
        hrir_side(0);
    } else if (part == 0) {
        plan_pre_stage(p0);
        if (b.lanes && n > 1) {
            // lane batch: the subjects' stages are ONE launch per kernel for all of them (plans 1.. at the arena stride).  The
            // few geometry operands those kernels read (conj(Y), R, the Householder-route factors, M_k and G_k of the
            // least-squares bins: ~40 MB) are copied into the subjects' own slots first, so that every pointer of a launch
            // moves by the same stride; the large ones (G_k, M_k of the swept bins) are only read by the sweep, through
            // plan 0's pointers.  The copies stay: a warm run reads them again.  (Only the stages that carry an HRIR set through the
            // factors read them; with the kept operand Yls nobody does.  The broadcast stays in place as long as
            // EMAGLS_GEO_LS_SHARED=0 can select those stages: it is cold-run work either way.)
            emagls_plan& g = p0;
            const bool cb = g.cplx_basis;
            const int gf = g.gram_from, hh_end = g.hh_end, ldSh = g.ldS_h;
            const int ls_end = std::min(g.kcut0, g.P);
            const size_t g_stride_b = sizeof(cplx) * (size_t)g.C * g.ldD;
            auto bc = [&](const char* name, size_t off, size_t bytes) {
                if (!g.has(name) || bytes == 0) return;
                bytes = std::min(bytes, g.bufs[name].bytes - off);
                launch_broadcast_lanes(g.get<char>(name) + off, bytes, b.stride, n - 1, b.stream);
            };
            if (hh_end > 1) {
                bc("Yc", 0, g.bufs["Yc"].bytes);
                bc(cb ? "R" : "Rc", 0, g.bufs[cb ? "R" : "Rc"].bytes);
                bc("Vws", 0, sizeof(cplx) * (size_t)(hh_end - 1) * g.C * ldSh);
                bc("Nw", 0, sizeof(cplx) * (size_t)(hh_end - 1) * g.C * g.C);
                bc("tauw", 0, sizeof(double) * (size_t)(hh_end - 1) * g.C);
                bc("cond_ok", 0, sizeof(double) * (size_t)g.P);
            }
            if (gf > 0 && gf < ls_end) {
                bc("G", (size_t)(gf - g.g0) * g_stride_b, (size_t)(ls_end - gf) * g_stride_b);
                bc("Mw", 0, sizeof(cplx) * (size_t)ls_end * g.C * g.C);
            }
        }
        if (b.geo_ls_shared) geo_yls_stage(b, b.stream);
        hrir_side(1);
    } else if (b.lanes) {
        BatchScope sc(n, b.stride);
        Scoped from(p0.geo_from, &p0);   // (the filters' rows of every lane from plan 0's Pm and M_k)
        emagls_post_sweep(p0);
    } else {
        for (auto* p : b.plans) {
            Scoped from(p->geo_from, &p0);
            emagls_post_sweep(*p);
        }
    }
}
void batch_execute_geo(emagls_batch& b) {
    const bool warm = batch_geo_next_is_warm(b);
    if (!warm) {   // (this run rewrites the kept state: it counts again once its flags have come back clean)
        b.geo_kept_version = ~0ull;
        b.geo_ran_version = batch_geo_version(b);
        b.geo_cold_pending = true;
        if (b.geo_ls_shared) {   // room for the kept operand (grown, never shrunk; graphs captured on an earlier block are dropped)
            const emagls_plan& p0 = *b.plans[0];
            const int ls_end = std::min(p0.kcut0, p0.P), hh_ls = std::min(p0.hh_end, ls_end);
            const void *y0 = b.yls.get(), *z0 = b.zls.get();
            b.yls.grow(sizeof(cplx) * (size_t)(ls_end - 1) * p0.C * p0.ldD);
            b.zls.grow(sizeof(cplx) * (size_t)std::max(hh_ls, 1) * p0.C * p0.ldS_h);
            if (b.yls.get() != y0 || b.zls.get() != z0) { b.group[0].reset(); b.warm.reset(); }
        }
    }
    // the cold and the warm form each have a captured graph of their stages before the sweep, captured the first time the form runs
    // with replays on -- a batch's second execute is normally its first warm one, so the warm form needs no eager run of its own
    batch_run_two_graphs(b, warm ? b.warm : b.group[0], batch_geo_stage, warm ? 1 : 0, sweep_launch_count(*b.plans[0]));
    b.last_form = warm ? 2 : 1;
    ++(warm ? b.geo_warm_runs : b.geo_cold_runs);
}

// ---------------------------------------------------------------------------------------------
// MagLS / MagLS-2D batches (lib/getMagLsFilters.m:30, getMagLsFilters2D.m:1 in a loop over HRIR sets): every plan's stages before
// and after the sweep on the batch's stream (two single-stream graphs) and ONE resident sweep launch for all designs instead
// of one per design.  With geometry sharing (same grid: SH matrix, its Cholesky factor, pinv(Y_conj), the sweep's operands
// G = Y_conj and M = R^-1 R^-H are the same for every set) plan 0 computes that side and the other plans run their HRIR
// prologue and least-squares bins on it.
// ---------------------------------------------------------------------------------------------
// sweep_needed: a resident sweep is a precondition of sharing (LS has no sweep)
void batch_magls_decide_sharing(emagls_batch& b, bool sweep_needed) {
    bool share = false;
    emagls_plan& p0 = *b.plans[0];
    if (b.geo_want && b.plans.size() > 1 && !p0.custom_basis && !p0.diffuse && (p0.sweep_persist || !sweep_needed)) {
        share = batch_inputs_same(b, {"hrir_azi", "hrir_zen"}, b.geo_checked_version, b.geo_inputs_same);
        for (auto* p : b.plans) share = share && !p->custom_basis && p->d.fs == p0.d.fs;
    }
    batch_set_sharing(b, b.geo_share, share);
}
void batch_magls_stage(emagls_batch& b, int part) {
    emagls_plan& g = *b.plans[0];
    StreamLoan loan(b.plans, b.stream);
    if (part == 2) {
        for (auto* p : b.plans) magls_post_sweep(*p);
        return;
    }
    for (size_t j = 0; j < b.plans.size(); ++j) {
        emagls_plan& p = *b.plans[j];
        if (j == 0 || !b.geo_share) { plan_pre_stage(p); continue; }
        // a subject of plan 0's grid: spectra, least-squares bins on plan 0's pinv(Y_conj)
        subject_reset(p, b.stream);
        stage_prologue(p, 0, nullptr, p.D);
        launch_ls_apply(p.get("Hc"), p.ldD, std::min(p.kcut0, p.P), g.get("Ypinv"), g.cplx_basis, g.ldD, (int)p.D, p.C, p.P, 0,
                        std::min(p.kcut0, p.P), p.get("W"), b.stream);
    }
}
void batch_execute_magls(emagls_batch& b) {
    emagls_plan& p0 = *b.plans[0];
    for (auto* p : b.plans)
        if (!p->have_hrirs || (p->custom_basis ? !p->have_basis : !p->have_hrir_grid))
            throw Error(EMAGLS_ERR_ARG, "every plan of the batch needs its grid (or SH matrix) and HRIRs");
    if (p0.d.kind == EMAGLS_KIND_LS) {
        // getLsFilters (lib/getLsFilters.m:30-34) has no sweep: wLs = h pinv(Y).  Sets on one grid: pinv(Y) once (plan 0), one
        // small product per set; otherwise every plan's own pipeline, all on the batch's stream.
        batch_magls_decide_sharing(b, false);
        for (size_t j = 0; j < b.plans.size(); ++j) {
            emagls_plan& p = *b.plans[j];
            {
                Scoped stream(p.stream, b.stream);
                p.stage_names.clear();
                launch_zero(p.get("flag"), sizeof(int) * NFLAG, b.stream);
                if (j == 0 || !b.geo_share) execute_ls(p);
                else launch_ls_filters(p.get<double>("hL"), p.get<double>("hR"), p.d.nsamp, (int)p.D, p0.get("Ypinv"), p0.cplx_basis, p0.ldD, p.C,
                                       p.get("wL"), p.get("wR"), b.stream);
            }
            p.executed = true;
        }
        return;
    }
    bool persist = true;
    for (auto* p : b.plans) persist = persist && p->sweep_persist;
    if (!persist) {   // (an ill-conditioned basis or a sweep that did not become resident: the designs one at a time, launch-per-bin sweeps)
        batch_set_sharing(b, b.geo_share, false);
        for (auto* p : b.plans) {
            Scoped stream(p->stream, b.stream);
            plan_execute(*p);
        }
        return;
    }
    batch_magls_decide_sharing(b, true);
    batch_run_two_graphs(b, b.group[0], batch_magls_stage, 0, 1);
}
// re-run a whole batch after one of its designs raised a recoverable flag: in lane mode all designs share the captured
// graphs, so every plan of the batch changes its configuration together
// Lane mode needs plans of identical shape (same buffers of the same sizes, same derived constants).  Their
// buffers are moved into one arena at a constant stride; the plans keep working on their own afterwards.
// Lane mode launches every kernel once for all designs with the routes of the first one, so the designs of a batch get
// common routes first: the latest start of the Gram route and the most Householder-route orders any of them asks for (both are
// valid for every member: the Householder route is accurate anywhere, more orders only add terms below the noise floor).
// Designs of one simulation-order class but different radii (BASELINE config 4) differ by a bin or an order here.
// returns true when a plan's routes were changed
bool batch_unify_routes_once(emagls_batch& b) {
    int gf = 0, nh = 0;
    bool differ = false;
    for (auto* p : b.plans) {
        if (p->gram_from <= 0 || p->d.kind == EMAGLS_KIND_EMA_SH) return false;
        differ = differ || p->gram_from != b.plans[0]->gram_from || p->n_h != b.plans[0]->n_h;
        gf = std::max(gf, p->gram_from);
        nh = std::max(nh, p->n_h);
    }
    if (!differ) return false;
    for (auto* p : b.plans) {
        if (p->gram_from == gf && p->n_h == nh) continue;
        const int keep_floor = p->gram_floor, keep_nh = p->nh_floor;
        try {
            p->gram_floor = std::max(p->gram_floor, gf);
            p->nh_floor = nh;
            plan_routes(*p);
            plan_alloc_routes(*p);
        } catch (const Error& e) {   // (e.g. more Householder-route orders than the register tile holds: keep the plan's own routes)
            if (sw_on<Sw::DEBUG_LANES>()) fprintf(stderr, "common routes refused: %s\n", e.what());
            p->gram_floor = keep_floor; p->nh_floor = keep_nh;
            plan_routes(*p);
            plan_alloc_routes(*p);
            return false;
        }
        drop_plan_graphs(*p);
    }
    return true;
}
void batch_unify_routes(emagls_batch& b) {
    // (moving a design's route boundary changes the orders its Householder bins need: repeat until nothing moves)
    for (int it = 0; it < 4 && batch_unify_routes_once(b); ++it) {}
}
std::vector<int> batch_read_flags(emagls_batch& b) {
    const size_t n = b.plans.size();
    std::vector<int> flags(NFLAG * n, 0);
    for (size_t j = 0; j < n; ++j)
        HIP_CHECK(hipMemcpyAsync(&flags[NFLAG * j], b.plans[j]->get("flag"), NFLAG * sizeof(int), hipMemcpyDeviceToHost, b.stream));
    HIP_CHECK(hipStreamSynchronize(b.stream));
    return flags;
}
}  // namespace

namespace emagls {
void batch_geo_forget(emagls_batch& b) {
    b.geo_kept_version = ~0ull;
    b.geo_cold_pending = false;
}
// the form the next sharing execute takes while nothing else changes (also asked by the job scheduler: slot_will_capture)
bool batch_geo_next_is_warm(const emagls_batch& b) {
    if (!sw_on<Sw::GEO_KEEP>() || !b.geo_share || b.geo_kept_version == ~0ull || b.geo_kept_version != batch_geo_version(b)) return false;
    for (const emagls_plan* p : b.plans) if (p->prof_level > 0) return false;   // (a profiled plan shows the stages of a whole design)
    return true;
}

void batch_execute(emagls_batch& b) {
    for (auto* p : b.plans)
        if (!p) throw Error(EMAGLS_ERR_ARG, "a plan of this batch has been destroyed");
    b.last_form = 0;
    if (b.atf) { batch_execute_atf(b); return; }
    if (b.magls) { batch_execute_magls(b); return; }
    for (auto* p : b.plans)
        if (!p->have_hrirs || (p->custom_basis ? !p->have_basis : (!p->have_hrir_grid || !p->have_mic_grid)))
            throw Error(EMAGLS_ERR_ARG, "every plan of the batch needs its grids (or SH matrices) and HRIRs");
    batch_geo_decide_sharing(b);
    if (b.geo_share) { batch_execute_geo(b); return; }
    if (b.lanes) {
        batch_execute_lanes(b);
        return;
    }
    const bool replay = b.use_graph && b.eager_runs >= 1 && std::none_of(b.plans.begin(), b.plans.end(), [](const emagls_plan* p) { return forks_streams(*p); });
    batch_run_per_plan(b, replay, plan_pre_stage, emagls_post_sweep, b.plans[0]->P - std::max(b.plans[0]->kcut0, 1));
}
void drop_batch_graphs(emagls_batch& b) {
    for (auto& g : b.group) g.reset();
    for (auto& g : b.group_hh) g.reset();
    b.post.reset();
    b.warm.reset();
    b.eager_runs = 0;
}

// One sweep launch serves every design of a batch: the synthesising form only when all of them qualify
void batch_unify_synth(emagls_batch& b) {
    bool all = true, any = false;
    for (auto* p : b.plans) { all = all && p->synth; any = any || p->synth; }
    if (all || !any) return;
    for (auto* p : b.plans)
        if (p->synth) { p->synth_block = true; plan_alloc_routes(*p); HIP_CHECK(hipStreamSynchronize(p->stream)); drop_plan_graphs(*p); }
}
// Can the resident sweep of the form the batch will launch keep all its workgroups on the device?  Decided before any launch, from the
// runtime's occupancy of that kernel variant (a sweep that cannot be resident would wait for its peers until the time-out); re-evaluated
// whenever the form changes (batch_redo).  A batch that does not fit takes one launch per bin.
void batch_decide_residency(emagls_batch& b) {
    emagls_plan& f0 = *b.plans[0];
    const int n = (int)b.plans.size();
    if (f0.d.kind == EMAGLS_KIND_LS) return;
    bool all_persist = true;
    for (auto* p : b.plans) all_persist = all_persist && p->sweep_persist;
    if (!all_persist) return;
    const int64_t Dh0 = f0.d.kind == EMAGLS_KIND_FROM_ATF ? f0.Dm : f0.D;
    const bool fits = f0.synth ? (reg_sweep_wanted(b.plans.data(), n) || (n <= SWEEP_MULTI_MAX && synth_sweep_fits((int)Dh0, (int)f0.d.nmics, f0.simOrder + 1, n)))
                               : (n <= SWEEP_MULTI_MAX && persist_sweep_fits((int)Dh0, f0.C, n));
    if (fits) return;
    for (auto* p : b.plans) {
        p->sweep_persist = false;
        if (p->synth_want) { plan_alloc_routes(*p); HIP_CHECK(hipStreamSynchronize(p->stream)); }
    }
}

void batch_try_lanes(emagls_batch& b) {
    if (!sw_on<Sw::BATCH_LANES>()) return;
    emagls_plan& q = *b.plans[0];
    if (!q.sweep_persist) return;
    for (auto* p : b.plans)
        if (p->S != q.S || p->simOrder != q.simOrder || p->d.kind != q.d.kind || p->C != q.C || p->P != q.P) return;
    trace_mark("lanes: start");
    batch_unify_routes(b);
    trace_mark("lanes: routes unified");
    batch_unify_synth(b);
    const bool dbg = sw_on<Sw::DEBUG_LANES>();
    for (auto* p : b.plans) {
        if (p->S != q.S || p->simOrder != q.simOrder || p->nOut != q.nOut || p->nfft != q.nfft || p->ldS != q.ldS || p->ldD != q.ldD ||
            p->Dpad != q.Dpad || p->k_cut != q.k_cut || p->cplx_basis != q.cplx_basis || p->out_cplx != q.out_cplx ||
            p->d.kind != q.d.kind || p->d.nsamp != q.d.nsamp || p->d.nmics != q.d.nmics || p->d.len != q.d.len || p->d.order != q.d.order ||
            p->bufs.size() != q.bufs.size()) {
            if (dbg) fprintf(stderr, "lanes refused: shape fields differ (bufs %zu vs %zu, gram_from %d vs %d, n_h %d vs %d)\n", p->bufs.size(),
                             q.bufs.size(), p->gram_from, q.gram_from, p->n_h, q.n_h);
            return;
        }
        auto it = q.bufs.begin();
        for (auto& kv : p->bufs) {
            if (kv.first != it->first || kv.second.bytes != it->second.bytes) {
                if (dbg) fprintf(stderr, "lanes refused: buffer %s %zu vs %s %zu (gram_from %d vs %d, hh_end %d vs %d, n_h %d vs %d)\n", kv.first.c_str(),
                                 kv.second.bytes, it->first.c_str(), it->second.bytes, p->gram_from, q.gram_from, p->hh_end, q.hh_end, p->n_h, q.n_h);
                return;
            }
            ++it;
        }
    }
    size_t stride = 0;
    std::vector<size_t> off;
    for (auto& kv : q.bufs) {
        off.push_back(stride);
        stride += (kv.second.bytes + 255) / 256 * 256;
    }
    stride = (stride + 4095) / 4096 * 4096;
    trace_mark("lanes: shapes compared");
    auto arena = std::make_shared<Arena>();
    {
        const size_t need = stride * b.plans.size();
        arena->base = BlockPool::get().take(need, &arena->bytes, BlockPool::size_class(need + need / 8));
    }
    for (size_t j = 0; j < b.plans.size(); ++j) {   // (one launch per 96 buffers: move_buffers_kernel)
        emagls_plan& p = *b.plans[j];
        size_t i = 0;
        BufferMoves mv{};
        for (auto& kv : p.bufs) {
            char* dst = static_cast<char*>(arena->base) + j * stride + off[i++];
            if ((reinterpret_cast<uintptr_t>(kv.second.p) & 15) != 0) { HIP_CHECK(hipMemcpyAsync(dst, kv.second.p, kv.second.bytes, hipMemcpyDeviceToDevice, b.stream)); continue; }
            mv.src[mv.n] = kv.second.p; mv.dst[mv.n] = dst; mv.bytes[mv.n] = kv.second.bytes;
            if (++mv.n == 96) { launch_move_buffers(mv, b.stream); mv.n = 0; }
        }
        launch_move_buffers(mv, b.stream);
    }
    trace_mark("lanes: arena taken, copies enqueued");
    HIP_CHECK(hipStreamSynchronize(b.stream));   // (every plan's streams were synchronised by the caller: the buffers are final)
    trace_mark("lanes: copies done");
    for (size_t j = 0; j < b.plans.size(); ++j) {
        emagls_plan& p = *b.plans[j];
        size_t i = 0;
        for (auto& kv : p.bufs) {
            if (kv.second.owned) HIP_CHECK(hipFree(kv.second.p));
            kv.second.p = static_cast<char*>(arena->base) + j * stride + off[i++];
            kv.second.owned = false;
        }
        p.release_slabs();
        p.arena = arena;  // (a previous arena is released when its last plan has moved out)
        // the captured graphs hold the old addresses
        drop_plan_graphs(p);
    }
    HIP_CHECK(hipDeviceSynchronize());
    b.lanes = true;
    b.stride = stride;
    {   // more than 8 designs: two lane groups before the sweep (EMAGLS_BATCH_GROUPS=1 keeps one launch sequence for all lanes, 3 / 4
        // allow groups of 8 for 17 ... 32 designs: measured with 32-design batches, 3125 / 3345 sets/s at 128 / 512 steps with four
        // groups against 3296 / 3499 with two, and the same 2070 at 20 steps)
        b.groups = std::max(1, std::min(sw_int<Sw::BATCH_GROUPS>(), (int)ceil_div((int64_t)b.plans.size(), 8)));
    }
}

void batch_redo(emagls_batch& b, const std::vector<int>& flags) {
    int any[NFLAG] = {};
    for (size_t j = 0; j < b.plans.size(); ++j) for (int i = 0; i < NFLAG; ++i) any[i] = std::max(any[i], flags[NFLAG * j + i]);
    bool moved = false;
    for (auto* q : b.plans) {
        const int64_t before = q->total_bytes;
        plan_recover(*q, any, true);
        moved = moved || q->total_bytes != before;
        drop_plan_graphs(*q);
    }
    drop_batch_graphs(b);
    batch_geo_forget(b);   // (routes, sweep form or lane layout change: a sharing batch runs its geometry stages again)
    {
        const std::vector<int64_t> before = [&] { std::vector<int64_t> v; for (auto* q : b.plans) v.push_back(q->total_bytes); return v; }();
        batch_unify_synth(b);
        batch_decide_residency(b);   // (the form may have changed: the residency of the kernel that will be launched)
        for (size_t j = 0; j < b.plans.size(); ++j) moved = moved || b.plans[j]->total_bytes != before[j];
    }
    if (b.lanes && moved) {   // re-allocated buffers left the arena: lane mode needs them at the common stride again
        b.lanes = false;
        batch_try_lanes(b);
    }
    batch_execute(b);
    HIP_CHECK(hipStreamSynchronize(b.stream));
}
void plan_check_flags(emagls_plan& p) {
    int flag[NFLAG] = {};
    HIP_CHECK(hipMemcpy(flag, p.get("flag"), sizeof flag, hipMemcpyDeviceToHost));
    if (plan_recover(p, flag, false)) {
        if (p.owner) {   // a member of a batch: the batch re-runs as a whole (its graphs cover every member)
            emagls_batch& b = *p.owner;
            for (auto* q : b.plans) if (!q) throw Error(EMAGLS_ERR_ARG, "a plan of this batch has been destroyed");
            batch_redo(b, batch_read_flags(b));
        } else {
            plan_recover(p, flag, true);
            drop_plan_graphs(p);
            plan_execute(p);
            HIP_CHECK(hipStreamSynchronize(p.stream));
        }
        HIP_CHECK(hipMemcpy(flag, p.get("flag"), sizeof flag, hipMemcpyDeviceToHost));
        if (plan_recover(p, flag, false)) {   // e.g. first the Gram route, then the persistent sweep
            if (p.owner) batch_redo(*p.owner, batch_read_flags(*p.owner));
            else { plan_recover(p, flag, true); drop_plan_graphs(p); plan_execute(p); HIP_CHECK(hipStreamSynchronize(p.stream)); }
            HIP_CHECK(hipMemcpy(flag, p.get("flag"), sizeof flag, hipMemcpyDeviceToHost));
        }
    }
    if (p.persist_suspended) {   // (the re-run on the launch-per-bin sweep is done: the next call starts on the persistent form again)
        p.persist_suspended = false;
        p.sweep_persist = true;
    }
    throw_fatal_flags(flag);
    p.geo_done_version = p.geo_run_version;   // (clean: a later set on the same grids may keep this run's geometry stages)
}
}  // namespace emagls
