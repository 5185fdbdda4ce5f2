// Every environment switch libemagls.so reads, declared once: name, kind, default, clamp, read time.  DESIGN.md section 8 lists the
// same rows in the same order, and tests/test_switches_host.py holds the two (and the names the tests and tools set) together.
// No other file under csrc/ calls getenv.
//
//   X(name, kind, default, lo, hi, when, description)       the variable is EMAGLS_<name>
//   kind   ON0   flag, on unless the value starts with '0'  (default 1)
//          ON1   flag, on only if the value starts with '1' (default 0)
//          ONH   flag, on only if the value starts with 'h' (default 0; EMAGLS_DECODE_FILTER_FFT=hipfft)
//          INT   atoi of the value, clamped to lo .. hi;  REAL  atof of the value, clamped to lo .. hi
//          (the default stands for "unset" and is not clamped: 0 often means "decided by the library")
//   when   PROCESS  parsed at the first query, that value for the rest of the process
//          CALL     parsed at every query (every launch, or every plan / batch creation: the call site decides); tests switch these
//                   forms inside one process
#pragma once
#include <climits>
#include <cmath>

namespace emagls {

#define EMAGLS_SWITCHES(X) \
    X(PLAN_CACHE,        INT,  4,     0, INT_MAX,   PROCESS, "shapes the one-shot entry points keep alive (0 = off)") \
    X(BATCH_MAX,         INT,  8,     1, 32,        PROCESS, "initial limit of designs per batch, read at load time (emagls_set_batch_max changes it at run time; the job scheduler sets it per chunk)") \
    X(BATCH_GROUPS,      INT,  2,     1, 4,         CALL,    "lane groups of a batch of more than 8 designs before its sweep (1 = one launch sequence)") \
    X(BATCH_LANES,       ON0,  1,     0, 1,         CALL,    "=0: batches in stream mode (per-plan pipelines) instead of lane mode") \
    X(DEBUG_LANES,       ON1,  0,     0, 1,         CALL,    "=1: why a batch was refused lane mode or common routes, on stderr") \
    X(STAGGER,           ON0,  1,     0, 1,         PROCESS, "=0: both lane groups of a batch issue the stages before the sweep in one order (default: complementary orders)") \
    X(DEFER_HH,          INT,  1,     0, 2,         PROCESS, "the orthonormal route of the low bins next to the sweep: 0 never, 1 batches and designs that have the device to themselves, 2 every lane batch") \
    X(GEO_KEEP,          ON0,  1,     0, 1,         PROCESS, "=0: sharing batches run their geometry stages on every execute") \
    X(GEO_LS_SHARED,     ON0,  1,     0, 1,         CALL,    "=0: sharing batches carry every HRIR set's least-squares rows through the factors instead of one kept Y_reg_inv per bin") \
    X(GRAM_LDS,          ON0,  1,     0, 1,         PROCESS, "=0: lane batches take the K-split Gram kernel + reduce instead of the LDS-staged one") \
    X(GRAM_MFMA4,        ON1,  0,     0, 1,         CALL,    "=1: the Gram tile on the 4 x 4 x 4 MFMA shape (measured slower; the tests' second form)") \
    X(XCD_RUNS,          ON0,  1,     0, 1,         PROCESS, "=0: gram_lds, gemm_tn_f64, synth_ls take their tiles in dispatch order instead of XCD-aware runs") \
    X(GRAM_ROUTE,        ON0,  1,     0, 1,         CALL,    "=0: no Gram route (all bins Householder + Jacobi)") \
    X(GRAM_COND_EST,     REAL, 3e3,   -HUGE_VAL, HUGE_VAL, CALL, "conditioning estimate below which the Gram route starts (the device check stays at 3e4)") \
    X(JACOBI_RUN,        INT,  0,     1, INT_MAX,   PROCESS, "bins per Jacobi workgroup on the Gram route (0: single bins where the stages are forked, runs of 2 in lane groups)") \
    X(REAL_INTERNAL,     ON0,  1,     0, 1,         CALL,    "=0: complex-basis eMagLS / eMagLS2 designs on the complex-arithmetic pipeline") \
    X(NO_GRAPH,          ON1,  0,     0, 1,         CALL,    "=1: eager launches instead of hipGraph replay (plans and batches, when they are created)") \
    X(STREAMS,           INT,  0,     1, 4,         CALL,    "streams of a single plan (0: one, until emagls_plan_set_streams)") \
    X(ONESHOT_STREAMS,   INT,  1,     1, 3,         CALL,    "streams of the one-shot plans of array designs") \
    X(SWEEP_PERSIST,     ON0,  1,     0, 1,         CALL,    "=0: launch-per-bin sweep instead of the persistent one") \
    X(PERSIST_GLOBAL,    ON1,  0,     0, 1,         CALL,    "=1: write-through granules even when a design sits on one XCD") \
    X(SWEEP_SYNTH,       ON0,  1,     0, 1,         CALL,    "=0: array designs on materialised operands instead of the synthesising sweep (when a plan is created)") \
    X(SWEEP_TWIN,        ON0,  1,     0, 1,         CALL,    "=0: launches of 9-16 designs as two independent workgroups per CU instead of twin workgroups") \
    X(SWEEP_REG,         INT,  1,     0, 2,         CALL,    "register-resident sweep: 0 never (the slab form), 1 for launches of more than 8 designs, 2 always") \
    X(REG_WAVES,         INT,  0,     INT_MIN, INT_MAX, CALL, "waves per workgroup of the register-resident sweep (4, 6, 8, 10, 12 whenever it fits; 0: the smallest count with which every workgroup owns a CU)") \
    X(REG_SPREAD,        INT,  2,     0, 2,         CALL,    "a launch's designs spread over all XCDs: 0 never, 1 whenever it fits, 2 when it needs fewer waves per workgroup than the one-XCD layout") \
    X(REG_PRIO,          INT,  1,     INT_MIN, INT_MAX, PROCESS, "=0: the register-resident sweep's waves at the default issue priority") \
    X(SWEEP_FETCH,       INT,  0,     0, 4,         PROCESS, "where the persistent sweep requests the next bin's operands") \
    X(SWEEP_WAIT_MS,     INT,  20,    1, INT_MAX,   PROCESS, "wall-clock limit of a wait for peers inside a resident sweep, in ms") \
    X(SWEEP_TIMING,      ON1,  0,     0, 1,         CALL,    "=1: in-kernel wall-clock stamps of the persistent sweep (when a plan is created)") \
    X(CU_BUDGET,         INT,  0,     0, INT_MAX,   CALL,    "CUs the resident sweeps may count on when their residency is decided (0: the device's)") \
    X(SYNTH_PAIRS,       ON0,  1,     0, 1,         PROCESS, "=0: synthesising sweep without antipodal microphone pairs") \
    X(SYNTH_SPLIT,       INT,  67,    INT_MIN, INT_MAX, PROCESS, "synthesising sweep: per cent of the producers' unit groups evaluated before barrier B1") \
    X(SYNTH_PRIO,        INT,  5,     0, 5,         PROCESS, "synthesising sweep: issue priorities (5: the chains of the two designs of an XCD tilted against the age order; 0: all chains 3, producers 0)") \
    X(STREAM_POOL,       ON0,  1,     0, 1,         PROCESS, "=0: destroy streams instead of recycling them (exposes a HIP runtime crash in long sessions)") \
    X(STREAM_WARM,       INT,  8,     0, INT_MAX,   PROCESS, "streams the pool parks before it hands the first one out") \
    X(POOL_GB,           INT,  128,   0, INT_MAX,   PROCESS, "device memory the block pool keeps for the next plans and arenas, in GB") \
    X(JOBS_FORK,         INT,  3,     1, 4,         PROCESS, "job scheduler: streams of a job list that is a single chunk (1 = lane groups as for chunks in flight)") \
    X(JOBS_RESIDENT,     INT,  0,     0, INT_MAX,   CALL,    "job scheduler: designs whose plans and batches stay resident between calls (0: max(256, 2 x batch x in flight))") \
    X(JOBS_AUTO_SHARE,   ON0,  1,     0, 1,         PROCESS, "=0: job scheduler shares no geometry unless the caller asks") \
    X(JOBS_TRACE,        ON1,  0,     0, 1,         PROCESS, "=1: time stamps of every chunk's steps and of block pool misses on stderr") \
    X(HRIR_FFT_WAVE,     ON0,  1,     0, 1,         CALL,    "=0: the HRIR prologue at nfft = 1024 on the LDS radix-2^2 transform instead of wave-private transforms") \
    X(HRIR_FFT_LDS_KB,   INT,  0,     40, 158,      CALL,    "LDS budget of the LDS-form HRIR transform's sub-tiles (0: 83, 110 at nfft = 2048)") \
    X(DECODE_FUSED,      ON0,  1,     0, 1,         CALL,    "=0: binauralDecode on the hipFFT passes for every filter length") \
    X(DECODE_REGFFT,     ON0,  1,     0, 1,         CALL,    "=0: the fused decode kernel on LDS transform passes also up to 512 taps") \
    X(DECODE_WAVE,       ON0,  1,     0, 1,         CALL,    "=0: the half-wave two-factor decode form also at 257-512 taps") \
    X(DECODE_FILTER_FFT, ONH,  0,     0, 1,         CALL,    "=hipfft: the filter side of the decode's wave form through hipFFT") \
    X(WA_REG,            ON0,  1,     0, 1,         CALL,    "=0: the 33-64-channel path's Householder kernels walk the columns through L2") \
    X(WA_TALL,           ON0,  1,     0, 1,         CALL,    "=0: the plain Householder kernels for problems of more than 448 rows instead of the LDS-reflector forms") \
    X(WA_YRI_MFMA,       ON0,  1,     0, 1,         CALL,    "=0: the 33-64-channel path's Y_reg_inv_k product on the vector pipe") \
    X(WA_JACOBI_FLAG,    REAL, 1e-14, -HUGE_VAL, HUGE_VAL, PROCESS, "the 33-64-channel path's Jacobi: another sweep follows one in which some rotation had |gamma| > x sqrt(alpha beta)") \
    X(WA_LEAF_ROWS,      INT,  0,     INT_MIN, INT_MAX, PROCESS, "tiled QR: upper bound of the leaf height, 1024 .. 4096 (anything else: 3072)")

enum class Sw : int {
#define X(name, kind, def, lo, hi, when, doc) name,
    EMAGLS_SWITCHES(X)
#undef X
    COUNT
};
enum class SwKind { ON0, ON1, ONH, INT, REAL };
constexpr SwKind sw_kind(Sw s) {
    constexpr SwKind kinds[] = {
#define X(name, kind, def, lo, hi, when, doc) SwKind::kind,
        EMAGLS_SWITCHES(X)
#undef X
    };
    return kinds[(int)s];
}

double sw_value(Sw s);   // switches.hip: the parsed value (flags: 0 / 1); usable during static initialisation of any file

// the accessors: the switch is an enumerator (a misspelt name does not compile) and its kind is checked against the table
template <Sw S> inline bool sw_on() {
    static_assert(sw_kind(S) == SwKind::ON0 || sw_kind(S) == SwKind::ON1 || sw_kind(S) == SwKind::ONH, "not a flag");
    return sw_value(S) != 0.0;
}
template <Sw S> inline int sw_int() { static_assert(sw_kind(S) == SwKind::INT, "not an integer switch"); return (int)sw_value(S); }
template <Sw S> inline double sw_real() { static_assert(sw_kind(S) == SwKind::REAL, "not a real switch"); return sw_value(S); }

}  // namespace emagls
