// The one reader of the environment (switches.hpp).  Everything here is constant-initialised: the table is a constexpr array and the
// cache of the once-per-process switches is zero-initialised atomics, so a query during the static initialisation of another file
// (g_batch_max, capi.hip) finds them ready.
#include "switches.hpp"

#include <algorithm>
#include <atomic>
#include <cstdlib>

namespace emagls {
namespace {

enum class SwWhen { PROCESS, CALL };
struct SwRow { const char* name; SwKind kind; double def, lo, hi; SwWhen when; };
constexpr SwRow kRows[] = {
#define X(name, kind, def, lo, hi, when, doc) {"EMAGLS_" #name, SwKind::kind, def, lo, hi, SwWhen::when},
    EMAGLS_SWITCHES(X)
#undef X
};
constexpr int kCount = (int)Sw::COUNT;

double parse(const SwRow& r) {
    const char* e = getenv(r.name);
    if (!e) return r.def;
    switch (r.kind) {
        case SwKind::ON0: return e[0] != '0';
        case SwKind::ON1: return e[0] == '1';
        case SwKind::ONH: return e[0] == 'h';
        case SwKind::INT: return std::max(r.lo, std::min(r.hi, (double)atoi(e)));
        default: return std::max(r.lo, std::min(r.hi, atof(e)));
    }
}

// PROCESS switches: a load after the first query (threads that race to it parse the same environment and store the same value)
std::atomic<bool> g_known[kCount];
std::atomic<double> g_value[kCount];

}  // namespace

double sw_value(Sw s) {
    const int i = (int)s;
    const SwRow& r = kRows[i];
    if (r.when == SwWhen::CALL) return parse(r);
    if (!g_known[i].load(std::memory_order_acquire)) {
        g_value[i].store(parse(r), std::memory_order_relaxed);
        g_known[i].store(true, std::memory_order_release);
    }
    return g_value[i].load(std::memory_order_relaxed);
}

}  // namespace emagls
