// What the debug entries (factor_debug.hip, fft_debug.hip, gram_debug.hip) share: the sentinel their outputs are filled with before a launch, and the
// filling of one call's device buffers (a Scratch of device_mem.hpp).
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "device_mem.hpp"

namespace emagls {
namespace debug {

// what the outputs hold where the launcher wrote nothing: a quiet NaN with a payload of its own (EMAGLS_DEBUG_SENTINEL_BITS)
inline double sentinel() {
    const uint64_t bits = 0x7ff8dead0000beefULL;
    double v;
    std::memcpy(&v, &bits, sizeof v);
    return v;
}
inline void fill_sentinel(void* p, size_t ndoubles) {
    const double v = sentinel();
    double* d = static_cast<double*>(p);
    for (size_t i = 0; i < ndoubles; ++i) d[i] = v;
}

// the debug entries' device buffers are a Scratch's; their copies are synchronous
template <typename T> T* filled(Scratch& s, size_t n, double v) {   // n values of T, every double of them = v
    std::vector<double> h(std::max<size_t>(n, 1) * sizeof(T) / sizeof(double), v);
    T* p = s.get<T>(h.size() * sizeof(double));
    HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return p;
}
template <typename T> T* copy(Scratch& s, const void* src, size_t n) {
    T* p = s.get<T>(n * sizeof(T));
    HIP_CHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

}  // namespace debug
}  // namespace emagls
