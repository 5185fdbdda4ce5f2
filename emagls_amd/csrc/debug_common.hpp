// What the debug entries (factor_debug.hip, fft_debug.hip) share: the sentinel their outputs are filled with before a launch, and the
// device buffers of one call.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"

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

// device buffers of one call: freed together, whatever happens
struct Bufs {
    std::vector<void*> all;
    ~Bufs() { for (void* p : all) hipFree(p); }
    template <typename T> T* get(size_t n) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        all.push_back(p);
        return static_cast<T*>(p);
    }
    template <typename T> T* filled(size_t n, double v) {   // n values of T, every double of them = v
        std::vector<double> h(std::max<size_t>(n, 1) * sizeof(T) / sizeof(double), v);
        T* p = get<T>(n);
        HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        return p;
    }
    template <typename T> T* copy(const void* src, size_t n) {
        T* p = get<T>(n);
        HIP_CHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
};

}  // namespace debug
}  // namespace emagls
