// Device scratch of one host-array call of the C ABI (render_api.hip, response_api.hip).
#pragma once
#include <vector>

#include "kernels.hpp"

namespace emagls {

// device scratch of one call, freed on every exit path
struct Scratch {
    std::vector<void*> ptrs;
    hipStream_t st = nullptr;
    Scratch() { st = pool_stream_take(); }
    ~Scratch() {
        for (void* p : ptrs) hipFree(p);
        pool_stream_give(st);
    }
    template <typename T = void> T* get(size_t bytes, bool zero = false) {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16));
        ptrs.push_back(p);
        if (zero) HIP_CHECK(hipMemsetAsync(p, 0, bytes, st));
        return reinterpret_cast<T*>(p);
    }
    template <typename T> T* put(const T* host, size_t count) {
        T* p = get<T>(sizeof(T) * count);
        HIP_CHECK(hipMemcpyAsync(p, host, sizeof(T) * count, hipMemcpyHostToDevice, st));
        return p;
    }
    void sync() { HIP_CHECK(hipStreamSynchronize(st)); }
};

}  // namespace emagls
