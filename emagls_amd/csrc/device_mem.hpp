// Owners of device memory outside the plans' slabs and arenas, and of hipFFT plans: one block (DevMem), one plan (FftPlan), and
// the scratch of one host-array call of the C ABI (Scratch).  Each frees in its destructor, on every exit path.
// Caches that live for the whole process must not run these destructors at exit (the HIP runtime may be gone by then): such a
// cache is held through the never-destroyed idiom, static T& get() { static T* p = new T; return *p; }, and released by
// emagls_cache_clear() alone.
#pragma once
#include <hipfft/hipfft.h>

#include <algorithm>
#include <deque>

#include "kernels.hpp"

namespace emagls {

// one hipMalloc'ed block
struct DevMem {
    DevMem() = default;
    explicit DevMem(size_t bytes) { alloc(bytes); }
    DevMem(DevMem&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevMem() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    void alloc(size_t bytes) {
        reset();
        HIP_CHECK(hipMalloc(&p_, bytes));
        cap_ = bytes;
    }
    // grown on demand and kept: the block stays while its capacity suffices
    void grow(size_t bytes) {
        bytes = std::max<size_t>(bytes, 16);
        if (bytes > cap_) alloc(bytes);
    }
    template <typename T = void> T* get() const { return static_cast<T*>(p_); }
    size_t capacity() const { return cap_; }

private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

// one hipFFT plan
struct FftPlan {
    FftPlan() = default;
    FftPlan(FftPlan&& o) noexcept : h_(o.h_) { o.h_ = 0; }
    FftPlan& operator=(FftPlan&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = 0; }
        return *this;
    }
    ~FftPlan() { reset(); }
    void reset() {
        if (h_) (void)hipfftDestroy(h_);
        h_ = 0;
    }
    hipfftHandle* fresh() { reset(); return &h_; }   // where hipfftPlanMany writes the plan
    operator hipfftHandle() const { return h_; }

private:
    hipfftHandle h_ = 0;
};

// device buffers and a pool stream of one host call
struct Scratch {
    std::deque<DevMem> bufs;
    hipStream_t st = nullptr;
    Scratch() { st = pool_stream_take(); }
    ~Scratch() {
        bufs.clear();
        pool_stream_give(st);
    }
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    template <typename T = void> T* get(size_t bytes, bool zero = false) {
        bufs.emplace_back(bytes ? bytes : 16);
        T* p = bufs.back().get<T>();
        if (zero) HIP_CHECK(hipMemsetAsync(p, 0, bytes, st));
        return p;
    }
    // a device copy of src[count], host or device memory
    template <typename T> T* put(const T* src, size_t count) {
        T* p = get<T>(sizeof(T) * count);
        HIP_CHECK(hipMemcpyAsync(p, src, sizeof(T) * count, hipMemcpyDefault, st));
        return p;
    }
    // the same of an array that may be absent: null for none
    template <typename T> const T* put_opt(const T* src, size_t count) { return src && count ? put(src, count) : nullptr; }
    void sync() { HIP_CHECK(hipStreamSynchronize(st)); }
};

}  // namespace emagls
