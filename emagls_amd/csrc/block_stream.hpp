// The host skeleton of the block-stream objects of the C ABI (decode_api.hip: the decode stream and the listener group;
// field_api.hip: the field stream): the lock, the device the object is bound to, its lazily built device side, the stage buffers of
// the host entries, and the frames of create, push, reset and destroy.  The argument checks, the shapes, the staging and the
// launches stay with the objects: the frames take them as callables and run inside the entry's guarded_call.
//
// An object derives from BlockStreamObject<itself, stage buffers> and has
//   void build_device();   its device buffers, the partition spectra, zero state (mu held, device current)
//   void drop_device();    lets go of those buffers; also called when build_device() threw
#pragma once
#include <mutex>

#include "device_mem.hpp"

namespace emagls {

template <typename Derived, int NStage>
struct BlockStreamObject {
    std::mutex mu;
    int device = -1;          // bound at the first use of the device (creation, when there is one)
    bool ready = false;
    DevMem stage[NStage];     // host entries: a push's arrays on the device, grown on demand and kept
    template <typename T> T* staged(int i, size_t bytes) {
        stage[i].grow(bytes);
        return stage[i].template get<T>();
    }
    // the device side, once (mu held)
    void ensure_device() {
        if (ready) return;
        HIP_CHECK(hipGetDevice(&device));
        try {
            self().build_device();
        } catch (...) { drop(); device = -1; throw; }
        ready = true;
    }
    // creation: on the device when the process has one; without one the first push or reset builds the device side
    void create_device_side() {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
            std::lock_guard<std::mutex> lk(mu);
            ensure_device();
        } else {
            (void)hipGetLastError();
        }
    }
    // a push of device arrays: run() on the object's device
    template <typename F> void device_frame(F&& run) {
        std::lock_guard<std::mutex> lk(mu);
        DeviceGuard dg(device);
        run();
    }
    // a push of host arrays: run(st) stages, pushes and copies back on a pool stream, which is synchronised afterwards
    template <typename F> void host_frame(F&& run) {
        std::lock_guard<std::mutex> lk(mu);
        DeviceGuard dg(device);
        ensure_device();
        hipStream_t st = pool_stream_take();
        struct Give { hipStream_t st; ~Give() { pool_stream_give(st); } } give{st};
        run(st);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    // a reset: zero(st) on the null stream, after the pushes in flight on whatever stream
    template <typename F> void reset_frame(F&& zero) {
        std::lock_guard<std::mutex> lk(mu);
        DeviceGuard dg(device);
        ensure_device();
        HIP_CHECK(hipDeviceSynchronize());
        zero((hipStream_t) nullptr);
        HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    // the body of the destroy entries (null: nothing)
    static int destroy(Derived* o) {
        return guarded_call([&] {
            if (!o) return;
            {
                std::lock_guard<std::mutex> lk(o->mu);
                if (o->ready) {
                    DeviceGuard dg(o->device);
                    (void)hipDeviceSynchronize();
                    o->drop();
                }
            }
            delete o;
        });
    }

private:
    Derived& self() { return static_cast<Derived&>(*this); }
    void drop() {
        self().drop_device();
        for (DevMem& m : stage) m.reset();
        ready = false;
    }
};

}  // namespace emagls
