// The state every host file shares: the thread's last-error string and the one place that writes it, the job lists' trace marks,
// and the stream pool's entry points for the other C ABI files (the pools themselves are header-only: host_internal.hpp).
#include "host_internal.hpp"

namespace emagls {

thread_local std::string g_last_error;
// EMAGLS_JOBS_TRACE=1: wall-clock marks of the job lists' host-side phases on stderr
void trace_mark(const char* what) {
    if (!sw_on<Sw::JOBS_TRACE>()) return;
    static const auto t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "emagls trace: %-44s %.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

}  // namespace emagls

hipStream_t emagls::pool_stream_take() { return StreamPool::get().take(); }
void emagls::pool_stream_give(hipStream_t st) { StreamPool::get().give(st); }
int emagls::guarded_call(const std::function<void()>& f) {
    try {
        f();
        return EMAGLS_OK;
    } catch (const Error& e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return EMAGLS_ERR_HIP;
    }
}
