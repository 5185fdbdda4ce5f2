// C ABI of the field stream and its bank of response sets (include/emagls.h: emagls_field_stream_*; DESIGN.md sections 9.7 and 9.8): the argument check, the shapes, the
// staging and the launches of the object; the lock, the lazily built device side, the stage buffers and the frames of create, push,
// reset and destroy are the shared skeleton's (BlockStreamObject, block_stream.hpp).  The kernels are field_stream.hip's and, for the
// response spectra, decode_stream.hip's.  The object owns its device buffers: emagls_cache_clear() does not reach them.
// No CPU fallback.
#include <memory>
#include <string>
#include <vector>

#include "../../include/emagls.h"
#include "block_stream.hpp"

using namespace emagls;

struct emagls_field_stream : BlockStreamObject<emagls_field_stream, 3> {   // stage: the push's input, output and set indices
    int64_t nch = 0, nr = 0;
    std::vector<double> rpl;      // [S][nsrc][planes][nr] the real response planes, until the device has their spectra
    FieldStreamState d;           // the launchers' view of mem
    struct Mem { DevMem Rf, ring, hist, pos, tag, sel; } mem;   // (tag, sel: a bank's, section 9.8)
    bool bank() const { return d.S > 1; }
    size_t ring_bytes() const { return sizeof(cplx) * (size_t)d.nsrc * d.P * (bank() ? kFieldStreamEntries : 1) * (d.B + 1); }
    size_t hist_bytes() const { return sizeof(double) * (size_t)d.nsrc * d.B; }
    size_t tag_bytes() const { return bank() ? sizeof(int) * (size_t)d.nsrc * d.P * kFieldStreamEntries : 0; }
    size_t sel_bytes() const { return bank() ? sizeof(int) * (size_t)d.nsrc * 2 : 0; }
    size_t state_bytes() const { return ring_bytes() + hist_bytes() + sizeof(int) + tag_bytes() + sel_bytes(); }
    size_t response_bytes() const { return sizeof(cplx) * (size_t)d.S * d.nsrc * d.P * d.planes * (d.B + 1); }
    size_t out_esz() const { return esz(d.out_c); }
    void bind() {
        d.Rf = mem.Rf.get<cplx>(); d.ring = mem.ring.get<cplx>(); d.hist = mem.hist.get<double>(); d.pos = mem.pos.get<int>();
        d.tag = mem.tag.get<int>(); d.sel = mem.sel.get<int>();
    }
    void zero_state(hipStream_t st) {
        HIP_CHECK(hipMemsetAsync(d.ring, 0, ring_bytes(), st));
        HIP_CHECK(hipMemsetAsync(d.hist, 0, hist_bytes(), st));
        HIP_CHECK(hipMemsetAsync(d.pos, 0, sizeof(int), st));
        if (bank()) {   // every entry empty, no previous index: all bits set is -1
            HIP_CHECK(hipMemsetAsync(d.tag, 0xff, tag_bytes(), st));
            HIP_CHECK(hipMemsetAsync(d.sel, 0xff, sel_bytes(), st));
        }
    }
    void build_device() {
        mem.Rf.alloc(response_bytes());
        mem.ring.alloc(ring_bytes());
        mem.hist.alloc(hist_bytes());
        mem.pos.alloc(sizeof(int));
        if (bank()) { mem.tag.alloc(tag_bytes()); mem.sel.alloc(sel_bytes()); }
        bind();
        Scratch s;
        launch_partition_spectra(s.put(rpl.data(), rpl.size()), d.planes, nr, d.B, d.P, (int64_t)d.S * d.nsrc, d.Rf, s.st);
        zero_state(s.st);
        s.sync();
        rpl = std::vector<double>();
    }
    void drop_device() { mem = Mem(); bind(); }
};

namespace {

constexpr int64_t kFieldMaxSources = kFieldStreamMaxSources, kFieldMaxChannels = 256, kFieldMaxTaps = 1048576;
constexpr int64_t kFieldMaxSets = 65536;
constexpr uint64_t kFieldMaxSpectraBytes = 4ull << 30;

// the set indices of a push: n_set = 0, nsrc, or nsrc * nsamp / block; host: the array can be read, and every index is checked
void check_push(const emagls_field_stream* f, const void* src, const void* out, int64_t nsamp, const int32_t* set, int64_t n_set, bool host) {
    if (!f) throw Error(EMAGLS_ERR_ARG, "null field stream");
    if (!src || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
    if (nsamp < 0 || nsamp % f->d.B) throw Error(EMAGLS_ERR_ARG, "a push needs a multiple of the block size of samples");
    if (n_set != 0 && n_set != f->d.nsrc && n_set != f->d.nsrc * (nsamp / f->d.B))
        throw Error(EMAGLS_ERR_ARG, "set indices: one per source, or one per source and block ([nsrc][nsamp / block]), or none");
    if (n_set > 0 && !set) throw Error(EMAGLS_ERR_ARG, "null set index array");
    if (host)
        for (int64_t i = 0; i < n_set; ++i)
            if (set[i] < 0 || set[i] >= f->d.S)
                throw Error(EMAGLS_ERR_ARG, "set index " + std::to_string(set[i]) + " outside [0, " + std::to_string(f->d.S - 1) + "]");
}

// The blocks of a push in order on st, two launches each; device pointers; not synchronised (f->mu held, device current).
// d_src [nsrc][nsamp], d_out [nch][nsamp]; d_set [n_set] (section 9.8; a stream of one set does not look at it)
void push_blocks(emagls_field_stream* f, const double* d_src, int64_t nsamp, const int32_t* d_set, int64_t n_set, void* d_out, hipStream_t st) {
    f->ensure_device();
    const int64_t B = f->d.B, nb = nsamp / B;
    const bool per_block = n_set != f->d.nsrc;   // [nsrc][nb]: block b's indices lie nb apart
    for (int64_t b = 0; b < nb; ++b) {
        const int* set = !f->bank() || n_set == 0 ? nullptr : per_block ? d_set + b : d_set;
        launch_field_stream_block(f->d, d_src + b * B, nsamp, set, per_block ? nb : 1, (char*)d_out + f->out_esz() * (size_t)(b * B), nsamp, st);
    }
}

void create_bank(int64_t nsrc, int64_t nch, int64_t n_sets, const void* rir, int rir_is_complex, int64_t nr, int64_t block,
                 emagls_field_stream** out) {
    if (!rir || !out) throw Error(EMAGLS_ERR_ARG, "null pointer");
    *out = nullptr;
    if (nsrc < 1 || nch < 1 || nr < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape");
    if (n_sets < 1) throw Error(EMAGLS_ERR_ARG, "a bank needs at least one response set");
    if (n_sets > kFieldMaxSets) throw Error(EMAGLS_ERR_UNSUPPORTED, "the field stream supports banks of up to 65536 response sets");
    if (nsrc > kFieldMaxSources) throw Error(EMAGLS_ERR_UNSUPPORTED, "the field stream supports 1 to 16 sources");
    if (nch > kFieldMaxChannels) throw Error(EMAGLS_ERR_UNSUPPORTED, "the field stream supports 1 to 256 channels");
    if (nr > kFieldMaxTaps) throw Error(EMAGLS_ERR_UNSUPPORTED, "the field stream supports responses of up to 1048576 taps");
    if (!decode_stream_block_ok(block))
        throw Error(EMAGLS_ERR_UNSUPPORTED, "the field stream supports block sizes 64, 128, 256, 512, 1024 and 2048");
    const bool rc = rir_is_complex != 0;
    const int64_t P = ceil_div(nr, block), planes = rc ? 2 * nch : nch;
    // (no factor overflows: n_sets nsrc P < 2^37, planes (block + 1) 16 < 2^25)
    if ((uint64_t)n_sets * (uint64_t)nsrc * (uint64_t)P * (uint64_t)planes * (uint64_t)(block + 1) * sizeof(cplx) > kFieldMaxSpectraBytes)
        throw Error(EMAGLS_ERR_UNSUPPORTED,
                    "the field stream supports response spectra of up to 4 GiB (n_sets nsrc ceil(nr / block) planes (block + 1) 16 bytes)");
    std::unique_ptr<emagls_field_stream> f(new emagls_field_stream);
    f->nch = nch; f->nr = nr;
    f->d.nsrc = (int)nsrc; f->d.planes = (int)planes; f->d.out_c = rc; f->d.B = (int)block; f->d.P = (int)P; f->d.S = (int)n_sets;
    // [nr x nch] column-major is [nch][nr] planes as it lies; a complex response is parted into plane 2c = re, 2c + 1 = im
    const double* r = reinterpret_cast<const double*>(rir);
    const size_t cols = (size_t)n_sets * nsrc * nch, total = cols * nr;
    if (!rc) f->rpl.assign(r, r + total);
    else {
        f->rpl.resize(2 * total);
        for (size_t col = 0; col < cols; ++col)
            for (int64_t t = 0; t < nr; ++t) {
                f->rpl[(2 * col) * nr + t] = r[2 * (col * nr + t)];
                f->rpl[(2 * col + 1) * nr + t] = r[2 * (col * nr + t) + 1];
            }
    }
    f->create_device_side();
    *out = f.release();
}

}  // namespace

extern "C" {

int emagls_field_stream_create(int64_t nsrc, int64_t nch, const void* rir, int rir_is_complex, int64_t nr, int64_t block,
                               emagls_field_stream** out) {
    return guarded_call([&] { create_bank(nsrc, nch, 1, rir, rir_is_complex, nr, block, out); });
}

int emagls_field_stream_create_bank(int64_t nsrc, int64_t nch, int64_t n_sets, const void* rir, int rir_is_complex, int64_t nr, int64_t block,
                                    emagls_field_stream** out) {
    return guarded_call([&] { create_bank(nsrc, nch, n_sets, rir, rir_is_complex, nr, block, out); });
}

int emagls_field_stream_push_sets_device(emagls_field_stream* f, const double* d_src, int64_t nsamp, const int32_t* d_set, int64_t n_set,
                                         void* d_out, void* stream) {
    return guarded_call([&] {
        check_push(f, d_src, d_out, nsamp, d_set, n_set, false);
        if (nsamp == 0) return;
        f->device_frame([&] { push_blocks(f, d_src, nsamp, d_set, n_set, d_out, (hipStream_t)stream); });
    });
}

int emagls_field_stream_push_device(emagls_field_stream* f, const double* d_src, int64_t nsamp, void* d_out, void* stream) {
    return emagls_field_stream_push_sets_device(f, d_src, nsamp, nullptr, 0, d_out, stream);
}

int emagls_field_stream_push_sets(emagls_field_stream* f, const double* src, int64_t nsamp, const int32_t* set, int64_t n_set, void* out) {
    return guarded_call([&] {
        check_push(f, src, out, nsamp, set, n_set, true);
        if (nsamp == 0) return;
        f->host_frame([&](hipStream_t st) {
            const size_t bin = sizeof(double) * (size_t)nsamp * f->d.nsrc, bout = f->out_esz() * (size_t)nsamp * f->nch;
            double* d_src = f->staged<double>(0, bin);
            char* d_out = f->staged<char>(1, bout);
            HIP_CHECK(hipMemcpyAsync(d_src, src, bin, hipMemcpyHostToDevice, st));
            int32_t* d_set = nullptr;
            if (f->bank() && n_set > 0) {
                d_set = f->staged<int32_t>(2, sizeof(int32_t) * (size_t)n_set);
                HIP_CHECK(hipMemcpyAsync(d_set, set, sizeof(int32_t) * (size_t)n_set, hipMemcpyHostToDevice, st));
            }
            push_blocks(f, d_src, nsamp, d_set, n_set, d_out, st);
            HIP_CHECK(hipMemcpyAsync(out, d_out, bout, hipMemcpyDeviceToHost, st));
        });
    });
}

int emagls_field_stream_push(emagls_field_stream* f, const double* src, int64_t nsamp, void* out) {
    return emagls_field_stream_push_sets(f, src, nsamp, nullptr, 0, out);
}

int emagls_field_stream_sets(const emagls_field_stream* f, int64_t* n_sets) {
    return guarded_call([&] {
        if (!f || !n_sets) throw Error(EMAGLS_ERR_ARG, "null pointer");
        *n_sets = f->d.S;
    });
}

int emagls_field_stream_reset(emagls_field_stream* f) {
    return guarded_call([&] {
        if (!f) throw Error(EMAGLS_ERR_ARG, "null field stream");
        f->reset_frame([&](hipStream_t st) { f->zero_state(st); });
    });
}

int emagls_field_stream_info(const emagls_field_stream* f, int64_t* block, int64_t* partitions, int64_t* state_bytes, int64_t* response_bytes,
                             int* launches_per_block) {
    return guarded_call([&] {
        if (!f) throw Error(EMAGLS_ERR_ARG, "null field stream");
        if (block) *block = f->d.B;
        if (partitions) *partitions = f->d.P;
        if (state_bytes) *state_bytes = (int64_t)f->state_bytes();
        if (response_bytes) *response_bytes = (int64_t)f->response_bytes();
        if (launches_per_block) *launches_per_block = kFieldStreamLaunches;   // the sources' forward transform; the products with the inverse
    });
}

int emagls_field_stream_destroy(emagls_field_stream* f) {
    return emagls_field_stream::destroy(f);
}

}  // extern "C"
