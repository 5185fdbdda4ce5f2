// MEX gateway for the MI355X eMagLS library (include/emagls.h).  One gateway, dispatched on a
// command string, so that the MATLAB wrappers in this directory keep the reference's file names and
// signatures (lib/getLsFilters.m:1-2, lib/getMagLsFilters.m:1-2, lib/getEMagLsFilters.m:1-2,
// lib/getEMagLs2Filters.m:1-2, lib/getEMagLsFiltersFromAtf.m:1, lib/getEMagLsFiltersEMAinCH.m:1-2, lib/getMagLsFilters2D.m:1,
// lib/getMagLsSphericalHeadFilter.m:1, lib/getMagLsArrayDiffuseFilter.m:1, dependencies/getRadialFilter.m:1,
// dependencies/applyRadialFilter.m:1, dependencies/binauralDecode.m:1-2).
//
// Build on a machine that has MATLAB (R2018a+, interleaved complex) and ROCm:
//     mex -R2018a emagls_mex.cpp -I../include -L../emagls_amd/lib -lemagls
// The build image has neither mex.h nor MATLAB: there the file is compiled against a test stand-in for mex.h and driven
// by tests/test_mex_gateway.py (tests/mexstub/).  It is a thin adapter: argument checks, pointer hand-over, mxArray
// allocation, error forwarding.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "emagls.h"
#include "mex.h"

namespace {

void fail(int rc) { mexErrMsgIdAndTxt("eMagLS:native", "%s (code %d)", emagls_last_error(), rc); }

const double* dbl(const mxArray* a, const char* what) {
    if (!mxIsDouble(a) || mxIsComplex(a)) mexErrMsgIdAndTxt("eMagLS:arg", "%s must be a real double array", what);
    return mxGetDoubles(a);
}
int basis_of(const mxArray* a) {
    if (!a || mxIsEmpty(a)) return EMAGLS_BASIS_REAL;  // default 'real' (lib/getEMagLsFilters.m:33)
    char buf[16] = {0};
    mxGetString(a, buf, sizeof buf);
    if (!std::strcmp(buf, "real")) return EMAGLS_BASIS_REAL;
    if (!std::strcmp(buf, "complex")) return EMAGLS_BASIS_COMPLEX;
    mexErrMsgIdAndTxt("eMagLS:arg", "shDefinition must be 'real' or 'complex'");
    return 0;
}
mxArray* out_matrix(mwSize rows, mwSize cols, int basis) {
    return mxCreateDoubleMatrix(rows, cols, basis == EMAGLS_BASIS_COMPLEX ? mxCOMPLEX : mxREAL);
}
void* out_ptr(mxArray* a) { return mxIsComplex(a) ? (void*)mxGetComplexDoubles(a) : (void*)mxGetDoubles(a); }
const void* in_ptr(const mxArray* a) { return mxIsComplex(a) ? (const void*)mxGetComplexDoubles(a) : (const void*)mxGetDoubles(a); }
// the spectral array responses: nfft as given, or the smallest power of two >= 2 irLen (the library wants it
// stated: the spectra's length follows from it); a MATLAB matrix [rows x cols] as rows one after the other; exponents as int32
int64_t spectral_nfft(const mxArray* a, mwSize nr) {
    if (a) return (int64_t)mxGetScalar(a);
    int64_t n = 8;
    while (n < 2 * (int64_t)nr && n < 65536) n *= 2;
    return n;
}
std::vector<double> rows_of(const double* m, mwSize rows, mwSize cols) {
    std::vector<double> v((size_t)rows * cols);
    for (mwSize r = 0; r < rows; ++r)
        for (mwSize k = 0; k < cols; ++k) v[(size_t)r * cols + k] = m[r + rows * k];
    return v;
}
std::vector<int32_t> exponents_of(const double* m, mwSize J, mwSize W) {
    std::vector<int32_t> v((size_t)J * W);
    for (mwSize j = 0; j < J; ++j)
        for (mwSize w = 0; w < W; ++w) {
            const double e = m[j + J * w];
            if (e != std::floor(e) || std::fabs(e) > 2147483647.0) mexErrMsgIdAndTxt("eMagLS:arg", "exponents must hold integers");
            v[(size_t)j * W + w] = (int32_t)e;
        }
    return v;
}
// source directivity: a MATLAB matrix [numSources Kd x P], real or complex, whose row q Kd + i holds c_{q,i}(k)
// (the .m wrappers build it), as [numSources][Kd][P] interleaved complex; returns Nd
int directivity_of(const mxArray* a, mwSize Q, mwSize P, std::vector<double>& coef) {
    const mwSize rows = mxGetM(a), Kd = rows / Q;
    if (!mxIsDouble(a) || mxGetN(a) != P || rows != Kd * Q || Kd < 1)
        mexErrMsgIdAndTxt("eMagLS:arg", "directivity must be [numSources*Kd x %d] (nfft / 2 + 1 bins) with Kd coefficients per source", (int)P);
    const int Nd = (int)std::floor(std::sqrt((double)Kd) + 0.5) - 1;
    if ((mwSize)((Nd + 1) * (Nd + 1)) != Kd) mexErrMsgIdAndTxt("eMagLS:arg", "directivity holds %d coefficients per source and bin, which is not a square (Nd + 1)^2", (int)Kd);
    const bool cplx = mxIsComplex(a);
    const double* d = (const double*)in_ptr(a);
    coef.assign((size_t)2 * rows * P, 0.0);
    for (mwSize r = 0; r < rows; ++r)
        for (mwSize k = 0; k < P; ++k) {
            const size_t src = r + (size_t)rows * k, dst = (size_t)r * P + k;
            coef[2 * dst] = cplx ? d[2 * src] : d[src];
            if (cplx) coef[2 * dst + 1] = d[2 * src + 1];
        }
    return Nd;
}
// sourceOrientation as the gateway takes it: [numSources x 9], row q = R_q row by row
std::vector<double> rotations_of(const mxArray* a, mwSize Q) {
    if (mxGetM(a) != Q || mxGetN(a) != 9) mexErrMsgIdAndTxt("eMagLS:arg", "sourceOrientation must be [numSources x 9] (each rotation matrix row by row)");
    return rows_of(dbl(a, "sourceOrientation"), Q, 9);
}
// the emission vectors of a room's lists (emagls_shoebox_emission; refl null: the images) as a MATLAB matrix [J x 3]
mxArray* shoebox_emission(const double* dim, const double* refl, const double* pos, mwSize Q, const double* src, double fs, double max_delay,
                          int max_order, mwSize J) {
    std::vector<int64_t> ptr(Q + 1);
    std::vector<double> e(3 * (size_t)J);
    if (J) {
        const int rc = emagls_shoebox_emission(dim, refl, pos, (int64_t)Q, src, fs, max_delay, max_order, (int64_t)J, ptr.data(), e.data());
        if (rc) fail(rc);
    }
    mxArray* out = mxCreateDoubleMatrix(J, 3, mxREAL);
    for (mwSize j = 0; j < J; ++j)
        for (int i = 0; i < 3; ++i) mxGetDoubles(out)[j + J * i] = e[3 * j + i];
    return out;
}
// a caller-evaluated SH matrix must be real / complex like the basis asked for
const void* basis_matrix(const mxArray* a, int basis, mwSize rows, mwSize cols, const char* what) {
    if (!mxIsDouble(a) || mxGetM(a) != rows || mxGetN(a) != cols) mexErrMsgIdAndTxt("eMagLS:arg", "%s must be a %d x %d double matrix", what, (int)rows, (int)cols);
    if ((basis == EMAGLS_BASIS_COMPLEX) != (bool)mxIsComplex(a)) mexErrMsgIdAndTxt("eMagLS:arg", "%s does not match shDefinition", what);
    return in_ptr(a);
}
int radial_type(const mxArray* a) {
    char buf[16] = {0};
    mxGetString(a, buf, sizeof buf);
    for (char* q = buf; *q; ++q) *q = (char)tolower(*q);     // strcmpi / lower() in getRadialFilter.m:44,56
    if (!std::strcmp(buf, "tikhonov")) return EMAGLS_RADIAL_TIKHONOV;
    if (!std::strcmp(buf, "softlimit")) return EMAGLS_RADIAL_SOFTLIMIT;
    if (!std::strcmp(buf, "full")) return EMAGLS_RADIAL_FULL;
    if (!std::strcmp(buf, "none")) return EMAGLS_RADIAL_NONE;
    mexErrMsgIdAndTxt("eMagLS:arg", "Unkown radialFilter parameter \"%s\".", buf);
    return 0;
}
// decode streams and listener groups live in a table each; MATLAB holds the 1-based index (mex/binauralDecodeStream.m,
// mex/binauralDecodeGroup.m).  what: the kind's word in the messages
template <typename H> struct HandleTable {
    struct Entry { H* h; mwSize cols; bool in_complex; mwSize listeners; };   // with what a push checks its block against
    const char* what;
    std::vector<Entry> entries;
    const char* family = "decode";   // "invalid <family> <what> handle"
    Entry& of(const mxArray* a) {
        const double v = (a && mxIsDouble(a) && mxGetNumberOfElements(a) == 1) ? mxGetScalar(a) : 0.0;
        const size_t i = (v >= 1 && v <= (double)entries.size() && v == std::floor(v)) ? (size_t)v : 0;
        if (!i || !entries[i - 1].h) mexErrMsgIdAndTxt("eMagLS:arg", "invalid %s %s handle", family, what);
        return entries[i - 1];
    }
    mxArray* add(const Entry& e) {   // into the first free slot
        size_t slot = 0;
        while (slot < entries.size() && entries[slot].h) ++slot;
        if (slot == entries.size()) entries.push_back(e);
        else entries[slot] = e;
        return mxCreateDoubleScalar((double)(slot + 1));
    }
    // the block of a push: [n x cols], real or complex as the object was created
    void check_block(const Entry& e, const mxArray* in) const {
        if (!mxIsDouble(in) || mxGetN(in) != e.cols)
            mexErrMsgIdAndTxt("eMagLS:arg", "in must be a double array with the filters' channel count (%d)", (int)e.cols);
        if ((bool)mxIsComplex(in) != e.in_complex)
            mexErrMsgIdAndTxt("eMagLS:arg", "in must be %s, as the %s was created", e.in_complex ? "complex" : "real", what);
    }
};
HandleTable<emagls_decode_stream> g_streams{"stream"};
HandleTable<emagls_decode_group> g_groups{"group"};
// field streams (mex/sourceFieldStream.m): an entry's cols are the sources of a pushed block, in_complex says that the OUTPUT is
// complex (a complex response), and listeners holds the output's channel count
HandleTable<emagls_field_stream> g_fields{"stream", {}, "field"};
// an array of one listener's worth of values but the wrong orientation would be read as another listener's: the last dimension
// must be the listeners
void per_listener(const mxArray* a, const char* what, mwSize listeners) {
    if (mxGetNumberOfDimensions(a) > 2 || mxGetN(a) != listeners)
        mexErrMsgIdAndTxt("eMagLS:arg", "%s must have one column per listener (%d)", what, (int)listeners);
}
// the three optional angles of a push, prhs[3..5]: [] or absent: none.  listeners > 0: a group's, one column per listener
struct PushAngles { const double* p[3] = {nullptr, nullptr, nullptr}; int64_t n[3] = {0, 0, 0}; };
PushAngles push_angles(int nrhs, const mxArray* const* prhs, mwSize listeners) {
    static const char* const names[3] = {"horRotAngleRad", "pitchRad", "rollRad"};
    PushAngles a;
    for (int i = 0; i < 3; ++i)
        if (nrhs > 3 + i && !mxIsEmpty(prhs[3 + i])) {
            if (listeners) per_listener(prhs[3 + i], names[i], listeners);
            a.p[i] = dbl(prhs[3 + i], names[i]);
            a.n[i] = (int64_t)mxGetNumberOfElements(prhs[3 + i]);
        }
    return a;
}
int layout_of(const mxArray* a) {
    if (!a || mxIsEmpty(a)) return EMAGLS_LAYOUT_SH;
    char buf[8] = {0};
    mxGetString(a, buf, sizeof buf);
    if (!std::strcmp(buf, "ch")) return EMAGLS_LAYOUT_CH;
    if (std::strcmp(buf, "sh")) mexErrMsgIdAndTxt("eMagLS:arg", "rotation domain must be 'sh' or 'ch'");
    return EMAGLS_LAYOUT_SH;
}
// the decoding filters of 'stream_create' / 'group_create', prhs[1] and prhs[2]: [len x nch], or [len x nch x numSets] -- column-major,
// the sets of a bank lie one after the other as the library takes them
struct FilterArgs { mwSize len, ch, nsets; bool wc; };
FilterArgs filter_args(const mxArray* const* prhs) {
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    const mwSize* dims = mxGetDimensions(prhs[1]);
    if (nd > 3) mexErrMsgIdAndTxt("eMagLS:arg", "the decoding filters must be [len x numChannels] or [len x numChannels x numSets]");
    const FilterArgs f{mxGetM(prhs[1]), nd >= 2 ? dims[1] : 1, nd == 3 ? dims[2] : 1, (bool)mxIsComplex(prhs[1])};
    bool same = mxIsDouble(prhs[1]) && mxIsDouble(prhs[2]) && mxGetNumberOfDimensions(prhs[2]) == nd;
    for (mwSize i = 0; same && i < nd; ++i) same = mxGetDimensions(prhs[2])[i] == dims[i];
    if (!same) mexErrMsgIdAndTxt("eMagLS:arg", "the two decoding filters must be double arrays of equal size");
    if (f.wc != (bool)mxIsComplex(prhs[2])) mexErrMsgIdAndTxt("eMagLS:arg", "the two decoding filters must both be real or both complex");
    return f;
}
// the optional encoder of 'stream_create' / 'group_create' (DESIGN.md section 9.6): [] or absent: none; else [numChannels x numMics],
// real or complex -- column-major, as the library takes it.  Returns the microphone count (0: none)
mwSize encoder_arg(const mxArray* a, mwSize ch, bool complex_input) {
    if (!a || mxIsEmpty(a)) return 0;
    if (!mxIsDouble(a) || mxGetNumberOfDimensions(a) > 2 || mxGetM(a) != ch)
        mexErrMsgIdAndTxt("eMagLS:arg", "encoder must be a double [numChannels x numMics] array with the filters' channel count (%d) of rows", (int)ch);
    if (complex_input) mexErrMsgIdAndTxt("eMagLS:arg", "an encoder takes real microphone blocks: complexInput must be false");
    return mxGetN(a);
}
bool truthy(const mxArray* a) { return mxIsLogicalScalarTrue(a) || (mxIsDouble(a) && !mxIsEmpty(a) && mxGetScalar(a) != 0); }
// a ONE-based set index array as the library's zero-based int32
std::vector<int32_t> zero_based(const mxArray* a) {
    std::vector<int32_t> sets;
    if (!a || mxIsEmpty(a)) return sets;
    const double* v = dbl(a, "setIndex");
    sets.resize(mxGetNumberOfElements(a));
    for (size_t i = 0; i < sets.size(); ++i) {
        if (!(v[i] >= 1.0 && v[i] <= 2147483647.0) || v[i] != std::floor(v[i]))
            mexErrMsgIdAndTxt("eMagLS:arg", "setIndex must hold positive integers (the sets count from 1)");
        sets[i] = (int32_t)v[i] - 1;
    }
    return sets;
}
// the plans the one-shot entry points cache (device buffers, captured graphs) are released when the MEX file is cleared
void at_exit() {
    for (auto& e : g_streams.entries) { if (e.h) emagls_decode_stream_destroy(e.h); e.h = nullptr; }
    for (auto& e : g_groups.entries) { if (e.h) emagls_decode_group_destroy(e.h); e.h = nullptr; }
    for (auto& e : g_fields.entries) { if (e.h) emagls_field_stream_destroy(e.h); e.h = nullptr; }
    emagls_cache_clear();
}

}  // namespace

// emagls_mex('ls',      hL, hR, azi, zen, order, shDefinition)
// emagls_mex('magls',   hL, hR, azi, zen, order, fs, len, shDefinition)
// emagls_mex('emagls',  hL, hR, azi, zen, micRadius, micAzi, micZen, order, fs, len, shDefinition)
// emagls_mex('emagls2', ... same ...)
// emagls_mex('fromatf', hL, hR, hrirGridAziZen, atfIrs, atfGridAziZen, fs, filterLen, fTrans)
// emagls_mex('emainch' | 'emainsh', hL, hR, azi, zen, micRadius, micAzi, order, fs, len, shDefinition)
// emagls_mex('magls_dc' | 'emagls_dc' | 'emagls2_dc', <the arguments of 'magls' / 'emagls' / 'emagls2'>, applyDiffusenessConst)
// emagls_mex('decode',  in, wL, wR, compensateDelay[, yawRad, signal, shDefinition, domain, pitchRad, rollRad])   real or complex in / filters; [out, imagAbsSum] = ...
// h = emagls_mex('stream_create', wL, wR, blockSize[, shDefinition, domain, complexInput, encoder])   a decode stream (mex/binauralDecodeStream.m);
//                                     wL / wR [len x nch], or [len x nch x numSets]: a bank of filter sets; encoder [nch x numMics]: the
//                                     stream is pushed real microphone blocks [n x numMics] (also on 'group_create', after complexInput)
// out = emagls_mex('stream_push', h, in[, yawRad, pitchRad, rollRad, setIndex])   in [k*blockSize x nch]; each angle [], a scalar or one per
//                                     sample; setIndex ONE-based: [] (keep the set), a scalar or one per block
// emagls_mex('stream_reset', h)      emagls_mex('stream_destroy', h)
// h = emagls_mex('group_create', wL, wR, blockSize, numListeners[, shDefinition, domain, complexInput, encoder])   a listener group
//                                     (mex/binauralDecodeGroup.m): many listeners of one sound field in one push
// out = emagls_mex('group_push', h, in[, yawRad, pitchRad, rollRad, setIndex])   in [k*blockSize x nch], the common signal; listeners run
//                                     along the last dimension: out [n x 2 x L]; each angle [], [1 x L] or [n x L]; setIndex ONE-based,
//                                     [], [1 x L] or [nBlocks x L]
// emagls_mex('group_reset', h[, listener])   ONE-based; without it all listeners      emagls_mex('group_destroy', h)
// h = emagls_mex('field_create', rirs, blockSize)   a field stream (mex/sourceFieldStream.m): rirs [nr x nch], or [nr x nch x numSources],
//                                     real or complex: dry sources through room responses, a block at a time; rirs
//                                     [nr x nch x numSources x numSets]: a bank of response sets, for sources that move
// out = emagls_mex('field_push', h, src[, setIndex])   src [k*blockSize x numSources] real; out [k*blockSize x nch], complex for a complex
//                                     response; setIndex ONE-based: [] (every source keeps its set), a scalar (every source),
//                                     [numSources] or [numSources x k]
// emagls_mex('field_reset', h)       emagls_mex('field_destroy', h)
// emagls_mex('resample', x, p, q)   MATLAB's resample(x, p, q) (N = 10, bta = 5): a row vector along its length, else per column
// emagls_mex('rotate',  in, yawRad[, shDefinition, domain])    yaw rotation of an SH ('sh', default) or CH ('ch') signal
// emagls_mex('rotate3', in, yawRad, pitchRad, rollRad[, shDefinition])   three-axis rotation of an SH signal (orders 0-15)
// emagls_mex('shrotmtx', order, yawRad, pitchRad, rollRad[, shDefinition])   its matrix M: out = in * M.'
// emagls_mex('sets', kind, hL, hR, azi, zen, micRadius, micAzi, micZen, order, fs, len, shDefinition)   3-D hL / hR: a loop over HRIR sets in one call
// emagls_mex('fromatfsets', hL, hR, hrirGridAziZen, atfIrs, atfGridAziZen, fs, filterLen, fTrans)      3-D hL / hR: the subjects of one ATF set
// emagls_mex('jobs', jobs[, batchSize, inFlight, shareGeometry, devices])   struct array of independent designs (any kinds, radii, HRIR sets): W = {wL, wR} per job
// caller-evaluated shFunction handles (the wrappers evaluate them at emagls_mex('simorder', kind, order, fs, micRadius)):
// emagls_mex('ls_y', hL, hR, Yhrir, order, shDefinition)        emagls_mex('magls_y', hL, hR, Yhrir, order, fs, len, shDefinition)
// emagls_mex('emagls_y' | 'emagls2_y', hL, hR, Yhrir, micRadius, Ymic, order, fs, len, shDefinition)
// render side:
// emagls_mex('magls2d', hLHor, hRHor, azi, order, fs, len, chDefinition)
// emagls_mex('radial', order, fs, smaRadius, irLen, oversamplingFactor, radialFilter, regulConst, noiseGainDb)
// emagls_mex('applyradial', inSig, order, fs, smaRadius, irLen, oversamplingFactor, radialFilter, regulConst, noiseGainDb)
// emagls_mex('encode', smaRecording, micAzi, micZen, order, shDefinition)
// emagls_mex('ch', N, aziRad, basisType)        emagls_mex('smair', order, fs, irLen, oversamplingFactor, smaRadius, micAzi, micZen, ...)
// emagls_mex('shf', micRadius, order, fs, len)                  [wShf, W_Shf] = ...
// emagls_mex('adf', micRadius, micAzi, micZen, order, fs, len, shDefinition[, Yhi])
// array responses: 'array_irs', 'shoebox_components', 'shoebox_images', 'array_room_irs' (their argument lists stand at their branches;
// directive sources, DESIGN.md section 15, are further arguments and outputs of the four)
void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    static bool registered = false;
    if (!registered) { mexAtExit(at_exit); registered = true; }
    if (nrhs < 1 || !mxIsChar(prhs[0])) mexErrMsgIdAndTxt("eMagLS:arg", "first argument must be a command string");
    char cmd[32] = {0};
    mxGetString(prhs[0], cmd, sizeof cmd);
    const std::string c(cmd);
    if (c == "decode" && nrhs > 5) {
        // dependencies/binauralDecode.m:27-31,44-48 on the GPU: yaw ([] / 0: none, a scalar, or one angle per input sample), the
        // dry source signal ([]: none; its first column), the basis of `in` and the rotation domain ('sh' / 'ch')
        const mwSize n = mxGetM(prhs[1]), ch = mxGetN(prhs[1]), len = mxGetM(prhs[2]);
        const int comp = mxIsLogicalScalarTrue(prhs[4]) || (mxIsDouble(prhs[4]) && !mxIsEmpty(prhs[4]) && mxGetScalar(prhs[4]) != 0);
        const bool ic = mxIsComplex(prhs[1]), wc = mxIsComplex(prhs[2]);
        if (wc != (bool)mxIsComplex(prhs[3])) mexErrMsgIdAndTxt("eMagLS:arg", "the two decoding filters must both be real or both complex");
        const mxArray* ayaw = prhs[5];
        const mwSize nyaw_in = mxIsEmpty(ayaw) ? 0 : mxGetNumberOfElements(ayaw);
        const double* yaw = nyaw_in ? dbl(ayaw, "horRotAngleRad") : nullptr;
        const mwSize nyaw = (nyaw_in == 1 && yaw[0] == 0.0) ? 0 : nyaw_in;        // :28: horRotAngleRad ~= 0
        const mxArray* asig = nrhs > 6 ? prhs[6] : nullptr;
        const mwSize nsig = (asig && !mxIsEmpty(asig)) ? mxGetM(asig) : 0;
        const double* sig = nsig ? dbl(asig, "signal") : nullptr;                // (column-major: the first column leads)
        const int basis = basis_of(nrhs > 7 ? prhs[7] : nullptr);
        int layout = EMAGLS_LAYOUT_SH;
        if (nrhs > 8 && !mxIsEmpty(prhs[8])) {
            char buf[8] = {0};
            mxGetString(prhs[8], buf, sizeof buf);
            if (!std::strcmp(buf, "ch")) layout = EMAGLS_LAYOUT_CH;
            else if (std::strcmp(buf, "sh")) mexErrMsgIdAndTxt("eMagLS:arg", "rotation domain must be 'sh' or 'ch'");
        }
        const mwSize rows = nsig ? nsig : n, skip = comp ? (len / 2 > 0 ? len / 2 - 1 : 0) : 0;
        plhs[0] = mxCreateDoubleMatrix(rows > skip ? rows - skip : 0, 2, mxREAL);
        double imag_sum[2] = {0, 0};
        // pitch (prhs[9]) and roll (prhs[10]): [] or absent: none, a scalar, or one angle per input sample
        const mwSize npitch = (nrhs > 9 && !mxIsEmpty(prhs[9])) ? mxGetNumberOfElements(prhs[9]) : 0;
        const mwSize nroll = (nrhs > 10 && !mxIsEmpty(prhs[10])) ? mxGetNumberOfElements(prhs[10]) : 0;
        const double* pitch = npitch ? dbl(prhs[9], "pitchRad") : nullptr;
        const double* roll = nroll ? dbl(prhs[10], "rollRad") : nullptr;
        const int rc = emagls_binaural_decode_render_ypr(in_ptr(prhs[1]), ic, n, ch, in_ptr(prhs[2]), in_ptr(prhs[3]), wc, len, comp, layout,
                                                         basis, yaw, nyaw, pitch, npitch, roll, nroll, sig, nsig, mxGetDoubles(plhs[0]), imag_sum);
        if (rc) fail(rc);
        if (nlhs > 1) { plhs[1] = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetDoubles(plhs[1])[0] = imag_sum[0]; mxGetDoubles(plhs[1])[1] = imag_sum[1]; }
        return;
    }
    if (c == "stream_create") {
        if (nrhs < 4) mexErrMsgIdAndTxt("eMagLS:arg", "stream_create needs (wL, wR, blockSize[, shDefinition, domain, complexInput, encoder])");
        const FilterArgs f = filter_args(prhs);
        const int basis = basis_of(nrhs > 4 ? prhs[4] : nullptr), layout = layout_of(nrhs > 5 ? prhs[5] : nullptr);
        const int ic = nrhs > 6 && truthy(prhs[6]);
        const mxArray* enc = nrhs > 7 ? prhs[7] : nullptr;
        const mwSize nmics = encoder_arg(enc, f.ch, ic != 0);
        emagls_decode_stream* st = nullptr;
        const int rc = nmics ? emagls_decode_stream_create_encoded((int64_t)nmics, in_ptr(enc), mxIsComplex(enc), (int64_t)f.ch, (int64_t)f.nsets, in_ptr(prhs[1]),
                                                                   in_ptr(prhs[2]), f.wc, (int64_t)f.len, layout, basis, (int64_t)mxGetScalar(prhs[3]), &st)
                             : emagls_decode_stream_create_bank((int64_t)f.ch, (int64_t)f.nsets, in_ptr(prhs[1]), in_ptr(prhs[2]), f.wc, (int64_t)f.len, ic,
                                                                layout, basis, (int64_t)mxGetScalar(prhs[3]), &st);
        if (rc) fail(rc);
        plhs[0] = g_streams.add({st, nmics ? nmics : f.ch, ic != 0, 0});   // (an encoded stream is pushed [n x numMics] blocks)
        return;
    }
    if (c == "stream_push") {
        if (nrhs < 3) mexErrMsgIdAndTxt("eMagLS:arg", "stream_push needs (handle, in[, yawRad, pitchRad, rollRad, setIndex])");
        const auto& e = g_streams.of(prhs[1]);
        g_streams.check_block(e, prhs[2]);
        const mwSize n = mxGetM(prhs[2]);
        const PushAngles a = push_angles(nrhs, prhs, 0);
        // setIndex (prhs[6]): MATLAB counts the sets from 1, the library from 0
        const std::vector<int32_t> sets = zero_based(nrhs > 6 ? prhs[6] : nullptr);
        plhs[0] = mxCreateDoubleMatrix(n, 2, mxREAL);
        const int rc = emagls_decode_stream_push_sets(e.h, in_ptr(prhs[2]), (int64_t)n, sets.empty() ? nullptr : sets.data(), (int64_t)sets.size(),
                                                      a.p[0], a.n[0], a.p[1], a.n[1], a.p[2], a.n[2], mxGetDoubles(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "stream_reset" || c == "stream_destroy") {
        if (nrhs < 2) mexErrMsgIdAndTxt("eMagLS:arg", "%s needs (handle)", cmd);
        auto& e = g_streams.of(prhs[1]);
        const int rc = c == "stream_reset" ? emagls_decode_stream_reset(e.h) : emagls_decode_stream_destroy(e.h);
        if (c == "stream_destroy") e.h = nullptr;
        if (rc) fail(rc);
        return;
    }
    if (c == "field_create") {
        if (nrhs < 3) mexErrMsgIdAndTxt("eMagLS:arg", "field_create needs (rirs, blockSize)");
        const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
        const mwSize* dims = mxGetDimensions(prhs[1]);
        if (!mxIsDouble(prhs[1]) || nd > 4)
            mexErrMsgIdAndTxt("eMagLS:arg",
                              "rirs must be a double [nr x numChannels], [nr x numChannels x numSources] or [nr x numChannels x numSources x numSets] array");
        // column-major, the sets of a bank lie one after the other, each the sources one after the other, as the library takes them
        const mwSize nr = dims[0], ch = nd >= 2 ? dims[1] : 1, nsrc = nd >= 3 ? dims[2] : 1, nsets = nd == 4 ? dims[3] : 1;
        const double bs = mxGetScalar(prhs[2]);
        if (!(bs == std::floor(bs)) || std::fabs(bs) > 1e9) mexErrMsgIdAndTxt("eMagLS:arg", "blockSize must be an integer");
        const bool rc_ = mxIsComplex(prhs[1]);
        emagls_field_stream* f = nullptr;
        const int rc = emagls_field_stream_create_bank((int64_t)nsrc, (int64_t)ch, (int64_t)nsets, in_ptr(prhs[1]), rc_, (int64_t)nr, (int64_t)bs, &f);
        if (rc) fail(rc);
        plhs[0] = g_fields.add({f, nsrc, rc_, ch});
        return;
    }
    if (c == "field_push") {
        if (nrhs < 3) mexErrMsgIdAndTxt("eMagLS:arg", "field_push needs (handle, src[, setIndex])");
        const auto& e = g_fields.of(prhs[1]);
        if (!mxIsDouble(prhs[2]) || mxIsComplex(prhs[2]) || mxGetNumberOfDimensions(prhs[2]) > 2 || mxGetN(prhs[2]) != e.cols)
            mexErrMsgIdAndTxt("eMagLS:arg", "src must be a real double array with the responses' source count (%d) of columns", (int)e.cols);
        const mwSize n = mxGetM(prhs[2]);
        // setIndex: a scalar (every source), [numSources] or [numSources x k], which the library takes source-major: [numSources][k]
        std::vector<int32_t> sets;
        if (nrhs > 3 && !mxIsEmpty(prhs[3])) {
            const std::vector<int32_t> given = zero_based(prhs[3]);
            const mwSize rows = mxGetM(prhs[3]), cols = mxGetN(prhs[3]);
            const bool as_it_lies = given.size() == e.cols || (e.cols == 1 && (rows == 1 || cols == 1));   // (one source: a vector over the blocks)
            if (mxGetNumberOfDimensions(prhs[3]) > 2 || !(given.size() == 1 || as_it_lies || rows == e.cols))
                mexErrMsgIdAndTxt("eMagLS:arg", "setIndex must be a scalar, [numSources] or [numSources x k] with %d sources", (int)e.cols);
            if (given.size() == 1) sets.assign(e.cols, given[0]);
            else if (as_it_lies) sets = given;
            else {
                sets.resize(given.size());
                for (mwSize q = 0; q < rows; ++q)
                    for (mwSize b = 0; b < cols; ++b) sets[q * cols + b] = given[b * rows + q];
            }
        }
        plhs[0] = mxCreateDoubleMatrix(n, e.listeners, e.in_complex ? mxCOMPLEX : mxREAL);
        const int rc = emagls_field_stream_push_sets(e.h, mxGetDoubles(prhs[2]), (int64_t)n, sets.empty() ? nullptr : sets.data(),
                                                     (int64_t)sets.size(), out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "field_reset" || c == "field_destroy") {
        if (nrhs < 2) mexErrMsgIdAndTxt("eMagLS:arg", "%s needs (handle)", cmd);
        auto& e = g_fields.of(prhs[1]);
        const int rc = c == "field_reset" ? emagls_field_stream_reset(e.h) : emagls_field_stream_destroy(e.h);
        if (c == "field_destroy") e.h = nullptr;
        if (rc) fail(rc);
        return;
    }
    if (c == "group_create") {
        if (nrhs < 5)
            mexErrMsgIdAndTxt("eMagLS:arg", "group_create needs (wL, wR, blockSize, numListeners[, shDefinition, domain, complexInput, encoder])");
        const FilterArgs f = filter_args(prhs);
        const int basis = basis_of(nrhs > 5 ? prhs[5] : nullptr), layout = layout_of(nrhs > 6 ? prhs[6] : nullptr);
        const int ic = nrhs > 7 && truthy(prhs[7]);
        const double nl = mxGetScalar(prhs[4]);
        if (!(nl == std::floor(nl)) || std::fabs(nl) > 1e9) mexErrMsgIdAndTxt("eMagLS:arg", "numListeners must be an integer");
        const mxArray* enc = nrhs > 8 ? prhs[8] : nullptr;
        const mwSize nmics = encoder_arg(enc, f.ch, ic != 0);
        emagls_decode_group* g = nullptr;
        const int rc = nmics ? emagls_decode_group_create_encoded((int64_t)nmics, in_ptr(enc), mxIsComplex(enc), (int64_t)f.ch, (int64_t)f.nsets, in_ptr(prhs[1]),
                                                                  in_ptr(prhs[2]), f.wc, (int64_t)f.len, layout, basis, (int64_t)mxGetScalar(prhs[3]), (int64_t)nl, &g)
                             : emagls_decode_group_create((int64_t)f.ch, (int64_t)f.nsets, in_ptr(prhs[1]), in_ptr(prhs[2]), f.wc, (int64_t)f.len, ic, layout,
                                                          basis, (int64_t)mxGetScalar(prhs[3]), (int64_t)nl, &g);
        if (rc) fail(rc);
        plhs[0] = g_groups.add({g, nmics ? nmics : f.ch, ic != 0, (mwSize)nl});
        return;
    }
    if (c == "group_push") {
        // listeners run along the LAST dimension: column-major [n x L] is the library's listener-major [L][n]
        if (nrhs < 3) mexErrMsgIdAndTxt("eMagLS:arg", "group_push needs (handle, in[, yawRad, pitchRad, rollRad, setIndex])");
        const auto& e = g_groups.of(prhs[1]);
        g_groups.check_block(e, prhs[2]);
        const mwSize n = mxGetM(prhs[2]);
        const PushAngles a = push_angles(nrhs, prhs, e.listeners);
        if (nrhs > 6 && !mxIsEmpty(prhs[6])) per_listener(prhs[6], "setIndex", e.listeners);
        const std::vector<int32_t> sets = zero_based(nrhs > 6 ? prhs[6] : nullptr);   // [nBlocks x L], one-based
        const mwSize dims[3] = {n, 2, e.listeners};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL);
        const int rc = emagls_decode_group_push(e.h, in_ptr(prhs[2]), (int64_t)n, sets.empty() ? nullptr : sets.data(), (int64_t)sets.size(), a.p[0],
                                                a.n[0], a.p[1], a.n[1], a.p[2], a.n[2], mxGetDoubles(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "group_reset" || c == "group_destroy") {
        if (nrhs < 2) mexErrMsgIdAndTxt("eMagLS:arg", "%s needs (handle)", cmd);
        auto& e = g_groups.of(prhs[1]);
        int64_t listener = -1;   // 'group_reset', h, listener: ONE-based; [] or absent: all listeners
        if (c == "group_reset" && nrhs > 2 && !mxIsEmpty(prhs[2])) {
            const double v = mxGetScalar(prhs[2]);
            if (!(v >= 1.0 && v <= 2147483647.0) || v != std::floor(v))
                mexErrMsgIdAndTxt("eMagLS:arg", "listener must be a positive integer (the listeners count from 1)");
            listener = (int64_t)v - 1;
        }
        const int rc = c == "group_reset" ? emagls_decode_group_reset(e.h, listener) : emagls_decode_group_destroy(e.h);
        if (c == "group_destroy") e.h = nullptr;
        if (rc) fail(rc);
        return;
    }
    if (c == "resample") {
        // y = emagls_mex('resample', x, p, q): emagls_resample; p and q positive integers
        if (nrhs < 4) mexErrMsgIdAndTxt("eMagLS:arg", "resample needs (x, p, q)");
        const mwSize M = mxGetM(prhs[1]), N = mxGetN(prhs[1]);
        const bool row = M == 1, ic = mxIsComplex(prhs[1]);
        const mwSize n = row ? N : M, ch = row ? 1 : N;
        if (!mxIsDouble(prhs[1])) mexErrMsgIdAndTxt("eMagLS:arg", "x must be a double array");
        auto rate = [](const mxArray* a, const char* what) -> int64_t {
            const double v = (mxIsDouble(a) && !mxIsComplex(a) && mxGetNumberOfElements(a) == 1) ? mxGetScalar(a) : 0.0;
            if (!(v >= 1.0 && v <= 9.0e15 && v == std::floor(v))) mexErrMsgIdAndTxt("eMagLS:arg", "%s must be a positive integer", what);
            return (int64_t)v;
        };
        const int64_t p = rate(prhs[2], "p"), q = rate(prhs[3], "q");
        const mwSize ny = (mwSize)emagls_resample_length((int64_t)n, p, q);
        plhs[0] = row ? mxCreateDoubleMatrix(1, ny, ic ? mxCOMPLEX : mxREAL) : mxCreateDoubleMatrix(ny, ch, ic ? mxCOMPLEX : mxREAL);
        if (n && ch) {
            const int rc = emagls_resample(in_ptr(prhs[1]), ic, n, ch, p, q, out_ptr(plhs[0]));
            if (rc) fail(rc);
        }
        return;
    }
    if (c == "rotate") {
        // out = emagls_mex('rotate', in, yawRad[, shDefinition, domain]): the yaw rotation alone (emagls_rotate_yaw)
        if (nrhs < 3) mexErrMsgIdAndTxt("eMagLS:arg", "rotate needs (in, yawRad[, shDefinition, domain])");
        const mwSize n = mxGetM(prhs[1]), ch = mxGetN(prhs[1]);
        const bool ic = mxIsComplex(prhs[1]);
        const int basis = basis_of(nrhs > 3 ? prhs[3] : nullptr);
        int layout = EMAGLS_LAYOUT_SH;
        if (nrhs > 4 && !mxIsEmpty(prhs[4])) {
            char buf[8] = {0};
            mxGetString(prhs[4], buf, sizeof buf);
            if (!std::strcmp(buf, "ch")) layout = EMAGLS_LAYOUT_CH;
            else if (std::strcmp(buf, "sh")) mexErrMsgIdAndTxt("eMagLS:arg", "rotation domain must be 'sh' or 'ch'");
        }
        plhs[0] = mxCreateDoubleMatrix(n, ch, (ic || basis == EMAGLS_BASIS_COMPLEX) ? mxCOMPLEX : mxREAL);
        const int rc = emagls_rotate_yaw(in_ptr(prhs[1]), ic, n, ch, layout, basis, dbl(prhs[2], "yawRad"), mxGetNumberOfElements(prhs[2]),
                                         out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "rotate3") {
        // out = emagls_mex('rotate3', in, yaw, pitch, roll[, shDefinition]): three-axis rotation of an SH signal (emagls_rotate_sh);
        // each angle a scalar or one per sample
        if (nrhs < 5) mexErrMsgIdAndTxt("eMagLS:arg", "rotate3 needs (in, yawRad, pitchRad, rollRad[, shDefinition])");
        const mwSize n = mxGetM(prhs[1]), ch = mxGetN(prhs[1]);
        const bool ic = mxIsComplex(prhs[1]);
        const int basis = basis_of(nrhs > 5 ? prhs[5] : nullptr);
        plhs[0] = mxCreateDoubleMatrix(n, ch, (ic || basis == EMAGLS_BASIS_COMPLEX) ? mxCOMPLEX : mxREAL);
        const int rc = emagls_rotate_sh(in_ptr(prhs[1]), ic, n, ch, basis, dbl(prhs[2], "yawRad"), mxGetNumberOfElements(prhs[2]),
                                        dbl(prhs[3], "pitchRad"), mxGetNumberOfElements(prhs[3]), dbl(prhs[4], "rollRad"),
                                        mxGetNumberOfElements(prhs[4]), out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "shrotmtx") {
        // M = emagls_mex('shrotmtx', order, yaw, pitch, roll[, shDefinition]): rotate3's matrix, out_row = in_row * M.'
        if (nrhs < 5) mexErrMsgIdAndTxt("eMagLS:arg", "shrotmtx needs (order, yawRad, pitchRad, rollRad[, shDefinition])");
        const int order = (int)mxGetScalar(prhs[1]);
        const int basis = basis_of(nrhs > 5 ? prhs[5] : nullptr);
        const mwSize C = order >= 0 ? (mwSize)(order + 1) * (order + 1) : 0;
        plhs[0] = mxCreateDoubleMatrix(C, C, basis == EMAGLS_BASIS_COMPLEX ? mxCOMPLEX : mxREAL);
        const int rc = emagls_sh_rotation_matrix(order, basis, mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), mxGetScalar(prhs[4]),
                                                 out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "decode") {
        if (nrhs < 4) mexErrMsgIdAndTxt("eMagLS:arg", "decode needs (in, wL, wR[, compensateDelay])");
        const mwSize n = mxGetM(prhs[1]), ch = mxGetN(prhs[1]), len = mxGetM(prhs[2]);
        const int comp = nrhs > 4 && mxIsLogicalScalarTrue(prhs[4]);
        const mwSize nout = comp ? n - (len / 2 > 0 ? len / 2 - 1 : 0) : n;
        plhs[0] = mxCreateDoubleMatrix(nout, 2, mxREAL);
        const bool ic = mxIsComplex(prhs[1]), wc = mxIsComplex(prhs[2]);
        if (wc != (bool)mxIsComplex(prhs[3])) mexErrMsgIdAndTxt("eMagLS:arg", "the two decoding filters must both be real or both complex");
        // (complex: dependencies/binauralDecode.m:39-42,59-64, complex products accumulated, the real part kept)
        const bool cplx = ic || wc;
        const void* in = cplx ? in_ptr(prhs[1]) : dbl(prhs[1], "in");
        const void* wL = cplx ? in_ptr(prhs[2]) : dbl(prhs[2], "wL");
        const void* wR = cplx ? in_ptr(prhs[3]) : dbl(prhs[3], "wR");
        double imag_sum[2] = {0, 0};
        const int rc = emagls_binaural_decode_complex(in, ic, n, ch, wL, wR, wc, len, comp, mxGetDoubles(plhs[0]), imag_sum);
        if (cplx && nlhs > 1) { plhs[1] = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetDoubles(plhs[1])[0] = imag_sum[0]; mxGetDoubles(plhs[1])[1] = imag_sum[1]; }
        if (rc) fail(rc);
        return;
    }
    if (c == "sets") {
        // [wL, wR] = emagls_mex('sets', kind, hL, hR, azi, zen, micRadius, micAzi, micZen, order, fs, len, shDefinition)
        // hL, hR [numSamples x numDirections x numSets]; zen / micAzi / micZen may be [] where the single call has no such argument.
        // The loop over HRIR sets around lib/getLsFilters.m:30, getMagLsFilters.m:30, getMagLsFilters2D.m:1, getEMagLsFilters.m:32,
        // getEMagLs2Filters.m:32, getEMagLsFiltersEMAinCH.m:32 in one call (emagls_design_hrir_sets).
        if (nrhs < 13) mexErrMsgIdAndTxt("eMagLS:arg", "sets needs (kind, hL, hR, azi, zen, micRadius, micAzi, micZen, order, fs, len, shDefinition)");
        char kb[16] = {0};
        mxGetString(prhs[1], kb, sizeof kb);
        const std::string ks(kb);
        int kind;
        if (ks == "ls") kind = EMAGLS_KIND_LS; else if (ks == "magls") kind = EMAGLS_KIND_MAGLS; else if (ks == "magls2d") kind = EMAGLS_KIND_MAGLS_2D;
        else if (ks == "emagls") kind = EMAGLS_KIND_EMAGLS; else if (ks == "emagls2") kind = EMAGLS_KIND_EMAGLS2;
        else if (ks == "emainch") kind = EMAGLS_KIND_EMA_CH; else if (ks == "emainsh") kind = EMAGLS_KIND_EMA_SH;
        else { mexErrMsgIdAndTxt("eMagLS:arg", "unknown design kind '%s'", kb); return; }
        const double* hL = dbl(prhs[2], "hL");
        const double* hR = dbl(prhs[3], "hR");
        const mwSize nd = mxGetNumberOfDimensions(prhs[2]);
        const mwSize* hd = mxGetDimensions(prhs[2]);
        const mwSize nsamp = hd[0], ndirs = hd[1], nsets = nd > 2 ? hd[2] : 1;
        if (mxGetNumberOfElements(prhs[3]) != mxGetNumberOfElements(prhs[2])) mexErrMsgIdAndTxt("eMagLS:arg", "hL and hR must have the same size");
        auto opt = [&](int i, const char* what) -> const double* { return mxIsEmpty(prhs[i]) ? nullptr : dbl(prhs[i], what); };
        const double* azi = dbl(prhs[4], "hrirGridAziRad");
        const double* zen = opt(5, "hrirGridZenRad");
        const double r = mxIsEmpty(prhs[6]) ? 0.0 : mxGetScalar(prhs[6]);
        const double* mazi = opt(7, "micGridAziRad");
        const double* mzen = opt(8, "micGridZenRad");
        const mwSize nmics = mazi ? mxGetNumberOfElements(prhs[7]) : 0;
        const int order = (int)mxGetScalar(prhs[9]);
        const double fs = mxIsEmpty(prhs[10]) ? 48000.0 : mxGetScalar(prhs[10]);
        const mwSize len = kind == EMAGLS_KIND_LS ? nsamp : (mwSize)mxGetScalar(prhs[11]);
        const int basis = basis_of(prhs[12]);
        mwSize C;
        switch (kind) {
            case EMAGLS_KIND_MAGLS_2D: case EMAGLS_KIND_EMA_CH: C = (mwSize)(2 * order + 1); break;
            case EMAGLS_KIND_EMAGLS2: C = nmics; break;
            default: C = (mwSize)((order + 1) * (order + 1));
        }
        const mwSize od[3] = {len, C, nsets};
        plhs[0] = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, basis == EMAGLS_BASIS_COMPLEX ? mxCOMPLEX : mxREAL);
        mxArray* wR = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, basis == EMAGLS_BASIS_COMPLEX ? mxCOMPLEX : mxREAL);
        const int rc = emagls_design_hrir_sets(kind, hL, hR, nsamp, ndirs, nsets, azi, zen, r, mazi, mzen, nmics, order, fs, len, basis,
                                               out_ptr(plhs[0]), out_ptr(wR));
        if (nlhs > 1) plhs[1] = wR; else mxDestroyArray(wR);
        if (rc) fail(rc);
        return;
    }
    if (c == "jobs") {
        // W = emagls_mex('jobs', jobs, batchSize, inFlight, shareGeometry, devices)
        // The loop a user of the reference writes around one of its design functions (testEMagLs.m:75-95: array radii; HRIR sets;
        // testEMagLsFromAtfs.m:72-73: subjects) handed over in ONE call: the library's scheduler (emagls_jobs_run) cuts the list into
        // chunks of one shape, runs each as a lane batch and keeps several chunks in flight.  `jobs` is a struct array, one element per
        // design, with the reference's argument names as fields:
        //   kind ('ls' | 'magls' | 'magls2d' | 'emagls' | 'emagls2' | 'emainch' | 'emainsh' | 'fromatf'), hL, hR, hrirGridAziRad,
        //   hrirGridZenRad, order, fs, len, shDefinition, micRadius, micGridAziRad, micGridZenRad (array designs),
        //   atfIrs, atfGridAziRad, atfGridZenRad, fTrans (fromatf), applyDiffusenessConst, simOrderPad (optional)
        // Returns an n x 2 cell array {wL, wR} with the filters each single call would return.
        if (nrhs < 2 || !mxIsStruct(prhs[1])) mexErrMsgIdAndTxt("eMagLS:arg", "jobs needs a struct array of designs");
        const mxArray* J = prhs[1];
        const mwSize n = mxGetNumberOfElements(J);
        auto num = [&](int i, double dflt) { return nrhs > i && !mxIsEmpty(prhs[i]) ? mxGetScalar(prhs[i]) : dflt; };
        const int batch_size = (int)num(2, 0), in_flight = (int)num(3, 0);
        const int share = nrhs > 4 && (mxIsLogicalScalarTrue(prhs[4]) || (!mxIsEmpty(prhs[4]) && mxGetScalar(prhs[4]) != 0));
        plhs[0] = mxCreateCellMatrix(n, 2);
        std::vector<emagls_job> jobs(n);
        for (mwSize i = 0; i < n; ++i) {
            auto fld = [&](const char* name) -> const mxArray* { const mxArray* a = mxGetField(J, i, name); return (a && !mxIsEmpty(a)) ? a : nullptr; };
            auto req = [&](const char* name) -> const mxArray* {
                const mxArray* a = fld(name);
                if (!a) mexErrMsgIdAndTxt("eMagLS:arg", "jobs(%d).%s is missing", (int)i + 1, name);
                return a;
            };
            auto vec = [&](const char* name, mwSize want) -> const double* {
                const mxArray* a = fld(name);
                if (!a) return nullptr;
                if (mxGetNumberOfElements(a) != want) mexErrMsgIdAndTxt("eMagLS:arg", "jobs(%d).%s must have %d elements", (int)i + 1, name, (int)want);
                return dbl(a, name);
            };
            char kb[16] = {0};
            mxGetString(req("kind"), kb, sizeof kb);
            const std::string ks(kb);
            emagls_job& jb = jobs[i];
            std::memset(&jb, 0, sizeof jb);
            emagls_design_desc& d = jb.desc;
            if (ks == "ls") d.kind = EMAGLS_KIND_LS; else if (ks == "magls") d.kind = EMAGLS_KIND_MAGLS; else if (ks == "magls2d") d.kind = EMAGLS_KIND_MAGLS_2D;
            else if (ks == "emagls") d.kind = EMAGLS_KIND_EMAGLS; else if (ks == "emagls2") d.kind = EMAGLS_KIND_EMAGLS2;
            else if (ks == "emainch") d.kind = EMAGLS_KIND_EMA_CH; else if (ks == "emainsh") d.kind = EMAGLS_KIND_EMA_SH;
            else if (ks == "fromatf") d.kind = EMAGLS_KIND_FROM_ATF;
            else mexErrMsgIdAndTxt("eMagLS:arg", "jobs(%d).kind: unknown design kind '%s'", (int)i + 1, kb);
            const mxArray* hL = req("hL");
            const mxArray* hR = req("hR");
            if (mxGetM(hL) != mxGetM(hR) || mxGetN(hL) != mxGetN(hR)) mexErrMsgIdAndTxt("eMagLS:arg", "jobs(%d): hL and hR must have the same size", (int)i + 1);
            d.nsamp = (int64_t)mxGetM(hL); d.ndirs = (int64_t)mxGetN(hL);
            jb.hL = dbl(hL, "hL"); jb.hR = dbl(hR, "hR");
            d.basis = basis_of(fld("shDefinition"));
            const bool atf = d.kind == EMAGLS_KIND_FROM_ATF;
            d.order = atf ? 0 : (int)mxGetScalar(req("order"));
            d.fs = fld("fs") ? mxGetScalar(fld("fs")) : 48000.0;
            d.len = d.kind == EMAGLS_KIND_LS ? d.nsamp : (int64_t)mxGetScalar(req("len"));
            jb.hrir_azi = vec("hrirGridAziRad", (mwSize)d.ndirs);
            jb.hrir_zen = vec("hrirGridZenRad", (mwSize)d.ndirs);
            if (!jb.hrir_azi) mexErrMsgIdAndTxt("eMagLS:arg", "jobs(%d).hrirGridAziRad is missing", (int)i + 1);
            const bool arr = d.kind == EMAGLS_KIND_EMAGLS || d.kind == EMAGLS_KIND_EMAGLS2 || d.kind == EMAGLS_KIND_EMA_CH || d.kind == EMAGLS_KIND_EMA_SH;
            if (arr) {
                d.mic_radius = mxGetScalar(req("micRadius"));
                d.nmics = (int64_t)mxGetNumberOfElements(req("micGridAziRad"));
                jb.mic_azi = vec("micGridAziRad", (mwSize)d.nmics);
                jb.mic_zen = vec("micGridZenRad", (mwSize)d.nmics);
            }
            if (atf) {
                const mxArray* a = req("atfIrs");                      // [taps x mics x dirs] (lib/getEMagLsFiltersFromAtf.m:11)
                const mwSize* ad = mxGetDimensions(a);
                d.atf_taps = (int64_t)ad[0]; d.nmics = (int64_t)ad[1]; d.natf = mxGetNumberOfDimensions(a) > 2 ? (int64_t)ad[2] : 1;
                jb.atf = dbl(a, "atfIrs");
                jb.atf_azi = vec("atfGridAziRad", (mwSize)d.natf);
                jb.atf_zen = vec("atfGridZenRad", (mwSize)d.natf);
                d.f_trans = mxGetScalar(req("fTrans"));
                d.basis = EMAGLS_BASIS_REAL;
            }
            if (const mxArray* a = fld("applyDiffusenessConst")) d.diffuseness = mxIsLogicalScalarTrue(a) || mxGetScalar(a) != 0;
            if (const mxArray* a = fld("simOrderPad")) d.sim_order_pad = (int)mxGetScalar(a);
            int64_t rows = 0, cols = 0;
            int cplx = 0;
            const int rc = emagls_design_out_shape(&d, &rows, &cols, &cplx);
            if (rc) fail(rc);
            mxArray* wl = mxCreateDoubleMatrix((mwSize)rows, (mwSize)cols, cplx ? mxCOMPLEX : mxREAL);
            mxArray* wr = mxCreateDoubleMatrix((mwSize)rows, (mwSize)cols, cplx ? mxCOMPLEX : mxREAL);
            mxSetCell(plhs[0], i, wl);           // column-major n x 2: wL in column 1, wR in column 2
            mxSetCell(plhs[0], n + i, wr);
            jb.wL = out_ptr(wl); jb.wR = out_ptr(wr);
        }
        // devices (optional, 6th argument): HIP ordinals of the GPUs of this MATLAB process to split the list over -- one host thread per
        // device, every device writes its jobs' filters straight into the output arrays (emagls_jobs_run_devices; no gather)
        std::vector<int> devices;
        if (nrhs > 5 && !mxIsEmpty(prhs[5])) {
            const double* dv = dbl(prhs[5], "devices");
            for (mwSize i = 0; i < mxGetNumberOfElements(prhs[5]); ++i) devices.push_back((int)dv[i]);
        }
        const int fl = share ? EMAGLS_JOBS_SHARE_GEOMETRY : 0;
        const int rc = !n ? 0 : devices.empty() ? emagls_jobs_run(jobs.data(), (int64_t)n, batch_size, in_flight, fl)
                                                 : emagls_jobs_run_devices(jobs.data(), (int64_t)n, devices.data(), (int)devices.size(), batch_size, in_flight, fl);
        if (rc) fail(rc);
        return;
    }
    if (c == "fromatfsets") {
        // [wL, wR] = emagls_mex('fromatfsets', hL, hR, hrirGridAziZenRad, atfIrs, atfGridAziZenRad, fs, filterLen, fTrans)
        // hL, hR [numSamples x numDirections x numSubjects]: lib/getEMagLsFiltersFromAtf.m:1 in a loop over subjects, one call
        if (nrhs < 9) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const double* hL = dbl(prhs[1], "hL");
        const double* hR = dbl(prhs[2], "hR");
        const mwSize* hd = mxGetDimensions(prhs[1]);
        const mwSize nsamp = hd[0], ndirs = hd[1], nsets = mxGetNumberOfDimensions(prhs[1]) > 2 ? hd[2] : 1;
        if (mxGetNumberOfElements(prhs[2]) != mxGetNumberOfElements(prhs[1])) mexErrMsgIdAndTxt("eMagLS:arg", "hL and hR must have the same size");
        const double* hg = dbl(prhs[3], "hrirGridAziZenRad");
        const mwSize* ad = mxGetDimensions(prhs[4]);
        const mwSize taps = ad[0], mics = ad[1], natf = mxGetNumberOfDimensions(prhs[4]) > 2 ? ad[2] : 1;
        const double* ag = dbl(prhs[5], "atfGridAziZenRad");
        const mwSize len = (mwSize)mxGetScalar(prhs[7]);
        const mwSize od[3] = {len, mics, nsets};
        plhs[0] = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, mxREAL);
        mxArray* wR = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, mxREAL);
        double dev = 0.0;
        const int rc = emagls_from_atf_hrir_sets(hL, hR, nsamp, ndirs, nsets, hg, hg + ndirs, dbl(prhs[4], "atfIrs"), taps, mics, natf, ag, ag + natf,
                                                 mxGetScalar(prhs[6]), len, mxGetScalar(prhs[8]), mxGetDoubles(plhs[0]), mxGetDoubles(wR), &dev);
        if (nlhs > 1) plhs[1] = wR; else mxDestroyArray(wR);
        if (rc) fail(rc);
        mexPrintf("Matching HRTF and ATF grids, average grid deviation: %g deg\n", dev);  // FromAtf.m:96
        return;
    }
    if (c == "simorder") {   // kind: 'emagls' | 'emagls2'
        char kind[16] = {0};
        mxGetString(prhs[1], kind, sizeof kind);
        plhs[0] = mxCreateDoubleScalar(emagls_simulation_order(!std::strcmp(kind, "emagls2") ? EMAGLS_KIND_EMAGLS2 : EMAGLS_KIND_EMAGLS,
                                                               (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), mxGetScalar(prhs[4])));
        return;
    }
    if (c == "radial" || c == "applyradial") {
        const int o = c == "radial" ? 1 : 2;     // index of `order`
        if (nrhs < o + 8) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const int order = (int)mxGetScalar(prhs[o]);
        const double fs = mxGetScalar(prhs[o + 1]), r = mxGetScalar(prhs[o + 2]);
        const mwSize irLen = (mwSize)mxGetScalar(prhs[o + 3]);
        const int ovs = (int)mxGetScalar(prhs[o + 4]), type = radial_type(prhs[o + 5]);
        const double regul = mxGetScalar(prhs[o + 6]), gain = mxGetScalar(prhs[o + 7]);
        int rc;
        if (c == "radial") {
            plhs[0] = mxCreateDoubleMatrix((irLen * ovs) / 2 + 1, order + 1, mxCOMPLEX);
            rc = emagls_get_radial_filter(order, fs, r, irLen, ovs, type, regul, gain, mxGetComplexDoubles(plhs[0]));
        } else {
            const mwSize n = mxGetM(prhs[1]);
            plhs[0] = mxCreateDoubleMatrix(emagls_apply_radial_filter_rows(n, irLen, ovs), mxGetN(prhs[1]), mxREAL);
            if (mxGetN(prhs[1]) != (mwSize)((order + 1) * (order + 1))) mexErrMsgIdAndTxt("eMagLS:arg", "inSig must have (order+1)^2 columns");
            rc = emagls_apply_radial_filter(dbl(prhs[1], "inSig"), n, order, fs, r, irLen, ovs, type, regul, gain, mxGetDoubles(plhs[0]));
        }
        if (rc) fail(rc);
        return;
    }
    if (c == "ch") {   // getCH(N, aziRad, basisType)
        const int order = (int)mxGetScalar(prhs[1]), basis = basis_of(nrhs > 3 ? prhs[3] : nullptr);
        const mwSize nd = mxGetNumberOfElements(prhs[2]);
        plhs[0] = out_matrix(nd, 2 * order + 1, basis);
        int rc = emagls_ch_basis(order, nd, dbl(prhs[2], "aziRad"), basis, out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "smair") {   // (order, fs, irLen, oversamplingFactor, smaRadius, micAzi, micZen, shDefinition, returnRawMicSigs, radialFilter, regulConst, noiseGainDb)
        if (nrhs < 13) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const int order = (int)mxGetScalar(prhs[1]);
        const double fs = mxGetScalar(prhs[2]), r = mxGetScalar(prhs[5]);
        const mwSize irLen = (mwSize)mxGetScalar(prhs[3]), M = mxGetNumberOfElements(prhs[6]);
        const int ovs = (int)mxGetScalar(prhs[4]), basis = basis_of(prhs[8]);
        const int raw = mxIsLogicalScalarTrue(prhs[9]) || mxGetScalar(prhs[9]) != 0;
        const int so = emagls_simulation_order(EMAGLS_KIND_EMAGLS, order, fs, r);
        const mwSize dims[3] = {raw ? M : (mwSize)((order + 1) * (order + 1)), (mwSize)((so + 1) * (so + 1)), (irLen * ovs) / 2 + 1};
        plhs[0] = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
        int rc = emagls_get_smair_matrix(order, fs, irLen, ovs, r, dbl(prhs[6], "micAzi"), dbl(prhs[7], "micZen"), M, basis, raw,
                                         radial_type(prhs[10]), mxGetScalar(prhs[11]), mxGetScalar(prhs[12]), mxGetComplexDoubles(plhs[0]), nullptr);
        if (rc) fail(rc);
        return;
    }
    if (c == "rendered_hrtfs") {   // (wL, wR, model, dirsAziZenRad, fs, order, micRadius, micGridAziZenRad, atfIrs, nfft, shDefinition, hL, hR, weights, returnResponse)
        // [] for what a model does not use.  [H, magErrDb, ildErrDb, covHat, covRef] = ...: H [P x D x 2 x numSets], the metrics
        // [P x 2 x numSets], [P x numSets], [P x 4 x numSets] (empty without hL, hR; H empty with returnResponse false)
        if (nrhs < 16) mexErrMsgIdAndTxt("eMagLS:arg", "rendered_hrtfs needs 15 arguments ([] for those the model does not use)");
        const FilterArgs f = filter_args(prhs);
        char mbuf[16] = {0};
        mxGetString(prhs[3], mbuf, sizeof mbuf);
        const std::string mname(mbuf);
        const int model = mname == "sh" ? EMAGLS_MODEL_SH : mname == "emagls" ? EMAGLS_MODEL_EMAGLS : mname == "emagls2" ? EMAGLS_MODEL_EMAGLS2
                        : mname == "atf" ? EMAGLS_MODEL_ATF : mname == "ema_ch" ? EMAGLS_MODEL_EMA_CH : mname == "ema_sh" ? EMAGLS_MODEL_EMA_SH : -1;
        if (model < 0) mexErrMsgIdAndTxt("eMagLS:arg", "model must be 'sh', 'emagls', 'emagls2', 'atf', 'ema_ch' or 'ema_sh'");
        const bool ema = model == EMAGLS_MODEL_EMA_CH || model == EMAGLS_MODEL_EMA_SH;
        auto given = [&](int i) { return prhs[i] && !mxIsEmpty(prhs[i]); };
        auto grid = [&](int i, const char* what, mwSize* n) -> const double* {
            if (!given(i)) { *n = 0; return nullptr; }
            if (mxGetN(prhs[i]) != 2) mexErrMsgIdAndTxt("eMagLS:arg", "%s must be [n x 2] (azimuth, zenith)", what);
            *n = mxGetM(prhs[i]);
            return dbl(prhs[i], what);
        };
        mwSize D = 0, M = 0, taps = 0;
        const double* dirs = grid(4, "dirsAziZenRad", &D);
        // (an equatorial array: a vector of azimuths, or [M x 2] with every zenith pi/2; the library does not look at the zeniths)
        const bool azi_only = ema && given(8) && mxGetN(prhs[8]) != 2 && (mxGetM(prhs[8]) == 1 || mxGetN(prhs[8]) == 1);
        const double* mics = azi_only ? dbl(prhs[8], "micGridAziZenRad") : grid(8, "micGridAziZenRad", &M);
        if (azi_only) M = mxGetNumberOfElements(prhs[8]);
        for (mwSize i = 0; ema && mics && !azi_only && i < M; ++i)
            if (mics[M + i] != 1.5707963267948966) mexErrMsgIdAndTxt("eMagLS:arg", "an equatorial array's micGridAziZenRad must have every zenith at pi/2");
        const double* atf = nullptr;
        if (given(9)) {
            atf = dbl(prhs[9], "atfIrs");
            const mwSize nd = mxGetNumberOfDimensions(prhs[9]);
            const mwSize* d = mxGetDimensions(prhs[9]);
            if (nd != 3) mexErrMsgIdAndTxt("eMagLS:arg", "atfIrs must be [taps x numMics x numDirections]");
            if (D && d[2] != D) mexErrMsgIdAndTxt("eMagLS:arg", "atfIrs must be given on the evaluation directions");
            taps = d[0]; M = d[1]; D = d[2];
        }
        const double fs = given(5) ? mxGetScalar(prhs[5]) : 0.0, radius = given(7) ? mxGetScalar(prhs[7]) : 0.0;
        const int order = given(6) ? (int)mxGetScalar(prhs[6]) : 0, basis = basis_of(prhs[11]);
        const int64_t nfft = given(10) ? (int64_t)mxGetScalar(prhs[10]) : (int64_t)std::min<mwSize>(2048, 2 * f.len);
        const mwSize P = (mwSize)(nfft / 2 + 1);
        const double *hL = nullptr, *hR = nullptr, *wts = nullptr;
        mwSize nsamp = 0, nh = 0;
        if (given(12) != given(13)) mexErrMsgIdAndTxt("eMagLS:arg", "hL and hR go together");
        if (given(12)) {
            hL = dbl(prhs[12], "hL"); hR = dbl(prhs[13], "hR");
            const mwSize nd = mxGetNumberOfDimensions(prhs[12]);
            const mwSize* d = mxGetDimensions(prhs[12]);
            bool same = nd <= 3 && mxGetNumberOfDimensions(prhs[13]) == nd;
            for (mwSize i = 0; same && i < nd; ++i) same = mxGetDimensions(prhs[13])[i] == d[i];
            if (!same || d[1] != D) mexErrMsgIdAndTxt("eMagLS:arg", "hL and hR must be [numSamples x numDirections (x numSets)] arrays of equal size");
            nsamp = d[0]; nh = nd == 3 ? d[2] : 1;
            if (given(14)) {
                if (mxGetNumberOfElements(prhs[14]) != D) mexErrMsgIdAndTxt("eMagLS:arg", "weights must have one element per direction");
                wts = dbl(prhs[14], "weights");
            }
        }
        const bool want_h = truthy(prhs[15]);
        std::vector<double> H, mag, ild, ch, cr;
        if (want_h) H.resize((size_t)2 * f.nsets * 2 * P * D);
        if (hL) { mag.resize((size_t)f.nsets * P * 2); ild.resize((size_t)f.nsets * P); ch.resize((size_t)f.nsets * P * 4); cr.resize(ch.size()); }
        auto ptr = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
        const int rc = emagls_rendered_hrtfs(model, in_ptr(prhs[1]), in_ptr(prhs[2]), f.wc ? 1 : 0, (int64_t)f.len, (int64_t)f.ch, (int64_t)f.nsets, dirs,
                                             dirs ? dirs + D : nullptr, (int64_t)D, fs, order, basis, radius, mics, mics && !azi_only ? mics + M : nullptr,
                                             (int64_t)M, atf, (int64_t)taps, nfft, hL, hR, (int64_t)nsamp, (int64_t)nh, wts, ptr(H), ptr(mag), ptr(ild),
                                             ptr(ch), ptr(cr));
        if (rc) fail(rc);
        // the library's [set][ear][k][d] / [set][k][j] -> MATLAB's [k, d, ear, set] / [k, j, set]
        const mwSize hd[4] = {want_h ? P : 0, want_h ? D : 0, want_h ? (mwSize)2 : 0, want_h ? f.nsets : 0};
        plhs[0] = mxCreateNumericArray(4, hd, mxDOUBLE_CLASS, mxCOMPLEX);
        if (want_h) {
            double* o = (double*)mxGetComplexDoubles(plhs[0]);
            for (size_t se = 0; se < (size_t)2 * f.nsets; ++se)
                for (size_t k = 0; k < P; ++k)
                    for (size_t d = 0; d < D; ++d) {
                        const size_t src = (se * P + k) * D + d, dst = k + P * (d + D * se);
                        o[2 * dst] = H[2 * src]; o[2 * dst + 1] = H[2 * src + 1];
                    }
        }
        auto metric = [&](int idx, const std::vector<double>& v, mwSize cols) {
            if (nlhs <= idx) return;
            const mwSize md[3] = {v.empty() ? 0 : P, v.empty() ? 0 : cols, v.empty() ? 0 : f.nsets};
            plhs[idx] = mxCreateNumericArray(3, md, mxDOUBLE_CLASS, mxREAL);
            double* o = mxGetDoubles(plhs[idx]);
            for (size_t i = 0; i < v.size(); ++i) {
                const size_t j = i % cols, k = (i / cols) % P, set = i / (cols * P);
                o[k + P * (j + cols * set)] = v[i];
            }
        };
        metric(1, mag, 2); metric(2, ild, 1); metric(3, ch, 4); metric(4, cr, 4);
        return;
    }
    if (c == "array_irs") {   // (compPtr, comps, fs, irLen, preDelay, micRadius, micGridAziZenRad, order, encoder, nfft)
        // compPtr [numSources + 1]: zero-based offsets into the rows of comps [J x 4] = (azi, zen, delay, gain) (mex/getArrayIrs.m builds
        // both); encoder [numChannels x numMics] or []; nfft or [].  irs = ...: [irLen x numChannels x numSources], as the library lays it
        if (nrhs < 11) mexErrMsgIdAndTxt("eMagLS:arg", "array_irs needs 10 arguments ([] for no encoder and for the default nfft)");
        auto given = [&](int i) { return prhs[i] && !mxIsEmpty(prhs[i]); };
        const mwSize nptr = mxGetNumberOfElements(prhs[1]), J = mxGetM(prhs[2]);
        if (nptr < 2) mexErrMsgIdAndTxt("eMagLS:arg", "compPtr must have numSources + 1 elements");
        const double* pd = dbl(prhs[1], "compPtr");
        std::vector<int64_t> ptr(nptr);
        for (mwSize i = 0; i < nptr; ++i) {
            if (pd[i] != std::floor(pd[i]) || std::fabs(pd[i]) > 9e15) mexErrMsgIdAndTxt("eMagLS:arg", "compPtr must hold integers");
            ptr[i] = (int64_t)pd[i];
        }
        if (J && mxGetN(prhs[2]) != 4) mexErrMsgIdAndTxt("eMagLS:arg", "comps must be [J x 4] (azimuth, zenith, delay, gain)");
        if (ptr[nptr - 1] != (int64_t)J) mexErrMsgIdAndTxt("eMagLS:arg", "compPtr must end at the number of rows of comps");
        const double* comps = J ? dbl(prhs[2], "comps") : nullptr;
        if (mxGetN(prhs[7]) != 2) mexErrMsgIdAndTxt("eMagLS:arg", "micGridAziZenRad must be [n x 2] (azimuth, zenith)");
        const mwSize M = mxGetM(prhs[7]), nr = (mwSize)mxGetScalar(prhs[4]), Q = nptr - 1;
        const double* mics = dbl(prhs[7], "micGridAziZenRad");
        mwSize Cc = M;
        bool ec = false;
        if (given(9)) {
            if (!mxIsDouble(prhs[9]) || mxGetN(prhs[9]) != M) mexErrMsgIdAndTxt("eMagLS:arg", "encoder must be [numChannels x numMics] with one column per microphone (%d)", (int)M);
            Cc = mxGetM(prhs[9]);
            ec = mxIsComplex(prhs[9]);
        }
        const mwSize od[3] = {nr, Cc, Q};
        plhs[0] = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, ec ? mxCOMPLEX : mxREAL);
        // the spectral gain, four further arguments, [] or absent for none: surfaceReflection [W x P], exponents
        // [J x W], airAttenuation [P], pathLength [J]; P = nfft / 2 + 1
        // point sources, a fifteenth argument, [] or absent for none: distance [J] in metres, one per component
        auto extra = [&](int i) { return nrhs > i && given(i); };
        if (extra(15) && mxGetNumberOfElements(prhs[15]) != J) mexErrMsgIdAndTxt("eMagLS:arg", "distance must have one element per component (%d)", (int)J);
        // directive sources, three further arguments, [] or absent for none: emission [J x 3], sourceOrientation
        // [numSources x 9] ([]: the room's axes), directivity [numSources Kd x P]
        if ((extra(16) || extra(17)) && !extra(18)) mexErrMsgIdAndTxt("eMagLS:arg", "emission and sourceOrientation come with a directivity");
        if (extra(18) && J && (!extra(16) || mxGetM(prhs[16]) != J || mxGetN(prhs[16]) != 3))
            mexErrMsgIdAndTxt("eMagLS:arg", "a directivity needs emission [J x 3], one unit vector per component (%d)", (int)J);
        if (extra(11) || extra(12) || extra(13) || extra(14) || extra(15) || extra(18)) {
            if (extra(11) != extra(12)) mexErrMsgIdAndTxt("eMagLS:arg", "surfaceReflection and exponents must both be given or both be []");
            if (extra(13) != extra(14)) mexErrMsgIdAndTxt("eMagLS:arg", "airAttenuation and pathLength must both be given or both be []");
            const int64_t nfft = spectral_nfft(given(10) ? prhs[10] : nullptr, nr);
            const mwSize P = (mwSize)(nfft / 2 + 1), W = extra(11) ? mxGetM(prhs[11]) : 0;
            std::vector<double> refl;
            std::vector<int32_t> ex;
            if (W) {
                if (mxGetN(prhs[11]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "surfaceReflection must be [numSurfaces x %d] (nfft / 2 + 1 bins)", (int)P);
                if (mxGetM(prhs[12]) != J || mxGetN(prhs[12]) != W) mexErrMsgIdAndTxt("eMagLS:arg", "exponents must be [J x numSurfaces]");
                refl = rows_of(dbl(prhs[11], "surfaceReflection"), W, P);
                ex = exponents_of(dbl(prhs[12], "exponents"), J, W);
            }
            if (extra(13) && (mxGetNumberOfElements(prhs[13]) != P || mxGetNumberOfElements(prhs[14]) != (J ? J : mxGetNumberOfElements(prhs[14]))))
                mexErrMsgIdAndTxt("eMagLS:arg", "airAttenuation must have %d elements (nfft / 2 + 1 bins) and pathLength one per component", (int)P);
            const double *att = extra(13) ? dbl(prhs[13], "airAttenuation") : nullptr, *len = extra(13) ? dbl(prhs[14], "pathLength") : nullptr;
            if (extra(18)) {
                std::vector<double> coef, rot, emit;
                const int Nd = directivity_of(prhs[18], Q, P, coef);
                if (extra(17)) rot = rotations_of(prhs[17], Q);
                if (J) emit = rows_of(dbl(prhs[16], "emission"), J, 3);
                const int rc = emagls_array_irs_directive(mxGetScalar(prhs[3]), mxGetScalar(prhs[6]), (int)mxGetScalar(prhs[8]), mics, mics + M, (int64_t)M,
                                                          given(9) ? in_ptr(prhs[9]) : nullptr, ec ? 1 : 0, (int64_t)Cc, (int64_t)Q, ptr.data(), comps,
                                                          comps ? comps + J : nullptr, comps ? comps + 2 * J : nullptr, comps ? comps + 3 * J : nullptr,
                                                          (int64_t)W, W ? refl.data() : nullptr, ex.empty() ? nullptr : ex.data(), att, len,
                                                          extra(15) ? dbl(prhs[15], "distance") : nullptr, J ? emit.data() : nullptr,
                                                          extra(17) ? rot.data() : nullptr, Nd, coef.data(), mxGetScalar(prhs[5]), nfft, (int64_t)nr,
                                                          out_ptr(plhs[0]));
                if (rc) fail(rc);
                return;
            }
            const int rc = extra(15)
                ? emagls_array_irs_point(mxGetScalar(prhs[3]), mxGetScalar(prhs[6]), (int)mxGetScalar(prhs[8]), mics, mics + M, (int64_t)M,
                                         given(9) ? in_ptr(prhs[9]) : nullptr, ec ? 1 : 0, (int64_t)Cc, (int64_t)Q, ptr.data(), comps,
                                         comps ? comps + J : nullptr, comps ? comps + 2 * J : nullptr, comps ? comps + 3 * J : nullptr,
                                         (int64_t)W, W ? refl.data() : nullptr, ex.empty() ? nullptr : ex.data(), att, len,
                                         dbl(prhs[15], "distance"), mxGetScalar(prhs[5]), nfft, (int64_t)nr, out_ptr(plhs[0]))
                : emagls_array_irs_spectral(mxGetScalar(prhs[3]), mxGetScalar(prhs[6]), (int)mxGetScalar(prhs[8]), mics, mics + M, (int64_t)M,
                                            given(9) ? in_ptr(prhs[9]) : nullptr, ec ? 1 : 0, (int64_t)Cc, (int64_t)Q, ptr.data(), comps,
                                            comps ? comps + J : nullptr, comps ? comps + 2 * J : nullptr, comps ? comps + 3 * J : nullptr,
                                            (int64_t)W, W ? refl.data() : nullptr, ex.empty() ? nullptr : ex.data(), att, len,
                                            mxGetScalar(prhs[5]), nfft, (int64_t)nr, out_ptr(plhs[0]));
            if (rc) fail(rc);
            return;
        }
        const int rc = emagls_array_irs(mxGetScalar(prhs[3]), mxGetScalar(prhs[6]), (int)mxGetScalar(prhs[8]), mics, mics + M, (int64_t)M,
                                        given(9) ? in_ptr(prhs[9]) : nullptr, ec ? 1 : 0, (int64_t)Cc, (int64_t)Q, ptr.data(), comps,
                                        comps ? comps + J : nullptr, comps ? comps + 2 * J : nullptr, comps ? comps + 3 * J : nullptr,
                                        mxGetScalar(prhs[5]), given(10) ? (int64_t)mxGetScalar(prhs[10]) : 0, (int64_t)nr, out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "shoebox_images") {   // (roomDim [3], sourcePos [numSources x 3], arrayPos [3], fs, maxDelay, maxOrder)
        // [compPtr, comps, exponents, paths] = ...: the lists of 'shoebox_components' without the walls: comps [J x 4]
        // with gain = 1 / distance, exponents [J x 6] of the walls x=0, x=Lx, y=0, y=Ly, z=0, z=Lz, paths [J x 1] in metres
        if (nrhs < 7) mexErrMsgIdAndTxt("eMagLS:arg", "shoebox_images needs 6 arguments ([] for no limit on the reflection order)");
        if (mxGetNumberOfElements(prhs[1]) != 3 || mxGetNumberOfElements(prhs[3]) != 3) mexErrMsgIdAndTxt("eMagLS:arg", "roomDim and arrayPos must have 3 elements");
        const mwSize Q = mxGetM(prhs[2]);
        if (Q < 1 || mxGetN(prhs[2]) != 3) mexErrMsgIdAndTxt("eMagLS:arg", "sourcePos must be [numSources x 3] (x, y, z per row)");
        const double *dim = dbl(prhs[1], "roomDim"), *sp = dbl(prhs[2], "sourcePos"), *pos = dbl(prhs[3], "arrayPos");
        std::vector<double> src(3 * Q);
        for (mwSize q = 0; q < Q; ++q)
            for (int i = 0; i < 3; ++i) src[3 * q + i] = sp[q + Q * i];
        const double fs = mxGetScalar(prhs[4]), max_delay = mxGetScalar(prhs[5]);
        const int max_order = prhs[6] && !mxIsEmpty(prhs[6]) ? (int)mxGetScalar(prhs[6]) : -1;
        std::vector<int64_t> ptr(Q + 1);
        int rc = emagls_shoebox_images(dim, pos, (int64_t)Q, src.data(), fs, max_delay, max_order, 0, ptr.data(), nullptr, nullptr, nullptr, nullptr,
                                       nullptr, nullptr);
        if (rc) fail(rc);
        const mwSize J = (mwSize)ptr[Q];
        plhs[0] = mxCreateDoubleMatrix(Q + 1, 1, mxREAL);
        mxArray *comps = mxCreateDoubleMatrix(J, 4, mxREAL), *exps = mxCreateDoubleMatrix(J, 6, mxREAL), *paths = mxCreateDoubleMatrix(J, 1, mxREAL);
        double* o = mxGetDoubles(comps);
        std::vector<int32_t> e(6 * (size_t)J);
        if (J) rc = emagls_shoebox_images(dim, pos, (int64_t)Q, src.data(), fs, max_delay, max_order, (int64_t)J, ptr.data(), o, o + J, o + 2 * J,
                                          o + 3 * J, e.data(), mxGetDoubles(paths));
        for (mwSize j = 0; j < J; ++j)
            for (int w = 0; w < 6; ++w) mxGetDoubles(exps)[j + J * w] = (double)e[6 * j + w];
        for (mwSize q = 0; q <= Q; ++q) mxGetDoubles(plhs[0])[q] = (double)ptr[q];
        mxArray* outs[3] = {comps, exps, paths};
        for (int i = 0; i < 3; ++i)
            if (nlhs > i + 1) plhs[i + 1] = outs[i]; else mxDestroyArray(outs[i]);
        if (rc) fail(rc);
        if (nlhs > 4) plhs[4] = shoebox_emission(dim, nullptr, pos, Q, src.data(), fs, max_delay, max_order, J);   // emission [J x 3] (section 15)
        return;
    }
    if (c == "shoebox_components" || c == "array_room_irs") {
        // the room of both: (roomDim [3], wallReflection [6], sourcePos [numSources x 3], arrayPos [3], fs, ...
        //   shoebox_components: ... maxDelay, maxOrder)                       [compPtr, comps] = ...: zero-based offsets [numSources + 1] and
        //                                                                     comps [J x 4] = (azi, zen, delay, gain), the inputs of 'array_irs'
        //   array_room_irs:     ... irLen, preDelay, micRadius, micGridAziZenRad, order, encoder, nfft, maxOrder, maxDelay)
        //                                                                     [irs, counts] = ...: [irLen x numChannels x numSources], [numSources]
        // maxOrder []: no limit; maxDelay [] (array_room_irs): irLen - 1 - preDelay
        // array_room_irs, the spectral room: wallReflection [6 x P], P = nfft / 2 + 1, and / or a fifteenth argument
        // airAttenuation [P] ([] or absent: none; six coefficients with it are repeated over the bins)
        const bool irs = c == "array_room_irs";
        if (nrhs < (irs ? 15 : 8))
            mexErrMsgIdAndTxt("eMagLS:arg", irs ? "array_room_irs needs 14 arguments ([] for no encoder and for the defaults of nfft, maxOrder and maxDelay)"
                                                : "shoebox_components needs 7 arguments ([] for no limit on the reflection order)");
        auto given = [&](int i) { return prhs[i] && !mxIsEmpty(prhs[i]); };
        if (mxGetNumberOfElements(prhs[1]) != 3 || mxGetNumberOfElements(prhs[4]) != 3) mexErrMsgIdAndTxt("eMagLS:arg", "roomDim and arrayPos must have 3 elements");
        // array_room_irs, a sixteenth argument waveModel ([] or absent: 'planeWave'): 'pointSource' makes every image a point source at its
        // distance
        bool point = false;
        if (irs && nrhs > 16 && given(16)) {
            char wm[32] = {0};
            if (!mxIsChar(prhs[16]) || mxGetString(prhs[16], wm, sizeof wm)) wm[0] = '?';
            point = std::string(wm) == "pointSource";
            if (!point && std::string(wm) != "planeWave") mexErrMsgIdAndTxt("eMagLS:arg", "unknown waveModel: 'planeWave' or 'pointSource'");
        }
        const bool air = irs && nrhs > 15 && given(15);
        const bool spectral = irs && (air || (mxGetNumberOfElements(prhs[2]) > 6 && mxGetM(prhs[2]) == 6));
        if (!spectral && mxGetNumberOfElements(prhs[2]) != 6)
            mexErrMsgIdAndTxt("eMagLS:arg", "wallReflection must have 6 elements (x=0, x=Lx, y=0, y=Ly, z=0, z=Lz)");
        const mwSize Q = mxGetM(prhs[3]);
        if (Q < 1 || mxGetN(prhs[3]) != 3) mexErrMsgIdAndTxt("eMagLS:arg", "sourcePos must be [numSources x 3] (x, y, z per row)");
        const double *dim = dbl(prhs[1], "roomDim"), *refl = dbl(prhs[2], "wallReflection"), *sp = dbl(prhs[3], "sourcePos"), *pos = dbl(prhs[4], "arrayPos");
        std::vector<double> src(3 * Q);
        for (mwSize q = 0; q < Q; ++q)
            for (int i = 0; i < 3; ++i) src[3 * q + i] = sp[q + Q * i];
        const double fs = mxGetScalar(prhs[5]);
        const int mo = irs ? 13 : 7;
        const int max_order = given(mo) ? (int)mxGetScalar(prhs[mo]) : -1;
        if (!irs) {
            std::vector<int64_t> ptr(Q + 1);
            const double max_delay = mxGetScalar(prhs[6]);
            int rc = emagls_shoebox_components(dim, refl, pos, (int64_t)Q, src.data(), fs, max_delay, max_order, 0, ptr.data(), nullptr, nullptr,
                                               nullptr, nullptr);
            if (rc) fail(rc);
            const mwSize J = (mwSize)ptr[Q];
            plhs[0] = mxCreateDoubleMatrix(Q + 1, 1, mxREAL);
            mxArray* comps = mxCreateDoubleMatrix(J, 4, mxREAL);
            double* o = mxGetDoubles(comps);
            if (nlhs > 2) {                            // [compPtr, comps, dists] = ...: the distances [J x 1] in metres
                plhs[2] = mxCreateDoubleMatrix(J, 1, mxREAL);
                if (J) rc = emagls_shoebox_components_dist(dim, refl, pos, (int64_t)Q, src.data(), fs, max_delay, max_order, (int64_t)J, ptr.data(), o,
                                                           o + J, o + 2 * J, o + 3 * J, mxGetDoubles(plhs[2]));
            } else if (J) {
                rc = emagls_shoebox_components(dim, refl, pos, (int64_t)Q, src.data(), fs, max_delay, max_order, (int64_t)J, ptr.data(), o, o + J,
                                               o + 2 * J, o + 3 * J);
            }
            for (mwSize q = 0; q <= Q; ++q) mxGetDoubles(plhs[0])[q] = (double)ptr[q];
            if (nlhs > 1) plhs[1] = comps; else mxDestroyArray(comps);
            if (rc) fail(rc);
            if (nlhs > 3) plhs[3] = shoebox_emission(dim, refl, pos, Q, src.data(), fs, max_delay, max_order, J);   // emission [J x 3] (section 15)
            return;
        }
        if (mxGetN(prhs[9]) != 2) mexErrMsgIdAndTxt("eMagLS:arg", "micGridAziZenRad must be [n x 2] (azimuth, zenith)");
        const mwSize M = mxGetM(prhs[9]), nr = (mwSize)mxGetScalar(prhs[6]);
        const double* mics = dbl(prhs[9], "micGridAziZenRad");
        mwSize Cc = M;
        bool ec = false;
        if (given(11)) {
            if (!mxIsDouble(prhs[11]) || mxGetN(prhs[11]) != M) mexErrMsgIdAndTxt("eMagLS:arg", "encoder must be [numChannels x numMics] with one column per microphone (%d)", (int)M);
            Cc = mxGetM(prhs[11]);
            ec = mxIsComplex(prhs[11]);
        }
        const double pre = mxGetScalar(prhs[7]), max_delay = given(14) ? mxGetScalar(prhs[14]) : (double)nr - 1.0 - pre;
        const mwSize od[3] = {nr, Cc, Q};
        plhs[0] = mxCreateNumericArray(3, od, mxDOUBLE_CLASS, ec ? mxCOMPLEX : mxREAL);
        std::vector<int64_t> counts(Q);
        // directive sources, two further arguments: sourceOrientation [numSources x 9] ([]: the room's axes) and
        // directivity [numSources Kd x P] ([] or absent: none); with every wall and wave model above
        const bool rotated = nrhs > 17 && given(17), directive = nrhs > 18 && given(18);
        if (rotated && !directive) mexErrMsgIdAndTxt("eMagLS:arg", "sourceOrientation comes with a directivity");
        if (directive) {
            const int64_t nfft = spectral_nfft(given(12) ? prhs[12] : nullptr, nr);
            const mwSize P = (mwSize)(nfft / 2 + 1);
            const bool spectra = mxGetNumberOfElements(prhs[2]) != 6;
            std::vector<double> walls, coef, rot;
            if (spectra) {
                if (mxGetM(prhs[2]) != 6 || mxGetN(prhs[2]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "wallReflection must be [6 x %d] (nfft / 2 + 1 bins)", (int)P);
                walls = rows_of(refl, 6, P);
            }
            if (air && mxGetNumberOfElements(prhs[15]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "airAttenuation must have %d elements (nfft / 2 + 1 bins)", (int)P);
            const int Nd = directivity_of(prhs[18], Q, P, coef);
            if (rotated) rot = rotations_of(prhs[17], Q);
            const int rc = emagls_array_room_irs_directive(fs, mxGetScalar(prhs[8]), (int)mxGetScalar(prhs[10]), mics, mics + M, (int64_t)M,
                                                           given(11) ? in_ptr(prhs[11]) : nullptr, ec ? 1 : 0, (int64_t)Cc, dim, spectra ? walls.data() : refl,
                                                           spectra ? 1 : 0, air ? dbl(prhs[15], "airAttenuation") : nullptr, pos, (int64_t)Q, src.data(),
                                                           max_delay, max_order, point ? 1 : 0, rotated ? rot.data() : nullptr, Nd, coef.data(), pre, nfft,
                                                           (int64_t)nr, counts.data(), out_ptr(plhs[0]));
            if (rc) fail(rc);
        } else if (point) {
            const int64_t nfft = spectral_nfft(given(12) ? prhs[12] : nullptr, nr);
            const mwSize P = (mwSize)(nfft / 2 + 1);
            const bool spectra = mxGetNumberOfElements(prhs[2]) != 6;
            std::vector<double> walls;
            if (spectra) {
                if (mxGetM(prhs[2]) != 6 || mxGetN(prhs[2]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "wallReflection must be [6 x %d] (nfft / 2 + 1 bins)", (int)P);
                walls = rows_of(refl, 6, P);
            }
            if (air && mxGetNumberOfElements(prhs[15]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "airAttenuation must have %d elements (nfft / 2 + 1 bins)", (int)P);
            const int rc = emagls_array_room_irs_point(fs, mxGetScalar(prhs[8]), (int)mxGetScalar(prhs[10]), mics, mics + M, (int64_t)M,
                                                       given(11) ? in_ptr(prhs[11]) : nullptr, ec ? 1 : 0, (int64_t)Cc, dim, spectra ? walls.data() : refl,
                                                       spectra ? 1 : 0, air ? dbl(prhs[15], "airAttenuation") : nullptr, pos, (int64_t)Q, src.data(),
                                                       max_delay, max_order, pre, nfft, (int64_t)nr, counts.data(), out_ptr(plhs[0]));
            if (rc) fail(rc);
        } else if (spectral) {
            const int64_t nfft = spectral_nfft(given(12) ? prhs[12] : nullptr, nr);
            const mwSize P = (mwSize)(nfft / 2 + 1);
            std::vector<double> walls(6 * (size_t)P);
            if (mxGetNumberOfElements(prhs[2]) == 6) {
                for (size_t i = 0; i < walls.size(); ++i) walls[i] = refl[i / P];
            } else {
                if (mxGetM(prhs[2]) != 6 || mxGetN(prhs[2]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "wallReflection must be [6 x %d] (nfft / 2 + 1 bins)", (int)P);
                walls = rows_of(refl, 6, P);
            }
            if (air && mxGetNumberOfElements(prhs[15]) != P) mexErrMsgIdAndTxt("eMagLS:arg", "airAttenuation must have %d elements (nfft / 2 + 1 bins)", (int)P);
            const int rc = emagls_array_room_irs_spectral(fs, mxGetScalar(prhs[8]), (int)mxGetScalar(prhs[10]), mics, mics + M, (int64_t)M,
                                                          given(11) ? in_ptr(prhs[11]) : nullptr, ec ? 1 : 0, (int64_t)Cc, dim, walls.data(),
                                                          air ? dbl(prhs[15], "airAttenuation") : nullptr, pos, (int64_t)Q, src.data(), max_delay,
                                                          max_order, pre, nfft, (int64_t)nr, counts.data(), out_ptr(plhs[0]));
            if (rc) fail(rc);
        } else {
        const int rc = emagls_array_room_irs(fs, mxGetScalar(prhs[8]), (int)mxGetScalar(prhs[10]), mics, mics + M, (int64_t)M,
                                             given(11) ? in_ptr(prhs[11]) : nullptr, ec ? 1 : 0, (int64_t)Cc, dim, refl, pos, (int64_t)Q, src.data(),
                                             max_delay, max_order, pre, given(12) ? (int64_t)mxGetScalar(prhs[12]) : 0, (int64_t)nr, counts.data(),
                                             out_ptr(plhs[0]));
        if (rc) fail(rc);
        }
        if (nlhs > 1) {
            plhs[1] = mxCreateDoubleMatrix(Q, 1, mxREAL);
            for (mwSize q = 0; q < Q; ++q) mxGetDoubles(plhs[1])[q] = (double)counts[q];
        }
        return;
    }
    if (c == "encode") {
        if (nrhs < 5) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const mwSize n = mxGetM(prhs[1]), M = mxGetN(prhs[1]);
        const int order = (int)mxGetScalar(prhs[4]), basis = basis_of(nrhs > 5 ? prhs[5] : nullptr);
        plhs[0] = out_matrix(n, (order + 1) * (order + 1), basis);
        int rc = emagls_sh_encode(dbl(prhs[1], "smaRecording"), n, M, dbl(prhs[2], "micAzi"), dbl(prhs[3], "micZen"), order, basis, out_ptr(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (c == "shf") {
        const mwSize len = (mwSize)mxGetScalar(prhs[4]);
        plhs[0] = mxCreateDoubleMatrix(len, 1, mxREAL);
        mxArray* W = mxCreateDoubleMatrix(emagls_eq_filter_nfft(len), 1, mxREAL);
        int rc = emagls_get_magls_spherical_head_filter(mxGetScalar(prhs[1]), (int)mxGetScalar(prhs[2]), mxGetScalar(prhs[3]), len,
                                                        mxGetDoubles(plhs[0]), mxGetDoubles(W));
        if (nlhs > 1) plhs[1] = W; else mxDestroyArray(W);
        if (rc) fail(rc);
        return;
    }
    if (c == "adf") {
        if (nrhs < 8) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const mwSize M = mxGetNumberOfElements(prhs[2]), len = (mwSize)mxGetScalar(prhs[6]);
        const int basis = basis_of(prhs[7]);
        plhs[0] = mxCreateDoubleMatrix(len, 1, mxREAL);
        int rc = emagls_get_magls_array_diffuse_filter(mxGetScalar(prhs[1]), dbl(prhs[2], "micAzi"), dbl(prhs[3], "micZen"), M,
                                                       (int)mxGetScalar(prhs[4]), mxGetScalar(prhs[5]), len, basis,
                                                       nrhs > 8 ? in_ptr(prhs[8]) : nullptr, mxGetDoubles(plhs[0]));
        if (rc) fail(rc);
        return;
    }
    if (nrhs < 6) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
    if (c == "magls_dc" || c == "emagls_dc" || c == "emagls2_dc") {   // the removed applyDiffusenessConst option (include/emagls.h)
        const bool ml = c == "magls_dc", raw = c == "emagls2_dc";
        const int o = ml ? 5 : 8;                    // index of `order`
        if (nrhs < o + 5) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const mwSize ns = mxGetM(prhs[1]), nd = mxGetN(prhs[1]);
        const int order = (int)mxGetScalar(prhs[o]);
        const double fs = mxGetScalar(prhs[o + 1]);
        const mwSize len = (mwSize)mxGetScalar(prhs[o + 2]);
        const int basis = basis_of(prhs[o + 3]);
        const int dc = mxIsLogicalScalarTrue(prhs[o + 4]) || mxGetScalar(prhs[o + 4]) != 0;
        const mwSize nmics = ml ? 0 : mxGetNumberOfElements(prhs[6]);
        const mwSize C = raw ? nmics : (mwSize)((order + 1) * (order + 1));
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        int rc;
        if (ml)
            rc = emagls_get_magls_filters_dc(dbl(prhs[1], "hL"), dbl(prhs[2], "hR"), ns, nd, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), order, fs,
                                             len, dc, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
        else
            rc = (raw ? emagls_get_emagls2_filters_dc : emagls_get_emagls_filters_dc)(
                dbl(prhs[1], "hL"), dbl(prhs[2], "hR"), ns, nd, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), mxGetScalar(prhs[5]),
                dbl(prhs[6], "micAzi"), dbl(prhs[7], "micZen"), nmics, order, fs, len, dc, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
        if (rc) fail(rc);
        return;
    }
    const double* hL = dbl(prhs[1], "hL");
    const double* hR = dbl(prhs[2], "hR");
    const mwSize nsamp = mxGetM(prhs[1]), ndirs = mxGetN(prhs[1]);
    int rc = 0;
    if (c == "ls") {
        const int order = (int)mxGetScalar(prhs[5]);
        const int basis = basis_of(nrhs > 6 ? prhs[6] : nullptr);
        const mwSize C = (order + 1) * (order + 1);
        plhs[0] = out_matrix(nsamp, C, basis);
        plhs[1] = out_matrix(nsamp, C, basis);
        rc = emagls_get_ls_filters(hL, hR, nsamp, ndirs, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), order, basis,
                                   out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "magls") {
        const int order = (int)mxGetScalar(prhs[5]);
        const double fs = mxGetScalar(prhs[6]);
        const mwSize len = (mwSize)mxGetScalar(prhs[7]);
        const int basis = basis_of(nrhs > 8 ? prhs[8] : nullptr);
        const mwSize C = (order + 1) * (order + 1);
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        rc = emagls_get_magls_filters(hL, hR, nsamp, ndirs, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), order, fs, len, basis,
                                      out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "emagls" || c == "emagls2") {
        if (nrhs < 11) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const double r = mxGetScalar(prhs[5]);
        const mwSize nmics = mxGetNumberOfElements(prhs[6]);
        const int order = (int)mxGetScalar(prhs[8]);
        const double fs = mxGetScalar(prhs[9]);
        const mwSize len = (mwSize)mxGetScalar(prhs[10]);
        const int basis = basis_of(nrhs > 11 ? prhs[11] : nullptr);
        const bool raw = c == "emagls2";
        const mwSize C = raw ? nmics : (mwSize)((order + 1) * (order + 1));
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        rc = (raw ? emagls_get_emagls2_filters : emagls_get_emagls_filters)(
            hL, hR, nsamp, ndirs, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), r, dbl(prhs[6], "micAzi"), dbl(prhs[7], "micZen"),
            nmics, order, fs, len, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "magls2d") {   // getMagLsFilters2D(hLHor, hRHor, horHrirGridAziRad, order, fs, len, chDefinition)
        if (nrhs < 7) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const int order = (int)mxGetScalar(prhs[4]);
        const double fs = mxGetScalar(prhs[5]);
        const mwSize len = (mwSize)mxGetScalar(prhs[6]);
        const int basis = basis_of(nrhs > 7 ? prhs[7] : nullptr);
        plhs[0] = out_matrix(len, 2 * order + 1, basis);
        plhs[1] = out_matrix(len, 2 * order + 1, basis);
        rc = emagls_get_magls_filters_2d(hL, hR, nsamp, ndirs, dbl(prhs[3], "azi"), order, fs, len, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "ls_y" || c == "magls_y") {
        const bool ls = c == "ls_y";
        const int order = (int)mxGetScalar(prhs[4]);
        const double fs = ls ? 0.0 : mxGetScalar(prhs[5]);
        const mwSize len = ls ? nsamp : (mwSize)mxGetScalar(prhs[6]);
        const int basis = basis_of(nrhs > (ls ? 5 : 7) ? prhs[ls ? 5 : 7] : nullptr);
        const mwSize C = (order + 1) * (order + 1);
        const void* Y = basis_matrix(prhs[3], basis, ndirs, C, "shFunction(order, hrirGrid)");
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        rc = ls ? emagls_get_ls_filters_with_basis(hL, hR, nsamp, ndirs, Y, order, basis, out_ptr(plhs[0]), out_ptr(plhs[1]))
                : emagls_get_magls_filters_with_basis(hL, hR, nsamp, ndirs, Y, order, fs, len, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "emagls_y" || c == "emagls2_y") {
        if (nrhs < 10) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const bool raw = c == "emagls2_y";
        const double r = mxGetScalar(prhs[4]);
        const mwSize nmics = mxGetM(prhs[5]);
        const int order = (int)mxGetScalar(prhs[6]);
        const double fs = mxGetScalar(prhs[7]);
        const mwSize len = (mwSize)mxGetScalar(prhs[8]);
        const int basis = basis_of(nrhs > 9 ? prhs[9] : nullptr);
        const int so = emagls_simulation_order(raw ? EMAGLS_KIND_EMAGLS2 : EMAGLS_KIND_EMAGLS, order, fs, r);
        const mwSize S = (mwSize)(so + 1) * (so + 1), C = raw ? nmics : (mwSize)((order + 1) * (order + 1));
        const void* Yh = basis_matrix(prhs[3], basis, ndirs, S, "shFunction(simulationOrder, hrirGrid)");
        const void* Ym = basis_matrix(prhs[5], basis, nmics, S, "shFunction(simulationOrder, micGrid)");
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        rc = (raw ? emagls_get_emagls2_filters_with_basis : emagls_get_emagls_filters_with_basis)(
            hL, hR, nsamp, ndirs, Yh, r, Ym, nmics, order, fs, len, basis, out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "emainch" || c == "emainsh") {   // getEMagLsFiltersEMAinCH(hL, hR, azi, zen, micRadius, micGridAziRad, order, fs, len, shDefinition)
        if (nrhs < 10) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const double r = mxGetScalar(prhs[5]);
        const mwSize nmics = mxGetNumberOfElements(prhs[6]);
        const int order = (int)mxGetScalar(prhs[7]);
        const double fs = mxGetScalar(prhs[8]);
        const mwSize len = (mwSize)mxGetScalar(prhs[9]);
        const int basis = basis_of(nrhs > 10 ? prhs[10] : nullptr);
        const bool sh = c == "emainsh";   // getEMagLsFiltersEMAinSH: same arguments, (order+1)^2 spherical-harmonic channels
        const mwSize C = sh ? (mwSize)((order + 1) * (order + 1)) : (mwSize)(2 * order + 1);
        plhs[0] = out_matrix(len, C, basis);
        plhs[1] = out_matrix(len, C, basis);
        rc = (sh ? emagls_get_emagls_filters_ema_in_sh : emagls_get_emagls_filters_ema_in_ch)(
            hL, hR, nsamp, ndirs, dbl(prhs[3], "azi"), dbl(prhs[4], "zen"), r, dbl(prhs[6], "micAzi"), nmics, order, fs, len, basis,
            out_ptr(plhs[0]), out_ptr(plhs[1]));
    } else if (c == "fromatf") {
        if (nrhs < 9) mexErrMsgIdAndTxt("eMagLS:arg", "not enough input arguments");
        const double* hg = dbl(prhs[3], "hrirGridAziZenRad");   // [ndirs x 2], column-major: azi then zen
        const mwSize* ad = mxGetDimensions(prhs[4]);             // [taps x mics x dirs]
        const mwSize taps = ad[0], mics = ad[1], natf = mxGetNumberOfDimensions(prhs[4]) > 2 ? ad[2] : 1;
        const double* ag = dbl(prhs[5], "atfGridAziZenRad");
        const double fs = mxGetScalar(prhs[6]);
        const mwSize len = (mwSize)mxGetScalar(prhs[7]);
        const double ftrans = mxGetScalar(prhs[8]);
        plhs[0] = mxCreateDoubleMatrix(len, mics, mxREAL);
        plhs[1] = mxCreateDoubleMatrix(len, mics, mxREAL);
        double dev = 0.0;
        rc = emagls_get_emagls_filters_from_atf(hL, hR, nsamp, ndirs, hg, hg + ndirs, dbl(prhs[4], "atfIrs"), taps, mics, natf,
                                                ag, ag + natf, fs, len, ftrans, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]), &dev);
        if (!rc) mexPrintf("Matching HRTF and ATF grids, average grid deviation: %g deg\n", dev);  // FromAtf.m:96
    } else {
        mexErrMsgIdAndTxt("eMagLS:arg", "unknown command '%s'", cmd);
    }
    if (rc) fail(rc);
}
