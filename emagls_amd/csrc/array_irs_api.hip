// C ABI of the array impulse responses (include/emagls.h; DESIGN.md sections 11 to 14): emagls_array_irs from listed components,
// emagls_shoebox_components and emagls_array_room_irs from a shoebox room, and their spectral forms (reflection spectra per surface
// and air absorption: emagls_array_irs_spectral, emagls_shoebox_images, emagls_array_room_irs_spectral), and their point-source forms
// (section 14: emagls_array_irs_point, emagls_shoebox_components_dist, emagls_array_room_irs_point), and the directive, oriented sources
// of section 15 (emagls_array_irs_directive, emagls_shoebox_emission, emagls_array_room_irs_directive).  Host arrays in, host array out; every argument is
// checked before the device is touched (a room call's scratch estimate, which needs the component count, after its count pass), and
// every array operation runs in the kernels of array_irs.hip, shoebox.hip, modal.hip and fft.hip (the twiddles), with hipFFT's Z2D
// above 4096 points (the precedent of decode.hip above 2048 taps).  The speed of sound and the simulation order are
// array_model.hpp's; the bin spacing fs / nfft of stage 1 stays its own expression.  No CPU fallback.
//
// Both response entries end in air_run: stages 1 to 4 on components that are already on the device.  emagls_array_irs uploads its
// lists; emagls_array_room_irs enumerates them there and reads back only the nsrc + 1 offsets, for the two source lists of the main
// kernel's forms.
#include <hipfft/hipfft.h>

#include <cmath>
#include <vector>

#include "../../include/emagls.h"
#include "array_model.hpp"

using namespace emagls;

namespace {

constexpr int AIR_SIM_ORDER_MAX = 85;
constexpr int64_t AIR_NFFT_MAX = 65536;
constexpr int AIR_NFFT_LDS_MAX = 4096;     // the LDS transforms of lds_fft.hpp; hipFFT above
constexpr size_t AIR_SCRATCH_MAX = (size_t)24 << 30;
constexpr int AIR_SURFACES_MAX = 8;
constexpr int64_t SBX_CAND_MAX = (int64_t)1 << 28;   // image-source candidates of one call, all sources together

void fft_check(hipfftResult r, const char* what) {
    if (r != HIPFFT_SUCCESS) throw Error(EMAGLS_ERR_HIP, std::string("hipFFT error ") + std::to_string((int)r) + " in " + what);
}

// device events around the kernels of a call, read after the call's synchronisation (emagls_array_irs_kernel_time,
// emagls_shoebox_kernel_time)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() { HIP_CHECK(hipEventCreate(&a)); HIP_CHECK(hipEventCreate(&b)); }
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    EventPair(const EventPair&) = delete;
    EventPair& operator=(const EventPair&) = delete;
    double ms() const {
        float t = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&t, a, b));
        return (double)t;
    }
};
thread_local double g_main_ms = -1.0, g_shoebox_ms = -1.0;

// the checked arguments of a response call that do not concern its components, and the sizes that follow from them
struct AirCall {
    double fs, mic_radius, pre_delay;
    const double *mic_azi, *mic_zen;
    const void* enc;
    bool ec, lds;                           // complex encoder; transforms in LDS
    int N, nfft, P, M, C, np;
    int64_t nsrc, nr, Pld, rows;
    size_t out_bytes;
    void* out;
};

AirCall air_check(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics, const void* enc,
                  int enc_is_complex, int64_t nch, int64_t nsrc, double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    if (!mic_azi || !mic_zen) throw Error(EMAGLS_ERR_ARG, "null pointer: microphone grid");
    if (!out) throw Error(EMAGLS_ERR_ARG, "null pointer: out");
    if (nsrc < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nsrc");
    if (nmics < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nmics");
    if (nmics > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 microphones are not supported");
    if (nch < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nch");
    if (nch > 64) throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 64 channels are not supported");
    if (!enc && nch != nmics) throw Error(EMAGLS_ERR_ARG, "without an encoder nch must equal nmics (raw microphone responses)");
    if (!(fs > 0) || !(mic_radius > 0) || !std::isfinite(fs) || !std::isfinite(mic_radius)) throw Error(EMAGLS_ERR_ARG, "fs and micRadius must be positive");
    if (order < 0) throw Error(EMAGLS_ERR_ARG, "negative SH order");
    if (nr < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nr");
    if (nfft_in < 0) throw Error(EMAGLS_ERR_ARG, "nfft must be positive (0: the smallest power of two from 2*nr)");
    int64_t nfft64 = nfft_in;
    if (nfft64 == 0) {
        nfft64 = 8;
        while (nfft64 < 2 * nr && nfft64 <= AIR_NFFT_MAX) nfft64 *= 2;
    }
    if (nfft64 & (nfft64 - 1)) throw Error(EMAGLS_ERR_ARG, "nfft must be a power of two");
    if (nfft64 < 8) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft below 8 is not supported");
    if (nfft64 > AIR_NFFT_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "nfft above 65536 is not supported");
    if (nr > nfft64) throw Error(EMAGLS_ERR_ARG, "nr exceeds nfft");
    if (!(pre_delay >= 0.0) || !std::isfinite(pre_delay)) throw Error(EMAGLS_ERR_ARG, "pre_delay must be non-negative and finite");
    AirCall c{};
    c.fs = fs; c.mic_radius = mic_radius; c.pre_delay = pre_delay; c.mic_azi = mic_azi; c.mic_zen = mic_zen; c.enc = enc; c.out = out;
    c.nfft = (int)nfft64; c.P = c.nfft / 2 + 1; c.M = (int)nmics; c.C = (int)nch; c.nsrc = nsrc; c.nr = nr;
    if (pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "pre_delay beyond nfft - 1 would wrap");
    c.N = smair_sim_order(order, fs, mic_radius);
    if (c.N > AIR_SIM_ORDER_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "simulation order above 85 is not supported");
    c.ec = enc && enc_is_complex; c.lds = c.nfft <= AIR_NFFT_LDS_MAX;
    c.np = c.ec ? 2 : 1;
    c.Pld = air_bins_padded(c.P); c.rows = nsrc * c.C;
    c.out_bytes = esz(c.ec) * (size_t)c.rows * nr;
    return c;
}

// the spectral gain of a call, checked: nsurf reflection spectra refl [nsurf][P] and the attenuation att [P] or
// null on the host; the exponents exp [ncomp][nsurf] and the paths path [ncomp] (with att) on the device
struct AirSpectral {
    int nsurf = 0;
    const double *refl = nullptr, *att = nullptr;
    const int* d_exp = nullptr;
    const double* d_path = nullptr;
    const double* d_dist = nullptr;       // [ncomp] on the device: point sources
    bool any() const { return nsurf > 0 || att; }
};

// source directivity of a call, checked: the order, the coefficients coef [nsrc][Kd][P] (interleaved complex)
// and the rotations rot [nsrc][9] or null on the host; the emission vectors emit [ncomp][3] on the device
constexpr int AIR_DIR_ORDER_MAX = 8;
struct AirDirective {
    int order = 0;
    const double *coef = nullptr, *rot = nullptr;
    const double* d_emit = nullptr;
    bool any() const { return coef != nullptr; }
    int Kd() const { return (order + 1) * (order + 1); }
};

// the rules of dir_order, dir_coef and src_rot: finite coefficients; proper rotations, max|R^T R - I| <= 1e-12 and det > 0
AirDirective air_check_directive(const AirCall& c, int dir_order, const double* dir_coef, const double* src_rot) {
    if (dir_order < 0) throw Error(EMAGLS_ERR_ARG, "dir_order must be non-negative");
    if (dir_order > AIR_DIR_ORDER_MAX) throw Error(EMAGLS_ERR_UNSUPPORTED, "directivity orders above 8 are not supported");
    AirDirective dv;
    dv.order = dir_order; dv.coef = dir_coef; dv.rot = src_rot;
    const int64_t ncoef = c.nsrc * dv.Kd() * c.P * 2;
    for (int64_t i = 0; i < ncoef; ++i)
        if (!std::isfinite(dir_coef[i])) throw Error(EMAGLS_ERR_ARG, "directivity coefficients must be finite");
    for (int64_t q = 0; src_rot && q < c.nsrc; ++q) {
        const double* R = src_rot + 9 * q;
        double dev = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const double g = R[i] * R[j] + R[3 + i] * R[3 + j] + R[6 + i] * R[6 + j];   // (R^T R)(i, j)
                dev = std::max(dev, std::fabs(g - (i == j ? 1.0 : 0.0)));
            }
        const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
        if (!(dev <= 1e-12) || !(det > 0.0))
            throw Error(EMAGLS_ERR_ARG, "src_rot of source " + std::to_string(q) + " is not a proper rotation (max|R^T R - I| <= 1e-12, det > 0)");
    }
    return dv;
}

// the rules of a point-source call's distances: finite and beyond the sphere; returns the largest
double air_check_dist(const AirCall& c, const double* comp_dist, int64_t ncomp) {
    double far = 0.0;
    for (int64_t j = 0; j < ncomp; ++j) {
        if (!std::isfinite(comp_dist[j]) || !(comp_dist[j] > c.mic_radius))
            throw Error(EMAGLS_ERR_ARG, "component distances must be finite and greater than mic_radius (component " + std::to_string(j) + ")");
        far = std::max(far, comp_dist[j]);
    }
    return far;
}

// the scaled radial recurrence G_n(x) of array_irs.hip grows like x^n / (2n-1)!!: a call whose largest x = kappa_max rho_max brings it
// within reach of FP64's range at n = N is refused
void air_check_point_range(const AirCall& c, double rho_max) {
    const double x = kPi * c.fs / C_SOUND * rho_max;
    double lg = 0.0;                                   // log10 (2N-1)!!
    for (int n = 1; n <= c.N; ++n) lg += std::log10((double)(2 * n - 1));
    if (x > 0.0 && (double)c.N * std::log10(x) - lg >= 300.0)
        throw Error(EMAGLS_ERR_UNSUPPORTED, "a point source this far away at this simulation order leaves the range of FP64 "
                                            "(N log10(kappa_max rho_max) - log10((2N-1)!!) >= 300): treat it as a plane wave");
}

// the rules of the spectra: finite, |R| <= 1, alpha >= 0
void air_check_spectra(int64_t nsurf, const double* refl, const double* att, int P, const char* what) {
    if (nsurf < 0 || nsurf > AIR_SURFACES_MAX) throw Error(EMAGLS_ERR_ARG, "nsurf must lie in 0 .. 8");
    if (nsurf > 0 && !refl) throw Error(EMAGLS_ERR_ARG, std::string("null pointer: ") + what);
    for (int64_t i = 0; i < nsurf * P; ++i)
        if (!(std::fabs(refl[i]) <= 1.0)) throw Error(EMAGLS_ERR_ARG, "reflection spectra must be finite and lie in [-1, 1]");
    for (int k = 0; att && k < P; ++k)
        if (!(att[k] >= 0.0) || !std::isfinite(att[k])) throw Error(EMAGLS_ERR_ARG, "air attenuation must be non-negative and finite");
}

// the device memory estimate of a call with ncomp components, nsurf surfaces and (air) an air term (in long double: the counts of a
// refused call may overflow 64 bits); room: the enumeration's lists are counted too
void air_check_scratch(const AirCall& c, int64_t ncomp, int nsurf = 0, bool air = false, bool point = false, int dir_kd = 0) {
    // (directivity: Yd, the two angles and the emission vectors per component, the padded coefficient table and the rotations per source)
    const long double dir = dir_kd > 0 ? (long double)ncomp * (8 * dir_kd + 40) + (long double)c.nsrc * ((long double)dir_kd * c.Pld * 16 + 72) : 0.0L;
    const long double spectral = nsurf > 0 || air ? (long double)(nsurf + 1) * (c.Pld + c.P) * 8 + (long double)c.Pld * 4 +
                                                        (long double)ncomp * (4 * nsurf + (air ? 8 : 0)) : 0.0L;
    // (point sources: the scaled table in the place of b', the reciprocals and the distances)
    const long double pt = point ? (long double)(c.N + 1) * 8 + (long double)ncomp * 8 : 0.0L;
    const long double need = spectral + pt + dir + (long double)c.nsrc * c.M * c.Pld * 16 + (long double)(c.N + 1) * c.Pld * 16 + (long double)ncomp * 52 +
                             (long double)c.nsrc * 12 + (long double)c.out_bytes +
                             (c.lds ? 0.0L : (c.enc ? (long double)c.rows * c.np * c.P * 16 : 0.0L) + (long double)c.rows * c.np * c.nfft * 8);
    if (need > (long double)AIR_SCRATCH_MAX)
        throw Error(EMAGLS_ERR_UNSUPPORTED, "the call needs more than 24 GiB of device memory; split the sources over several calls");
}

// stages 1 to 4 on components that are on the device: d_ptr [nsrc + 1] and its host copy h_ptr, d_azi, d_zen [ncomp], d_delay and
// d_gain [ncomp] or null (zeros, ones); sp: the spectral gain, or none.  The result is copied to c.out and the stream synchronised.
void air_run(Scratch& s, const AirCall& c, const int64_t* h_ptr, const int64_t* d_ptr, const double* d_azi, const double* d_zen,
             const double* d_delay, const double* d_gain, const AirSpectral& sp = AirSpectral(), const AirDirective& dv = AirDirective()) {
    const int N = c.N, nfft = c.nfft, P = c.P, M = c.M, C = c.C, np = c.np;
    const int64_t nsrc = c.nsrc, nr = c.nr, Pld = c.Pld, rows = c.rows, ncomp = h_ptr[nsrc];
    const double* enc = (const double*)c.enc;
    // the two forms' source lists (array_irs.hip): by each source's own count
    std::vector<int> list_long, list_short;
    for (int64_t q = 0; q < nsrc; ++q) (h_ptr[q + 1] - h_ptr[q] > AIR_LANE_SOURCE_MAX ? list_long : list_short).push_back((int)q);
    std::vector<double> e_re, e_im;
    if (enc) {
        e_re.resize((size_t)C * M);
        if (c.ec) e_im.resize((size_t)C * M);
        for (size_t i = 0; i < (size_t)C * M; ++i) {
            e_re[i] = c.ec ? enc[2 * i] : enc[i];
            if (c.ec) e_im[i] = enc[2 * i + 1];
        }
    }
    // 1. mode coefficients b'_n(k) = -b_n (2n+1) / (4 pi) as rows [N+1][Pld]
    // (point sources: the scaled table of section 14 in their place, from a kernel of its own that needs no b_n)
    const bool point = sp.d_dist != nullptr;
    cplx* bn = s.get<cplx>(sizeof(cplx) * (size_t)(N + 1) * Pld, !point);
    double* rec = s.get<double>(sizeof(double) * 2 * (N + 1));
    double* ginv = point ? s.get<double>(sizeof(double) * (N + 1)) : nullptr;
    const double kappa_step = 2.0 * kPi * (c.fs / (double)nfft) / C_SOUND, kr_step = kappa_step * c.mic_radius;
    if (point) {
        launch_air_modes(N, 0, Pld, nullptr, rec, s.st);                                // (the Legendre coefficients alone)
        launch_air_point_modes(N, P, Pld, kr_step, bn, ginv, s.st);
    } else {
        launch_modal_bn(N, P, nullptr, kr_step, -1.0 / (4.0 * kPi), bn, 1, Pld, s.st);     // bnAll = -sphModalCoeffs(...)  (:107)
        launch_air_modes(N, P, Pld, bn, rec, s.st);
    }
    // 2. components and microphones
    AirMain m{};
    double* v = s.get<double>(sizeof(double) * 3 * M);
    launch_air_units(M, s.put(c.mic_azi, (size_t)M), s.put(c.mic_zen, (size_t)M), v, s.st);
    if (ncomp > 0) {
        double* u = s.get<double>(sizeof(double) * 3 * (size_t)ncomp);
        int* dint = s.get<int>(sizeof(int) * (size_t)ncomp);
        double* dfrac = s.get<double>(sizeof(double) * (size_t)ncomp);
        launch_air_units(ncomp, d_azi, d_zen, u, s.st);
        launch_air_delays(ncomp, d_delay, c.pre_delay, nfft, dint, dfrac, s.st);
        m.u = u; m.dint = dint; m.dfrac = dfrac;
        m.gain = d_gain;
    }
    m.bn = bn; m.rec = rec; m.v = v;
    if (point) { m.dist = sp.d_dist; m.bh = bn; m.ginv = ginv; m.mic_radius = c.mic_radius; m.kappa_step = kappa_step; }
    m.ptr = d_ptr;
    m.list_long = s.put_opt(list_long.data(), list_long.size());
    m.list_short = s.put_opt(list_short.data(), list_short.size());
    m.n_long = (int)list_long.size(); m.n_short = (int)list_short.size();
    m.N = N; m.M = M; m.P = P; m.nfft = nfft; m.Pld = Pld; m.ncomp = ncomp;
    if (sp.any()) {                                    // the per-bin tables of the spectral gain
        double* lnr = s.get<double>(sizeof(double) * (size_t)std::max(sp.nsurf, 1) * Pld);
        unsigned* neg = s.get<unsigned>(sizeof(unsigned) * (size_t)Pld);
        double* att = sp.att ? s.get<double>(sizeof(double) * (size_t)Pld) : nullptr;
        launch_air_spectra(sp.nsurf, P, Pld, s.put_opt(sp.refl, (size_t)sp.nsurf * P), s.put_opt(sp.att, sp.att ? (size_t)P : 0), lnr, neg, att, s.st);
        m.nsurf = sp.nsurf; m.lnr = lnr; m.neg = neg; m.att = att; m.exp = sp.d_exp; m.path = sp.d_path;
    }
    double *dir_tab = nullptr, *dir_ang = nullptr, *dir_Y = nullptr;
    const double* dir_rot = nullptr;
    if (dv.any()) {                                    // source directivity: the padded coefficients, room for the basis at the emission directions
        const int Kd = dv.Kd();
        cplx* dc = s.get<cplx>(sizeof(cplx) * (size_t)nsrc * Kd * Pld, true);
        HIP_CHECK(hipMemcpy2DAsync(dc, sizeof(cplx) * (size_t)Pld, dv.coef, sizeof(cplx) * (size_t)P, sizeof(cplx) * (size_t)P, (size_t)nsrc * Kd,
                                   hipMemcpyHostToDevice, s.st));
        if (ncomp > 0) {
            dir_tab = s.get<double>(sizeof(double) * sh_coeff_count(dv.order));
            dir_ang = s.get<double>(sizeof(double) * 2 * (size_t)ncomp);
            dir_Y = s.get<double>(sizeof(double) * (size_t)Kd * ncomp);
            dir_rot = s.put_opt(dv.rot, (size_t)9 * nsrc);
        }
        m.Yd = dir_Y; m.dc = dc; m.Kd = Kd;
    }
    cplx* H = s.get<cplx>(sizeof(cplx) * (size_t)nsrc * M * Pld);
    m.H = H;
    // 3. the main kernel (and, inside the timed span, the basis pass of a directive call)
    EventPair ev;
    HIP_CHECK(hipEventRecord(ev.a, s.st));
    if (dir_Y) {
        launch_sh_coeff(dv.order, dir_tab, s.st);
        launch_air_emission_angles(ncomp, nsrc, d_ptr, dv.d_emit, dir_rot, dir_ang, dir_ang + ncomp, s.st);
        launch_sh_basis(dv.order, ncomp, dir_ang, dir_ang + ncomp, dir_tab, false, dir_Y, ncomp, s.st);
    }
    launch_air_main(m, s.st);
    HIP_CHECK(hipEventRecord(ev.b, s.st));
    // 4. encoder and inverse real transform
    const double* d_re = s.put_opt(e_re.data(), e_re.size());
    const double* d_im = s.put_opt(e_im.data(), e_im.size());
    void* d_out = s.get(c.out_bytes);
    FftPlan plan;
    if (c.lds) {
        cplx* tw = s.get<cplx>(sizeof(cplx) * (size_t)nfft);
        launch_twiddles(nfft, tw, s.st);
        launch_air_irfft(H, Pld, d_re, d_im, C, M, nsrc, nfft, tw, (int)nr, d_out, s.st);
    } else {
        cplx* X = H;
        int64_t ldx = Pld;
        if (enc) {
            X = s.get<cplx>(sizeof(cplx) * (size_t)rows * np * P);
            ldx = P;
            launch_air_encode(H, Pld, d_re, d_im, C, M, nsrc, P, X, s.st);
        }
        double* y = s.get<double>(sizeof(double) * (size_t)rows * np * nfft);
        int nn[1] = {nfft}, inembed[1] = {P}, onembed[1] = {nfft};
        fft_check(hipfftPlanMany(plan.fresh(), 1, nn, inembed, 1, (int)ldx, onembed, 1, nfft, HIPFFT_Z2D, (int)(rows * np)), "plan Z2D");
        fft_check(hipfftSetStream(plan, s.st), "set stream");
        fft_check(hipfftExecZ2D(plan, (hipfftDoubleComplex*)X, y), "exec Z2D");
        launch_air_pick(y, rows, np, nfft, (int)nr, d_out, s.st);
    }
    HIP_CHECK(hipMemcpyAsync(c.out, d_out, c.out_bytes, hipMemcpyDeviceToHost, s.st));
    s.sync();   // (the host vectors above live until their copies have run)
    g_main_ms = ev.ms();
}

// ---- the shoebox room
// The argument rules of a room; mic_radius 0 for the component lists alone.  Returns the search box and the tiling.
ShoeboxArgs shoebox_check(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc, const double* src_pos,
                          double fs, double mic_radius, double max_delay, int max_order) {
    if (!room_dim || !wall_refl || !array_pos || !src_pos) throw Error(EMAGLS_ERR_ARG, "null pointer: room_dim, wall_refl, array_pos or src_pos");
    // (the spectral entries pass SBX_ONES: the enumeration does not see their walls)
    if (nsrc < 1) throw Error(EMAGLS_ERR_ARG, "invalid shape: nsrc");
    if (!(fs > 0) || !std::isfinite(fs)) throw Error(EMAGLS_ERR_ARG, "fs must be positive");
    if (!(max_delay > 0.0) || !std::isfinite(max_delay)) throw Error(EMAGLS_ERR_ARG, "max_delay must be positive and finite");
    if (max_order < -1) throw Error(EMAGLS_ERR_ARG, "max_order must be -1 (no limit) or non-negative");
    ShoeboxArgs a{};
    for (int i = 0; i < 3; ++i) {
        if (!(room_dim[i] > 0.0) || !std::isfinite(room_dim[i])) throw Error(EMAGLS_ERR_ARG, "room_dim must be positive and finite");
        if (!(array_pos[i] >= mic_radius && array_pos[i] <= room_dim[i] - mic_radius))
            throw Error(EMAGLS_ERR_ARG, "the array's sphere must lie inside the room (mic_radius <= array_pos <= room_dim - mic_radius)");
        a.L[i] = room_dim[i]; a.pos[i] = array_pos[i];
    }
    for (int i = 0; i < 6; ++i) {
        if (!(std::fabs(wall_refl[i]) <= 1.0)) throw Error(EMAGLS_ERR_ARG, "wall reflection coefficients must lie in [-1, 1]");
        a.beta[i] = wall_refl[i];
    }
    for (int64_t q = 0; q < nsrc; ++q) {
        const double* p = src_pos + 3 * q;
        double d2 = 0.0;
        for (int i = 0; i < 3; ++i) {
            if (!(p[i] > 0.0 && p[i] < room_dim[i]))
                throw Error(EMAGLS_ERR_ARG, "source " + std::to_string(q) + " does not lie strictly inside the room");
            d2 += (p[i] - array_pos[i]) * (p[i] - array_pos[i]);
        }
        if (!(std::sqrt(d2) > mic_radius))
            throw Error(EMAGLS_ERR_ARG, "source " + std::to_string(q) + " lies inside the array's sphere (or on its centre)");
    }
    a.fs = fs; a.max_delay = max_delay; a.max_order = max_order;
    // the box: an image with |n_i| beyond floor(reach / (2 L_i)) + 1 is farther than reach; one of reflection order <= max_order
    // has |n_i| <= floor((max_order + 1) / 2)
    const double reach = max_delay * C_SOUND / fs;
    long double ncand = 8.0L * nsrc;
    double B[3];
    for (int i = 0; i < 3; ++i) {
        B[i] = std::floor(reach / (2.0 * room_dim[i])) + 1.0;
        if (max_order >= 0) B[i] = std::min(B[i], (double)(((int64_t)max_order + 1) / 2));
        ncand *= 2.0L * B[i] + 1.0L;
    }
    if (!(ncand <= (long double)SBX_CAND_MAX))
        throw Error(EMAGLS_ERR_UNSUPPORTED, "more than 2^28 image-source candidates in one call: lower max_delay or max_order, or split the sources");
    for (int i = 0; i < 3; ++i) { a.B[i] = (int)B[i]; a.W[i] = 2 * a.B[i] + 1; }
    a.ncand = (int64_t)8 * a.W[0] * a.W[1] * a.W[2];
    a.tiles = ceil_div(a.ncand, SBX_TILE);
    return a;
}

// the enumeration in two steps around the host's look at the count: count() runs the count pass and the scan and returns with
// comp_ptr on the host; fill() allocates the lists and runs the write pass (asynchronous on s.st)
struct Shoebox {
    Scratch& s;
    ShoeboxArgs a;
    int64_t nsrc;
    const double* src = nullptr;
    uint64_t* mask = nullptr;
    int64_t *base = nullptr, *ptr = nullptr;
    double *azi = nullptr, *zen = nullptr, *delay = nullptr, *gain = nullptr, *path = nullptr, *emit = nullptr;   // emit [total][3]: fill(.., .., true)
    int* exp = nullptr;                      // [total][6], with path: fill(true)
    std::vector<int64_t> h_ptr;
    EventPair ev_count, ev_write;
    bool written = false;

    Shoebox(Scratch& s_, const ShoeboxArgs& a_, int64_t nsrc_) : s(s_), a(a_), nsrc(nsrc_), h_ptr((size_t)nsrc_ + 1) {}
    void count(const double* src_pos) {
        const size_t ntiles = (size_t)(nsrc * a.tiles);
        src = s.put(src_pos, (size_t)3 * nsrc);
        mask = s.get<uint64_t>(sizeof(uint64_t) * ntiles * (SBX_TILE / 64));
        int* cnt = s.get<int>(sizeof(int) * ntiles);
        base = s.get<int64_t>(sizeof(int64_t) * (ntiles + 1));
        ptr = s.get<int64_t>(sizeof(int64_t) * ((size_t)nsrc + 1));
        HIP_CHECK(hipEventRecord(ev_count.a, s.st));
        launch_shoebox_count(a, nsrc, src, mask, cnt, s.st);
        launch_shoebox_scan(a, nsrc, cnt, base, ptr, s.st);
        HIP_CHECK(hipEventRecord(ev_count.b, s.st));
        HIP_CHECK(hipMemcpyAsync(h_ptr.data(), ptr, sizeof(int64_t) * h_ptr.size(), hipMemcpyDeviceToHost, s.st));
        s.sync();
    }
    int64_t total() const { return h_ptr.back(); }
    void fill(bool images = false, bool dist = false, bool emission = false) {    // dist: path beside the flat lists (images has it anyway)
        const size_t n = (size_t)total();
        if (emission) emit = s.get<double>(sizeof(double) * 3 * n);
        azi = s.get<double>(sizeof(double) * n); zen = s.get<double>(sizeof(double) * n);
        delay = s.get<double>(sizeof(double) * n); gain = s.get<double>(sizeof(double) * n);
        if (images) exp = s.get<int>(sizeof(int) * 6 * n);
        if (images || dist) path = s.get<double>(sizeof(double) * n);
        HIP_CHECK(hipEventRecord(ev_write.a, s.st));
        if (n && emission) launch_shoebox_write_emit(a, nsrc, src, mask, base, azi, zen, delay, gain, exp, path, emit, s.st);
        else if (n && images) launch_shoebox_write_images(a, nsrc, src, mask, base, azi, zen, delay, gain, exp, path, s.st);
        else if (n && dist) launch_shoebox_write_dist(a, nsrc, src, mask, base, azi, zen, delay, gain, path, s.st);
        else if (n) launch_shoebox_write(a, nsrc, src, mask, base, azi, zen, delay, gain, s.st);
        HIP_CHECK(hipEventRecord(ev_write.b, s.st));
        written = true;
    }
    // after a synchronisation of s.st
    void keep_time() const { g_shoebox_ms = ev_count.ms() + (written ? ev_write.ms() : 0.0); }
};

const double SBX_ONES[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};   // the walls of a spectral room's enumeration: gain = 1 / d, nothing dropped

// the component lists of emagls_array_irs and emagls_array_irs_spectral, checked; returns ncomp
int64_t air_check_lists(const AirCall& c, const int64_t* comp_ptr, const double* comp_azi, const double* comp_zen, const double* comp_delay,
                        const double* comp_gain) {
    if (comp_ptr[0] != 0) throw Error(EMAGLS_ERR_ARG, "comp_ptr must start at 0");
    for (int64_t q = 0; q < c.nsrc; ++q)
        if (comp_ptr[q + 1] < comp_ptr[q]) throw Error(EMAGLS_ERR_ARG, "comp_ptr must not decrease");
    const int64_t ncomp = comp_ptr[c.nsrc];
    if (ncomp > 0 && (!comp_azi || !comp_zen)) throw Error(EMAGLS_ERR_ARG, "null pointer: component directions");
    for (int64_t j = 0; comp_delay && j < ncomp; ++j) {
        if (!(comp_delay[j] >= 0.0) || !std::isfinite(comp_delay[j])) throw Error(EMAGLS_ERR_ARG, "component delays must be non-negative and finite");
        if (comp_delay[j] + c.pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "a component's delay plus pre_delay beyond nfft - 1 would wrap");
    }
    for (int64_t j = 0; comp_gain && j < ncomp; ++j)
        if (!std::isfinite(comp_gain[j])) throw Error(EMAGLS_ERR_ARG, "component gains must be finite");
    return ncomp;
}

// the spectral gain's arguments of a listed call, checked
void air_check_gain_lists(const AirCall& c, int64_t ncomp, int64_t nsurf, const double* surf_refl, const int32_t* comp_exp, const double* air_atten,
                          const double* comp_path) {
    if ((air_atten == nullptr) != (comp_path == nullptr)) throw Error(EMAGLS_ERR_ARG, "air_atten and comp_path must both be given or both be NULL");
    air_check_spectra(nsurf, surf_refl, air_atten, c.P, "surf_refl");
    if (nsurf > 0 && ncomp > 0 && !comp_exp) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_exp");
    for (int64_t i = 0; i < ncomp * nsurf; ++i)
        if (comp_exp[i] < 0) throw Error(EMAGLS_ERR_ARG, "component exponents must be non-negative");
    for (int64_t j = 0; comp_path && j < ncomp; ++j)
        if (!(comp_path[j] >= 0.0) || !std::isfinite(comp_path[j])) throw Error(EMAGLS_ERR_ARG, "component path lengths must be non-negative and finite");
}

}  // namespace

extern "C" int emagls_array_irs(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr,
                                const double* comp_azi, const double* comp_zen, const double* comp_delay, const double* comp_gain,
                                double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    return guarded_call([&] {
        // ---- arguments (nothing below this block fails on what the caller passed)
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        const int64_t ncomp = air_check_lists(c, comp_ptr, comp_azi, comp_zen, comp_delay, comp_gain);
        air_check_scratch(c, ncomp);
        // ---- device
        Scratch s;
        const size_t n = (size_t)ncomp;
        const int64_t* d_ptr = s.put(comp_ptr, (size_t)nsrc + 1);
        air_run(s, c, comp_ptr, d_ptr, s.put_opt(comp_azi, n), s.put_opt(comp_zen, n), s.put_opt(comp_delay, n), s.put_opt(comp_gain, n));
    });
}

extern "C" int emagls_array_irs_spectral(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                         const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr,
                                         const double* comp_azi, const double* comp_zen, const double* comp_delay, const double* comp_gain,
                                         int64_t nsurf, const double* surf_refl, const int32_t* comp_exp, const double* air_atten,
                                         const double* comp_path, double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    return guarded_call([&] {
        // ---- arguments (nothing below this block fails on what the caller passed)
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (nfft_in == 0) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the spectra have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        const int64_t ncomp = air_check_lists(c, comp_ptr, comp_azi, comp_zen, comp_delay, comp_gain);
        air_check_gain_lists(c, ncomp, nsurf, surf_refl, comp_exp, air_atten, comp_path);
        air_check_scratch(c, ncomp, (int)nsurf, air_atten != nullptr);
        // ---- device (nsurf = 0 and no air: the flat kernels, the bits of emagls_array_irs)
        Scratch s;
        const size_t n = (size_t)ncomp;
        AirSpectral sp;
        sp.nsurf = (int)nsurf; sp.refl = surf_refl; sp.att = air_atten;
        sp.d_exp = nsurf > 0 ? s.put_opt(comp_exp, n * (size_t)nsurf) : nullptr;
        sp.d_path = air_atten ? s.put_opt(comp_path, n) : nullptr;
        const int64_t* d_ptr = s.put(comp_ptr, (size_t)nsrc + 1);
        air_run(s, c, comp_ptr, d_ptr, s.put_opt(comp_azi, n), s.put_opt(comp_zen, n), s.put_opt(comp_delay, n), s.put_opt(comp_gain, n), sp);
    });
}

extern "C" int emagls_array_irs_point(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                      const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr,
                                      const double* comp_azi, const double* comp_zen, const double* comp_delay, const double* comp_gain,
                                      int64_t nsurf, const double* surf_refl, const int32_t* comp_exp, const double* air_atten,
                                      const double* comp_path, const double* comp_dist, double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    return guarded_call([&] {
        // ---- arguments (nothing below this block fails on what the caller passed)
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (nfft_in == 0 && (nsurf > 0 || air_atten)) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the spectra have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        const int64_t ncomp = air_check_lists(c, comp_ptr, comp_azi, comp_zen, comp_delay, comp_gain);
        if (ncomp > 0 && !comp_dist) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_dist (distances are given for all components or, in emagls_array_irs, for none)");
        air_check_point_range(c, air_check_dist(c, comp_dist, ncomp));
        air_check_gain_lists(c, ncomp, nsurf, surf_refl, comp_exp, air_atten, comp_path);
        air_check_scratch(c, ncomp, (int)nsurf, air_atten != nullptr, true);
        // ---- device
        Scratch s;
        const size_t n = (size_t)ncomp;
        AirSpectral sp;
        sp.nsurf = (int)nsurf; sp.refl = surf_refl; sp.att = air_atten;
        sp.d_exp = nsurf > 0 ? s.put_opt(comp_exp, n * (size_t)nsurf) : nullptr;
        sp.d_path = air_atten ? s.put_opt(comp_path, n) : nullptr;
        sp.d_dist = s.put(comp_dist ? comp_dist : &c.mic_radius, std::max<size_t>(n, comp_dist ? 0 : 1));   // (never null: it selects the kernel)
        const int64_t* d_ptr = s.put(comp_ptr, (size_t)nsrc + 1);
        air_run(s, c, comp_ptr, d_ptr, s.put_opt(comp_azi, n), s.put_opt(comp_zen, n), s.put_opt(comp_delay, n), s.put_opt(comp_gain, n), sp);
    });
}

extern "C" int emagls_array_irs_kernel_time(double* ms) {
    return guarded_call([&] {
        if (!ms) throw Error(EMAGLS_ERR_ARG, "null pointer: ms");
        if (g_main_ms < 0.0) throw Error(EMAGLS_ERR_ARG, "no emagls_array_irs call has completed on this thread");
        *ms = g_main_ms;
    });
}

// emagls_shoebox_components, and with want_dist its sibling with the distances beside the lists
static int shoebox_components(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc, const double* src_pos,
                              double fs, double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_azi,
                              double* comp_zen, double* comp_delay, double* comp_gain, bool want_dist, double* comp_dist) {
    return guarded_call([&] {
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (capacity < 0) throw Error(EMAGLS_ERR_ARG, "invalid shape: capacity");
        if (capacity > 0 && (!comp_azi || !comp_zen || !comp_delay || !comp_gain || (want_dist && !comp_dist)))
            throw Error(EMAGLS_ERR_ARG, "null pointer: component arrays (capacity 0 for a count-only call)");
        const ShoeboxArgs a = shoebox_check(room_dim, wall_refl, array_pos, nsrc, src_pos, fs, 0.0, max_delay, max_order);
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        std::copy(box.h_ptr.begin(), box.h_ptr.end(), comp_ptr);
        const size_t n = (size_t)box.total();
        if (n > 0 && box.total() <= capacity) {
            box.fill(false, want_dist);
            HIP_CHECK(hipMemcpyAsync(comp_azi, box.azi, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_zen, box.zen, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_delay, box.delay, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_gain, box.gain, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            if (want_dist) HIP_CHECK(hipMemcpyAsync(comp_dist, box.path, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            s.sync();
        }
        box.keep_time();
    });
}

extern "C" int emagls_shoebox_components(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc,
                                         const double* src_pos, double fs, double max_delay, int max_order, int64_t capacity,
                                         int64_t* comp_ptr, double* comp_azi, double* comp_zen, double* comp_delay, double* comp_gain) {
    return shoebox_components(room_dim, wall_refl, array_pos, nsrc, src_pos, fs, max_delay, max_order, capacity, comp_ptr, comp_azi, comp_zen,
                              comp_delay, comp_gain, false, nullptr);
}

extern "C" int emagls_shoebox_components_dist(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc,
                                              const double* src_pos, double fs, double max_delay, int max_order, int64_t capacity,
                                              int64_t* comp_ptr, double* comp_azi, double* comp_zen, double* comp_delay, double* comp_gain,
                                              double* comp_dist) {
    return shoebox_components(room_dim, wall_refl, array_pos, nsrc, src_pos, fs, max_delay, max_order, capacity, comp_ptr, comp_azi, comp_zen,
                              comp_delay, comp_gain, true, comp_dist);
}

extern "C" int emagls_shoebox_images(const double* room_dim, const double* array_pos, int64_t nsrc, const double* src_pos, double fs,
                                     double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_azi, double* comp_zen,
                                     double* comp_delay, double* comp_gain, int32_t* comp_exp, double* comp_path) {
    return guarded_call([&] {
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (capacity < 0) throw Error(EMAGLS_ERR_ARG, "invalid shape: capacity");
        if (capacity > 0 && (!comp_azi || !comp_zen || !comp_delay || !comp_gain || !comp_exp || !comp_path))
            throw Error(EMAGLS_ERR_ARG, "null pointer: component arrays (capacity 0 for a count-only call)");
        const ShoeboxArgs a = shoebox_check(room_dim, SBX_ONES, array_pos, nsrc, src_pos, fs, 0.0, max_delay, max_order);
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        std::copy(box.h_ptr.begin(), box.h_ptr.end(), comp_ptr);
        const size_t n = (size_t)box.total();
        if (n > 0 && box.total() <= capacity) {
            box.fill(true);
            HIP_CHECK(hipMemcpyAsync(comp_azi, box.azi, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_zen, box.zen, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_delay, box.delay, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_gain, box.gain, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_exp, box.exp, sizeof(int) * 6 * n, hipMemcpyDeviceToHost, s.st));
            HIP_CHECK(hipMemcpyAsync(comp_path, box.path, sizeof(double) * n, hipMemcpyDeviceToHost, s.st));
            s.sync();
        }
        box.keep_time();
    });
}

extern "C" int emagls_array_room_irs_spectral(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                              const void* enc, int enc_is_complex, int64_t nch, const double* room_dim,
                                              const double* wall_refl_spec, const double* air_atten, const double* array_pos, int64_t nsrc,
                                              const double* src_pos, double max_delay, int max_order, double pre_delay, int64_t nfft_in,
                                              int64_t nr, int64_t* comp_count, void* out) {
    return guarded_call([&] {
        if (nfft_in == 0) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the spectra have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        if (!wall_refl_spec) throw Error(EMAGLS_ERR_ARG, "null pointer: wall_refl_spec");
        const ShoeboxArgs a = shoebox_check(room_dim, SBX_ONES, array_pos, nsrc, src_pos, fs, mic_radius, max_delay, max_order);
        air_check_spectra(6, wall_refl_spec, air_atten, c.P, "wall_refl_spec");
        if (max_delay + pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "max_delay plus pre_delay beyond nfft - 1 would wrap");
        air_check_scratch(c, 0, 6, air_atten != nullptr);
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        air_check_scratch(c, box.total(), 6, air_atten != nullptr);
        box.fill(true);
        AirSpectral sp;
        sp.nsurf = 6; sp.refl = wall_refl_spec; sp.att = air_atten; sp.d_exp = box.exp; sp.d_path = air_atten ? box.path : nullptr;
        air_run(s, c, box.h_ptr.data(), box.ptr, box.azi, box.zen, box.delay, box.gain, sp);
        box.keep_time();
        for (int64_t q = 0; comp_count && q < nsrc; ++q) comp_count[q] = box.h_ptr[q + 1] - box.h_ptr[q];
    });
}

extern "C" int emagls_array_room_irs(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                     const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                                     const double* array_pos, int64_t nsrc, const double* src_pos, double max_delay, int max_order,
                                     double pre_delay, int64_t nfft_in, int64_t nr, int64_t* comp_count, void* out) {
    return guarded_call([&] {
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        const ShoeboxArgs a = shoebox_check(room_dim, wall_refl, array_pos, nsrc, src_pos, fs, mic_radius, max_delay, max_order);
        if (max_delay + pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "max_delay plus pre_delay beyond nfft - 1 would wrap");
        air_check_scratch(c, 0);     // (what does not depend on the count; the whole estimate follows the count pass)
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        air_check_scratch(c, box.total());
        box.fill();
        air_run(s, c, box.h_ptr.data(), box.ptr, box.azi, box.zen, box.delay, box.gain);
        box.keep_time();
        for (int64_t q = 0; comp_count && q < nsrc; ++q) comp_count[q] = box.h_ptr[q + 1] - box.h_ptr[q];
    });
}

extern "C" int emagls_array_room_irs_point(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                           const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                                           int wall_is_spectral, const double* air_atten, const double* array_pos, int64_t nsrc,
                                           const double* src_pos, double max_delay, int max_order, double pre_delay, int64_t nfft_in,
                                           int64_t nr, int64_t* comp_count, void* out) {
    return guarded_call([&] {
        const bool spectral = wall_is_spectral != 0 || air_atten != nullptr;
        if (nfft_in == 0 && spectral) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the spectra have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        if (!wall_refl) throw Error(EMAGLS_ERR_ARG, "null pointer: wall_refl");
        const ShoeboxArgs a = shoebox_check(room_dim, spectral ? SBX_ONES : wall_refl, array_pos, nsrc, src_pos, fs, mic_radius, max_delay, max_order);
        std::vector<double> rep;                       // six coefficients with air: repeated over the bins
        const double* walls = wall_refl;
        if (spectral && !wall_is_spectral) {
            rep.resize((size_t)6 * c.P);
            for (int w = 0; w < 6; ++w) std::fill(rep.begin() + (size_t)w * c.P, rep.begin() + (size_t)(w + 1) * c.P, wall_refl[w]);
            walls = rep.data();
        }
        if (spectral) air_check_spectra(6, walls, air_atten, c.P, "wall_refl");
        if (max_delay + pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "max_delay plus pre_delay beyond nfft - 1 would wrap");
        air_check_point_range(c, max_delay * C_SOUND / fs);      // (no kept image is farther than the reach of max_delay)
        const int nsurf = spectral ? 6 : 0;
        air_check_scratch(c, 0, nsurf, air_atten != nullptr, true);
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        air_check_scratch(c, box.total(), nsurf, air_atten != nullptr, true);
        box.fill(spectral, true);
        AirSpectral sp;
        if (spectral) { sp.nsurf = 6; sp.refl = walls; sp.att = air_atten; sp.d_exp = box.exp; sp.d_path = air_atten ? box.path : nullptr; }
        sp.d_dist = box.path;                          // (shoebox_check: every image lies beyond the sphere)
        air_run(s, c, box.h_ptr.data(), box.ptr, box.azi, box.zen, box.delay, box.gain, sp);
        box.keep_time();
        for (int64_t q = 0; comp_count && q < nsrc; ++q) comp_count[q] = box.h_ptr[q + 1] - box.h_ptr[q];
    });
}

// ---- source directivity
extern "C" int emagls_array_irs_directive(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                          const void* enc, int enc_is_complex, int64_t nch, int64_t nsrc, const int64_t* comp_ptr,
                                          const double* comp_azi, const double* comp_zen, const double* comp_delay, const double* comp_gain,
                                          int64_t nsurf, const double* surf_refl, const int32_t* comp_exp, const double* air_atten,
                                          const double* comp_path, const double* comp_dist, const double* comp_emit, const double* src_rot,
                                          int dir_order, const double* dir_coef, double pre_delay, int64_t nfft_in, int64_t nr, void* out) {
    if (!dir_coef) {                                   // no directivity: the existing entries and their bits
        if (comp_emit || src_rot || dir_order != 0)
            return guarded_call([] { throw Error(EMAGLS_ERR_ARG, "without dir_coef, comp_emit and src_rot must be NULL and dir_order 0"); });
        if (comp_dist)
            return emagls_array_irs_point(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, comp_ptr, comp_azi, comp_zen,
                                          comp_delay, comp_gain, nsurf, surf_refl, comp_exp, air_atten, comp_path, comp_dist, pre_delay, nfft_in, nr, out);
        if (nsurf != 0 || surf_refl || comp_exp || air_atten || comp_path)
            return emagls_array_irs_spectral(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, comp_ptr, comp_azi,
                                             comp_zen, comp_delay, comp_gain, nsurf, surf_refl, comp_exp, air_atten, comp_path, pre_delay, nfft_in, nr, out);
        return emagls_array_irs(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, comp_ptr, comp_azi, comp_zen, comp_delay,
                                comp_gain, pre_delay, nfft_in, nr, out);
    }
    return guarded_call([&] {
        // ---- arguments (nothing below this block fails on what the caller passed)
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (nfft_in == 0) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the directivity coefficients have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        const int64_t ncomp = air_check_lists(c, comp_ptr, comp_azi, comp_zen, comp_delay, comp_gain);
        const AirDirective dv = air_check_directive(c, dir_order, dir_coef, src_rot);
        if (ncomp > 0 && !comp_emit) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_emit (dir_coef needs the emission vector of every component)");
        for (int64_t j = 0; j < ncomp; ++j) {
            const double* e = comp_emit + 3 * j;
            if (!(std::fabs((e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) - 1.0) <= 1e-12))
                throw Error(EMAGLS_ERR_ARG, "emission vectors must have unit length (component " + std::to_string(j) + ")");
        }
        if (comp_dist) air_check_point_range(c, air_check_dist(c, comp_dist, ncomp));
        air_check_gain_lists(c, ncomp, nsurf, surf_refl, comp_exp, air_atten, comp_path);
        air_check_scratch(c, ncomp, (int)nsurf, air_atten != nullptr, comp_dist != nullptr, dv.Kd());
        // ---- device
        Scratch s;
        const size_t n = (size_t)ncomp;
        AirSpectral sp;
        sp.nsurf = (int)nsurf; sp.refl = surf_refl; sp.att = air_atten;
        sp.d_exp = nsurf > 0 ? s.put_opt(comp_exp, n * (size_t)nsurf) : nullptr;
        sp.d_path = air_atten ? s.put_opt(comp_path, n) : nullptr;
        if (comp_dist) sp.d_dist = s.put(n ? comp_dist : &c.mic_radius, std::max<size_t>(n, 1));   // (never null: it selects the kernel)
        AirDirective d = dv;
        d.d_emit = s.put_opt(comp_emit, 3 * n);
        const int64_t* d_ptr = s.put(comp_ptr, (size_t)nsrc + 1);
        air_run(s, c, comp_ptr, d_ptr, s.put_opt(comp_azi, n), s.put_opt(comp_zen, n), s.put_opt(comp_delay, n), s.put_opt(comp_gain, n), sp, d);
    });
}

extern "C" int emagls_shoebox_emission(const double* room_dim, const double* wall_refl, const double* array_pos, int64_t nsrc, const double* src_pos,
                                       double fs, double max_delay, int max_order, int64_t capacity, int64_t* comp_ptr, double* comp_emit) {
    return guarded_call([&] {
        if (!comp_ptr) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_ptr");
        if (capacity < 0) throw Error(EMAGLS_ERR_ARG, "invalid shape: capacity");
        if (capacity > 0 && !comp_emit) throw Error(EMAGLS_ERR_ARG, "null pointer: comp_emit (capacity 0 for a count-only call)");
        // (wall_refl null: the images of emagls_shoebox_images, nothing dropped; else the keep rule of emagls_shoebox_components)
        const ShoeboxArgs a = shoebox_check(room_dim, wall_refl ? wall_refl : SBX_ONES, array_pos, nsrc, src_pos, fs, 0.0, max_delay, max_order);
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        std::copy(box.h_ptr.begin(), box.h_ptr.end(), comp_ptr);
        const size_t n = (size_t)box.total();
        if (n > 0 && box.total() <= capacity) {
            box.fill(false, false, true);
            HIP_CHECK(hipMemcpyAsync(comp_emit, box.emit, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s.st));
            s.sync();
        }
        box.keep_time();
    });
}

extern "C" int emagls_array_room_irs_directive(double fs, double mic_radius, int order, const double* mic_azi, const double* mic_zen, int64_t nmics,
                                               const void* enc, int enc_is_complex, int64_t nch, const double* room_dim, const double* wall_refl,
                                               int wall_is_spectral, const double* air_atten, const double* array_pos, int64_t nsrc,
                                               const double* src_pos, double max_delay, int max_order, int point_source, const double* src_rot,
                                               int dir_order, const double* dir_coef, double pre_delay, int64_t nfft_in, int64_t nr,
                                               int64_t* comp_count, void* out) {
    if (point_source != 0 && point_source != 1) return guarded_call([] { throw Error(EMAGLS_ERR_ARG, "point_source must be 0 or 1"); });
    if (!dir_coef) {                                   // no directivity: the existing entries and their bits
        if (src_rot || dir_order != 0) return guarded_call([] { throw Error(EMAGLS_ERR_ARG, "without dir_coef, src_rot must be NULL and dir_order 0"); });
        if (point_source)
            return emagls_array_room_irs_point(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, room_dim, wall_refl,
                                               wall_is_spectral, air_atten, array_pos, nsrc, src_pos, max_delay, max_order, pre_delay, nfft_in, nr,
                                               comp_count, out);
        if (wall_is_spectral)
            return emagls_array_room_irs_spectral(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, room_dim, wall_refl, air_atten,
                                                  array_pos, nsrc, src_pos, max_delay, max_order, pre_delay, nfft_in, nr, comp_count, out);
        if (air_atten) return guarded_call([] { throw Error(EMAGLS_ERR_ARG, "air_atten without dir_coef needs wall spectra (wall_is_spectral) or point_source"); });
        return emagls_array_room_irs(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, room_dim, wall_refl, array_pos, nsrc,
                                     src_pos, max_delay, max_order, pre_delay, nfft_in, nr, comp_count, out);
    }
    return guarded_call([&] {
        const bool spectral = wall_is_spectral != 0 || air_atten != nullptr, point = point_source != 0;
        if (nfft_in == 0) throw Error(EMAGLS_ERR_ARG, "nfft must be given: the directivity coefficients have nfft / 2 + 1 bins");
        const AirCall c = air_check(fs, mic_radius, order, mic_azi, mic_zen, nmics, enc, enc_is_complex, nch, nsrc, pre_delay, nfft_in, nr, out);
        if (!wall_refl) throw Error(EMAGLS_ERR_ARG, "null pointer: wall_refl");
        const ShoeboxArgs a = shoebox_check(room_dim, spectral ? SBX_ONES : wall_refl, array_pos, nsrc, src_pos, fs, mic_radius, max_delay, max_order);
        const AirDirective dv = air_check_directive(c, dir_order, dir_coef, src_rot);
        std::vector<double> rep;                       // six coefficients with air: repeated over the bins
        const double* walls = wall_refl;
        if (spectral && !wall_is_spectral) {
            rep.resize((size_t)6 * c.P);
            for (int w = 0; w < 6; ++w) std::fill(rep.begin() + (size_t)w * c.P, rep.begin() + (size_t)(w + 1) * c.P, wall_refl[w]);
            walls = rep.data();
        }
        if (spectral) air_check_spectra(6, walls, air_atten, c.P, "wall_refl");
        if (max_delay + pre_delay > (double)(c.nfft - 1)) throw Error(EMAGLS_ERR_ARG, "max_delay plus pre_delay beyond nfft - 1 would wrap");
        if (point) air_check_point_range(c, max_delay * C_SOUND / fs);
        const int nsurf = spectral ? 6 : 0;
        air_check_scratch(c, 0, nsurf, air_atten != nullptr, point, dv.Kd());
        Scratch s;
        Shoebox box(s, a, nsrc);
        box.count(src_pos);
        air_check_scratch(c, box.total(), nsurf, air_atten != nullptr, point, dv.Kd());
        box.fill(spectral, point, true);
        AirSpectral sp;
        if (spectral) { sp.nsurf = 6; sp.refl = walls; sp.att = air_atten; sp.d_exp = box.exp; sp.d_path = air_atten ? box.path : nullptr; }
        if (point) sp.d_dist = box.path;
        AirDirective d = dv;
        d.d_emit = box.emit;
        air_run(s, c, box.h_ptr.data(), box.ptr, box.azi, box.zen, box.delay, box.gain, sp, d);
        box.keep_time();
        for (int64_t q = 0; comp_count && q < nsrc; ++q) comp_count[q] = box.h_ptr[q + 1] - box.h_ptr[q];
    });
}

extern "C" int emagls_shoebox_kernel_time(double* ms) {
    return guarded_call([&] {
        if (!ms) throw Error(EMAGLS_ERR_ARG, "null pointer: ms");
        if (g_shoebox_ms < 0.0) throw Error(EMAGLS_ERR_ARG, "no emagls_shoebox_components, emagls_shoebox_images or emagls_array_room_irs call has completed on this thread");
        *ms = g_shoebox_ms;
    });
}
