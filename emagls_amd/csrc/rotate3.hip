// Three-axis rotation of SH signals (rotateHOA_N3D(in, yaw, pitch, roll), called by dependencies/binauralDecode.m:27-31).  OWN
// SPECIFICATION: axes of getSH (x front, y left, z up); R = Rz(yaw) Ry(pitch) Rx(roll), right-handed
// active rotations about fixed axes; the signal of a plane wave from u, conj(getSH(N, u, basis)), becomes the one from R u.
//
// Per order n the operator is M_n = Z(a) J_n Z(b) J_n^T Z(g) in the real basis, with R = Rz(a) Ry(b) Rz(g) (zyz Euler angles)
// and Ry(b) = Xm Rz(b) Xm^T, Xm = Rx(-pi/2):
//   - Z(t) is the yaw rule of rotate.hip (only (n, m) and (n, -m) mix, through cos(m t), sin(m t));
//   - J_n = M_n(Xm) is constant.  It is built once per device in FP64 by the Ivanic-Ruedenberg recursion from the exact 3 x 3
//     matrix of Xm (entries 0 and +-1), so its zeros are exact: column m has nonzeros only in one of the four classes
//     {even m >= 0, odd m > 0, even m < 0, odd m < 0} of rows, a quarter of the entries (J_PACK below stores only those).
// The complex basis goes through the real one: Y_c = U Y_r per order, so M_c = conj(U) M_r U^T (to_real / from_real).
// The transposed form (w M instead of x M^T, for decoding filters): M^T = Z(-g) J Z(-b) J^T Z(-a) in the real basis and
// U M_r^T U^H in the complex one, i.e. the same code with (a, b, g) -> (-g, -b, -a) and the conversions conjugated.
#include "kernels.hpp"
#include "encode_tile.hpp"

namespace emagls {

namespace {

constexpr int R3_NMAX = 15;

// packed J: order l at [jpk_off(l), jpk_off(l + 1)), l^2 + l + 1 values: column m = 0, then per k the columns +m, -m of
// m = 2k + 1 and +m, -m of m = 2k + 2 (when m <= l), 2l + 1 values per k; each column holds its nonzero rows in the order of
// cls_row() below
__host__ __device__ constexpr int jpk_off(int l) { return l * (l * l + 2) / 3; }

// classes of an index m: 0 even m >= 0, 1 odd m > 0, 2 even m < 0, 3 odd m < 0
__host__ __device__ constexpr int cls_of(int m) { return (m >= 0 ? 0 : 2) + ((m < 0 ? -m : m) & 1); }
__host__ __device__ constexpr int cls_first(int c) { return c == 0 ? 0 : c == 1 ? 1 : c == 2 ? -2 : -1; }
__host__ __device__ constexpr int cls_step(int c) { return c < 2 ? 2 : -2; }
__host__ __device__ constexpr int cls_size(int l, int c) { return c == 0 ? l / 2 + 1 : c == 2 ? l / 2 : (l + 1) / 2; }
// the class of the rows a column of class c has nonzeros in (order l); found from the recursion, checked in tests
__host__ __device__ constexpr int cls_row(int l, int c) {
    return (l & 1) ? (c == 0 ? 3 : c == 3 ? 0 : c) : (c == 1 ? 2 : c == 2 ? 1 : c);
}
// offset of column m within order l's pack
__host__ __device__ constexpr int col_off(int l, int m) {
    if (m == 0) return 0;
    const int am = m < 0 ? -m : m, base = l / 2 + 1 + ((am - 1) / 2) * (2 * l + 1);
    if (am & 1) return base + (m > 0 ? 0 : cls_size(l, cls_row(l, 1)));
    const int b2 = base + cls_size(l, cls_row(l, 1)) + cls_size(l, cls_row(l, 3));
    return b2 + (m > 0 ? 0 : cls_size(l, cls_row(l, 0)));
}

// ---- J_n by the Ivanic-Ruedenberg recursion (real SH; M_l(R) with Y_l(R u) = M_l(R) Y_l(u)), one block, FP64
__global__ void __launch_bounds__(1024) build_j_kernel(double* __restrict__ jpk) {
    __shared__ double A[31 * 31], B[31 * 31];
    // order 1 in the row / column order (y, z, x) of m = -1, 0, 1: Xm maps x -> x, y -> -z, z -> y
    // (rows y, z, x) = (x -> x, y -> -z, z -> y): R1(-1, 0) = 1, R1(0, -1) = -1, R1(1, 1) = 1
    auto R1 = [](int i, int j) { return (i == -1 && j == 0) ? 1.0 : (i == 0 && j == -1) ? -1.0 : (i == 1 && j == 1) ? 1.0 : 0.0; };
    const int tid = threadIdx.x;
    if (tid == 0) jpk[0] = 1.0;
    if (tid < 9) {
        const int i = tid / 3 - 1, j = tid % 3 - 1;
        A[tid] = R1(i, j);
        if (R1(i, j) != 0.0) {
            const int c = cls_row(1, cls_of(j));
            jpk[jpk_off(1) + col_off(1, j) + (i - cls_first(c)) / cls_step(c)] = R1(i, j);
        }
    }
    __syncthreads();
    double* prev = A;
    double* cur = B;
    for (int l = 2; l <= R3_NMAX; ++l) {
        const int w = 2 * l + 1, wp = 2 * l - 1;
        auto Rp = [&](int a, int b) { return prev[(a + l - 1) * wp + (b + l - 1)]; };
        auto P = [&](int i, int a, int b) {
            if (b == l) return R1(i, 1) * Rp(a, l - 1) - R1(i, -1) * Rp(a, -l + 1);
            if (b == -l) return R1(i, 1) * Rp(a, -l + 1) + R1(i, -1) * Rp(a, l - 1);
            return R1(i, 0) * Rp(a, b);
        };
        if (tid < w * w) {
            const int m = tid / w - l, n = tid % w - l, am = m < 0 ? -m : m;
            const double d = m == 0 ? 1.0 : 0.0;
            const double den = (n == l || n == -l) ? (double)(2 * l) * (2 * l - 1) : (double)(l + n) * (l - n);
            const double u = sqrt((double)(l + m) * (l - m) / den);
            const double v = 0.5 * sqrt((1.0 + d) * (l + am - 1) * (l + am) / den) * (1.0 - 2.0 * d);
            const double ww = -0.5 * sqrt((double)(l - am - 1) * (l - am) / den) * (1.0 - d);
            double val = 0.0;
            if (u != 0.0) val += u * P(0, m, n);
            if (v != 0.0) {
                double V;
                if (m == 0) V = P(1, 1, n) + P(-1, -1, n);
                else if (m > 0) V = P(1, m - 1, n) * (m == 1 ? sqrt(2.0) : 1.0) - (m != 1 ? P(-1, -m + 1, n) : 0.0);
                else V = (m != -1 ? P(1, m + 1, n) : 0.0) + P(-1, -m - 1, n) * (m == -1 ? sqrt(2.0) : 1.0);
                val += v * V;
            }
            if (ww != 0.0) val += ww * (m > 0 ? P(1, m + 1, n) + P(-1, -m - 1, n) : P(1, m - 1, n) - P(-1, -m + 1, n));
            cur[tid] = val;
            const int c = cls_row(l, cls_of(n));
            if (cls_of(m) == c) jpk[jpk_off(l) + col_off(l, n) + (m - cls_first(c)) / cls_step(c)] = val;
        }
        __syncthreads();
        double* t = prev; prev = cur; cur = t;
    }
}

// ---- the per-sample operator
__device__ __forceinline__ double fmav(double a, double x, double acc) { return fma(a, x, acc); }
__device__ __forceinline__ cplx fmav(double a, cplx x, cplx acc) { return mk(fma(a, x.x, acc.x), fma(a, x.y, acc.y)); }
__device__ __forceinline__ double mulv(double a, double x) { return a * x; }
__device__ __forceinline__ cplx mulv(double a, cplx x) { return mk(a * x.x, a * x.y); }
template <typename V> __device__ __forceinline__ V zero_v() { return V{}; }
__device__ __forceinline__ cplx to_v(cplx v, cplx*) { return v; }
__device__ __forceinline__ cplx to_v(double v, cplx*) { return mk(v, 0.0); }
__device__ __forceinline__ double to_v(double v, double*) { return v; }

struct Ang { double ca, sa, cb, sb, cg, sg, isgn; };   // cos / sin of the zyz angles; isgn: the sign of i in the conversions

// R = Rz(yaw) Ry(pitch) Rx(roll) -> zyz angles.  b = atan2(hypot(R13, R23), R33) keeps all digits near 0 and pi.  Near b = 0
// only a + g is well determined (from the 2 x 2 block, to full precision) and only a - g near b = pi; a and g from the third row
// and column carry an error of eps / sin b, which the operator only sees multiplied by sin b.  sin b = 0 exactly (gimbal): those
// two atan2 are not formed.
__device__ __forceinline__ Ang zyz(double yaw, double pitch, double roll, bool transpose) {
    double sy, cy, sp, cp, sr, cr;
    sincos(yaw, &sy, &cy);
    sincos(pitch, &sp, &cp);
    sincos(roll, &sr, &cr);
    const double R11 = cy * cp, R12 = -sy * cr + cy * sp * sr, R13 = sy * sr + cy * sp * cr;
    const double R21 = sy * cp, R22 = cy * cr + sy * sp * sr, R23 = -cy * sr + sy * sp * cr;
    const double R31 = -sp, R32 = cp * sr, R33 = cp * cr;
    const double h = hypot(R13, R23);
    const double b = atan2(h, R33);
    const double a0 = h > 0.0 ? atan2(R23, R13) : 0.0, g0 = h > 0.0 ? atan2(R32, -R31) : 0.0;
    double a, g;
    if (R33 >= 0.0) {   // a + g from (1 + cos b) (cos, sin)(a + g)
        const double d = remainder(atan2(R21 - R12, R11 + R22) - (a0 + g0), 2.0 * kPi);
        a = a0 + 0.5 * d; g = g0 + 0.5 * d;
    } else {            // a - g from (cos b - 1) (cos, sin)(a - g)
        const double d = remainder(atan2(-(R12 + R21), R22 - R11) - (a0 - g0), 2.0 * kPi);
        a = a0 + 0.5 * d; g = g0 - 0.5 * d;
    }
    Ang r;
    if (transpose) { const double t = a; a = -g; g = -t; }
    sincos(a, &r.sa, &r.ca);
    sincos(transpose ? -b : b, &r.sb, &r.cb);
    sincos(g, &r.sg, &r.cg);
    r.isgn = transpose ? -1.0 : 1.0;
    return r;
}

// Z(t) on the 2l + 1 values of order l (local index l + m): cos / sin(m t) by angle addition from (c1, s1)
template <int l, typename V> __device__ __forceinline__ void zrot(V* v, double c1, double s1) {
    double c = c1, s = s1;
#pragma unroll
    for (int m = 1; m <= l; ++m) {
        if (m > 1) {
            const double cn = fma(c, c1, -s * s1);
            s = fma(s, c1, c * s1);
            c = cn;
        }
        const V p = v[l + m], q = v[l - m];
        v[l + m] = fmav(c, p, mulv(-s, q));
        v[l - m] = fmav(c, q, mulv(s, p));
    }
}

// complex basis <-> real coordinates of order l (m > 0): r_m = ((-1)^m c_m + c_-m) / sqrt2, r_-m = i ((-1)^m c_m - c_-m) / sqrt2,
// and back c_m = (-1)^m (r_m - i r_-m) / sqrt2, c_-m = (r_m + i r_-m) / sqrt2; i -> -i in the transposed form
template <int l> __device__ __forceinline__ void to_real(cplx* v, double is) {
    const double h = 0.70710678118654752440;
#pragma unroll
    for (int m = 1; m <= l; ++m) {
        const cplx p = (m & 1) ? -v[l + m] : v[l + m], q = v[l - m];
        const cplx s = p + q, d = p - q;
        v[l + m] = mk(h * s.x, h * s.y);
        v[l - m] = mk(-is * h * d.y, is * h * d.x);
    }
}
template <int l> __device__ __forceinline__ void from_real(cplx* v, double is) {
    const double h = 0.70710678118654752440;
#pragma unroll
    for (int m = 1; m <= l; ++m) {
        const cplx p = v[l + m], q = v[l - m];
        const cplx iq = mk(-is * q.y, is * q.x);
        const cplx a = p - iq;
        v[l + m] = (m & 1) ? mk(-h * a.x, -h * a.y) : mk(h * a.x, h * a.y);
        const cplx b = p + iq;
        v[l - m] = mk(h * b.x, h * b.y);
    }
}

// w = sum over the nonzero rows of column m of J_l (class cls_row(l, cls_of(m))) of J v, and the rank-one update y += J w
template <int l, int m, typename V> __device__ __forceinline__ V col_dot(const double* __restrict__ Jc, const V* v) {
    constexpr int c = cls_row(l, cls_of(m)), f = cls_first(c), st = cls_step(c), k = cls_size(l, c);
    V w = zero_v<V>();
#pragma unroll
    for (int r = 0; r < k; ++r) w = fmav(Jc[r], v[l + f + r * st], w);
    return w;
}
template <int l, int m, typename V> __device__ __forceinline__ void col_axpy(const double* __restrict__ Jc, V w, V* y) {
    constexpr int c = cls_row(l, cls_of(m)), f = cls_first(c), st = cls_step(c), k = cls_size(l, c);
#pragma unroll
    for (int r = 0; r < k; ++r) y[l + f + r * st] = fmav(Jc[r], w, y[l + f + r * st]);
}

// the columns +m and -m of J for m = M .. l, with Z(b) between J^T and J; (c, s) = (cos, sin)((M - 1) b) on entry (m b for M = 1)
template <int l, int M, typename V>
__device__ __forceinline__ void cols_from(const double* __restrict__ Jl, const V* v, V* y, double& c, double& s, double cb, double sb) {
    if constexpr (M <= l) {
        if constexpr (M > 1) { const double cn = fma(c, cb, -s * sb); s = fma(s, cb, c * sb); c = cn; }
        asm volatile("" ::: "memory");   // read J column pair by column pair (else the reads of a whole order are hoisted)
        const double* Jp = Jl + col_off(l, M);
        const double* Jq = Jl + col_off(l, -M);
        const V p = col_dot<l, M>(Jp, v), q = col_dot<l, -M>(Jq, v);
        col_axpy<l, M>(Jp, fmav(c, p, mulv(-s, q)), y);
        col_axpy<l, -M>(Jq, fmav(c, q, mulv(s, p)), y);
        cols_from<l, M + 1>(Jl, v, y, c, s, cb, sb);
    }
}

// one order: v <- Z(a) J Z(b) J^T Z(g) v.  The columns of J^T and J are the same values: one LDS read feeds two FMAs per part
template <int l, bool CB, typename V, typename Ld, typename St>
__device__ __forceinline__ void rot_order(const double* __restrict__ J, const Ang& a0, Ld ld, St st) {
    // the cos / sin(m t) of the three angles are recomputed per order: opaque copies keep the compiler from merging the
    // recurrences of all orders, which would hold 6 N values live through the whole sample
    Ang a = a0;
    asm volatile("" : "+v"(a.ca), "+v"(a.sa), "+v"(a.cb), "+v"(a.sb), "+v"(a.cg), "+v"(a.sg));
    // J is loop-invariant LDS: without this fence the compiler hoists every order's J reads out of the sample loop into registers
    asm volatile("" ::: "memory");
    V v[2 * l + 1], y[2 * l + 1];
#pragma unroll
    for (int i = 0; i < 2 * l + 1; ++i) { v[i] = ld(l * l + i); y[i] = zero_v<V>(); }
    if constexpr (CB) to_real<l>(v, a.isgn);
    zrot<l>(v, a.cg, a.sg);
    const double* Jl = J + jpk_off(l);
    { const V w = col_dot<l, 0>(Jl, v); col_axpy<l, 0>(Jl, w, y); }
    double c = a.cb, s = a.sb;   // cos / sin(m b)
    cols_from<l, 1>(Jl, v, y, c, s, a.cb, a.sb);
    zrot<l>(y, a.ca, a.sa);
    if constexpr (CB) from_real<l>(y, a.isgn);
#pragma unroll
    for (int i = 0; i < 2 * l + 1; ++i) st(l * l + i, y[i]);
}

// orders 0 .. N (N <= NB, wave-uniform): the branch per order also keeps the compiler from hoisting the next order's loads
template <int l, int NB, bool CB, typename V, typename Ld, typename St>
__device__ __forceinline__ void rot_orders(int N, const double* __restrict__ J, const Ang& a, Ld ld, St st) {
    if constexpr (l == 0) st(0, ld(0));   // order 0 is invariant
    else rot_order<l, CB, V>(J, a, ld, st);
    if constexpr (l < NB) { if (l < N) rot_orders<l + 1, NB, CB, V>(N, J, a, ld, st); }
}

__device__ __forceinline__ void load_j(int N, double* J, const double* __restrict__ jpk) {
    for (int i = threadIdx.x; i < jpk_off(N + 1); i += blockDim.x) J[i] = jpk[i];
    __syncthreads();
}

// one lane = one sample (row); columns are channel planes of n values, so a wave's loads and stores are contiguous.  IC: complex
// input; CB: complex basis (output complex when IC || CB).  Each angle: null (0), one value (ps* = 0) or one per sample.
// the occupancy asked of an instantiation: the live values of one order, 2 (2 NB + 1) doubles (twice that complex), and the
// loads of the next order in flight; the trigonometry of zyz() needs about 120 VGPRs whatever NB is
__host__ __device__ constexpr int r3_waves(int NB, bool cplx_v) { return NB <= 2 ? 4 : NB <= 4 ? (cplx_v ? 3 : 4) : NB <= 8 ? (cplx_v ? 2 : 3) : (cplx_v ? 1 : 2); }

// grid (., L): listener blockIdx.y turns the one signal by its angles (each at + l la[.]) into out_ + l lo (a listener group)
struct R3Listener { int64_t la[3], lo; };

// NB: the largest order of the instantiation (buckets 2, 4, 8, 15), N the order of the call
template <int NB, bool IC, bool CB>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(r3_waves(NB, IC || CB)))) rotate3_kernel(int N, const void* __restrict__ in_, int64_t n, const double* __restrict__ yaw, int yps,
                                                      const double* __restrict__ pitch, int pps, const double* __restrict__ roll, int rps,
                                                      int transpose, const double* __restrict__ jpk, void* __restrict__ out_, int64_t ldi, int64_t ldo,
                                                      R3Listener ls) {
    using TI = std::conditional_t<IC, cplx, double>;
    using V = std::conditional_t<IC || CB, cplx, double>;
    __shared__ double J[jpk_off(NB + 1)];
    load_j(N, J, jpk);
    const TI* __restrict__ in = reinterpret_cast<const TI*>(in_);
    const int64_t lis = blockIdx.y;   // the listener
    V* __restrict__ out = reinterpret_cast<V*>(out_) + lis * ls.lo;
    const int64_t oy = lis * ls.la[0], op = lis * ls.la[1], orl = lis * ls.la[2];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const Ang a = zyz(yaw ? yaw[oy + (yps ? t : 0)] : 0.0, pitch ? pitch[op + (pps ? t : 0)] : 0.0, roll ? roll[orl + (rps ? t : 0)] : 0.0,
                          transpose != 0);
        rot_orders<0, NB, CB, V>(N, J, a, [&](int k) { return to_v(in[(int64_t)k * ldi + t], (V*)nullptr); },
                                [&](int k, V v) { out[(int64_t)k * ldo + t] = v; });
    }
}

// The ENC form (encode_tile.hpp): the workgroup encodes its tile of ENC_T samples of the microphone block
// into LDS and its first ENC_T lanes turn the tile from there, one sample each, through the same rot_orders as the kernel above.
// EC: complex encoder, so a complex encoded signal.  grid (n / ENC_T, L); dynamic LDS enc_lds_bytes(C, M, EC, true) beside J
template <int NB, bool EC, bool CB>
__global__ void __launch_bounds__(ENC_NT) __attribute__((amdgpu_waves_per_eu(r3_waves(NB, EC || CB)))) rotate3_enc_kernel(int N, EncIn e, int C, int64_t n, const double* __restrict__ yaw, int yps,
                                                      const double* __restrict__ pitch, int pps, const double* __restrict__ roll, int rps,
                                                      const double* __restrict__ jpk, void* __restrict__ out_, int64_t ldo, R3Listener ls) {
    using TI = std::conditional_t<EC, cplx, double>;
    using V = std::conditional_t<EC || CB, cplx, double>;
    __shared__ double J[jpk_off(NB + 1)];
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    TI* enc_s = reinterpret_cast<TI*>(dyn);
    TI* tile = enc_s + C * e.M;   // [C][ENC_T]
    for (int i = threadIdx.x; i < jpk_off(N + 1); i += ENC_NT) J[i] = jpk[i];   // (the barriers of encode_tile cover it)
    const int64_t t0 = (int64_t)blockIdx.x * ENC_T;
    encode_tile<EC>(e, C, t0, n, enc_s, [&](int c, int t, TI v) { tile[c * ENC_T + t] = v; });
    __syncthreads();
    const int tl = threadIdx.x;
    const int64_t t = t0 + tl;
    if (tl >= ENC_T || t >= n) return;
    const int64_t lis = blockIdx.y;   // the listener
    V* __restrict__ out = reinterpret_cast<V*>(out_) + lis * ls.lo;
    const int64_t oy = lis * ls.la[0], op = lis * ls.la[1], orl = lis * ls.la[2];
    const Ang a = zyz(yaw ? yaw[oy + (yps ? t : 0)] : 0.0, pitch ? pitch[op + (pps ? t : 0)] : 0.0, roll ? roll[orl + (rps ? t : 0)] : 0.0, false);
    rot_orders<0, NB, CB, V>(N, J, a, [&](int k) { return to_v(tile[k * ENC_T + tl], (V*)nullptr); },
                            [&](int k, V v) { out[(int64_t)k * ldo + t] = v; });
}

// the matrix M itself, column j = the pass applied to e_j: out [(N+1)^2 x (N+1)^2] column-major, out_row = in_row M^T
template <int NB, bool CB>
__global__ void __launch_bounds__(256) rotate3_matrix_kernel(int N, double yaw, double pitch, double roll, const double* __restrict__ jpk,
                                                             void* __restrict__ out_) {
    using V = std::conditional_t<CB, cplx, double>;
    const int C = (N + 1) * (N + 1);
    __shared__ double J[jpk_off(NB + 1)];
    load_j(N, J, jpk);
    V* __restrict__ out = reinterpret_cast<V*>(out_);
    const int j = threadIdx.x + blockIdx.x * blockDim.x;
    if (j >= C) return;
    const Ang a = zyz(yaw, pitch, roll, false);
    rot_orders<0, NB, CB, V>(N, J, a, [&](int k) { return to_v(k == j ? 1.0 : 0.0, (V*)nullptr); },
                            [&](int k, V v) { out[(int64_t)j * C + k] = v; });
}

// J of every order up to R3_NMAX, per device, built on first use and kept (released by rotate3_cache_clear)
std::mutex g_j_mu;
double* g_j[64] = {};

const double* j_pack(hipStream_t st) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) throw Error(2, "rotate3: device index out of range");
    std::lock_guard<std::mutex> lk(g_j_mu);
    if (!g_j[dev]) {
        double* p = nullptr;
        HIP_CHECK(hipMalloc(&p, sizeof(double) * jpk_off(R3_NMAX + 1)));
        build_j_kernel<<<1, 1024, 0, st>>>(p);
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess && hipStreamSynchronize(st) == hipSuccess) g_j[dev] = p;
        else { hipFree(p); HIP_CHECK(e != hipSuccess ? e : hipErrorLaunchFailure); }
    }
    return g_j[dev];
}

template <int NB> void launch_nb(int N, const void* in, bool ic, int64_t n, bool cb, const double* yaw, bool yps, const double* pitch,
                                bool pps, const double* roll, bool rps, bool transpose, const double* jpk, void* out, hipStream_t st, int64_t ldi, int64_t ldo,
                                int L, const R3Listener& ls) {
    const dim3 grid((unsigned)std::min<int64_t>(ceil_div(n, 256), 1 << 20), (unsigned)L);   // one sample per lane up to 268 M samples
    auto k = ic ? (cb ? rotate3_kernel<NB, true, true> : rotate3_kernel<NB, true, false>)
                : (cb ? rotate3_kernel<NB, false, true> : rotate3_kernel<NB, false, false>);
    k<<<grid, 256, 0, st>>>(N, in, n, yaw, yps, pitch, pps, roll, rps, transpose ? 1 : 0, jpk, out, ldi, ldo, ls);
    KERNEL_CHECK();
}

template <int NB> void launch_nb_enc(int N, const EncodeBlock& e, int C, int64_t n, bool cb, const double* yaw, bool yps, const double* pitch, bool pps,
                                    const double* roll, bool rps, const double* jpk, void* out, hipStream_t st, int64_t ldo, int L, const R3Listener& ls) {
    static PerDeviceOnce once;
    if (once.first()) {
#define EMAGLS_R3_ATTR(K) HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024))
        EMAGLS_R3_ATTR((rotate3_enc_kernel<NB, true, true>));
        EMAGLS_R3_ATTR((rotate3_enc_kernel<NB, true, false>));
        EMAGLS_R3_ATTR((rotate3_enc_kernel<NB, false, true>));
        EMAGLS_R3_ATTR((rotate3_enc_kernel<NB, false, false>));
#undef EMAGLS_R3_ATTR
    }
    const dim3 grid((unsigned)ceil_div(n, ENC_T), (unsigned)L);
    auto k = e.enc_cplx ? (cb ? rotate3_enc_kernel<NB, true, true> : rotate3_enc_kernel<NB, true, false>)
                        : (cb ? rotate3_enc_kernel<NB, false, true> : rotate3_enc_kernel<NB, false, false>);
    k<<<grid, ENC_NT, enc_lds_bytes(C, e.M, e.enc_cplx, true), st>>>(N, EncIn{e.enc, e.M, e.x, e.ldx}, C, n, yaw, yps, pitch, pps, roll, rps, jpk, out, ldo, ls);
    KERNEL_CHECK();
}

template <int NB> void launch_mat(int N, bool cb, double yaw, double pitch, double roll, const double* jpk, void* out, hipStream_t st) {
    const unsigned grid = (unsigned)ceil_div((N + 1) * (N + 1), 256);
    if (cb) rotate3_matrix_kernel<NB, true><<<grid, 256, 0, st>>>(N, yaw, pitch, roll, jpk, out);
    else rotate3_matrix_kernel<NB, false><<<grid, 256, 0, st>>>(N, yaw, pitch, roll, jpk, out);
    KERNEL_CHECK();
}

void check_order(int N) {
    if (N < 0) throw Error(1, "rotate3: the channel count is not (N+1)^2");
    if (N > R3_NMAX) throw Error(2, "the three-axis rotation supports SH orders 0 to 15");
}

}  // namespace

int rotate3_max_order() { return R3_NMAX; }

void launch_rotate3(const void* in, bool in_cplx, int64_t n, int C, bool cplx_basis, const double* yaw, bool yaw_ps, const double* pitch,
                    bool pitch_ps, const double* roll, bool roll_ps, bool transpose, void* out, hipStream_t st, int64_t ld_in, int64_t ld_out, int L,
                    const int64_t* la, int64_t lo) {
    if (n <= 0) return;
    const int64_t ldi = ld_in ? ld_in : n, ldo = ld_out ? ld_out : n;
    const int N = rotate_order(0, C);
    check_order(N);
    const double* jpk = j_pack(st);
    const R3Listener ls{{la ? la[0] : 0, la ? la[1] : 0, la ? la[2] : 0}, lo};
    if (N <= 2) launch_nb<2>(N, in, in_cplx, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, transpose, jpk, out, st, ldi, ldo, L, ls);
    else if (N <= 4) launch_nb<4>(N, in, in_cplx, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, transpose, jpk, out, st, ldi, ldo, L, ls);
    else if (N <= 8) launch_nb<8>(N, in, in_cplx, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, transpose, jpk, out, st, ldi, ldo, L, ls);
    else launch_nb<R3_NMAX>(N, in, in_cplx, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, transpose, jpk, out, st, ldi, ldo, L, ls);
}

void launch_rotate3_encoded(const EncodeBlock& e, int64_t n, int C, bool cplx_basis, const double* yaw, bool yaw_ps, const double* pitch, bool pitch_ps,
                            const double* roll, bool roll_ps, void* out, hipStream_t st, int64_t ld_out, int L, const int64_t* la, int64_t lo) {
    if (n <= 0) return;
    if (e.M < 1 || e.M > ENC_MAX || C > ENC_MAX) throw Error(2, "the stream's encoder supports 1 to 64 microphones and 1 to 64 channels");
    const int64_t ldo = ld_out ? ld_out : n;
    const int N = rotate_order(0, C);
    check_order(N);
    const double* jpk = j_pack(st);
    const R3Listener ls{{la ? la[0] : 0, la ? la[1] : 0, la ? la[2] : 0}, lo};
    if (N <= 2) launch_nb_enc<2>(N, e, C, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, jpk, out, st, ldo, L, ls);
    else if (N <= 4) launch_nb_enc<4>(N, e, C, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, jpk, out, st, ldo, L, ls);
    else launch_nb_enc<8>(N, e, C, n, cplx_basis, yaw, yaw_ps, pitch, pitch_ps, roll, roll_ps, jpk, out, st, ldo, L, ls);   // (C <= 64: N <= 7)
}

void launch_rotate3_matrix(int N, bool cplx_basis, double yaw, double pitch, double roll, void* out, hipStream_t st) {
    check_order(N);
    const double* jpk = j_pack(st);
    if (N <= 2) launch_mat<2>(N, cplx_basis, yaw, pitch, roll, jpk, out, st);
    else if (N <= 4) launch_mat<4>(N, cplx_basis, yaw, pitch, roll, jpk, out, st);
    else if (N <= 8) launch_mat<8>(N, cplx_basis, yaw, pitch, roll, jpk, out, st);
    else launch_mat<R3_NMAX>(N, cplx_basis, yaw, pitch, roll, jpk, out, st);
}

void rotate3_cache_clear() {
    std::lock_guard<std::mutex> lk(g_j_mu);
    for (double*& p : g_j) { if (p) hipFree(p); p = nullptr; }
}

}  // namespace emagls
