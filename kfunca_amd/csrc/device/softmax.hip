// Row softmax and log_softmax over the last dimension for gfx950, forward and backward, on [rows, V] operands addressed by a leading
// dimension. With s = scale * x and lse = log sum_v exp(s_v):
//
//   softmax       y_v = exp(s_v - lse)            dx_v = scale * y_v * (dy_v - sum_u dy_u y_u)
//   log_softmax   y_v = s_v - lse                 dx_v = scale * (dy_v - exp(y_v) * sum_u dy_u)
//
// The backward works from the forward's OUTPUT y (and dy): the operator keeps y, not x.
//
// Both directions are HBM streams with one row reduction each. Regimes, picked from (rows, V) alone (sm_regime):
//   wave    V <= 2048            one wave per row, four rows per 256-thread block; the row lives in the registers of the lanes that
//                                loaded it (8 or 32 f32 per lane, plus the head and tail element): read once, written once
//   block   2048 < V <= 16384    one 256-thread block per row, the row in registers (32 or 64 f32 per lane); the row's max and sum go
//                                across the four waves through LDS, combined in wave order: read once, written once
//   stream  V > 16384            one block per row; pass 1 is the online (max, sum) of cross_entropy.hip, pass 2 re-reads x and writes y.
//                                The backward likewise: pass 1 the row sum, pass 2 re-reads y and dy and writes dx.
// The backward holds y and dy in registers in the two resident regimes.
//
// Alignment: a row is read as a scalar head up to the first 16-byte boundary, 16-byte packs, and a scalar tail, so odd V and odd leading
// dimensions keep the vector access. A lane owns whole packs; the order in which a row's elements are combined is a function of V, the
// regime and the phase of the FIRST operand's row (x, or y in the backward) within 16 bytes, nothing else. Where the rows of another
// operand sit differently against the 16-byte boundaries the call takes the element path: the same lanes own the same elements and do
// the same arithmetic, with element loads and stores, so both paths give the same bits.
//
// Precision at large logits, as in cross_entropy.hip: with k = scale * log2(e) (f32), x k - h is formed in ONE rounding inside the FMA
// against h = m k rounded to f32, and the exact residual lo = fma(m, k, -h) is folded into the finish (lse = scale m + ln S - lo ln 2).
// log_softmax is (x - m) scale - (ln S - lo ln 2): no cancellation against a large lse.
//
// -inf never produces exp(-inf - (-inf)): a state whose max is still -inf uses offset 0. A row that holds a NaN or +inf, or only -inf,
// comes out NaN throughout (the sum is NaN, or 0 / 0); every other row is untouched by it.
//
// No workspace, no atomics, a fixed combination order: bitwise reproducible, safe under graph capture. All row offsets are 64-bit.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// Every fused multiply-add here is written out (fmaf), as in cross_entropy.hip: contraction would fuse m_old * k - h_new into one FMA whose
// exact product no longer cancels against the rounded h_old; and the packed and the element path must round alike, bit for bit.
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr double kLog2ed = 1.44269504088896340736;
constexpr float kLog2e = (float)kLog2ed, kLog2eLo = (float)(kLog2ed - (double)kLog2e);
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kSmBlock = 256;
constexpr int64_t kSmWaveMax = 2048;     // V up to this: one wave per row
constexpr int64_t kSmBlockMax = 16384;   // V up to this: one block per row, the row in registers
// elements a lane holds at most: the smaller tile serves V <= 64 * 8 (wave) and V <= 256 * 32 (block)
constexpr int kSmWaveSmall = 8, kSmWaveLarge = 32, kSmBlockSmall = 32, kSmBlockLarge = 64;
static_assert(64 * kSmWaveLarge == kSmWaveMax && kSmBlock * kSmBlockLarge == kSmBlockMax, "a resident row must fit its lanes' tiles");

struct SmArgs {
    const void *a, *b;        // forward: x, -; backward: y, dy
    void *o;                  // forward: y; backward: dx
    int64_t rows, V, lda, ldb, ldo;
    float scale, k;           // k = scale * log2(e)
};

__device__ __forceinline__ float sm_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float sm_h(float m, float k) { return m == -INFINITY ? 0.f : m * k; }

// exp(y) of a stored log-probability: y log2(e) in two parts, so that the rounding of the product (|y| 2^-24 of exponent) stays out
__device__ __forceinline__ float sm_exp(float y) {
    const float t = y * kLog2e;
    if (t == -INFINITY) return 0.f;
    const float r = fmaf(y, kLog2e, -t) + y * kLog2eLo;
    const float e = sm_exp2(t);
    return fmaf(e, r * kLn2, e);
}

// Vp elements at p: one 16-byte pack, or Vp single elements
template <typename T, bool VEC, int Vp>
__device__ __forceinline__ void sm_load(const T *p, float (&f)[Vp]) {
    if constexpr (VEC) {
        unpack16<T>(*(const uint4 *)p, f);
    } else {
#pragma unroll
        for (int i = 0; i < Vp; ++i) f[i] = load_f32(p + i);
    }
}
// one rounding per element, the same in both paths (store_hw and pack16 use the same converters). f32 -> f16 of values the compiler
// cannot see through: left to itself it folds the last multiply into the conversion in one path only (see glu.hip)
template <typename T> __device__ __forceinline__ float sm_opaque(float v) {
    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(v));
    return v;
}
template <typename T> __device__ __forceinline__ void sm_store1(T *p, float v) { store_hw(p, sm_opaque<T>(v)); }
template <typename T, bool VEC, int Vp>
__device__ __forceinline__ void sm_store(T *p, const float (&f)[Vp]) {
    float r[Vp];
#pragma unroll
    for (int i = 0; i < Vp; ++i) r[i] = sm_opaque<T>(f[i]);
    if constexpr (VEC) {
        *(uint4 *)p = pack16<T>(r);
    } else {
#pragma unroll
        for (int i = 0; i < Vp; ++i) store_hw(p + i, r[i]);
    }
}

// elements in front of the first 16-byte boundary of a row of n elements at p
template <typename T> __device__ __forceinline__ int64_t sm_head(const T *p, int64_t n) {
    return std::min<int64_t>(n, (int64_t)((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u) / (int64_t)sizeof(T));
}

// ---- reductions over the NT lanes of a row: the wave by an xor butterfly, the block's waves through LDS in wave order. Every lane
// gets the result. red: kSmBlock / 64 floats per call, not reused within a kernel.
template <int NT> __device__ __forceinline__ float sm_all_max(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v = fmaxf(v, red[w]);
    }
    return v;
}
template <int NT> __device__ __forceinline__ float sm_all_sum(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
        __syncthreads();
        v = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) v += red[w];
    }
    return v;
}

// ---- the finish of an element, shared by all regimes ------------------------------------------------------------------------------
// forward: from the row's max m and S = sum 2^(x k - h)
template <int KIND> struct SmFwdFin {
    float m, h, k, scale, c;   // c: 1 / S (softmax), ln S - lo ln 2 (log_softmax)
    __device__ __forceinline__ SmFwdFin(float m_, float s, float k_, float scale_) : m(m_), h(sm_h(m_, k_)), k(k_), scale(scale_) {
        if constexpr (KIND == KF_SOFTMAX) {
            c = 1.f / s;
        } else {
            const float lo = m == -INFINITY ? 0.f : fmaf(m, k, -h);
            c = logf(s) - lo * kLn2;
        }
    }
    __device__ __forceinline__ float e(float x) const { return sm_exp2(fmaf(x, k, -h)); }
    __device__ __forceinline__ float operator()(float x) const {
        if constexpr (KIND == KF_SOFTMAX) return e(x) * c;
        else return fmaf(x - m, scale, -c);
    }
};
// backward: the term of the row sum, and dx from the sum d
template <int KIND> __device__ __forceinline__ float sm_bwd_term(float acc, float y, float dy) {
    if constexpr (KIND == KF_SOFTMAX) return fmaf(dy, y, acc);
    else return acc + dy;
}
template <int KIND> __device__ __forceinline__ float sm_bwd_dx(float y, float dy, float d, float scale) {
    if constexpr (KIND == KF_SOFTMAX) return y * (dy - d) * scale;
    else return fmaf(-sm_exp(y), d, dy) * scale;
}

// ---- resident rows: NT lanes per row, PJ packs per lane ------------------------------------------------------------------------------
// A lane owns the head element `lane` (lane < head), the tail element t0 + lane, and the packs lane, lane + NT, ... of the row; slots
// it does not own hold the neutral value of the reduction and are never stored.
template <int NT> __device__ __forceinline__ bool sm_row_of(const SmArgs &a, int64_t &row, int &lane) {
    if constexpr (NT == 64) {
        row = (int64_t)blockIdx.x * (kSmBlock / 64) + (threadIdx.x >> 6);
        lane = threadIdx.x & 63;
        return row < a.rows;   // whole waves
    } else {
        row = blockIdx.x;
        lane = threadIdx.x;
        return true;
    }
}

template <typename T, int NT, int PJ, int KIND, bool VEC>
__global__ __launch_bounds__(kSmBlock) void sm_fwd_resident(const SmArgs a) {
    constexpr int Vp = kPack16<T>;
    __shared__ float red[2 * kSmBlock / 64];
    int64_t row;
    int lane;
    if (!sm_row_of<NT>(a, row, lane)) return;
    const T *x = (const T *)a.a + row * a.lda;
    T *y = (T *)a.o + row * a.ldo;
    const int n = (int)a.V, head = (int)sm_head(x, n), nb = (n - head) / Vp, t0 = head + nb * Vp;
    const bool has_h = lane < head, has_t = t0 + lane < n;
    float hv = has_h ? load_f32(x + lane) : -INFINITY, tv = has_t ? load_f32(x + t0 + lane) : -INFINITY;
    float f[PJ][Vp];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        if (lane + j * NT < nb) {
            sm_load<T, VEC>(x + head + (lane + j * NT) * Vp, f[j]);
        } else {
#pragma unroll
            for (int i = 0; i < Vp; ++i) f[j][i] = -INFINITY;
        }
    }
    float m = fmaxf(hv, tv);
#pragma unroll
    for (int j = 0; j < PJ; ++j)
#pragma unroll
        for (int i = 0; i < Vp; ++i) m = fmaxf(m, f[j][i]);
    m = sm_all_max<NT>(m, red);
    const float h = sm_h(m, a.k);
    // the sum; softmax keeps the exponentials in place of the logits
    float ev[2] = {sm_exp2(fmaf(hv, a.k, -h)), sm_exp2(fmaf(tv, a.k, -h))};
    float s = ev[0] + ev[1];
#pragma unroll
    for (int j = 0; j < PJ; ++j)
#pragma unroll
        for (int i = 0; i < Vp; ++i) {
            const float e = sm_exp2(fmaf(f[j][i], a.k, -h));
            s += e;
            if constexpr (KIND == KF_SOFTMAX) f[j][i] = e;
        }
    s = sm_all_sum<NT>(s, red + kSmBlock / 64);
    const SmFwdFin<KIND> fin(m, s, a.k, a.scale);
    if (has_h) sm_store1(y + lane, KIND == KF_SOFTMAX ? ev[0] * fin.c : fin(hv));
    if (has_t) sm_store1(y + t0 + lane, KIND == KF_SOFTMAX ? ev[1] * fin.c : fin(tv));
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        if (lane + j * NT < nb) {
            float r[Vp];
#pragma unroll
            for (int i = 0; i < Vp; ++i) r[i] = KIND == KF_SOFTMAX ? f[j][i] * fin.c : fin(f[j][i]);
            sm_store<T, VEC>(y + head + (lane + j * NT) * Vp, r);
        }
    }
}

template <typename T, int NT, int PJ, int KIND, bool VEC>
__global__ __launch_bounds__(kSmBlock) void sm_bwd_resident(const SmArgs a) {
    constexpr int Vp = kPack16<T>;
    __shared__ float red[kSmBlock / 64];
    int64_t row;
    int lane;
    if (!sm_row_of<NT>(a, row, lane)) return;
    const T *y = (const T *)a.a + row * a.lda, *dy = (const T *)a.b + row * a.ldb;
    T *dx = (T *)a.o + row * a.ldo;
    const int n = (int)a.V, head = (int)sm_head(y, n), nb = (n - head) / Vp, t0 = head + nb * Vp;
    const bool has_h = lane < head, has_t = t0 + lane < n;
    // a slot the lane does not own adds nothing: dy = 0 and y = 0 (log_softmax never reads y for the sum)
    const float yh = has_h ? load_f32(y + lane) : 0.f, dh = has_h ? load_f32(dy + lane) : 0.f;
    const float yt = has_t ? load_f32(y + t0 + lane) : 0.f, dt = has_t ? load_f32(dy + t0 + lane) : 0.f;
    float fy[PJ][Vp], fd[PJ][Vp];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        if (lane + j * NT < nb) {
            sm_load<T, VEC>(y + head + (lane + j * NT) * Vp, fy[j]);
            sm_load<T, VEC>(dy + head + (lane + j * NT) * Vp, fd[j]);
        } else {
#pragma unroll
            for (int i = 0; i < Vp; ++i) fy[j][i] = fd[j][i] = 0.f;
        }
    }
    float d = sm_bwd_term<KIND>(sm_bwd_term<KIND>(0.f, yh, dh), yt, dt);
#pragma unroll
    for (int j = 0; j < PJ; ++j)
#pragma unroll
        for (int i = 0; i < Vp; ++i) d = sm_bwd_term<KIND>(d, fy[j][i], fd[j][i]);
    d = sm_all_sum<NT>(d, red);
    if (has_h) sm_store1(dx + lane, sm_bwd_dx<KIND>(yh, dh, d, a.scale));
    if (has_t) sm_store1(dx + t0 + lane, sm_bwd_dx<KIND>(yt, dt, d, a.scale));
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
        if (lane + j * NT < nb) {
            float r[Vp];
#pragma unroll
            for (int i = 0; i < Vp; ++i) r[i] = sm_bwd_dx<KIND>(fy[j][i], fd[j][i], d, a.scale);
            sm_store<T, VEC>(dx + head + (lane + j * NT) * Vp, r);
        }
    }
}

// ---- streamed rows: one block per row, two passes -----------------------------------------------------------------------------------
// the online state of cross_entropy.hip with k in place of log2(e): s = sum 2^(x k - h(m)), h(m) = m k rounded to f32 (0 while m = -inf)
struct SmState { float m, s; };
// s taken relative to h(m_old), moved to h(m_new), m_new >= m_old. m_old * k (not h: -inf stays -inf) makes the factor 0 for a state that
// has seen only -inf
__device__ __forceinline__ float sm_rescale(float s, float m_old, float m_new, float h_new, float k) {
    return m_old == m_new ? s : s * sm_exp2(m_old * k - h_new);
}
__device__ __forceinline__ SmState sm_combine(const SmState &a, const SmState &b, float k) {
    const float m = fmaxf(a.m, b.m), h = sm_h(m, k);
    return {m, sm_rescale(a.s, a.m, m, h, k) + sm_rescale(b.s, b.m, m, h, k)};
}
template <int N> __device__ __forceinline__ void sm_absorb(SmState &st, const float (&f)[N], float k) {
    float pm = f[0];
#pragma unroll
    for (int i = 1; i < N; ++i) pm = fmaxf(pm, f[i]);
    const float m = fmaxf(st.m, pm), h = sm_h(m, k);
    float s = sm_rescale(st.s, st.m, m, h, k);
#pragma unroll
    for (int i = 0; i < N; ++i) s += sm_exp2(fmaf(f[i], k, -h));
    st.m = m;
    st.s = s;
}

// a row of n elements with `head` of them in front of the first pack, as seen by one of the block's threads: one(i) for its head and
// tail elements, pack(i) for every pack it owns (i: the element offset of the pack)
template <int Vp, typename One, typename Pack>
__device__ __forceinline__ void sm_walk(int64_t n, int64_t head, One &&one, Pack &&pack) {
    const int lane = threadIdx.x;
    const int64_t nb = (n - head) / Vp, t0 = head + nb * Vp;
    if (lane < head) one((int64_t)lane);
    if (t0 + lane < n) one(t0 + lane);
    for (int64_t k = lane; k < nb; k += kSmBlock) pack(head + k * Vp);
}

template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(kSmBlock) void sm_fwd_stream(const SmArgs a) {
    constexpr int Vp = kPack16<T>;
    __shared__ SmState red[kSmBlock / 64];
    const int64_t row = blockIdx.x, n = a.V;
    const T *x = (const T *)a.a + row * a.lda;
    T *y = (T *)a.o + row * a.ldo;
    const int64_t head = sm_head(x, n);
    const float k = a.k;
    // pass 1 reads x alone: packs whatever y's phase is
    SmState st{-INFINITY, 0.f};
    sm_walk<Vp>(n, head,
                [&](int64_t i) { const float f[1] = {load_f32(x + i)}; sm_absorb<1>(st, f, k); },
                [&](int64_t i) { float f[Vp]; sm_load<T, true>(x + i, f); sm_absorb<Vp>(st, f, k); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) st = sm_combine(st, SmState{__shfl_xor(st.m, o, 64), __shfl_xor(st.s, o, 64)}, k);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = st;
    __syncthreads();   // also: every read of pass 1 comes before any write of pass 2 (y == x)
    st = red[0];
#pragma unroll
    for (int w = 1; w < kSmBlock / 64; ++w) st = sm_combine(st, red[w], k);
    const SmFwdFin<KIND> fin(st.m, st.s, k, a.scale);
    if constexpr (VEC) {
        sm_walk<Vp>(n, head,
                    [&](int64_t i) { sm_store1(y + i, fin(load_f32(x + i))); },
                    [&](int64_t i) {
                        float f[Vp];
                        sm_load<T, true>(x + i, f);
#pragma unroll
                        for (int e = 0; e < Vp; ++e) f[e] = fin(f[e]);
                        sm_store<T, true>(y + i, f);
                    });
    } else {
        for (int64_t i = threadIdx.x; i < n; i += kSmBlock) sm_store1(y + i, fin(load_f32(x + i)));
    }
}

template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(kSmBlock) void sm_bwd_stream(const SmArgs a) {
    constexpr int Vp = kPack16<T>;
    __shared__ float red[kSmBlock / 64];
    const int64_t row = blockIdx.x, n = a.V;
    const T *y = (const T *)a.a + row * a.lda, *dy = (const T *)a.b + row * a.ldb;
    T *dx = (T *)a.o + row * a.ldo;
    const int64_t head = sm_head(y, n);
    const float scale = a.scale;
    // pass 1: the lanes own the packs of y's row in both paths, so the sum is the same sum
    float d = 0.f;
    sm_walk<Vp>(n, head,
                [&](int64_t i) { d = sm_bwd_term<KIND>(d, load_f32(y + i), load_f32(dy + i)); },
                [&](int64_t i) {
                    float fy[Vp], fd[Vp];
                    if constexpr (KIND == KF_SOFTMAX) sm_load<T, VEC>(y + i, fy);
                    sm_load<T, VEC>(dy + i, fd);
#pragma unroll
                    for (int e = 0; e < Vp; ++e) d = sm_bwd_term<KIND>(d, KIND == KF_SOFTMAX ? fy[e] : 0.f, fd[e]);
                });
    d = sm_all_sum<kSmBlock>(d, red);   // its barrier: every read of pass 1 comes before any write of pass 2 (dx == dy)
    if constexpr (VEC) {
        sm_walk<Vp>(n, head,
                    [&](int64_t i) { sm_store1(dx + i, sm_bwd_dx<KIND>(load_f32(y + i), load_f32(dy + i), d, scale)); },
                    [&](int64_t i) {
                        float fy[Vp], fd[Vp];
                        sm_load<T, true>(y + i, fy);
                        sm_load<T, true>(dy + i, fd);
#pragma unroll
                        for (int e = 0; e < Vp; ++e) fd[e] = sm_bwd_dx<KIND>(fy[e], fd[e], d, scale);
                        sm_store<T, true>(dx + i, fd);
                    });
    } else {
        for (int64_t i = threadIdx.x; i < n; i += kSmBlock) sm_store1(dx + i, sm_bwd_dx<KIND>(load_f32(y + i), load_f32(dy + i), d, scale));
    }
}

// ---- the partition and the host side ---------------------------------------------------------------------------------------------------
enum SmRegime { SM_WAVE = 0, SM_BLOCK = 1, SM_STREAM = 2 };
int sm_regime(int64_t rows, int64_t V) {
    (void)rows;
    return V <= kSmWaveMax ? SM_WAVE : V <= kSmBlockMax ? SM_BLOCK : SM_STREAM;
}

struct SmOperand { const char *name; const void *p; int64_t ld; };

// [p, p + (rows - 1) ld + V) of one operand against another's: true when no element of one is an element of the other. Rows of one
// leading dimension may interleave (two column blocks of one wider buffer).
bool sm_disjoint(const SmOperand &u, const SmOperand &v, int64_t rows, int64_t V, int es) {
    if (rows == 0 || V == 0) return true;
    const uintptr_t a = (uintptr_t)u.p, b = (uintptr_t)v.p;
    const uintptr_t ea = a + (uintptr_t)((rows - 1) * u.ld + V) * es, eb = b + (uintptr_t)((rows - 1) * v.ld + V) * es;
    if (ea <= b || eb <= a) return true;
    if (u.ld != v.ld) return false;
    const uintptr_t diff = a > b ? a - b : b - a;
    if (diff % es) return false;
    const int64_t r = (int64_t)(diff / es) % u.ld;
    return r >= V && r <= u.ld - V;
}

int sm_check(const char *who, int kind, int dtype, int64_t rows, int64_t V, float scale, const SmOperand *ops, int n) {
    KF_REQUIRE(kind == KF_SOFTMAX || kind == KF_LOG_SOFTMAX, KF_ERR_INVALID, "%s: kind %d is not KF_SOFTMAX or KF_LOG_SOFTMAX", who, kind);
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(rows >= 0 && V >= 0 && rows <= 0x7fffffffLL, KF_ERR_INVALID, "%s: bad extents rows %lld V %lld (rows in [0, 2^31), V >= 0)", who,
               (long long)rows, (long long)V);
    KF_REQUIRE(scale > 0.f && scale <= 3.402823466e38f, KF_ERR_INVALID, "%s: scale %g is not finite and greater than 0", who, (double)scale);
    const int es = dtype_size(dtype);
    for (int i = 0; i < n; ++i) {
        KF_REQUIRE(ops[i].p, KF_ERR_INVALID, "%s: null %s", who, ops[i].name);
        KF_REQUIRE(ops[i].ld >= V, KF_ERR_INVALID, "%s: leading dimension of %s %lld < V = %lld", who, ops[i].name, (long long)ops[i].ld, (long long)V);
        KF_REQUIRE((uintptr_t)ops[i].p % es == 0, KF_ERR_INVALID, "%s: %s not aligned to its element size", who, ops[i].name);
    }
    return KF_OK;
}

// the rows of every operand sit alike against the 16-byte boundaries
bool sm_same_phase(const SmOperand *ops, int n, int64_t rows, int es) {
    bool ok = true;
    for (int i = 1; i < n; ++i)
        ok = ok && (((uintptr_t)ops[i].p ^ (uintptr_t)ops[0].p) & 15u) == 0 && (rows == 1 || ((ops[i].ld - ops[0].ld) * es) % 16 == 0);
    return ok;
}

template <bool BWD>
int sm_run(int kind, int dtype, int64_t rows, int64_t V, const SmArgs &a, bool vec, void *stream) {
    static const char *const labels[2][3] = {{"softmax_fwd_wave", "softmax_fwd_block", "softmax_fwd_stream"},
                                             {"softmax_bwd_wave", "softmax_bwd_block", "softmax_bwd_stream"}};
    const int regime = sm_regime(rows, V);
    hipStream_t st = as_stream(stream);
    KF_PROF(labels[BWD][regime], st);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (regime == SM_STREAM) {
            return with_flags([&](auto LOG, auto VEC) {
                constexpr int KIND = LOG ? KF_LOG_SOFTMAX : KF_SOFTMAX;
                if constexpr (BWD) return launch(sm_bwd_stream<T, KIND, VEC>, (unsigned)rows, kSmBlock, 0, st, a);
                else return launch(sm_fwd_stream<T, KIND, VEC>, (unsigned)rows, kSmBlock, 0, st, a);
            }, kind == KF_LOG_SOFTMAX, vec);
        }
        const bool wave = regime == SM_WAVE;
        const bool small = wave ? V <= 64 * kSmWaveSmall : V <= (int64_t)kSmBlock * kSmBlockSmall;
        const unsigned grid = (unsigned)(wave ? (rows + kSmBlock / 64 - 1) / (kSmBlock / 64) : rows);
        return with_flags([&](auto LOG, auto VEC, auto WAVE, auto SMALL) {
            constexpr int KIND = LOG ? KF_LOG_SOFTMAX : KF_SOFTMAX;
            constexpr int NT = WAVE ? 64 : kSmBlock;
            constexpr int PJ = (WAVE ? (SMALL ? kSmWaveSmall : kSmWaveLarge) : (SMALL ? kSmBlockSmall : kSmBlockLarge)) / kPack16<T>;
            if constexpr (BWD) return launch(sm_bwd_resident<T, NT, PJ, KIND, VEC>, grid, kSmBlock, 0, st, a);
            else return launch(sm_fwd_resident<T, NT, PJ, KIND, VEC>, grid, kSmBlock, 0, st, a);
        }, kind == KF_LOG_SOFTMAX, vec, wave, small);
    });
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_softmax_fwd(int kind, int dtype, int64_t rows, int64_t V, float scale, const void *x, int64_t ldx, void *y, int64_t ldy,
                              void *stream) {
    const SmOperand ops[2] = {{"x", x, ldx}, {"y", y, ldy}};
    const int rc = sm_check("kf_softmax_fwd", kind, dtype, rows, V, scale, ops, 2);
    if (rc != KF_OK) return rc;
    const int es = dtype_size(dtype);
    KF_REQUIRE((y == x && ldy == ldx) || sm_disjoint(ops[1], ops[0], rows, V, es), KF_ERR_INVALID,
               "kf_softmax_fwd: y overlaps x (the only alias allowed is y == x with ldy == ldx)");
    if (rows == 0 || V == 0) return KF_OK;
    SmArgs a{x, nullptr, y, rows, V, ldx, 0, ldy, scale, (float)((double)scale * kLog2ed)};
    return sm_run<false>(kind, dtype, rows, V, a, sm_same_phase(ops, 2, rows, es), stream);
}

extern "C" int kf_softmax_bwd(int kind, int dtype, int64_t rows, int64_t V, float scale, const void *y, int64_t ldy, const void *dy, int64_t lddy,
                              void *dx, int64_t lddx, void *stream) {
    const SmOperand ops[3] = {{"y", y, ldy}, {"dy", dy, lddy}, {"dx", dx, lddx}};
    const int rc = sm_check("kf_softmax_bwd", kind, dtype, rows, V, scale, ops, 3);
    if (rc != KF_OK) return rc;
    const int es = dtype_size(dtype);
    KF_REQUIRE(sm_disjoint(ops[2], ops[0], rows, V, es), KF_ERR_INVALID, "kf_softmax_bwd: dx overlaps y (no alias of dx and y is allowed)");
    KF_REQUIRE((dx == dy && lddx == lddy) || sm_disjoint(ops[2], ops[1], rows, V, es), KF_ERR_INVALID,
               "kf_softmax_bwd: dx overlaps dy (the only alias allowed is dx == dy with lddx == lddy)");
    if (rows == 0 || V == 0) return KF_OK;
    SmArgs a{y, dy, dx, rows, V, ldy, lddy, lddx, scale, 0.f};
    return sm_run<true>(kind, dtype, rows, V, a, sm_same_phase(ops, 3, rows, es), stream);
}
