// The router of a mixture-of-experts layer for gfx950: the top-k choice with its gates, and the auxiliary losses (load balance and
// z-loss), each with its backward. One wave owns a token's E <= 1024 logits in registers. With l = a row of logits:
//
//   kf_moe_router_fwd     ids = the first k positions of the stable descending order of l in kf_sort's key order (on the stored bits);
//                         s_j = softmax(l)[ids_j] or sigmoid(l[ids_j]); gate_j = s_j or s_j / (s_0 + ... + s_(k-1))
//   kf_moe_router_bwd     dl = the derivative of that gate contracted with dgate, every element of [T, E] written; l is re-read, the
//                         stored gate is not
//   kf_moe_aux_loss_fwd   p = softmax(l); L_bal = E / (T k) sum_e c_e mean_t p[t, e], c_e = offsets[e + 1] - offsets[e];
//                         L_z = mean_t lse_t^2; loss = balance_coef L_bal + z_coef L_z
//   kf_moe_aux_loss_bwd   dl[t, e] = dloss p_e (a_e - sum_u a_u p_u + z_t), a_e = balance_coef E c_e / (T^2 k), z_t = z_coef 2 lse_t / T
//
// Ownership, for every kernel here: with Vp = kPack16<T> a lane owns the spans lane, lane + 64, ... of Vp elements (NS of them at the
// most) and, of the E % Vp elements behind the last whole span, the element `lane`. With 16-byte aligned rows a span is one 16-byte
// access, otherwise the same lane moves the same Vp elements one by one: the arithmetic, its order and so the bits are the same.
//
// Selection: a logit's stored bits become an unsigned key of the same order (sort.hip's to_ordered), and (key + 1) << 10 | (1023 - index)
// is a composite that is unique in the row, larger for a larger key and, among equal keys, for the lower index; 0 stands for "not there".
// k rounds of: the lane's maximum, a wave maximum by an xor butterfly over the lanes that own anything, the winner struck out where it lives. The winner's value is
// recovered from its key, so every lane computes s_j and the running sum in the order j; lane j keeps choice j. No LDS, no barrier.
//
// The aux forward keeps the column sums of p and the sum of lse^2 in registers over the rows a wave walks; the block's four waves meet
// in LDS in wave order and one partial row of E + 1 floats goes to the workspace. The fold (one block of 1024 threads) gives each of
// its 16 waves a contiguous slice of the partial rows, summed in block order, then adds the slices in order: no atomics, one fixed
// order, bitwise reproducible.
#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// products and sums are written out: the packed and the element path must round alike, and the sums are defined term by term
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kRtBlock = 256;
constexpr int kRtWaves = kRtBlock / 64;
constexpr int64_t kRtMaxE = 1024;        // one wave holds the row: at most 16 values per lane (and one of the ragged tail)
constexpr int64_t kRtMaxK = 64;          // lane j keeps choice j
constexpr int kRtIdxBits = 10;           // an index < kRtMaxE
constexpr uint32_t kRtIdxMask = (1u << kRtIdxBits) - 1;
constexpr float kRtLog2e = 1.44269504088896340736f, kRtLn2 = 0.6931471805599453f;
constexpr int kAuxFoldThreads = 1024, kAuxFoldSlices = kAuxFoldThreads / 64;
constexpr unsigned kAuxBwdBlocks = 2048; // the aux backward's waves walk rows: a_e is read once per wave

// the stored bits of a dtype as a sortable key, and the composite (key + 1) << 10 | (1023 - index)
template <typename T> struct RtBits {
    using C = uint32_t;
    static constexpr uint32_t sign = 0x8000u, all = 0xffffu;
};
template <> struct RtBits<float> {
    using C = uint64_t;
    static constexpr uint32_t sign = 0x80000000u, all = 0xffffffffu;
};

template <typename T> __device__ __forceinline__ uint32_t rt_raw(const T &v) { return v.x; }
template <> __device__ __forceinline__ uint32_t rt_raw<float>(const float &v) { return __float_as_uint(v); }
template <typename T> __device__ __forceinline__ float rt_value(uint32_t raw) { return __uint_as_float(raw); }
template <> __device__ __forceinline__ float rt_value<bf16_t>(uint32_t raw) { return __uint_as_float(raw << 16); }
template <> __device__ __forceinline__ float rt_value<f16_t>(uint32_t raw) { return f16_to_f32(f16_t{(uint16_t)raw}); }

// sort.hip's to_ordered / from_ordered for a floating key
template <typename T> __device__ __forceinline__ uint32_t rt_ordered(uint32_t raw) {
    using B = RtBits<T>;
    return raw ^ ((raw & B::sign) ? B::all : B::sign);
}
template <typename T> __device__ __forceinline__ uint32_t rt_unordered(uint32_t ord) {
    using B = RtBits<T>;
    return ord ^ ((ord & B::sign) ? B::sign : B::all);
}

// N elements at a row position: one 16-byte access (VECL, N = kPack16<T>) or N element accesses
template <typename T, int N, bool VECL> struct alignas(VECL ? 16 : sizeof(T)) RtSpan { T e[N]; };

// f32 -> f16 of values the compiler cannot see through, as softmax.hip: it would fold the last operation into the conversion in one path only
template <typename T> __device__ __forceinline__ float rt_opaque(float v) {
    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float rt_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float rt_exp(float v) { return rt_exp2(v * kRtLog2e); }
__device__ __forceinline__ float rt_log(float v) { return __builtin_amdgcn_logf(v) * kRtLn2; }

// Wave reductions over the lanes that own something: `al` lanes (a power of two, uniform), an xor butterfly among them (the lanes
// beyond hold the identity), then lane 0's result for everyone. A row of 8 bf16 logits lives in one lane and needs no step at all.
__device__ __forceinline__ float rt_first(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ float rt_lane(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }
__device__ __forceinline__ float rt_wave_max(float v, int al) {
    for (int o = al >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return rt_first(v);
}
__device__ __forceinline__ float rt_wave_sum(float v, int al) {
    for (int o = al >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return rt_first(v);
}
__device__ __forceinline__ uint32_t rt_wave_maxc(uint32_t v, int al) {
    for (int o = al >> 1; o > 0; o >>= 1) {
        const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
        v = u > v ? u : v;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ uint64_t rt_wave_maxc(uint64_t v, int al) {
    for (int o = al >> 1; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const uint64_t u = ((uint64_t)hi << 32) | lo;
        v = u > v ? u : v;
    }
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// what a lane owns of a row of E elements: NS spans of Vp and one element of the tail; slot r < NS Vp is element i = r % Vp of span
// r / Vp, slot NS Vp the tail's
template <typename T, int NS> struct RtOwn {
    static constexpr int Vp = kPack16<T>, R = NS * Vp + 1;
    int lane, nb, t0, E, al;   // nb whole spans, the tail starts at t0; al: the lanes that own anything, rounded up to a power of two
    __device__ __forceinline__ RtOwn(int64_t E_, int lane_) : lane(lane_), nb((int)(E_ / Vp)), t0((int)(E_ / Vp) * Vp), E((int)E_) {
        const int lanes = max(min(nb, 64), E - t0);   // E >= 1: at least one
        al = 1;
        while (al < lanes) al <<= 1;
    }
    __device__ __forceinline__ bool span(int s) const { return s * 64 + lane < nb; }
    __device__ __forceinline__ bool tail() const { return t0 + lane < E; }
    __device__ __forceinline__ bool has(int r) const { return r < NS * Vp ? span(r / Vp) : tail(); }
    __device__ __forceinline__ int index(int r) const { return r < NS * Vp ? ((r / Vp) * 64 + lane) * Vp + r % Vp : t0 + lane; }
};

// the stored bits of the lane's slots (0 where it owns nothing)
template <typename T, int NS, bool VEC>
__device__ __forceinline__ void rt_load(const RtOwn<T, NS> &o, const T *row, uint32_t (&raw)[NS * kPack16<T> + 1]) {
    constexpr int Vp = kPack16<T>;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        RtSpan<T, Vp, VEC> v{};
        if (o.span(s)) v = *(const RtSpan<T, Vp, VEC> *)(row + (int64_t)(s * 64 + o.lane) * Vp);
#pragma unroll
        for (int i = 0; i < Vp; ++i) raw[s * Vp + i] = rt_raw<T>(v.e[i]);
    }
    T tl{};
    if (o.tail()) tl = row[o.t0 + o.lane];
    raw[NS * Vp] = rt_raw<T>(tl);
}

// one rounding per element, through the hardware converters (float_pack.h: pack16 and store_hw agree on every bit)
template <typename T, int NS, bool VEC>
__device__ __forceinline__ void rt_store(const RtOwn<T, NS> &o, T *row, const float (&f)[NS * kPack16<T> + 1]) {
    constexpr int Vp = kPack16<T>;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!o.span(s)) continue;
        float r[Vp];
#pragma unroll
        for (int i = 0; i < Vp; ++i) r[i] = rt_opaque<T>(f[s * Vp + i]);
        T *at = row + (int64_t)(s * 64 + o.lane) * Vp;
        if constexpr (VEC) {
            *(uint4 *)at = pack16<T>(r);
        } else {
#pragma unroll
            for (int i = 0; i < Vp; ++i) store_hw(at + i, r[i]);
        }
    }
    if (o.tail()) store_hw(row + o.t0 + o.lane, rt_opaque<T>(f[NS * Vp]));
}

// the row's softmax state: f <- e_v = exp(l_v - m) (0 where the lane owns nothing), m the row maximum, Z = sum_v e_v: the lane's slots in
// slot order, then the lanes by an xor butterfly
template <typename T, int NS>
__device__ __forceinline__ void rt_softmax_state(const RtOwn<T, NS> &o, const uint32_t (&raw)[NS * kPack16<T> + 1], float (&f)[NS * kPack16<T> + 1],
                                                 float &m, float &Z) {
    constexpr int R = NS * kPack16<T> + 1;
    m = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        f[r] = rt_value<T>(raw[r]);
        if (o.has(r)) m = fmaxf(m, f[r]);
    }
    m = rt_wave_max(m, o.al);
    Z = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        f[r] = o.has(r) ? rt_exp(f[r] - m) : 0.f;
        Z += f[r];
    }
    Z = rt_wave_sum(Z, o.al);
}

template <int SCORE> __device__ __forceinline__ float rt_score(float l, float m, float Z) {
    if constexpr (SCORE == KF_MOE_SCORE_SOFTMAX) return rt_exp(l - m) / Z;
    else return 1.f / (1.f + rt_exp(-l));
}

// the wave of a thread and the first row it takes; rows step by `step`
__device__ __forceinline__ int rt_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

struct RtArgs {
    const void *logits, *dgate;
    const int64_t *ids_in;
    int64_t *ids;
    void *gate, *dlogits;
    int64_t T, E, k, ldl, ldg, lddg, lddl;
    int normalize;
};

// ---- router forward ------------------------------------------------------------------------------------------------------------------------
template <typename T, int NS, bool VEC, int SCORE>
__global__ __launch_bounds__(kRtBlock) void rt_fwd_kernel(const RtArgs a) {
    using C = typename RtBits<T>::C;
    constexpr int R = NS * kPack16<T> + 1;
    const int64_t t = (int64_t)blockIdx.x * kRtWaves + rt_wave();
    if (t >= a.T) return;
    const int lane = threadIdx.x & 63;
    const RtOwn<T, NS> o(a.E, lane);
    uint32_t raw[R];
    rt_load<T, NS, VEC>(o, (const T *)a.logits + t * a.ldl, raw);
    float m = 0.f, Z = 1.f;
    if constexpr (SCORE == KF_MOE_SCORE_SOFTMAX) {
        float f[R];
        rt_softmax_state<T, NS>(o, raw, f, m, Z);
    }
    C comp[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        comp[r] = o.has(r) ? (((C)rt_ordered<T>(raw[r]) + 1) << kRtIdxBits) | (C)(kRtIdxMask - (uint32_t)o.index(r)) : (C)0;
    const int k = (int)a.k;
    float mine = 0.f, S = 0.f;
    int64_t id = 0;
    for (int j = 0; j < k; ++j) {   // k <= E: every round finds an element
        C best = comp[0];
#pragma unroll
        for (int r = 1; r < R; ++r) best = comp[r] > best ? comp[r] : best;
        best = rt_wave_maxc(best, o.al);
#pragma unroll
        for (int r = 0; r < R; ++r) comp[r] = comp[r] == best ? (C)0 : comp[r];
        const float l = rt_value<T>(rt_unordered<T>((uint32_t)(best >> kRtIdxBits) - 1u));
        const float s = rt_score<SCORE>(l, m, Z);
        S += s;
        if (lane == j) {
            mine = s;
            id = (int64_t)(kRtIdxMask - ((uint32_t)best & kRtIdxMask));
        }
    }
    if (lane < k) {
        a.ids[t * a.k + lane] = id;
        store_hw((T *)a.gate + t * a.ldg + lane, rt_opaque<T>(a.normalize ? mine / S : mine));
    }
}

// ---- router backward -----------------------------------------------------------------------------------------------------------------------
// dl_e = base_e (G_e - sub), G_e = the sum in the order j of c_j over the pairs with ids_j == e:
//   softmax             base_e = p_e   c_j = dgate_j                  sub = sum_j dgate_j s_j
//   softmax, normalize  base_e = p_e   c_j = (dgate_j - D) / S        sub = 0       D = sum_j dgate_j s_j / S  (the sum of c_j s_j vanishes)
//   sigmoid             base_e = 1     c_j = dgate_j s_j (1 - s_j)    sub = 0       (1 - s_j = 1 / (1 + exp(l_j)), without cancellation)
//   sigmoid, normalize  base_e = 1     c_j = (dgate_j - D) / S s_j (1 - s_j)
// A pair whose id lies outside [0, E) is in no sum. The sigmoid form does not read the row, only the k chosen logits.
template <typename T, int NS, bool VEC, int SCORE>
__global__ __launch_bounds__(kRtBlock) void rt_bwd_kernel(const RtArgs a) {
    constexpr int R = NS * kPack16<T> + 1;
    const int64_t t = (int64_t)blockIdx.x * kRtWaves + rt_wave();
    if (t >= a.T) return;
    const int lane = threadIdx.x & 63;
    const RtOwn<T, NS> o(a.E, lane);
    const T *row = (const T *)a.logits + t * a.ldl;
    float f[R];
    float m = 0.f, Z = 1.f;
    if constexpr (SCORE == KF_MOE_SCORE_SOFTMAX) {
        uint32_t raw[R];
        rt_load<T, NS, VEC>(o, row, raw);
        rt_softmax_state<T, NS>(o, raw, f, m, Z);
    }
    const int k = (int)a.k;
    // lane j: pair j
    int idj = -1;
    float dg = 0.f, s = 0.f, q = 0.f;
    if (lane < k) {
        const int64_t id = a.ids_in[t * a.k + lane];
        if (id >= 0 && id < a.E) {
            idj = (int)id;
            dg = load_f32((const T *)a.dgate + t * a.lddg + lane);
            const float l = load_f32(row + id);
            s = rt_score<SCORE>(l, m, Z);
            if constexpr (SCORE == KF_MOE_SCORE_SIGMOID) q = 1.f / (1.f + rt_exp(l));
        }
    }
    float S = 1.f, D = 0.f;
    if (a.normalize) {
        S = 0.f;
        for (int j = 0; j < k; ++j) {
            if (__builtin_amdgcn_readlane(idj, j) >= 0) S += rt_lane(s, j);
        }
    }
    if (a.normalize || SCORE == KF_MOE_SCORE_SOFTMAX) {
        const float w = a.normalize ? dg * (s / S) : dg * s;
        for (int j = 0; j < k; ++j) {
            if (__builtin_amdgcn_readlane(idj, j) >= 0) D += rt_lane(w, j);
        }
    }
    float c = a.normalize ? (dg - D) / S : dg;
    if constexpr (SCORE == KF_MOE_SCORE_SIGMOID) c = c * s * q;
    const float sub = (SCORE == KF_MOE_SCORE_SOFTMAX && !a.normalize) ? D : 0.f;
    float G[R];
#pragma unroll
    for (int r = 0; r < R; ++r) G[r] = 0.f;
    for (int j = 0; j < k; ++j) {
        const int ij = __builtin_amdgcn_readlane(idj, j);
        const float cj = rt_lane(c, j);
        if (ij < 0) continue;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o.index(r) == ij) G[r] += cj;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if constexpr (SCORE == KF_MOE_SCORE_SOFTMAX) G[r] = (f[r] / Z) * (G[r] - sub);
    }
    rt_store<T, NS, VEC>(o, (T *)a.dlogits + t * a.lddl, G);
}

// ---- auxiliary losses ----------------------------------------------------------------------------------------------------------------------
struct AuxArgs {
    const void *logits;
    const int64_t *offsets;
    const float *dloss;
    float *part, *loss, *parts;
    void *dlogits;
    int64_t T, E, ldl, lddl;
    int nblocks;                     // partial rows of E + 1 floats in `part`
    float balance_coef, z_coef;
    float bal_scale, inv_T;          // E / (T^2 k), 1 / T
    float a_scale, z_scale;          // balance_coef E / (T^2 k), z_coef 2 / T
};

template <typename T, int NS, bool VEC>
__global__ __launch_bounds__(kRtBlock) void aux_fwd_kernel(const AuxArgs a) {
    constexpr int R = NS * kPack16<T> + 1;
    __shared__ float red[kRtWaves][kRtMaxE + 1];
    const int wave = rt_wave(), lane = threadIdx.x & 63;
    const RtOwn<T, NS> o(a.E, lane);
    float col[R];
#pragma unroll
    for (int r = 0; r < R; ++r) col[r] = 0.f;
    float zsum = 0.f;
    for (int64_t t = (int64_t)blockIdx.x * kRtWaves + wave; t < a.T; t += (int64_t)gridDim.x * kRtWaves) {
        uint32_t raw[R];
        float f[R], m, Z;
        rt_load<T, NS, VEC>(o, (const T *)a.logits + t * a.ldl, raw);
        rt_softmax_state<T, NS>(o, raw, f, m, Z);
        const float inv = 1.f / Z, lse = m + rt_log(Z);
#pragma unroll
        for (int r = 0; r < R; ++r) col[r] += f[r] * inv;
        zsum += lse * lse;
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (o.has(r)) red[wave][o.index(r)] = col[r];
    if (lane == 0) red[wave][a.E] = zsum;
    __syncthreads();
    float *out = a.part + (int64_t)blockIdx.x * (a.E + 1);
    for (int e = threadIdx.x; e <= (int)a.E; e += kRtBlock) {
        float v = red[0][e];
#pragma unroll
        for (int w = 1; w < kRtWaves; ++w) v += red[w][e];
        out[e] = v;
    }
}

// one block: 64 columns at a time, wave w the partial rows of slice w in block order, then the slices in order. Column E is the sum of lse^2.
__global__ __launch_bounds__(kAuxFoldThreads) void aux_fold_kernel(const AuxArgs a) {
    __shared__ float red[kAuxFoldSlices][64];
    const int wave = rt_wave(), lane = threadIdx.x & 63;
    const int E = (int)a.E, per = (a.nblocks + kAuxFoldSlices - 1) / kAuxFoldSlices;
    const int b0 = wave * per, b1 = min(a.nblocks, b0 + per);
    float bal = 0.f, zs = 0.f;   // wave 0
    for (int c0 = 0; c0 <= E; c0 += 64) {
        const int e = c0 + lane;
        float v = 0.f;
        if (e <= E) {
#pragma unroll 8
            for (int b = b0; b < b1; ++b) v += a.part[(int64_t)b * (E + 1) + e];   // (unrolled: the loads of eight partial rows are in flight together)
        }
        red[wave][lane] = v;
        __syncthreads();
        if (wave == 0 && e <= E) {
            float tot = red[0][lane];
#pragma unroll
            for (int w = 1; w < kAuxFoldSlices; ++w) tot += red[w][lane];
            if (e < E) bal += (float)(a.offsets[e + 1] - a.offsets[e]) * tot;
            else zs = tot;
        }
        __syncthreads();
    }
    if (wave != 0) return;
    bal = rt_wave_sum(bal, 64);
    zs = rt_wave_sum(zs, 64);   // one lane holds it, the others +0
    if (lane == 0) {
        const float l_bal = bal * a.bal_scale, l_z = zs * a.inv_T;
        a.loss[0] = a.balance_coef * l_bal + a.z_coef * l_z;
        if (a.parts) {
            a.parts[0] = l_bal;
            a.parts[1] = l_z;
        }
    }
}

template <typename T, int NS, bool VEC>
__global__ __launch_bounds__(kRtBlock) void aux_bwd_kernel(const AuxArgs a) {
    constexpr int R = NS * kPack16<T> + 1;
    const int wave = rt_wave(), lane = threadIdx.x & 63;
    const RtOwn<T, NS> o(a.E, lane);
    const float dloss = *a.dloss;
    float ae[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ae[r] = o.has(r) ? a.a_scale * (float)(a.offsets[o.index(r) + 1] - a.offsets[o.index(r)]) : 0.f;
    for (int64_t t = (int64_t)blockIdx.x * kRtWaves + wave; t < a.T; t += (int64_t)gridDim.x * kRtWaves) {
        uint32_t raw[R];
        float f[R], m, Z;
        rt_load<T, NS, VEC>(o, (const T *)a.logits + t * a.ldl, raw);
        rt_softmax_state<T, NS>(o, raw, f, m, Z);
        const float zt = a.z_scale * (m + rt_log(Z));
        float A = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            f[r] = f[r] / Z;
            A += ae[r] * f[r];
        }
        A = rt_wave_sum(A, o.al);
#pragma unroll
        for (int r = 0; r < R; ++r) f[r] = dloss * f[r] * ((ae[r] - A) + zt);
        rt_store<T, NS, VEC>(o, (T *)a.dlogits + t * a.lddl, f);
    }
}

// ---- the host side -------------------------------------------------------------------------------------------------------------------------
struct RtOperand {
    const char *name;
    const void *p;
    int64_t ld, extent;
};

bool rt_dtype_ok(int dtype) { return dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16; }

// dtype and extents, the regime, then the row operands: null, pitch, alignment
int rt_check(const char *who, int dtype, int64_t T, int64_t E, int64_t k, const RtOperand *ops, int nops) {
    KF_REQUIRE(rt_dtype_ok(dtype), KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(T >= 0 && E >= 1 && k >= 1, KF_ERR_INVALID, "%s: bad extents T %lld E %lld k %lld (T >= 0; E, k >= 1)", who, (long long)T, (long long)E,
               (long long)k);
    KF_REQUIRE(E <= kRtMaxE && k <= std::min(E, kRtMaxK), KF_ERR_UNSUPPORTED, "%s: E %lld k %lld: one wave holds a token's row (E <= %lld, k <= min(E, %lld))", who,
               (long long)E, (long long)k, (long long)kRtMaxE, (long long)kRtMaxK);
    KF_REQUIRE(T <= INT64_MAX / E, KF_ERR_INVALID, "%s: T E = %lld x %lld (or T k) overflows", who, (long long)T, (long long)E);
    const int es = dtype_size(dtype);
    for (int i = 0; i < nops; ++i) {
        KF_REQUIRE(ops[i].p, KF_ERR_INVALID, "%s: null %s", who, ops[i].name);
        KF_REQUIRE(ops[i].ld >= ops[i].extent, KF_ERR_INVALID, "%s: leading dimension of %s %lld < %lld", who, ops[i].name, (long long)ops[i].ld,
                   (long long)ops[i].extent);
        KF_REQUIRE((uintptr_t)ops[i].p % es == 0, KF_ERR_INVALID, "%s: %s not aligned to its element size", who, ops[i].name);
    }
    return KF_OK;
}
int rt_check_ptr(const char *who, const char *name, const void *p, int align) {
    KF_REQUIRE(p, KF_ERR_INVALID, "%s: null %s", who, name);
    KF_REQUIRE((uintptr_t)p % align == 0, KF_ERR_INVALID, "%s: %s not aligned to %d bytes", who, name, align);
    return KF_OK;
}

// the 16-byte path: every [T, E] operand 16-byte aligned with a pitch in whole packs (the ragged tail moves by elements in both paths)
bool rt_vec(int dtype, const void *a, int64_t lda, const void *b, int64_t ldb) {
    const int vp = 16 / dtype_size(dtype);
    bool ok = (uintptr_t)a % 16 == 0 && lda % vp == 0;
    if (b) ok = ok && (uintptr_t)b % 16 == 0 && ldb % vp == 0;
    return ok;
}

unsigned rt_grid(int64_t T) { return (unsigned)((T + kRtWaves - 1) / kRtWaves); }

// f(T{}, NS, VEC): NS the spans a lane owns at the most, the smallest of 1, 2, 4 that covers E
template <typename F> int rt_dispatch(int dtype, int64_t E, bool vec, F &&f) {
    return with_dtype(dtype, [&](auto t) {
        using Tp = decltype(t);
        const int64_t spans = (E / kPack16<Tp> + 63) / 64;
        return with_flags(
            [&](auto VEC) {
                if (spans <= 1) return f(Tp{}, std::integral_constant<int, 1>{}, VEC);
                if (spans <= 2) return f(Tp{}, std::integral_constant<int, 2>{}, VEC);
                if constexpr (sizeof(Tp) == 4) return f(Tp{}, std::integral_constant<int, 4>{}, VEC);
                else return (int)KF_ERR_UNSUPPORTED;   // (16-bit rows of E <= 1024 are two spans at the most)
            },
            vec);
    });
}

int aux_blocks(int64_t T, int64_t E) {
    const int64_t cap = E <= 256 ? 512 : 256;   // the fold reads cap (E + 1) floats in one block
    return (int)std::min<int64_t>((T + kRtWaves - 1) / kRtWaves, cap);
}
size_t aux_bytes(int64_t T, int64_t E) { return ((size_t)aux_blocks(T, E) * (size_t)(E + 1) * sizeof(float) + 15) / 16 * 16; }

int router_run(const char *who, bool bwd, int dtype, int64_t T, int64_t E, int64_t k, int score, int normalize, const void *logits, int64_t ldl,
               const int64_t *ids, void *gate, int64_t ldg, void *dlogits, int64_t lddl, void *stream) {
    const RtOperand ops[3] = {{"logits", logits, ldl, E}, {bwd ? "dgate" : "gate", gate, ldg, k}, {"dlogits", dlogits, lddl, E}};
    int rc = rt_check(who, dtype, T, E, k, ops, bwd ? 3 : 2);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(score == KF_MOE_SCORE_SOFTMAX || score == KF_MOE_SCORE_SIGMOID, KF_ERR_INVALID, "%s: score %d is not KF_MOE_SCORE_SOFTMAX or KF_MOE_SCORE_SIGMOID",
               who, score);
    KF_REQUIRE(normalize == 0 || normalize == 1, KF_ERR_INVALID, "%s: normalize %d is not 0 or 1", who, normalize);
    if ((rc = rt_check_ptr(who, "ids", ids, 8)) != KF_OK) return rc;
    if (T == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    KF_PROF(bwd ? "moe_router_bwd" : "moe_router_fwd", st);
    RtArgs a{};
    a.logits = logits;
    a.T = T, a.E = E, a.k = k, a.ldl = ldl, a.normalize = normalize;
    if (bwd) a.ids_in = ids, a.dgate = gate, a.lddg = ldg, a.dlogits = dlogits, a.lddl = lddl;
    else a.ids = const_cast<int64_t *>(ids), a.gate = gate, a.ldg = ldg;
    const bool vec = bwd ? rt_vec(dtype, logits, ldl, dlogits, lddl) : rt_vec(dtype, logits, ldl, nullptr, 0);
    return rt_dispatch(dtype, E, vec, [&](auto t, auto NS, auto VEC) {
        using Tp = decltype(t);
        return with_flags(
            [&](auto SIG) {
                constexpr int SC = SIG ? KF_MOE_SCORE_SIGMOID : KF_MOE_SCORE_SOFTMAX;
                if (bwd) return launch(rt_bwd_kernel<Tp, NS, VEC, SC>, rt_grid(T), kRtBlock, 0, st, a);
                return launch(rt_fwd_kernel<Tp, NS, VEC, SC>, rt_grid(T), kRtBlock, 0, st, a);
            },
            score == KF_MOE_SCORE_SIGMOID);
    });
}

// what the two aux entries share: the checks, and the scalars of the formulas (in double, rounded once)
int aux_prepare(const char *who, int dtype, int64_t T, int64_t E, int64_t k, const void *logits, int64_t ldl, const int64_t *offsets, float balance_coef,
                float z_coef, const void *dlogits, int64_t lddl, bool bwd, AuxArgs &a) {
    const RtOperand ops[2] = {{"logits", logits, ldl, E}, {"dlogits", dlogits, lddl, E}};
    int rc = rt_check(who, dtype, T, E, k, ops, bwd ? 2 : 1);
    if (rc != KF_OK) return rc;
    if ((rc = rt_check_ptr(who, "offsets", offsets, 8)) != KF_OK) return rc;
    a = AuxArgs{};
    a.logits = logits, a.offsets = offsets, a.T = T, a.E = E, a.ldl = ldl, a.lddl = lddl;
    a.dlogits = const_cast<void *>(dlogits);
    a.balance_coef = balance_coef, a.z_coef = z_coef;
    if (T > 0) {
        const double bal = (double)E / ((double)T * (double)T * (double)k);
        a.bal_scale = (float)bal, a.inv_T = (float)(1.0 / (double)T);
        a.a_scale = (float)((double)balance_coef * bal), a.z_scale = (float)((double)z_coef * 2.0 / (double)T);
    }
    return KF_OK;
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_moe_router_fwd(int dtype, int64_t T, int64_t E, int64_t k, int score, int normalize, const void *logits, int64_t ldl, int64_t *ids, void *gate,
                                 int64_t ldg, void *stream) {
    return router_run("kf_moe_router_fwd", false, dtype, T, E, k, score, normalize, logits, ldl, ids, gate, ldg, nullptr, 0, stream);
}

extern "C" int kf_moe_router_bwd(int dtype, int64_t T, int64_t E, int64_t k, int score, int normalize, const void *logits, int64_t ldl, const int64_t *ids,
                                 const void *dgate, int64_t lddg, void *dlogits, int64_t lddl, void *stream) {
    return router_run("kf_moe_router_bwd", true, dtype, T, E, k, score, normalize, logits, ldl, ids, const_cast<void *>(dgate), lddg, dlogits, lddl, stream);
}

extern "C" int kf_moe_aux_loss_workspace_bytes(int64_t T, int64_t E, size_t *bytes) {
    const char *who = "kf_moe_aux_loss_workspace_bytes";
    KF_REQUIRE(T >= 0 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld E %lld (T >= 0; E >= 1)", who, (long long)T, (long long)E);
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null bytes", who);
    KF_REQUIRE(E <= kRtMaxE, KF_ERR_UNSUPPORTED, "%s: E %lld: one wave holds a token's row (E <= %lld)", who, (long long)E, (long long)kRtMaxE);
    *bytes = aux_bytes(T, E);
    return KF_OK;
}

extern "C" int kf_moe_aux_loss_fwd(int dtype, int64_t T, int64_t E, int64_t k, const void *logits, int64_t ldl, const int64_t *offsets, float balance_coef,
                                   float z_coef, float *loss, float *parts, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_moe_aux_loss_fwd";
    AuxArgs a;
    int rc = aux_prepare(who, dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, nullptr, 0, false, a);
    if (rc != KF_OK) return rc;
    if ((rc = rt_check_ptr(who, "loss", loss, 4)) != KF_OK) return rc;
    KF_REQUIRE((uintptr_t)parts % 4 == 0, KF_ERR_INVALID, "%s: parts not aligned to 4 bytes", who);
    KF_REQUIRE((uintptr_t)workspace % 16 == 0, KF_ERR_INVALID, "%s: workspace not 16-byte aligned", who);
    const size_t need = aux_bytes(T, E);
    KF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), KF_ERR_INVALID, "%s: workspace too small or missing: %zu bytes required, got %zu", who, need,
               workspace ? workspace_bytes : (size_t)0);
    if (T == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    a.part = (float *)workspace, a.loss = loss, a.parts = parts, a.nblocks = aux_blocks(T, E);
    {
        KF_PROF("moe_aux_fwd", st);
        rc = rt_dispatch(dtype, E, rt_vec(dtype, logits, ldl, nullptr, 0), [&](auto t, auto NS, auto VEC) {
            return launch(aux_fwd_kernel<decltype(t), NS, VEC>, (unsigned)a.nblocks, kRtBlock, 0, st, a);
        });
        if (rc != KF_OK) return rc;
    }
    KF_PROF("moe_aux_fold", st);
    return launch(aux_fold_kernel, 1u, kAuxFoldThreads, 0, st, a);
}

extern "C" int kf_moe_aux_loss_bwd(int dtype, int64_t T, int64_t E, int64_t k, const void *logits, int64_t ldl, const int64_t *offsets, float balance_coef,
                                   float z_coef, const float *dloss, void *dlogits, int64_t lddl, void *stream) {
    const char *who = "kf_moe_aux_loss_bwd";
    AuxArgs a;
    int rc = aux_prepare(who, dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, dlogits, lddl, true, a);
    if (rc != KF_OK) return rc;
    if ((rc = rt_check_ptr(who, "dloss", dloss, 4)) != KF_OK) return rc;
    if (T == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    a.dloss = dloss;
    KF_PROF("moe_aux_bwd", st);
    const unsigned grid = std::min(rt_grid(T), kAuxBwdBlocks);
    return rt_dispatch(dtype, E, rt_vec(dtype, logits, ldl, dlogits, lddl), [&](auto t, auto NS, auto VEC) {
        return launch(aux_bwd_kernel<decltype(t), NS, VEC>, grid, kRtBlock, 0, st, a);
    });
}
