// Token routing of a mixture-of-experts layer for gfx950, entirely on the device: the plan (a stable sort of the (token, choice) pairs by
// expert, as two 32-bit tables and the experts' row offsets), the gate (the chosen probabilities, optionally renormalised), the dispatch
// (a row gather by the plan) and the weighted combine, each with its backward. With n = T k and pair p = t k + j:
//
//   kf_moe_plan          key_p = ids[p] if 0 <= ids[p] < E else E; row_pair = the stable ascending order of the pairs by key, pair_row its
//                        inverse, offsets[e] = the number of keys < e
//   kf_moe_gate_fwd      gate[t, j] = p[t, ids[t, j]] (/ their sum over j); kf_moe_gate_bwd scatters back into a zeroed dp [T, E]
//   kf_moe_dispatch      xs[r, :] = x[row_pair[r] / k, :]
//   kf_moe_combine       y[t, :] = sum_j gate[t, j] ys[pair_row[t, j], :]   (no gate: the backward of the dispatch)
//   kf_moe_combine_bwd   dys[pair_row[t, j], :] = gate[t, j] dy[t, :] and dgate[t, j] = dy[t, :] . ys[pair_row[t, j], :], in one pass
//
// Because the inverse table is at hand, every backward is a gather-sum or a scatter of whole rows to rows that the permutation names
// exactly once: no sort, no atomics, a fixed order of every sum, bitwise reproducible. Nothing synchronises or allocates, and no extent
// reaches the host: n_valid is read from the device (offsets + E), so a layer can be captured in a graph.
//
// Every index a kernel reads is range-checked where it is read: an expert id outside [0, E) is a dropped pair, a table entry outside
// [0, n) names no row. Malformed tables change what is computed, never what memory is touched.
//
// The row movers are HBM streams. Regimes, from cols alone: cols <= 1024 one wave per row (four rows per 256-thread block), longer rows
// one block per row. A lane owns the spans lane, lane + G, ... of kPack16<T> elements and, for the cols % kPack16<T> elements behind
// them, the element `lane`; with 16-byte aligned bases and cols and every leading dimension a multiple of the pack a span is one
// 16-byte access, otherwise the same lanes move the same elements one by one, with the same arithmetic and the same bits. Table entries
// and gates are uniform per wave: the combine and its backward read the first kMoeK of a token once, in front of the span walk and of
// every store (scalar loads of the entries; behind a store the compiler would re-read them per span with vector loads and wait for each),
// and issue the kMoeK row loads of a span before the first is used. Pairs beyond kMoeK: the combine takes them one at a time, entry, gate
// and row read per span; the backward walks dy again per chunk of kMoeK.
#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// products and sums are written out: the packed and the element path must round alike, and the sums are defined term by term
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kMoeBlock = 256;
constexpr int kMoeWaves = kMoeBlock / 64;
constexpr int64_t kMoeWaveMax = 1024;   // cols up to this: one wave per row
constexpr int kMoeK = 8;                // pairs of a token whose rows are in flight together
constexpr int kMoeU = 4;                // spans a lane of the dispatch loads before it stores

// N elements at a row position: one 16-byte access (VECL, N = kPack16<T>) or N element accesses. The raw bits move rows that are copied.
template <typename T, int N, bool VECL> struct alignas(VECL ? 16 : sizeof(T)) MoeSpan { T e[N]; };

template <typename T, int N, bool VECL>
__device__ __forceinline__ void moe_unpack(const MoeSpan<T, N, VECL> &s, float (&f)[N]) {
    if constexpr (VECL) {
        uint4 u;
        __builtin_memcpy(&u, &s, 16);
        unpack16<T>(u, f);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) f[i] = load_f32(&s.e[i]);
    }
}
// f32 -> f16 of values the compiler cannot see through, as softmax.hip: it would fold the last operation into the conversion in one path only
template <typename T> __device__ __forceinline__ float moe_opaque(float v) {
    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(v));
    return v;
}
template <typename T, int N, bool VECL>
__device__ __forceinline__ MoeSpan<T, N, VECL> moe_pack(const float (&f)[N]) {
    MoeSpan<T, N, VECL> s;
    float r[N];
#pragma unroll
    for (int i = 0; i < N; ++i) r[i] = moe_opaque<T>(f[i]);
    if constexpr (VECL) {
        const uint4 u = pack16<T>(r);
        __builtin_memcpy(&s, &u, 16);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) store_hw(&s.e[i], r[i]);
    }
    return s;
}
template <typename T, int N, bool VECL> __device__ __forceinline__ MoeSpan<T, N, VECL> moe_ld(const T *p) { return *(const MoeSpan<T, N, VECL> *)p; }
template <typename T, int N, bool VECL> __device__ __forceinline__ void moe_st(T *p, const MoeSpan<T, N, VECL> &s) { *(MoeSpan<T, N, VECL> *)p = s; }

// the row and the lane of a thread: G = 64 four rows per block (whole waves leave), G = kMoeBlock one row per block
template <int G> __device__ __forceinline__ bool moe_row_of(int64_t rows, int64_t &row, int &lane) {
    if constexpr (G == 64) {
        row = (int64_t)blockIdx.x * kMoeWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        lane = threadIdx.x & 63;
        return row < rows;
    } else {
        row = blockIdx.x;
        lane = threadIdx.x;
        return true;
    }
}

__device__ __forceinline__ int64_t moe_live_rows(const int64_t *n_valid, int64_t n) {
    if (!n_valid) return n;
    const int64_t v = *n_valid;
    return v < 0 ? 0 : v > n ? n : v;
}

// ---- plan ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMoeBlock) void moe_keys_kernel(const int64_t *ids, int64_t n, int64_t E, int64_t *keys) {
    const int64_t p = (int64_t)blockIdx.x * kMoeBlock + threadIdx.x;
    if (p >= n) return;
    const int64_t id = ids[p];
    keys[p] = id >= 0 && id < E ? id : E;
}
// pos: the sort's positions, a permutation of [0, n); checked all the same before it is used as an index
__global__ __launch_bounds__(kMoeBlock) void moe_tables_kernel(const int64_t *pos, int64_t n, int32_t *row_pair, int32_t *pair_row) {
    const int64_t r = (int64_t)blockIdx.x * kMoeBlock + threadIdx.x;
    if (r >= n) return;
    const int64_t p = pos[r];
    row_pair[r] = (int32_t)p;
    if (p >= 0 && p < n) pair_row[p] = (int32_t)r;
}

// ---- gate ------------------------------------------------------------------------------------------------------------------------------------
struct MoeGate {
    const int64_t *ids;
    const void *p, *gate, *dgate;
    void *out;                 // forward: gate; backward: dp
    int64_t T, k, E, ldp, ldg, lddg, ldo;
    int normalize;
};

// the chosen probability of pair (t, j), 0 for a dropped pair; id: the expert, or -1
template <typename T> __device__ __forceinline__ float moe_chosen(const MoeGate &a, const T *prow, const int64_t *ids, int64_t j, int64_t &id) {
    id = ids[j];
    if (id < 0 || id >= a.E) {
        id = -1;
        return 0.f;
    }
    return load_f32(prow + id);
}

// one thread per token: k is small and the row of p is read at k places
template <typename T>
__global__ __launch_bounds__(kMoeBlock) void moe_gate_fwd_kernel(const MoeGate a) {
    const int64_t t = (int64_t)blockIdx.x * kMoeBlock + threadIdx.x;
    if (t >= a.T) return;
    const T *prow = (const T *)a.p + t * a.ldp;
    const int64_t *ids = a.ids + t * a.k;
    T *g = (T *)a.out + t * a.ldo;
    int64_t id;
    float S = 0.f;
    if (a.normalize)
        for (int64_t j = 0; j < a.k; ++j) S += moe_chosen(a, prow, ids, j, id);
    for (int64_t j = 0; j < a.k; ++j) {
        const float s = moe_chosen(a, prow, ids, j, id);
        store_hw(g + j, moe_opaque<T>(a.normalize ? s / S : s));
    }
}

// one wave per token, the lanes across the E columns of dp: a column collects the pairs that chose it, in the order j
template <typename T>
__global__ __launch_bounds__(kMoeBlock) void moe_gate_bwd_kernel(const MoeGate a) {
    int64_t t;
    int lane;
    if (!moe_row_of<64>(a.T, t, lane)) return;
    const T *prow = (const T *)a.p + t * a.ldp, *g = (const T *)a.gate + t * a.ldg, *dg = (const T *)a.dgate + t * a.lddg;
    const int64_t *ids = a.ids + t * a.k;
    T *dp = (T *)a.out + t * a.ldo;
    int64_t id;
    float S = 0.f, dot = 0.f;
    if (a.normalize)
        for (int64_t j = 0; j < a.k; ++j) {
            S += moe_chosen(a, prow, ids, j, id);
            if (id >= 0) dot += load_f32(dg + j) * load_f32(g + j);
        }
    for (int64_t e = lane; e < a.E; e += 64) {
        float v = 0.f;
        for (int64_t j = 0; j < a.k; ++j) {
            id = ids[j];
            if (id != e) continue;
            const float d = load_f32(dg + j);
            v += a.normalize ? (d - dot) / S : d;
        }
        store_hw(dp + e, moe_opaque<T>(v));
    }
}

// ---- dispatch --------------------------------------------------------------------------------------------------------------------------------
struct MoeMove {
    const int32_t *table;      // row_pair (dispatch), pair_row (combine)
    const int64_t *n_valid;
    const void *gate, *src, *dy;   // combine: ys; combine_bwd: ys and dy
    void *dst, *dgate;             // combine: y; combine_bwd: dys and dgate
    int64_t T, k, n, cols, ldg, lds, lddy, ldd, lddg;
};

template <typename T, int N, bool VECL>
__device__ __forceinline__ void moe_copy_spans(const T *src, T *dst, int64_t first, int64_t count, int64_t step, bool ok) {
    using S = MoeSpan<T, N, VECL>;
    for (int64_t c = first; c < count; c += kMoeU * step) {
        S v[kMoeU];
#pragma unroll
        for (int u = 0; u < kMoeU; ++u)
            if (c + u * step < count) v[u] = ok ? moe_ld<T, N, VECL>(src + (c + u * step) * N) : S{};
#pragma unroll
        for (int u = 0; u < kMoeU; ++u)
            if (c + u * step < count) moe_st<T, N, VECL>(dst + (c + u * step) * N, v[u]);
    }
}

template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kMoeBlock) void moe_dispatch_kernel(const MoeMove a) {
    constexpr int Vp = kPack16<T>;
    int64_t r;
    int lane;
    if (!moe_row_of<G>(a.n, r, lane)) return;
    const int64_t p = a.table[r];
    const bool ok = p >= 0 && p < a.n;   // anything else names no token: the row is +0 and nothing is read
    // p, k < 2^31: a 32-bit division (it stands in front of every load of the row)
    const T *src = (const T *)a.src + (int64_t)(ok ? (uint32_t)p / (uint32_t)a.k : 0u) * a.lds;
    T *dst = (T *)a.dst + r * a.ldd;
    const int64_t nb = a.cols / Vp, t0 = nb * Vp;
    moe_copy_spans<T, Vp, VEC>(src, dst, lane, nb, G, ok);
    if (t0 + lane < a.cols) moe_copy_spans<T, 1, false>(src + t0, dst + t0, lane, a.cols - t0, G, ok);
}

// ---- combine ---------------------------------------------------------------------------------------------------------------------------------
// the kMoeK pairs j0 .. of a token (the combine holds the first kMoeK): row = pair_row (-1 for a pair that is past k or outside [0, live): neither its row nor its gate is
// read), gv = its gate (1 without gates)
template <typename T>
__device__ __forceinline__ void moe_chunk(const int32_t *pr, const T *g, int64_t j0, int64_t k, int32_t live, int32_t (&row)[kMoeK], float (&gv)[kMoeK]) {
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj) {
        row[jj] = -1;
        gv[jj] = 1.f;
        if (j0 + jj < k) {
            // uniform per wave, and told so: behind a store to y the compiler reads them with vector loads
            const int32_t r = __builtin_amdgcn_readfirstlane(pr[j0 + jj]);
            if (r >= 0 && r < live) {
                row[jj] = r;
                if (g) gv[jj] = load_f32(g + j0 + jj);
            }
        }
    }
}
// acc += sum over the chunk's pairs of gate_j ys[row_j, col ..] in the order j: every row load is issued before the first is used
template <typename T, int N, bool VECL>
__device__ __forceinline__ void moe_add_chunk(const MoeMove &a, int64_t col, const int32_t (&row)[kMoeK], const float (&gv)[kMoeK], float (&acc)[N]) {
    MoeSpan<T, N, VECL> v[kMoeK];
    // the row offsets are formed here, per span, from the 32-bit entries (kept opaque), as in the backward: hoisted out of the walk they spill
    // scalar registers
    int32_t rw[kMoeK];
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj) {
        rw[jj] = row[jj];
        asm volatile("" : "+s"(rw[jj]));
    }
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj)
        if (rw[jj] >= 0) v[jj] = moe_ld<T, N, VECL>((const T *)a.src + (int64_t)rw[jj] * a.lds + col);
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj) {
        if (rw[jj] < 0) continue;
        float f[N];
        moe_unpack(v[jj], f);
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += gv[jj] * f[i];
    }
}
// one span of y: from +0, the first kMoeK pairs from the entries the kernel holds, their row loads in flight together; the pairs beyond
// them (k > kMoeK) one at a time, entry, gate and row read here
template <typename T, int N, bool VECL>
__device__ __forceinline__ void moe_weighted_sum(const MoeMove &a, const int32_t *pr, const T *g, int32_t live, int64_t col, const int32_t (&row0)[kMoeK],
                                                 const float (&gv0)[kMoeK], float (&acc)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.f;
    moe_add_chunk<T, N, VECL>(a, col, row0, gv0, acc);
    for (int64_t j = kMoeK; j < a.k; ++j) {
        const int32_t r = __builtin_amdgcn_readfirstlane(pr[j]);
        if (r < 0 || r >= live) continue;
        const float gj = g ? load_f32(g + j) : 1.f;
        float f[N];
        moe_unpack(moe_ld<T, N, VECL>((const T *)a.src + (int64_t)r * a.lds + col), f);
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] += gj * f[i];
    }
}

template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kMoeBlock) void moe_combine_kernel(const MoeMove a) {
    constexpr int Vp = kPack16<T>;
    int64_t t;
    int lane;
    if (!moe_row_of<G>(a.T, t, lane)) return;
    const int32_t live = (int32_t)moe_live_rows(a.n_valid, a.n);   // n < 2^31
    const int32_t *pr = a.table + t * a.k;
    const T *g = a.gate ? (const T *)a.gate + t * a.ldg : nullptr;
    T *y = (T *)a.dst + t * a.ldd;
    const int64_t nb = a.cols / Vp, t0 = nb * Vp;
    // the first kMoeK entries and gates of the token, once, in front of every store to y
    int32_t row0[kMoeK];
    float gv0[kMoeK];
    moe_chunk(pr, g, 0, a.k, live, row0, gv0);
    for (int64_t c = lane; c < nb; c += G) {
        float acc[Vp];
        moe_weighted_sum<T, Vp, VEC>(a, pr, g, live, c * Vp, row0, gv0, acc);
        moe_st<T, Vp, VEC>(y + c * Vp, moe_pack<T, Vp, VEC>(acc));
    }
    if (t0 + lane < a.cols) {
        float acc[1];
        moe_weighted_sum<T, 1, false>(a, pr, g, live, t0 + lane, row0, gv0, acc);
        moe_st<T, 1, false>(y + t0 + lane, moe_pack<T, 1, false>(acc));
    }
}

// ---- combine backward ------------------------------------------------------------------------------------------------------------------------
// one span of dy against the kMoeK pairs of a chunk: the spans of dys are written, dot_jj += dy . ys_jj in element order. What a pair does
// with its row of dys: nothing (row < 0: the table entry names no row), +0 (row >= live: a dropped pair), gate dy (a live pair)
template <typename T, int N, bool VECL>
__device__ __forceinline__ void moe_bwd_span(const MoeMove &a, const T *dy, int64_t col, int32_t live, const int32_t (&row)[kMoeK], const float (&gv)[kMoeK],
                                             float (&dot)[kMoeK]) {
    using S = MoeSpan<T, N, VECL>;
    const S d = moe_ld<T, N, VECL>(dy + col);
    float fd[N];
    moe_unpack(d, fd);
    S v[kMoeK];
    // the row offsets are formed here, per span, from the 32-bit entries (kept opaque): hoisted out of the walk they are 4 kMoeK scalar
    // registers too many
    int32_t rw[kMoeK];
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj) {
        rw[jj] = row[jj];
        asm volatile("" : "+s"(rw[jj]));
    }
    if (a.dgate) {
#pragma unroll
        for (int jj = 0; jj < kMoeK; ++jj)
            if (rw[jj] >= 0 && rw[jj] < live) v[jj] = moe_ld<T, N, VECL>((const T *)a.src + (int64_t)rw[jj] * a.lds + col);
    }
#pragma unroll
    for (int jj = 0; jj < kMoeK; ++jj) {
        if (rw[jj] < 0) continue;
        T *out = (T *)a.dst + (int64_t)rw[jj] * a.ldd + col;
        if (rw[jj] >= live) {
            moe_st<T, N, VECL>(out, S{});
            continue;
        }
        if (a.gate) {
            float r[N];
#pragma unroll
            for (int i = 0; i < N; ++i) r[i] = gv[jj] * fd[i];
            moe_st<T, N, VECL>(out, moe_pack<T, N, VECL>(r));
        } else {
            moe_st<T, N, VECL>(out, d);
        }
        if (a.dgate) {
            float fy[N];
            moe_unpack(v[jj], fy);
#pragma unroll
            for (int i = 0; i < N; ++i) dot[jj] += fd[i] * fy[i];
        }
    }
}

template <typename T, int G, bool VEC>
__global__ __launch_bounds__(kMoeBlock) void moe_combine_bwd_kernel(const MoeMove a) {
    constexpr int Vp = kPack16<T>;
    __shared__ float red[kMoeK][kMoeWaves];
    int64_t t;
    int lane;
    if (!moe_row_of<G>(a.T, t, lane)) return;
    const int32_t live = (int32_t)moe_live_rows(a.n_valid, a.n);   // n < 2^31
    const int32_t *pr = a.table + t * a.k;
    const T *g = a.gate ? (const T *)a.gate + t * a.ldg : nullptr;
    const T *dy = (const T *)a.dy + t * a.lddy;
    T *dg = a.dgate ? (T *)a.dgate + t * a.lddg : nullptr;
    const int64_t nb = a.cols / Vp, t0 = nb * Vp;
    // k <= kMoeK: one trip, dy is read once; beyond that once per chunk of kMoeK pairs
    for (int64_t j0 = 0; j0 < a.k; j0 += kMoeK) {
        int32_t row[kMoeK];   // -1: the entry names no row
        float gv[kMoeK], dot[kMoeK];
#pragma unroll
        for (int jj = 0; jj < kMoeK; ++jj) {
            row[jj] = -1;
            gv[jj] = 1.f;
            dot[jj] = 0.f;
            if (j0 + jj < a.k) {
                const int32_t r = pr[j0 + jj];
                if (r >= 0 && r < a.n) {
                    row[jj] = r;
                    if (g && r < live) gv[jj] = load_f32(g + j0 + jj);
                }
            }
        }
        for (int64_t c = lane; c < nb; c += G) moe_bwd_span<T, Vp, VEC>(a, dy, c * Vp, live, row, gv, dot);
        if (t0 + lane < a.cols) moe_bwd_span<T, 1, false>(a, dy, t0 + lane, live, row, gv, dot);
        if (!dg) continue;
        // the lanes of a wave by an xor butterfly, the waves of a block through LDS in wave order
#pragma unroll
        for (int jj = 0; jj < kMoeK; ++jj)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) dot[jj] += __shfl_xor(dot[jj], o, 64);
        if constexpr (G == 64) {
            if (lane == 0) {
#pragma unroll
                for (int jj = 0; jj < kMoeK; ++jj)
                    if (j0 + jj < a.k) store_hw(dg + j0 + jj, moe_opaque<T>(dot[jj]));
            }
        } else {
            if (j0 > 0) __syncthreads();   // the previous chunk's sums have been read
            if ((lane & 63) == 0) {
#pragma unroll
                for (int jj = 0; jj < kMoeK; ++jj) red[jj][lane >> 6] = dot[jj];
            }
            __syncthreads();
            if (lane < kMoeK && j0 + lane < a.k) {
                float s = red[lane][0];
#pragma unroll
                for (int w = 1; w < kMoeWaves; ++w) s += red[lane][w];
                store_hw(dg + j0 + lane, moe_opaque<T>(s));
            }
        }
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
struct MoeOperand {
    const char *name;
    const void *p;
    int64_t ld, extent;
    bool required;
};

bool moe_dtype_ok(int dtype) { return dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16; }

// n = T k < 2^31, without overflow
bool moe_pairs_fit(int64_t T, int64_t k) { return T == 0 || k <= 0x7fffffffLL / T; }

// dtype, extents (each >= 0, and k >= 1, E >= 1 when given), then the floating operands: null, pitch, alignment
int moe_check(const char *who, int dtype, int64_t T, int64_t k, int64_t E, int64_t cols, const MoeOperand *ops, int nops) {
    KF_REQUIRE(moe_dtype_ok(dtype), KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(T >= 0 && cols >= 0 && k >= 1 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld k %lld E %lld cols %lld (T, cols >= 0; k, E >= 1)", who,
               (long long)T, (long long)k, (long long)E, (long long)cols);
    const int es = dtype_size(dtype);
    for (int i = 0; i < nops; ++i) {
        KF_REQUIRE(ops[i].p || !ops[i].required, KF_ERR_INVALID, "%s: null %s", who, ops[i].name);
        if (!ops[i].p) continue;
        KF_REQUIRE(ops[i].ld >= ops[i].extent, KF_ERR_INVALID, "%s: leading dimension of %s %lld < %lld", who, ops[i].name, (long long)ops[i].ld,
                   (long long)ops[i].extent);
        KF_REQUIRE((uintptr_t)ops[i].p % es == 0, KF_ERR_INVALID, "%s: %s not aligned to its element size", who, ops[i].name);
    }
    return KF_OK;
}
int moe_check_table(const char *who, const char *name, const void *p, int align) {
    KF_REQUIRE(p, KF_ERR_INVALID, "%s: null %s", who, name);
    KF_REQUIRE((uintptr_t)p % align == 0, KF_ERR_INVALID, "%s: %s not aligned to %d bytes", who, name, align);
    return KF_OK;
}
int moe_check_pairs(const char *who, int64_t T, int64_t k) {
    KF_REQUIRE(moe_pairs_fit(T, k), KF_ERR_UNSUPPORTED, "%s: T k = %lld x %lld pairs, the tables are 32-bit (T k < 2^31)", who, (long long)T, (long long)k);
    return KF_OK;
}

// the 16-byte path: every given row operand (ops: the operands with rows of cols elements) 16-byte aligned with a pitch in whole packs, and cols in whole packs
bool moe_vec(int dtype, int64_t cols, const MoeOperand *ops, int nops) {
    const int vp = 16 / dtype_size(dtype);
    bool ok = cols % vp == 0;
    for (int i = 0; i < nops; ++i)
        if (ops[i].p) ok = ok && (uintptr_t)ops[i].p % 16 == 0 && ops[i].ld % vp == 0;
    return ok;
}

unsigned moe_grid(int64_t rows, bool wave) { return (unsigned)(wave ? (rows + kMoeWaves - 1) / kMoeWaves : rows); }

size_t up16(size_t v) { return (v + 15) / 16 * 16; }
int moe_key_bits(int64_t E) {   // keys are 0 .. E inclusive
    int bits = 1;
    while (bits < 63 && ((int64_t)1 << bits) <= E) ++bits;
    return bits;
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_moe_plan_workspace_bytes(int64_t T, int64_t k, int64_t E, size_t *bytes) {
    const char *who = "kf_moe_plan_workspace_bytes";
    KF_REQUIRE(T >= 0 && k >= 1 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld k %lld E %lld (T >= 0; k, E >= 1)", who, (long long)T, (long long)k,
               (long long)E);
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null bytes", who);
    const int rc = moe_check_pairs(who, T, k);
    if (rc != KF_OK) return rc;
    const int64_t n = T * k;
    // the keys, the sorted keys and the sort's positions (int64 each), then the sort's own scratch
    *bytes = 3 * up16((size_t)n * 8) + up16(kf_sort_workspace_bytes(KF_I64, 1, n));
    return KF_OK;
}

extern "C" int kf_moe_plan(const int64_t *ids, int64_t T, int64_t k, int64_t E, int64_t *offsets, int32_t *row_pair, int32_t *pair_row, void *workspace,
                           size_t workspace_bytes, void *stream) {
    const char *who = "kf_moe_plan";
    KF_REQUIRE(T >= 0 && k >= 1 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld k %lld E %lld (T >= 0; k, E >= 1)", who, (long long)T, (long long)k,
               (long long)E);
    int rc = moe_check_table(who, "offsets", offsets, 8);
    if (rc != KF_OK) return rc;
    const bool some = T > 0;
    if (some || ids) rc = moe_check_table(who, "ids", ids, 8);
    if (rc == KF_OK && (some || row_pair)) rc = moe_check_table(who, "row_pair", row_pair, 4);
    if (rc == KF_OK && (some || pair_row)) rc = moe_check_table(who, "pair_row", pair_row, 4);
    if (rc != KF_OK) return rc;
    KF_REQUIRE((uintptr_t)workspace % 16 == 0, KF_ERR_INVALID, "%s: workspace not 16-byte aligned", who);
    if ((rc = moe_check_pairs(who, T, k)) != KF_OK) return rc;
    size_t need = 0;
    if ((rc = kf_moe_plan_workspace_bytes(T, k, E, &need)) != KF_OK) return rc;
    KF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), KF_ERR_INVALID, "%s: workspace too small or missing: %zu bytes required, got %zu", who,
               need, workspace ? workspace_bytes : (size_t)0);
    const int64_t n = T * k;
    hipStream_t st = as_stream(stream);
    KF_PROF("moe_plan", st);
    if (n == 0) return kf_segment_offsets(nullptr, 0, E, offsets, stream);
    char *ws = (char *)workspace;
    const size_t col = up16((size_t)n * 8);
    int64_t *keys = (int64_t *)ws, *sorted = (int64_t *)(ws + col), *pos = (int64_t *)(ws + 2 * col);
    const size_t sws = kf_sort_workspace_bytes(KF_I64, 1, n);
    const unsigned grid = (unsigned)((n + kMoeBlock - 1) / kMoeBlock);
    if ((rc = launch(moe_keys_kernel, grid, kMoeBlock, 0, st, ids, n, E, keys)) != KF_OK) return rc;
    // kf_sort, told that the keys agree above the bits of E: stable, so equal experts keep pair order and dropped pairs (key E) come last
    rc = sort_with_key_bits(KF_I64, keys, sorted, pos, 1, n, 0, sws ? ws + 3 * col : nullptr, sws, stream, moe_key_bits(E));
    if (rc != KF_OK) return rc;
    if ((rc = launch(moe_tables_kernel, grid, kMoeBlock, 0, st, (const int64_t *)pos, n, row_pair, pair_row)) != KF_OK) return rc;
    return kf_segment_offsets(sorted, n, E, offsets, stream);
}

static int moe_gate_run(const char *who, bool bwd, int dtype, int64_t T, int64_t k, int64_t E, const int64_t *ids, const void *p, int64_t ldp, int normalize,
                        const void *gate, int64_t ldg, const void *dgate, int64_t lddg, void *out, int64_t ldo, void *stream) {
    const MoeOperand ops[4] = {{"p", p, ldp, E, true}, {"gate", gate, ldg, k, true}, {"dgate", dgate, lddg, k, bwd}, {"dp", out, ldo, E, bwd}};
    int rc = moe_check(who, dtype, T, k, E, 0, ops, 4);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(normalize == 0 || normalize == 1, KF_ERR_INVALID, "%s: normalize %d is not 0 or 1", who, normalize);
    if ((rc = moe_check_table(who, "ids", ids, 8)) != KF_OK) return rc;
    if ((rc = moe_check_pairs(who, T, k)) != KF_OK) return rc;
    if (T == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    KF_PROF(bwd ? "moe_gate_bwd" : "moe_gate_fwd", st);
    MoeGate a{ids, p, gate, dgate, bwd ? out : const_cast<void *>(gate), T, k, E, ldp, ldg, lddg, bwd ? ldo : ldg, normalize};
    return with_dtype(dtype, [&](auto t) {
        using Tp = decltype(t);
        if (bwd) return launch(moe_gate_bwd_kernel<Tp>, moe_grid(T, true), kMoeBlock, 0, st, a);
        return launch(moe_gate_fwd_kernel<Tp>, (unsigned)((T + kMoeBlock - 1) / kMoeBlock), kMoeBlock, 0, st, a);
    });
}

extern "C" int kf_moe_gate_fwd(int dtype, int64_t T, int64_t k, int64_t E, const int64_t *ids, const void *p, int64_t ldp, int normalize, void *gate,
                               int64_t ldg, void *stream) {
    return moe_gate_run("kf_moe_gate_fwd", false, dtype, T, k, E, ids, p, ldp, normalize, gate, ldg, nullptr, 0, nullptr, 0, stream);
}

extern "C" int kf_moe_gate_bwd(int dtype, int64_t T, int64_t k, int64_t E, const int64_t *ids, const void *p, int64_t ldp, int normalize, const void *gate,
                               int64_t ldg, const void *dgate, int64_t lddg, void *dp, int64_t lddp, void *stream) {
    return moe_gate_run("kf_moe_gate_bwd", true, dtype, T, k, E, ids, p, ldp, normalize, gate, ldg, dgate, lddg, dp, lddp, stream);
}

// the launch of one of the three row movers: the regime from cols, the access from the operands
#define KF_MOE_LAUNCH(KERNEL, ROWS)                                                                                                        \
    with_dtype(dtype, [&](auto t_) {                                                                                                       \
        using Tp = decltype(t_);                                                                                                           \
        const bool wave_ = cols <= kMoeWaveMax;                                                                                            \
        return with_flags([&](auto WAVE, auto VEC) { return launch(KERNEL<Tp, WAVE ? 64 : kMoeBlock, VEC>, moe_grid(ROWS, WAVE), kMoeBlock, 0, st, a); }, \
                          wave_, vec);                                                                                                     \
    })

extern "C" int kf_moe_dispatch(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *row_pair, const void *x, int64_t ldx, void *xs, int64_t ldxs,
                               void *stream) {
    const char *who = "kf_moe_dispatch";
    const MoeOperand ops[2] = {{"x", x, ldx, cols, true}, {"xs", xs, ldxs, cols, true}};
    int rc = moe_check(who, dtype, T, k, 1, cols, ops, 2);
    if (rc != KF_OK) return rc;
    if ((rc = moe_check_table(who, "row_pair", row_pair, 4)) != KF_OK) return rc;
    if ((rc = moe_check_pairs(who, T, k)) != KF_OK) return rc;
    if (T == 0 || cols == 0) return KF_OK;
    const bool vec = moe_vec(dtype, cols, ops, 2);
    hipStream_t st = as_stream(stream);
    KF_PROF("moe_dispatch", st);
    const MoeMove a{row_pair, nullptr, nullptr, x, nullptr, xs, nullptr, T, k, T * k, cols, 0, ldx, 0, ldxs, 0};
    return KF_MOE_LAUNCH(moe_dispatch_kernel, a.n);
}

extern "C" int kf_moe_combine(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *pair_row, const int64_t *n_valid, const void *gate, int64_t ldg,
                              const void *ys, int64_t ldys, void *y, int64_t ldy, void *stream) {
    const char *who = "kf_moe_combine";
    const MoeOperand ops[3] = {{"ys", ys, ldys, cols, true}, {"y", y, ldy, cols, true}, {"gate", gate, ldg, k, false}};
    int rc = moe_check(who, dtype, T, k, 1, cols, ops, 3);
    if (rc != KF_OK) return rc;
    if ((rc = moe_check_table(who, "pair_row", pair_row, 4)) != KF_OK) return rc;
    KF_REQUIRE((uintptr_t)n_valid % 8 == 0, KF_ERR_INVALID, "%s: n_valid not aligned to 8 bytes", who);
    if ((rc = moe_check_pairs(who, T, k)) != KF_OK) return rc;
    if (T == 0 || cols == 0) return KF_OK;
    const bool vec = moe_vec(dtype, cols, ops, 2);   // ys and y
    hipStream_t st = as_stream(stream);
    KF_PROF("moe_combine", st);
    const MoeMove a{pair_row, n_valid, gate, ys, nullptr, y, nullptr, T, k, T * k, cols, ldg, ldys, 0, ldy, 0};
    return KF_MOE_LAUNCH(moe_combine_kernel, a.T);
}

extern "C" int kf_moe_combine_bwd(int dtype, int64_t T, int64_t k, int64_t cols, const int32_t *pair_row, const int64_t *n_valid, const void *gate,
                                  int64_t ldg, const void *ys, int64_t ldys, const void *dy, int64_t lddy, void *dys, int64_t lddys, void *dgate,
                                  int64_t lddg, void *stream) {
    const char *who = "kf_moe_combine_bwd";
    const MoeOperand ops[5] = {{"dy", dy, lddy, cols, true},   {"dys", dys, lddys, cols, true},  {"ys", ys, ldys, cols, dgate != nullptr},
                               {"gate", gate, ldg, k, false}, {"dgate", dgate, lddg, k, false}};
    int rc = moe_check(who, dtype, T, k, 1, cols, ops, 5);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(gate || !dgate, KF_ERR_INVALID, "%s: dgate without a gate (gate == NULL requires dgate == NULL)", who);
    if ((rc = moe_check_table(who, "pair_row", pair_row, 4)) != KF_OK) return rc;
    KF_REQUIRE((uintptr_t)n_valid % 8 == 0, KF_ERR_INVALID, "%s: n_valid not aligned to 8 bytes", who);
    if ((rc = moe_check_pairs(who, T, k)) != KF_OK) return rc;
    if (T == 0) return KF_OK;
    if (cols == 0 && !dgate) return KF_OK;
    // ys is read only for dgate: without it its geometry does not count
    const MoeOperand moved[3] = {ops[0], ops[1], dgate ? ops[2] : MoeOperand{"ys", nullptr, 0, cols, false}};
    const bool vec = moe_vec(dtype, cols, moved, 3);
    hipStream_t st = as_stream(stream);
    KF_PROF("moe_combine_bwd", st);
    const MoeMove a{pair_row, n_valid, gate, dgate ? ys : nullptr, dy, dys, dgate, T, k, T * k, cols, ldg, ldys, lddy, lddys, lddg};
    return KF_MOE_LAUNCH(moe_combine_bwd_kernel, a.T);
}
