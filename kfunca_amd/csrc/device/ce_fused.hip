// Softmax cross-entropy of a BLOCK of logits with its gradient in the same launch, for gfx950: the row kernel of the chunked
// linear + cross-entropy loss (core/linear_ce.cpp), which never holds the [T, V] logits. Plus the two small kernels that operator needs
// around it: the loss sum over all T rows (kf_ce_fused_reduce) and a scale-and-convert stream (kf_scale_cast).
//
//   lse_r      = log(sum_v exp(x_rv))
//   rowloss_r  = (1 - eps) (lse_r - x_r,t) + eps (lse_r - mean_v x_rv) + z lse_r^2      eps = label smoothing, z = z-loss, t = target[r]
//   dlogits_rv = exp(x_rv - lse_r) (1 + 2 z lse_r) - (1 - eps) [v == t] - eps / V       UNSCALED: no 1 / count, no upstream gradient
//
// A row is walked twice by the SAME lanes: the first walk is cross_entropy.hip's online log-sum-exp (per lane a running max m, a sum s
// of exponentials relative to h = m log2e rounded, and sum x when smoothing; lane states combine across the wave by an xor butterfly and
// across the block through LDS in wave order), the second walk re-reads the row - from L2 / MALL for the row lengths of a vocabulary,
// the same lane re-reads the bytes it read - and writes the gradient once. The online-softmax state is duplicated from
// cross_entropy.hip (that file is pinned by bitwise tests and keeps its helpers private); the arithmetic is the same, the residual
// trick included: x log2e - h is one rounding inside an FMA and lo = fma(m, log2e, -h) is folded back at the end.
//
// The hot pair is f32 logits (a GEMM's unrounded accumulators) -> 16-bit gradient: a lane reads TWO 16-byte packs and writes ONE.
//
// Regimes, from (rows, V) alone (cross_entropy.hip's partition):
//   rows   V <= 4096                 one wave per row, four rows per 256-thread block; ONE launch
//   block  V > 4096, rows >= 1024    one 256-thread block per row; ONE launch
//   split  V > 4096, rows < 1024     each row cut into chunks of whole 64-element multiples, one block per chunk: a state launch writes
//                                    partial (m, s, sum x) to caller scratch, a combine launch merges them IN CHUNK ORDER and keeps the
//                                    row's lse in the scratch, a write launch produces the gradient
// No atomics anywhere: the same call gives the same bits.
//
// Alignment: the first walk reads a scalar head up to the first 16-byte boundary of the LOGITS, packs, and a scalar tail. The second walk
// aligns on the GRADIENT row: a scalar head up to its first 16-byte boundary, then packs when the logits are 16-byte aligned at that
// same element (contiguous buffers from an allocator always are: 4 (r V + h) is twice 2 (r V + h)), element by element otherwise.
//
// In place (dlogits == logits, one dtype, one stride): every element is read in the second walk by the lane that overwrites it, and no
// lane starts the second walk before the whole row's first walk is over (the butterfly / the block barrier / the launch boundary).
// The ONE other read of the logits is the target's logit for the row's loss, by a single lane: it is made before the row's first walk
// (one wave per row: earlier in the same wave's instruction stream than its stores; one block per row: parked in LDS before the block
// barrier every wave must pass before it writes; split rows: in the combine launch, before the write launch).
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// as in cross_entropy.hip: every fused multiply-add is written out (fmaf), nothing is contracted behind the residual's back
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kCfBlock = 256;
constexpr int64_t kCfShortRow = 4096;    // V up to this: one wave per row
constexpr int64_t kCfManyRows = 1024;    // at least this many long rows: one block per row
constexpr int64_t kCfSplitBlocks = 2048; // the split regime aims for this many blocks in all
constexpr int64_t kCfMinChunk = 4096;    // elements per chunk, at least

// ---- the online state (cross_entropy.hip's, duplicated) -----------------------------------------------------------------------
struct CfState { float m, s, sx; };
__device__ __forceinline__ float cf_h(float m) { return m == -INFINITY ? 0.f : m * kLog2e; }
__device__ __forceinline__ float cf_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float cf_rescale(float s, float m_old, float m_new, float h_new) {
    return m_old == m_new ? s : s * cf_exp2(m_old * kLog2e - h_new);
}
__device__ __forceinline__ CfState cf_combine(const CfState &a, const CfState &b) {
    const float m = fmaxf(a.m, b.m), h = cf_h(m);
    return {m, cf_rescale(a.s, a.m, m, h) + cf_rescale(b.s, b.m, m, h), a.sx + b.sx};
}

template <int N, bool SMOOTH>
__device__ __forceinline__ void cf_absorb(CfState &st, const float (&f)[N]) {
    float pm = f[0];
#pragma unroll
    for (int i = 1; i < N; ++i) pm = fmaxf(pm, f[i]);
    const float m = fmaxf(st.m, pm), h = cf_h(m);
    float s = cf_rescale(st.s, st.m, m, h);
#pragma unroll
    for (int i = 0; i < N; ++i) s += cf_exp2(fmaf(f[i], kLog2e, -h));
    if constexpr (SMOOTH) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < N; ++i) t += f[i];
        st.sx += t;
    }
    st.m = m;
    st.s = s;
}

// the state of the elements [c0, c1) of a row as seen by lane `lane` of the NT lanes that share the segment
template <typename T, int NT, bool SMOOTH>
__device__ __forceinline__ CfState cf_segment_state(const T *row, int64_t c0, int64_t c1, int lane) {
    constexpr int V = kPack16<T>, U = 2;
    CfState st{-INFINITY, 0.f, 0.f};
    const T *p = row + c0;
    const int64_t n = c1 - c0;
    const int64_t head = std::min<int64_t>(n, (int64_t)((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u) / (int64_t)sizeof(T));
    const int64_t nb = (n - head) / V, t0 = head + nb * V;
    if (lane < head) { const float f[1] = {load_f32(p + lane)}; cf_absorb<1, SMOOTH>(st, f); }
    if (t0 + lane < n) { const float f[1] = {load_f32(p + t0 + lane)}; cf_absorb<1, SMOOTH>(st, f); }
    const uint4 *q = (const uint4 *)(p + head);
    for (int64_t k = lane; k < nb; k += (int64_t)NT * U) {
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) raw[u] = k + (int64_t)u * NT < nb ? q[k + (int64_t)u * NT] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k + (int64_t)u * NT < nb) {
                float f[V];
                unpack16<T>(raw[u], f);
                cf_absorb<V, SMOOTH>(st, f);
            }
        }
    }
    return st;
}

// combine across the NT lanes of a segment (64: the wave; 256: the block through LDS, in wave order). EVERY lane returns the result:
// the butterfly's last step leaves lane 0's value to be broadcast, the LDS walk is the same arithmetic on every thread.
template <int NT>
__device__ __forceinline__ CfState cf_reduce_state(CfState st, CfState *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const CfState b{__shfl_xor(st.m, o, 64), __shfl_xor(st.s, o, 64), __shfl_xor(st.sx, o, 64)};
        st = cf_combine(st, b);
    }
    if constexpr (NT > 64) {
        const int wid = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) red[wid] = st;
        __syncthreads();
        st = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) st = cf_combine(st, red[w]);
    } else {
        st = CfState{__shfl(st.m, 0, 64), __shfl(st.s, 0, 64), __shfl(st.sx, 0, 64)};
    }
    return st;
}

struct CfArgs {
    const void *x;
    const int64_t *target;
    float *rowloss; // [rows]
    float *lse;     // [rows] or null
    void *dx;       // [rows, V] with stride ldd, or null (loss only)
    float *part;    // split: [rows][nchunk] states
    float *wlse;    // split: [rows], the lse the write launch reads
    int64_t rows, V, ld, ldd, ignore_index, chunk; // chunk: elements per chunk (split)
    int nchunk;
    float eps, z;
};

// log(sum exp(x - m)) and the row's lse from its combined state
__device__ __forceinline__ float cf_lns(const CfState &st) {
    const float lo = st.m == -INFINITY ? 0.f : fmaf(st.m, kLog2e, -cf_h(st.m));
    return logf(st.s) - lo * kLn2;
}

// The target's logit of a row (0 where the row is ignored or its target is out of range: cf_finish does not use it then). It is read
// on its own, BEFORE anything of the row is written: in place the gradient overwrites it.
template <typename T>
__device__ __forceinline__ float cf_target_logit(const CfArgs &a, int64_t row) {
    const int64_t t = a.target[row];
    return t == a.ignore_index || t < 0 || t >= a.V ? 0.f : load_f32((const T *)a.x + row * a.ld + t);
}

// one lane per row: the row's loss (and lse, when kept) from its combined state and the target's logit xt
__device__ __forceinline__ void cf_finish(const CfArgs &a, int64_t row, const CfState &st, float xt) {
    const int64_t t = a.target[row];
    const float lns = cf_lns(st), lse = st.m + lns;
    if (a.lse) a.lse[row] = lse;
    float loss;
    if (t == a.ignore_index) {
        loss = 0.f;
    } else if (t < 0 || t >= a.V) {
        loss = __builtin_nanf("");
    } else {
        loss = 0.f;
        if (a.eps < 1.f) loss = (1.f - a.eps) * ((st.m - xt) + lns);
        if (a.eps > 0.f) loss += a.eps * ((st.m - st.sx / (float)a.V) + lns);
        if (a.z != 0.f) loss += a.z * (lse * lse);
    }
    a.rowloss[row] = loss;
}

// the gradient over the elements [c0, c1) of a row, lane `lane` of NT. A written pack is 16 bytes of TO: G elements, read as R packs of TI.
template <typename TI, typename TO, int NT>
__device__ __forceinline__ void cf_write_segment(const CfArgs &a, int64_t row, int64_t c0, int64_t c1, int lane, float lse) {
    constexpr int G = kPack16<TO>, R = G / kPack16<TI>, U = 2;
    static_assert(R == 1 || R == 2, "the gradient is never wider than the logits");
    const TI *x = (const TI *)a.x + row * a.ld + c0;
    TO *dx = (TO *)a.dx + row * a.ldd + c0;
    const int64_t n = c1 - c0;
    const int64_t t = a.target[row];
    const bool ign = t == a.ignore_index; // a zero row, whatever the logits hold
    float k = 1.f + 2.f * a.z * lse;
    if (t < 0 || t >= a.V) k = __builtin_nanf("");
    // p = exp(x - lse) = 2^(fma(x, log2e, -hl)) * 2^-lo with hl = lse log2e rounded and lo its exact residual: 2^-lo goes into the factor
    const float hl = lse * kLog2e, lo = fmaf(lse, kLog2e, -hl);
    const float gs = k * cf_exp2(-lo), c0s = a.eps / (float)a.V, c1s = 1.f - a.eps; // (a NaN k makes every column NaN through the FMA)
    const int64_t tl = t - c0; // the target's position inside the segment (may lie outside it)
    auto one = [&](int64_t i) __attribute__((always_inline)) {
        if (ign) { store_canonical(dx + i, 0.f); return; }
        const float v = fmaf(gs, cf_exp2(fmaf(load_f32(x + i), kLog2e, -hl)), -c0s);
        store_canonical(dx + i, i == tl ? v - c1s : v);
    };
    const int64_t head = std::min<int64_t>(n, (int64_t)((16u - ((uint32_t)(uintptr_t)dx & 15u)) & 15u) / (int64_t)sizeof(TO));
    if (((uint32_t)(uintptr_t)(x + head) & 15u) != 0u) { // the two rows sit differently against 16-byte boundaries: element by element
        for (int64_t i = lane; i < n; i += NT) one(i);
        return;
    }
    const int64_t nb = (n - head) / G, t0 = head + nb * G;
    if (lane < head) one(lane);
    if (t0 + lane < n) one(t0 + lane);
    const uint4 *q = (const uint4 *)(x + head);
    uint4 *qd = (uint4 *)(dx + head);
    if (ign) {
        for (int64_t kk = lane; kk < nb; kk += NT) qd[kk] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    for (int64_t kb = lane; kb < nb; kb += (int64_t)NT * U) {
        uint4 raw[U][R];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int r = 0; r < R; ++r) raw[u][r] = kb + (int64_t)u * NT < nb ? q[(kb + (int64_t)u * NT) * R + r] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = kb + (int64_t)u * NT;
            if (kk < nb) {
                float f[G];
                if constexpr (R == 1) {
                    unpack16<TI>(raw[u][0], f);
                } else {
                    float lo4[4], hi4[4];
                    unpack16<TI>(raw[u][0], lo4);
                    unpack16<TI>(raw[u][1], hi4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) { f[i] = lo4[i]; f[4 + i] = hi4[i]; }
                }
#pragma unroll
                for (int i = 0; i < G; ++i) f[i] = fmaf(gs, cf_exp2(fmaf(f[i], kLog2e, -hl)), -c0s);
                const int64_t e = tl - head - kk * G;
                if (e >= 0 && e < G) {
#pragma unroll
                    for (int i = 0; i < G; ++i)
                        if (i == e) f[i] -= c1s;
                }
                qd[kk] = pack16<TO>(f);
            }
        }
    }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
template <typename TI, typename TO, bool SMOOTH, bool WRITE>
__global__ __launch_bounds__(kCfBlock) void ce_fused_rows(const CfArgs a) {
    const int64_t row = (int64_t)blockIdx.x * (kCfBlock / 64) + (threadIdx.x >> 6);
    if (row >= a.rows) return; // whole waves
    const int lane = threadIdx.x & 63;
    // lane 0 reads the target's logit first: the wave's own stores of the write walk come later in its instruction stream
    const float xt = lane == 0 ? cf_target_logit<TI>(a, row) : 0.f;
    CfState st = cf_segment_state<TI, 64, SMOOTH>((const TI *)a.x + row * a.ld, 0, a.V, lane);
    st = cf_reduce_state<64>(st, nullptr);
    if (lane == 0) cf_finish(a, row, st, xt);
    if constexpr (WRITE) cf_write_segment<TI, TO, 64>(a, row, 0, a.V, lane, st.m + cf_lns(st));
}

template <typename TI, typename TO, bool SMOOTH, bool WRITE>
__global__ __launch_bounds__(kCfBlock) void ce_fused_block(const CfArgs a) {
    __shared__ CfState red[kCfBlock / 64];
    __shared__ float xt_s;
    const int64_t row = blockIdx.x;
    // Thread 0 reads the target's logit and parks it in LDS BEFORE the barrier inside cf_reduce_state: the LDS store needs the loaded
    // value, so the load has returned before any wave passes that barrier and starts the write walk, which in place overwrites the
    // logit. (Read after the barrier, the load would race the stores of the wave that owns the target's column.)
    if (threadIdx.x == 0) xt_s = cf_target_logit<TI>(a, row);
    CfState st = cf_segment_state<TI, kCfBlock, SMOOTH>((const TI *)a.x + row * a.ld, 0, a.V, threadIdx.x);
    st = cf_reduce_state<kCfBlock>(st, red);
    if (threadIdx.x == 0) cf_finish(a, row, st, xt_s);
    if constexpr (WRITE) cf_write_segment<TI, TO, kCfBlock>(a, row, 0, a.V, threadIdx.x, st.m + cf_lns(st));
}

template <typename TI, bool SMOOTH>
__global__ __launch_bounds__(kCfBlock) void ce_fused_split_state(const CfArgs a) {
    __shared__ CfState red[kCfBlock / 64];
    const int64_t row = blockIdx.x / a.nchunk;
    const int j = (int)(blockIdx.x % a.nchunk);
    const int64_t c0 = (int64_t)j * a.chunk, c1 = std::min<int64_t>(a.V, c0 + a.chunk);
    CfState st = cf_segment_state<TI, kCfBlock, SMOOTH>((const TI *)a.x + row * a.ld, c0, c1, threadIdx.x);
    st = cf_reduce_state<kCfBlock>(st, red);
    if (threadIdx.x == 0) {
        float *o = a.part + ((int64_t)row * a.nchunk + j) * 3;
        o[0] = st.m; o[1] = st.s; o[2] = st.sx;
    }
}

// one thread per row: the chunk partials in chunk order, then the row's loss; the lse stays in the scratch for the write launch
template <typename TI>
__global__ __launch_bounds__(kCfBlock) void ce_fused_combine(const CfArgs a) {
    const int64_t row = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
    if (row >= a.rows) return;
    const float *p = a.part + row * a.nchunk * 3;
    CfState st{p[0], p[1], p[2]};
    for (int j = 1; j < a.nchunk; ++j) st = cf_combine(st, CfState{p[3 * j], p[3 * j + 1], p[3 * j + 2]});
    cf_finish(a, row, st, cf_target_logit<TI>(a, row)); // (the write launch comes after this one)
    a.wlse[row] = st.m + cf_lns(st);
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kCfBlock) void ce_fused_split_write(const CfArgs a) {
    const int64_t row = blockIdx.x / a.nchunk;
    const int j = (int)(blockIdx.x % a.nchunk);
    const int64_t c0 = (int64_t)j * a.chunk;
    cf_write_segment<TI, TO, kCfBlock>(a, row, c0, std::min<int64_t>(a.V, c0 + a.chunk), threadIdx.x, a.wlse[row]);
}

// loss = the sum (or the mean over the rows not ignored) of rowloss; count = the rows not ignored. One block, fixed order: thread i adds
// rows i, i + 1024, ... in turn, then a tree through LDS.
__global__ __launch_bounds__(1024) void ce_fused_reduce(const float *rowloss, const int64_t *target, int64_t rows, int64_t ignore_index, int mean,
                                                       float *loss, float *count) {
    __shared__ float rs[1024], rc[1024];
    float s = 0.f, c = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 1024) {
        s += rowloss[r];
        c += target[r] != ignore_index ? 1.f : 0.f;
    }
    rs[threadIdx.x] = s;
    rc[threadIdx.x] = c;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { rs[threadIdx.x] += rs[threadIdx.x + w]; rc[threadIdx.x] += rc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = mean ? rs[0] / rc[0] : rs[0];
        if (count) count[0] = rc[0];
    }
}

// The product as an f32 VALUE. Without the empty asm the compiler folds the multiply and a following f16 conversion into one
// v_fma_mixlo_f16, which rounds the exact product ONCE to f16: one element in a million then differs by an ulp from the documented
// result (the f32 product, rounded to the output type), and the pack and element paths would disagree with each other.
__device__ __forceinline__ float sc_mul(float a, float s) {
    float y = a * s;
    asm volatile("" : "+v"(y));
    return y;
}

// out[i] = in[i] * (g / count): one thread per written 16-byte pack (R packs read), the elements past the last whole pack by the first
// threads of the grid
template <typename TI, typename TO>
__global__ __launch_bounds__(kCfBlock) void scale_cast_packs(const TI *in, TO *out, int64_t n, const float *g, const float *count) {
    constexpr int G = kPack16<TO>, R = G / kPack16<TI>;
    static_assert(R == 1 || R == 2, "the output is never wider than the input");
    const float s = count ? g[0] / count[0] : g[0];
    const int64_t nb = n / G, idx = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
    if (idx < n - nb * G) store_canonical(out + nb * G + idx, sc_mul(load_f32(in + nb * G + idx), s));
    if (idx >= nb) return;
    const uint4 *q = (const uint4 *)in + idx * R;
    float f[G];
    if constexpr (R == 1) {
        unpack16<TI>(q[0], f);
    } else {
        const uint4 r0 = q[0], r1 = q[1];
        float lo4[4], hi4[4];
        unpack16<TI>(r0, lo4);
        unpack16<TI>(r1, hi4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[i] = lo4[i]; f[4 + i] = hi4[i]; }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) f[i] = sc_mul(f[i], s);
    ((uint4 *)out)[idx] = pack16<TO>(f);
}

template <typename TI, typename TO>
__global__ __launch_bounds__(kCfBlock) void scale_cast_elems(const TI *in, TO *out, int64_t n, const float *g, const float *count) {
    const float s = count ? g[0] / count[0] : g[0];
    const int64_t idx = (int64_t)blockIdx.x * kCfBlock + threadIdx.x;
    if (idx < n) store_canonical(out + idx, sc_mul(load_f32(in + idx), s));
}

// ---- the partition (cross_entropy.hip's ce_plan) ------------------------------------------------------------------------------
enum CfRegime { CF_ROWS = 0, CF_BLOCK = 1, CF_SPLIT = 2 };
struct CfPlan { int regime, nchunk; int64_t chunk; };
CfPlan cf_plan(int64_t rows, int64_t V) {
    if (V <= kCfShortRow) return {CF_ROWS, 1, V};
    if (rows >= kCfManyRows) return {CF_BLOCK, 1, V};
    const int64_t want = std::min((V + kCfMinChunk - 1) / kCfMinChunk, (kCfSplitBlocks + std::max<int64_t>(rows, 1) - 1) / std::max<int64_t>(rows, 1));
    if (want <= 1) return {CF_BLOCK, 1, V};
    const int64_t chunk = ((V + want - 1) / want + 63) / 64 * 64;
    return {CF_SPLIT, (int)((V + chunk - 1) / chunk), chunk};
}

size_t cf_align(size_t b) { return (b + 255) / 256 * 256; }
size_t cf_part_bytes(int64_t rows, const CfPlan &pl) { return pl.regime == CF_SPLIT ? cf_align((size_t)rows * pl.nchunk * 3 * sizeof(float)) : 0; }
size_t cf_wlse_bytes(int64_t rows, const CfPlan &pl) { return pl.regime == CF_SPLIT ? cf_align((size_t)rows * sizeof(float)) : 0; }

bool cf_float_dtype(int dt) { return dt == KF_F32 || dt == KF_BF16 || dt == KF_F16; }
// f32 -> f32 / bf16 / f16, or a 16-bit type to itself
bool cf_pair_ok(int in_dtype, int out_dtype) { return cf_float_dtype(in_dtype) && cf_float_dtype(out_dtype) && (in_dtype == out_dtype || in_dtype == KF_F32); }

// f(TI{}, TO{}) for a pair cf_pair_ok accepted
template <typename F> int cf_with_pair(int in_dtype, int out_dtype, F &&f) {
    if (in_dtype == KF_BF16) return f(bf16_t{}, bf16_t{});
    if (in_dtype == KF_F16) return f(f16_t{}, f16_t{});
    return out_dtype == KF_F32 ? f(float{}, float{}) : out_dtype == KF_BF16 ? f(float{}, bf16_t{}) : f(float{}, f16_t{});
}

bool cf_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + bbytes && pb < pa + abytes;
}

} // namespace
} // namespace kf

using namespace kf;

static int cf_check(const char *who, int64_t rows, int64_t V) {
    KF_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL, KF_ERR_INVALID, "%s: rows %lld outside [0, 2^31)", who, (long long)rows);
    KF_REQUIRE(V >= 1 && V <= 0x7fffffffLL, KF_ERR_INVALID, "%s: V %lld outside [1, 2^31)", who, (long long)V);
    return KF_OK;
}

extern "C" int kf_ce_fused_rows_workspace_bytes(int64_t rows, int64_t V, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_ce_fused_rows_workspace_bytes: null out pointer");
    *bytes = 0;
    const int rc = cf_check("kf_ce_fused_rows_workspace_bytes", rows, V);
    if (rc != KF_OK) return rc;
    const CfPlan pl = cf_plan(rows, V);
    *bytes = cf_part_bytes(rows, pl) + cf_wlse_bytes(rows, pl);
    return KF_OK;
}

extern "C" int kf_ce_fused_rows(int in_dtype, int out_dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target,
                                int64_t ignore_index, float label_smoothing, float z_loss, float *rowloss, float *lse, void *dlogits, int64_t ldd,
                                void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_ce_fused_rows";
    KF_REQUIRE(cf_pair_ok(in_dtype, out_dtype), KF_ERR_INVALID,
               "%s: dtype pair %d -> %d not supported (float -> float / half / bfloat16, or a 16-bit type to itself)", who, in_dtype, out_dtype);
    int rc = cf_check(who, rows, V);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(ld >= V, KF_ERR_INVALID, "%s: row stride %lld < V %lld", who, (long long)ld, (long long)V);
    KF_REQUIRE(!dlogits || ldd >= V, KF_ERR_INVALID, "%s: gradient row stride %lld < V %lld", who, (long long)ldd, (long long)V);
    KF_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, KF_ERR_INVALID, "%s: label_smoothing %g outside [0, 1]", who, (double)label_smoothing);
    KF_REQUIRE(z_loss >= 0.f && z_loss <= 3.0e38f, KF_ERR_INVALID, "%s: z_loss %g must be finite and not negative", who, (double)z_loss);
    if (rows == 0) return KF_OK;
    KF_REQUIRE(logits && target && rowloss, KF_ERR_INVALID, "%s: null logits, target or rowloss", who);
    KF_REQUIRE((uintptr_t)logits % dtype_size(in_dtype) == 0 && (uintptr_t)dlogits % dtype_size(out_dtype) == 0, KF_ERR_INVALID,
               "%s: logits or dlogits not aligned to their element size", who);
    if (dlogits) {
        const size_t xb = ((size_t)(rows - 1) * ld + V) * dtype_size(in_dtype), db = ((size_t)(rows - 1) * ldd + V) * dtype_size(out_dtype);
        const bool in_place = dlogits == logits && in_dtype == out_dtype && ld == ldd;
        KF_REQUIRE(in_place || !cf_overlap(logits, xb, dlogits, db), KF_ERR_INVALID,
                   "%s: dlogits overlaps logits; in place needs the same pointer, one dtype (%d -> %d) and one row stride (%lld, %lld)", who, in_dtype,
                   out_dtype, (long long)ld, (long long)ldd);
    }
    const CfPlan pl = cf_plan(rows, V);
    const size_t pb = cf_part_bytes(rows, pl), need = pb + cf_wlse_bytes(rows, pl);
    KF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), KF_ERR_INVALID, "%s: workspace of %zu bytes required, got %zu", who, need,
               workspace ? workspace_bytes : (size_t)0);
    hipStream_t st = as_stream(stream);
    CfArgs a{logits, target, rowloss, lse, dlogits, (float *)workspace, (float *)((char *)workspace + pb), rows, V, ld, ldd, ignore_index, pl.chunk,
             pl.nchunk, label_smoothing, z_loss};
    const bool smooth = label_smoothing > 0.f, write = dlogits != nullptr;
    return cf_with_pair(in_dtype, write ? out_dtype : in_dtype, [&](auto ti, auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        if (pl.regime != CF_SPLIT) {
            KF_PROF(pl.regime == CF_ROWS ? "ce_fused_rows" : "ce_fused_block", st);
            return with_flags([&](auto SMOOTH, auto WRITE) {
                return pl.regime == CF_ROWS
                           ? launch(ce_fused_rows<TI, TO, SMOOTH, WRITE>, (unsigned)((rows + kCfBlock / 64 - 1) / (kCfBlock / 64)), kCfBlock, 0, st, a)
                           : launch(ce_fused_block<TI, TO, SMOOTH, WRITE>, (unsigned)rows, kCfBlock, 0, st, a);
            }, smooth, write);
        }
        {
            KF_PROF("ce_fused_split_state", st);
            const int rs = with_flags([&](auto SMOOTH) { return launch(ce_fused_split_state<TI, SMOOTH>, (unsigned)(rows * pl.nchunk), kCfBlock, 0, st, a); },
                                      smooth);
            if (rs != KF_OK) return rs;
        }
        {
            KF_PROF("ce_fused_combine", st);
            const int rs = launch(ce_fused_combine<TI>, (unsigned)((rows + kCfBlock - 1) / kCfBlock), kCfBlock, 0, st, a);
            if (rs != KF_OK || !write) return rs;
        }
        KF_PROF("ce_fused_split_write", st);
        return launch(ce_fused_split_write<TI, TO>, (unsigned)(rows * pl.nchunk), kCfBlock, 0, st, a);
    });
}

extern "C" int kf_ce_fused_reduce(const float *rowloss, const int64_t *target, int64_t rows, int64_t ignore_index, int mean, float *loss,
                                  float *count, void *stream) {
    KF_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL, KF_ERR_INVALID, "kf_ce_fused_reduce: rows %lld outside [0, 2^31)", (long long)rows);
    KF_REQUIRE(mean == 0 || mean == 1, KF_ERR_INVALID, "kf_ce_fused_reduce: mean %d is neither 0 nor 1", mean);
    KF_REQUIRE(loss, KF_ERR_INVALID, "kf_ce_fused_reduce: null loss");
    KF_REQUIRE(rows == 0 || (rowloss && target), KF_ERR_INVALID, "kf_ce_fused_reduce: null rowloss or target");
    hipStream_t st = as_stream(stream);
    KF_PROF("ce_fused_reduce", st);
    return launch(ce_fused_reduce, 1, 1024, 0, st, rowloss, target, rows, ignore_index, mean, loss, count);
}

extern "C" int kf_scale_cast(int in_dtype, int out_dtype, int64_t n, const void *in, void *out, const float *g, const float *count, void *stream) {
    KF_REQUIRE(cf_pair_ok(in_dtype, out_dtype), KF_ERR_INVALID,
               "kf_scale_cast: dtype pair %d -> %d not supported (float -> float / half / bfloat16, or a 16-bit type to itself)", in_dtype, out_dtype);
    KF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 38), KF_ERR_INVALID, "kf_scale_cast: n %lld outside [0, 2^38]", (long long)n);
    KF_REQUIRE(g, KF_ERR_INVALID, "kf_scale_cast: null g");
    if (n == 0) return KF_OK;
    KF_REQUIRE(in && out, KF_ERR_INVALID, "kf_scale_cast: null in or out");
    KF_REQUIRE((uintptr_t)in % dtype_size(in_dtype) == 0 && (uintptr_t)out % dtype_size(out_dtype) == 0, KF_ERR_INVALID,
               "kf_scale_cast: in or out not aligned to its element size");
    KF_REQUIRE((in == out && in_dtype == out_dtype) || !cf_overlap(in, (size_t)n * dtype_size(in_dtype), out, (size_t)n * dtype_size(out_dtype)),
               KF_ERR_INVALID, "kf_scale_cast: out overlaps in; in place needs the same pointer and one dtype (%d -> %d)", in_dtype, out_dtype);
    hipStream_t st = as_stream(stream);
    const bool packs = (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
    KF_PROF("scale_cast", st);
    return cf_with_pair(in_dtype, out_dtype, [&](auto ti, auto to) {
        using TI = decltype(ti);
        using TO = decltype(to);
        if (!packs) return launch(scale_cast_elems<TI, TO>, (unsigned)((n + kCfBlock - 1) / kCfBlock), kCfBlock, 0, st, (const TI *)in, (TO *)out, n, g, count);
        const int64_t nb = std::max<int64_t>(n / kPack16<TO>, 1);
        return launch(scale_cast_packs<TI, TO>, (unsigned)((nb + kCfBlock - 1) / kCfBlock), kCfBlock, 0, st, (const TI *)in, (TO *)out, n, g, count);
    });
}
