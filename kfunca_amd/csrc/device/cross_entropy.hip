// Softmax cross-entropy over the last dimension for gfx950, forward and backward (torch's F.cross_entropy semantics, class axis last).
//
//   lse_r  = log(sum_v exp(x_rv))
//   loss_r = (1 - eps) (lse_r - x_r,t) + eps (lse_r - mean_v x_rv)                 eps = label smoothing, t = target[r]
//   dx_rv  = g_r (exp(x_rv - lse_r) - (1 - eps) [v == t] - eps / V)
//
// Both directions are HBM-bound row streams: a vocabulary row (128k bf16 = 256 KiB) is far too long to hold in registers the way
// norm.hip does, so the forward makes ONE pass with an online log-sum-exp: each lane keeps a running max m, a sum s of exponentials
// taken relative to h = m * log2(e) (f32-rounded), and sum x when smoothing. A 16-byte pack costs one max chain, one rescale
// (s *= 2^(h_old - h_new)) and per element one FMA (x log2e - h) plus one v_exp_f32 and one add. Lane states combine across the
// wave (xor butterfly) and the block (LDS, in wave order): a fixed order, no atomics, bitwise reproducible.
//
// Precision at large logits: x log2e - h is formed in ONE rounding inside the FMA, and h differs from m log2e by lo = fma(m, log2e, -h),
// an exactly representable residual that the finish folds back as - lo ln2: log(sum exp(x - m)) stays accurate to f32 rounding of the
// SUM even at |x| ~ 1e4, where m log2e itself has an ulp of 1e-3. The backward folds the same residual of lse into g.
//
// Regimes, picked from (rows, V) alone (the same partition on every device; ce_plan):
//   rows   V <= 4096                 one wave per row, four rows per 256-thread block
//   block  V > 4096, rows >= 1024    one 256-thread block per row
//   split  V > 4096, rows < 1024     each row cut into chunks of whole 64-element multiples, one block per chunk; every chunk writes
//                                    its partial (m, s, sum x) to caller scratch and ce_combine merges them IN CHUNK ORDER
// The backward walks the same partition without any reduction.
//
// Alignment: a segment (a row, or a chunk of one) is read as a scalar head up to the first 16-byte boundary, 16-byte packs, and a
// scalar tail, so odd row strides (V = 50257 contiguous) keep the vector loads. The backward takes the packed path when the
// logits' and the gradient's segments share their phase within 16 bytes (contiguous tensors always do), the scalar loop otherwise.
//
// -inf logits (a padded vocabulary) never produce exp(-inf - (-inf)): a state whose max is still -inf uses offset 0, and combining
// two states skips the rescale of the side whose max equals the result's.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// Every fused multiply-add here is written out (fmaf). Contraction would otherwise fuse m_old * log2e - h_new into one FMA, whose
// exact product no longer cancels against the rounded h_old that s was taken relative to: 2^-11 of exponent at |x| ~ 1e4.
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kCeBlock = 256;
constexpr int64_t kCeShortRow = 4096;   // V up to this: one wave per row
constexpr int64_t kCeManyRows = 1024;   // at least this many long rows: one block per row
constexpr int64_t kCeSplitBlocks = 2048; // the split regime aims for this many blocks in all
constexpr int64_t kCeMinChunk = 4096;   // elements per chunk, at least

// the online state: s = sum 2^(x log2e - h(m)), h(m) = m * log2e rounded to f32 (0 while m = -inf)
struct CeState { float m, s, sx; };
__device__ __forceinline__ float ce_h(float m) { return m == -INFINITY ? 0.f : m * kLog2e; }
__device__ __forceinline__ float ce_exp2(float v) { return __builtin_amdgcn_exp2f(v); }

// s taken relative to h(m_old), moved to h(m_new), m_new >= m_old. m_old * log2e (not h: -inf stays -inf) makes the factor 0 for a state
// that has seen only -inf; with 0 there, exp2(0 - h_new) overflows to inf for m_new below -89 and 0 * inf is NaN.
__device__ __forceinline__ float ce_rescale(float s, float m_old, float m_new, float h_new) {
    return m_old == m_new ? s : s * ce_exp2(m_old * kLog2e - h_new);
}

__device__ __forceinline__ CeState ce_combine(const CeState &a, const CeState &b) {
    const float m = fmaxf(a.m, b.m), h = ce_h(m);
    return {m, ce_rescale(a.s, a.m, m, h) + ce_rescale(b.s, b.m, m, h), a.sx + b.sx};
}

// N values of one lane into its state: one max chain, one rescale, per value one FMA + one exp + one add
template <int N, bool SMOOTH>
__device__ __forceinline__ void ce_absorb(CeState &st, const float (&f)[N]) {
    float pm = f[0];
#pragma unroll
    for (int i = 1; i < N; ++i) pm = fmaxf(pm, f[i]);
    const float m = fmaxf(st.m, pm), h = ce_h(m);
    float s = ce_rescale(st.s, st.m, m, h);
#pragma unroll
    for (int i = 0; i < N; ++i) s += ce_exp2(fmaf(f[i], kLog2e, -h));
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
__device__ __forceinline__ CeState ce_segment_state(const T *row, int64_t c0, int64_t c1, int lane) {
    constexpr int V = kPack16<T>, U = 2;
    CeState st{-INFINITY, 0.f, 0.f};
    const T *p = row + c0;
    const int64_t n = c1 - c0;
    const int64_t head = std::min<int64_t>(n, (int64_t)((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u) / (int64_t)sizeof(T));
    const int64_t nb = (n - head) / V, t0 = head + nb * V;
    if (lane < head) { const float f[1] = {load_f32(p + lane)}; ce_absorb<1, SMOOTH>(st, f); }
    if (t0 + lane < n) { const float f[1] = {load_f32(p + t0 + lane)}; ce_absorb<1, SMOOTH>(st, f); }
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
                ce_absorb<V, SMOOTH>(st, f);
            }
        }
    }
    return st;
}

// combine across the NT lanes of a segment (NT = 64: the wave; 256: the block through LDS, in wave order). Lane 0 holds the result.
template <int NT>
__device__ __forceinline__ CeState ce_reduce_state(CeState st, CeState *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const CeState b{__shfl_xor(st.m, o, 64), __shfl_xor(st.s, o, 64), __shfl_xor(st.sx, o, 64)};
        st = ce_combine(st, b);
    }
    if constexpr (NT > 64) {
        const int wid = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) red[wid] = st;
        __syncthreads();
        st = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) st = ce_combine(st, red[w]);
    }
    return st;
}

struct CeFwdArgs {
    const void *x;
    const int64_t *target;
    float *rowloss;  // [rows]: the loss per row (the caller's output for NONE, scratch otherwise)
    float *lse;      // [rows] or null
    float *part;     // split: [rows][nchunk] states
    int64_t rows, V, ld, ignore_index, chunk;  // chunk: elements per chunk (split)
    int nchunk;
    float eps;
};

// a row's loss and lse from its combined state
template <typename T>
__device__ __forceinline__ void ce_finish(const CeFwdArgs &a, int64_t row, const CeState &st) {
    const int64_t t = a.target[row];
    const float lo = st.m == -INFINITY ? 0.f : fmaf(st.m, kLog2e, -ce_h(st.m));
    const float lns = logf(st.s) - lo * kLn2; // log(sum exp(x - m))
    if (a.lse) a.lse[row] = st.m + lns;
    float loss;
    if (t == a.ignore_index) {
        loss = 0.f;
    } else if (t < 0 || t >= a.V) {
        loss = __builtin_nanf("");
    } else {
        const float xt = load_f32((const T *)a.x + row * a.ld + t);
        loss = 0.f;
        if (a.eps < 1.f) loss = (1.f - a.eps) * ((st.m - xt) + lns);
        if (a.eps > 0.f) loss += a.eps * ((st.m - st.sx / (float)a.V) + lns);
    }
    a.rowloss[row] = loss;
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(kCeBlock) void ce_fwd_rows(const CeFwdArgs a) {
    const int64_t row = (int64_t)blockIdx.x * (kCeBlock / 64) + (threadIdx.x >> 6);
    if (row >= a.rows) return; // whole waves
    const int lane = threadIdx.x & 63;
    CeState st = ce_segment_state<T, 64, SMOOTH>((const T *)a.x + row * a.ld, 0, a.V, lane);
    st = ce_reduce_state<64>(st, nullptr);
    if (lane == 0) ce_finish<T>(a, row, st);
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(kCeBlock) void ce_fwd_block(const CeFwdArgs a) {
    __shared__ CeState red[kCeBlock / 64];
    const int64_t row = blockIdx.x;
    CeState st = ce_segment_state<T, kCeBlock, SMOOTH>((const T *)a.x + row * a.ld, 0, a.V, threadIdx.x);
    st = ce_reduce_state<kCeBlock>(st, red);
    if (threadIdx.x == 0) ce_finish<T>(a, row, st);
}

template <typename T, bool SMOOTH>
__global__ __launch_bounds__(kCeBlock) void ce_fwd_split(const CeFwdArgs a) {
    __shared__ CeState red[kCeBlock / 64];
    const int64_t row = blockIdx.x / a.nchunk;
    const int j = (int)(blockIdx.x % a.nchunk);
    const int64_t c0 = (int64_t)j * a.chunk, c1 = std::min<int64_t>(a.V, c0 + a.chunk);
    CeState st = ce_segment_state<T, kCeBlock, SMOOTH>((const T *)a.x + row * a.ld, c0, c1, threadIdx.x);
    st = ce_reduce_state<kCeBlock>(st, red);
    if (threadIdx.x == 0) {
        float *o = a.part + ((int64_t)row * a.nchunk + j) * 3;
        o[0] = st.m; o[1] = st.s; o[2] = st.sx;
    }
}

// one thread per row: the chunk partials in chunk order, then the row's loss
template <typename T>
__global__ __launch_bounds__(kCeBlock) void ce_combine(const CeFwdArgs a) {
    const int64_t row = (int64_t)blockIdx.x * kCeBlock + threadIdx.x;
    if (row >= a.rows) return;
    const float *p = a.part + row * a.nchunk * 3;
    CeState st{p[0], p[1], p[2]};
    for (int j = 1; j < a.nchunk; ++j) st = ce_combine(st, CeState{p[3 * j], p[3 * j + 1], p[3 * j + 2]});
    ce_finish<T>(a, row, st);
}

// loss = sum (or mean over the rows not ignored) of rowloss; count = the rows not ignored. One block, fixed order: thread i adds
// rows i, i + 1024, ... in turn, then a tree through LDS.
__global__ __launch_bounds__(1024) void ce_reduce(const float *rowloss, const int64_t *target, int64_t rows, int64_t ignore_index, int mean,
                                                 float *loss, float *count) {
    __shared__ float rs[1024], rc[1024];
    float s = 0.f, c = 0.f;
    for (int64_t r = threadIdx.x; r < rows; r += 1024) {
        if (rowloss) s += rowloss[r];
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
        if (loss) loss[0] = mean ? rs[0] / rc[0] : rs[0];
        if (count) count[0] = rc[0];
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
struct CeBwdArgs {
    const void *x;
    const int64_t *target;
    const float *lse, *grad, *count;
    void *dx;
    int64_t rows, V, ld, ldd, ignore_index, chunk;
    int nchunk, reduction;
    float eps;
};

// dx over the elements [c0, c1) of a row, lane `lane` of NT
template <typename T, int NT>
__device__ __forceinline__ void ce_bwd_segment(const CeBwdArgs &a, int64_t row, int64_t c0, int64_t c1, int lane) {
    constexpr int V = kPack16<T>, U = 2;
    const T *x = (const T *)a.x + row * a.ld + c0;
    T *dx = (T *)a.dx + row * a.ldd + c0;
    const int64_t n = c1 - c0;
    const int64_t t = a.target[row];
    if (t == a.ignore_index) { // a zero row, whatever the logits hold
        for (int64_t i = lane; i < n; i += NT) store_canonical(dx + i, 0.f);
        return;
    }
    float g = a.reduction == KF_CE_NONE ? a.grad[row] : a.grad[0];
    if (a.reduction == KF_CE_MEAN) g /= a.count[0];
    if (t < 0 || t >= a.V) g = __builtin_nanf("");
    // p = exp(x - lse) = 2^(fma(x, log2e, -hl)) * 2^-lo with hl = lse log2e rounded and lo its exact residual: 2^-lo goes into g
    const float lse = a.lse[row], hl = lse * kLog2e, lo = fmaf(lse, kLog2e, -hl);
    const float gs = g * ce_exp2(-lo), c0s = g * a.eps / (float)a.V, c1s = g * (1.f - a.eps);
    const int64_t tl = t - c0; // the target's position inside the segment (may lie outside it)
    auto one = [&](int64_t i) __attribute__((always_inline)) {
        const float v = fmaf(gs, ce_exp2(fmaf(load_f32(x + i), kLog2e, -hl)), -c0s);
        store_canonical(dx + i, i == tl ? v - c1s : v);
    };
    const uint32_t px = (uint32_t)(uintptr_t)x & 15u, pd = (uint32_t)(uintptr_t)dx & 15u;
    if (px != pd) { // the two rows sit differently against 16-byte boundaries: element by element
        for (int64_t i = lane; i < n; i += NT) one(i);
        return;
    }
    const int64_t head = std::min<int64_t>(n, (int64_t)((16u - px) & 15u) / (int64_t)sizeof(T));
    const int64_t nb = (n - head) / V, t0 = head + nb * V;
    if (lane < head) one(lane);
    if (t0 + lane < n) one(t0 + lane);
    const uint4 *q = (const uint4 *)(x + head);
    uint4 *qd = (uint4 *)(dx + head);
    for (int64_t k = lane; k < nb; k += (int64_t)NT * U) {
        uint4 raw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) raw[u] = k + (int64_t)u * NT < nb ? q[k + (int64_t)u * NT] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = k + (int64_t)u * NT;
            if (kk < nb) {
                float f[V];
                unpack16<T>(raw[u], f);
#pragma unroll
                for (int i = 0; i < V; ++i) f[i] = fmaf(gs, ce_exp2(fmaf(f[i], kLog2e, -hl)), -c0s);
                const int64_t e = tl - head - kk * V;
                if (e >= 0 && e < V) {
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        if (i == e) f[i] -= c1s;
                }
                qd[kk] = pack16<T>(f);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kCeBlock) void ce_bwd_rows(const CeBwdArgs a) {
    const int64_t row = (int64_t)blockIdx.x * (kCeBlock / 64) + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    ce_bwd_segment<T, 64>(a, row, 0, a.V, threadIdx.x & 63);
}

template <typename T>
__global__ __launch_bounds__(kCeBlock) void ce_bwd(const CeBwdArgs a) {
    const int64_t row = blockIdx.x / a.nchunk;
    const int j = (int)(blockIdx.x % a.nchunk);
    const int64_t c0 = (int64_t)j * a.chunk;
    ce_bwd_segment<T, kCeBlock>(a, row, c0, std::min<int64_t>(a.V, c0 + a.chunk), threadIdx.x);
}

// ---- the partition --------------------------------------------------------------------------------------------------------
enum CeRegime { CE_ROWS = 0, CE_BLOCK = 1, CE_SPLIT = 2 };
struct CePlan { int regime, nchunk; int64_t chunk; };
CePlan ce_plan(int64_t rows, int64_t V) {
    if (V <= kCeShortRow) return {CE_ROWS, 1, V};
    if (rows >= kCeManyRows) return {CE_BLOCK, 1, V};
    const int64_t want = std::min((V + kCeMinChunk - 1) / kCeMinChunk, (kCeSplitBlocks + std::max<int64_t>(rows, 1) - 1) / std::max<int64_t>(rows, 1));
    if (want <= 1) return {CE_BLOCK, 1, V};
    const int64_t chunk = ((V + want - 1) / want + 63) / 64 * 64;
    return {CE_SPLIT, (int)((V + chunk - 1) / chunk), chunk};
}

size_t ce_align(size_t b) { return (b + 255) / 256 * 256; }
size_t ce_part_bytes(int64_t rows, const CePlan &pl) { return pl.regime == CE_SPLIT ? ce_align((size_t)rows * pl.nchunk * 3 * sizeof(float)) : 0; }
size_t ce_rowloss_bytes(int64_t rows, int reduction) { return reduction == KF_CE_NONE ? 0 : ce_align((size_t)rows * sizeof(float)); }

} // namespace
} // namespace kf

using namespace kf;

static int ce_check(const char *who, int dtype, int64_t rows, int64_t V, int64_t ld, float label_smoothing, int reduction) {
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(reduction == KF_CE_NONE || reduction == KF_CE_SUM || reduction == KF_CE_MEAN, KF_ERR_INVALID, "%s: unknown reduction %d", who, reduction);
    KF_REQUIRE(rows >= 0 && rows <= 0x7fffffffLL, KF_ERR_INVALID, "%s: rows %lld outside [0, 2^31)", who, (long long)rows);
    KF_REQUIRE(V >= 1 && V <= 0x7fffffffLL, KF_ERR_INVALID, "%s: V %lld outside [1, 2^31)", who, (long long)V);
    KF_REQUIRE(ld >= V, KF_ERR_INVALID, "%s: row stride %lld < V %lld", who, (long long)ld, (long long)V);
    KF_REQUIRE(label_smoothing >= 0.f && label_smoothing <= 1.f, KF_ERR_INVALID, "%s: label_smoothing %g outside [0, 1]", who, (double)label_smoothing);
    return KF_OK;
}

extern "C" int kf_cross_entropy_workspace_bytes(int dtype, int64_t rows, int64_t V, int reduction, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_cross_entropy_workspace_bytes: null out pointer");
    *bytes = 0;
    const int rc = ce_check("kf_cross_entropy_workspace_bytes", dtype, rows, V, V, 0.f, reduction);
    if (rc != KF_OK) return rc;
    *bytes = ce_part_bytes(rows, ce_plan(rows, V)) + ce_rowloss_bytes(rows, reduction);
    return KF_OK;
}

extern "C" int kf_cross_entropy_fwd(int dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target,
                                    int64_t ignore_index, float label_smoothing, int reduction, float *loss, float *lse, float *count,
                                    void *workspace, size_t workspace_bytes, void *stream) {
    int rc = ce_check("kf_cross_entropy_fwd", dtype, rows, V, ld, label_smoothing, reduction);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(loss, KF_ERR_INVALID, "kf_cross_entropy_fwd: null loss");
    KF_REQUIRE(rows == 0 || (logits && target), KF_ERR_INVALID, "kf_cross_entropy_fwd: null logits or target");
    KF_REQUIRE((uintptr_t)logits % dtype_size(dtype) == 0, KF_ERR_INVALID, "kf_cross_entropy_fwd: logits not aligned to their element size");
    const CePlan pl = ce_plan(rows, V);
    const size_t pb = ce_part_bytes(rows, pl), need = pb + ce_rowloss_bytes(rows, reduction);
    KF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), KF_ERR_INVALID, "kf_cross_entropy_fwd: workspace of %zu bytes required, got %zu",
               need, workspace ? workspace_bytes : (size_t)0);
    hipStream_t st = as_stream(stream);
    CeFwdArgs a{logits, target, reduction == KF_CE_NONE ? loss : (float *)((char *)workspace + pb), lse, (float *)workspace, rows, V, ld,
                ignore_index, pl.chunk, pl.nchunk, label_smoothing};
    const bool smooth = label_smoothing > 0.f;
    if (rows > 0) {
        rc = with_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return with_flags([&](auto SMOOTH) {
                if (pl.regime == CE_ROWS) {
                    KF_PROF("ce_fwd_rows", st);
                    return launch(ce_fwd_rows<T, SMOOTH>, (unsigned)((rows + kCeBlock / 64 - 1) / (kCeBlock / 64)), kCeBlock, 0, st, a);
                }
                if (pl.regime == CE_BLOCK) {
                    KF_PROF("ce_fwd_block", st);
                    return launch(ce_fwd_block<T, SMOOTH>, (unsigned)rows, kCeBlock, 0, st, a);
                }
                {
                    KF_PROF("ce_fwd_split", st);
                    const int rs = launch(ce_fwd_split<T, SMOOTH>, (unsigned)(rows * pl.nchunk), kCeBlock, 0, st, a);
                    if (rs != KF_OK) return rs;
                }
                KF_PROF("ce_combine", st);
                return launch(ce_combine<T>, (unsigned)((rows + kCeBlock - 1) / kCeBlock), kCeBlock, 0, st, a);
            }, smooth);
        });
        if (rc != KF_OK) return rc;
    }
    if (reduction != KF_CE_NONE || count) {
        KF_PROF("ce_reduce", st);
        return launch(ce_reduce, 1, 1024, 0, st, reduction == KF_CE_NONE ? nullptr : a.rowloss, target, rows, ignore_index, (int)(reduction == KF_CE_MEAN),
                      reduction == KF_CE_NONE ? nullptr : loss, count);
    }
    return KF_OK;
}

extern "C" int kf_cross_entropy_bwd(int dtype, int64_t rows, int64_t V, int64_t ld, const void *logits, const int64_t *target,
                                    int64_t ignore_index, float label_smoothing, int reduction, const float *lse, const float *count,
                                    const float *grad, void *dlogits, int64_t ldd, void *stream) {
    int rc = ce_check("kf_cross_entropy_bwd", dtype, rows, V, ld, label_smoothing, reduction);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(ldd >= V, KF_ERR_INVALID, "kf_cross_entropy_bwd: gradient row stride %lld < V %lld", (long long)ldd, (long long)V);
    if (rows == 0) return KF_OK;
    KF_REQUIRE(logits && target && lse && grad && dlogits, KF_ERR_INVALID, "kf_cross_entropy_bwd: null operand");
    KF_REQUIRE(reduction != KF_CE_MEAN || count, KF_ERR_INVALID, "kf_cross_entropy_bwd: the mean's backward needs count");
    KF_REQUIRE((uintptr_t)logits % dtype_size(dtype) == 0 && (uintptr_t)dlogits % dtype_size(dtype) == 0, KF_ERR_INVALID,
               "kf_cross_entropy_bwd: logits or dlogits not aligned to their element size");
    hipStream_t st = as_stream(stream);
    const CePlan pl = ce_plan(rows, V);
    CeBwdArgs a{logits, target, lse, grad, count, dlogits, rows, V, ld, ldd, ignore_index, pl.chunk, pl.nchunk, reduction, label_smoothing};
    KF_PROF("ce_bwd", st);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return pl.regime == CE_ROWS ? launch(ce_bwd_rows<T>, (unsigned)((rows + kCeBlock / 64 - 1) / (kCeBlock / 64)), kCeBlock, 0, st, a)
                                    : launch(ce_bwd<T>, (unsigned)(rows * pl.nchunk), kCeBlock, 0, st, a);
    });
}
