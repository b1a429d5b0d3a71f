// Fused multi-tensor AdamW step for gfx950 (torch.optim.AdamW: decoupled weight decay, no amsgrad, no maximize), with optional
// global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) in the same call.
//
// Per element, in f32, with g = grad * grad_scale * clip_coef and s the tensor's step count after it advances:
//   p = p (1 - lr wd);  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p = p + (-lr / (1 - b1^s)) m / (sqrt(v) / sqrt(1 - b2^s) + eps)
// The per-tensor scalars (1 - lr wd, lr / (1 - b1^s), sqrt(1 - b2^s)) are formed in double from the device lr and step and rounded
// once to f32, as torch forms them in Python floats.
//
// Multi-tensor: every launch carries up to kAdamK = 48 tensors' pointers, sizes, dtypes and weight decays in its kernel arguments
// (AdamwArgs, 3.2 KiB), as torch's multi_tensor_apply does: no host -> device table, nothing to copy, nothing to allocate. A tensor of
// n elements is cut into ceil(n / 4096) chunks; block b of a launch finds its (tensor, chunk) by a binary search over the chunk prefix
// sums, which are uniform values in SGPRs. Launches per call, a function of the tensor count N alone:
//   no clipping:    2 ceil(N / K)       per group: adamw_advance (steps += 1), adamw_update
//   clipping:       2 ceil(N / K) + 1   per group: adamw_norm (partial sums of g^2, steps += 1); then adamw_fold once; then adamw_update
// Clipping folds kAdamNormGrid f32 partial sums per group in a fixed order (double accumulation, no atomics) into the norm and
// clip_coef = min(1, max_norm / (norm + 1e-6)), which the update reads on the device: bitwise reproducible, graph-capturable.
//
// Layout: a tensor is read as a scalar head of h < 8 elements, 8-element packs (one 16-byte access per 16-bit stream, two per f32 stream),
// and a scalar tail. h is the one count after which every stream of the tensor (param, grad, master, exp_avg, exp_avg_sq) sits on a
// 16-byte boundary; when no such h exists (the streams' phases disagree) the tensor goes element by element. All index arithmetic is
// 64-bit.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

namespace kf {

namespace {

constexpr int kAdamK = 48;               // tensors per launch (kernel-argument bytes: sizeof(AdamwArgs) below 4 KiB)
constexpr int kAdamBlock = 256;
constexpr int64_t kAdamChunk = 4096;     // elements per block
constexpr int kAdamPack = 8;             // elements per pack
constexpr int kAdamNormGrid = 2048;      // blocks (and partial sums) of one norm launch
constexpr int kAdamFoldThreads = 1024;
constexpr size_t kAdamHeader = 256;      // workspace: clip_coef, then the partial sums

enum { AD_F32 = 0, AD_BF16 = 1, AD_F16 = 2 };

struct AdamwArgs {
    void *param[kAdamK];
    const void *grad[kAdamK];
    float *master[kAdamK];
    float *m[kAdamK];
    float *v[kAdamK];
    float *step[kAdamK];
    int64_t numel[kAdamK];
    float wd[kAdamK];
    int32_t chunk0[kAdamK + 1];          // chunk prefix sums: tensor t owns the launch's chunks [chunk0[t], chunk0[t + 1])
    uint8_t pdt[kAdamK], gdt[kAdamK];    // AD_*
    int count;
    double b1, b2;
    float b1f, omb1, b2f, omb2, eps, gscale;
    const float *lr;
    const float *coef;                   // clip_coef on the device; null: no clipping
    float *partial;                      // norm launch: this group's kAdamNormGrid partial sums
};
static_assert(sizeof(AdamwArgs) <= 4096, "kernel arguments above 4 KiB");

// pack k (8 elements) of a 16-byte-aligned stream: one 16-byte pack of a 16-bit stream, two of an f32 one
template <typename T>
__device__ __forceinline__ void ad_ldv(const T *base, int64_t k, float (&f)[kAdamPack]) {
    const uint4 *q = (const uint4 *)base;
    if constexpr (sizeof(T) == 4) {
        float lo[4], hi[4];
        unpack16<T>(q[2 * k], lo);
        unpack16<T>(q[2 * k + 1], hi);
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[i] = lo[i]; f[4 + i] = hi[i]; }
    } else {
        unpack16<T>(q[k], f);
    }
}
template <typename T>
__device__ __forceinline__ void ad_stv(T *base, int64_t k, const float (&f)[kAdamPack]) {
    uint4 *q = (uint4 *)base;
    if constexpr (sizeof(T) == 4) {
        const float lo[4] = {f[0], f[1], f[2], f[3]}, hi[4] = {f[4], f[5], f[6], f[7]};
        q[2 * k] = pack16<T>(lo);
        q[2 * k + 1] = pack16<T>(hi);
    } else {
        q[k] = pack16<T>(f);
    }
}

// the elements from `p` to its next 16-byte boundary, and that count's period (16 / element size)
__device__ __forceinline__ void ad_phase(const void *p, int esize, uint32_t &r2, uint32_t &r4, bool &have2, bool &have4, bool &ok) {
    const uint32_t r = ((16u - ((uint32_t)(uintptr_t)p & 15u)) & 15u) / (uint32_t)esize;
    if (esize == 2) { ok = ok && (!have2 || r == r2); r2 = r; have2 = true; }
    else { ok = ok && (!have4 || r == r4); r4 = r; have4 = true; }
}

// which tensor of the launch owns chunk q (uniform: q comes from blockIdx)
__device__ __forceinline__ int ad_find(const AdamwArgs &a, int32_t q) {
    int lo = 0, hi = a.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.chunk0[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct AdCoef { float decay, b1, omb1, b2, omb2, bc2s, eps, nss, gmul; };

// the tensor's per-step scalars: s is its step count (already advanced), lr and clip_coef are read on the device
__device__ __forceinline__ AdCoef ad_coef(const AdamwArgs &a, int t) {
    const double s = (double)*a.step[t], lr = (double)*a.lr;
    AdCoef c;
    c.decay = (float)(1.0 - lr * (double)a.wd[t]);
    c.b1 = a.b1f; c.omb1 = a.omb1; c.b2 = a.b2f; c.omb2 = a.omb2; c.eps = a.eps;
    c.bc2s = (float)sqrt(1.0 - pow(a.b2, s));
    c.nss = (float)(-lr / (1.0 - pow(a.b1, s)));
    c.gmul = a.gscale;
    return c;
}

__device__ __forceinline__ float ad_elem(float p, float g, float &m, float &v, const AdCoef &c) {
    p = p * c.decay;
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + c.omb2 * g * g;
    const float d = sqrtf(v) / c.bc2s + c.eps;
    return p + c.nss * m / d;
}

// chunk `ch` of one tensor: P the param's storage type, G the grad's, MASTER: the update runs on the f32 master copy
template <typename P, typename G, bool MASTER>
__device__ __forceinline__ void ad_update_chunk(const AdamwArgs &a, int t, int64_t ch, float clip) {
    P *p = (P *)a.param[t];
    const G *g = (const G *)a.grad[t];
    float *ms = a.master[t], *m = a.m[t], *v = a.v[t];
    const int64_t n = a.numel[t];
    AdCoef c = ad_coef(a, t);
    const int tid = threadIdx.x;
    auto one = [&](int64_t i) __attribute__((always_inline)) {
        const float gi = load_f32(g + i) * c.gmul * clip;
        float mi = m[i], vi = v[i];
        const float pi = ad_elem(MASTER ? ms[i] : load_f32(p + i), gi, mi, vi, c);
        m[i] = mi;
        v[i] = vi;
        if constexpr (MASTER) ms[i] = pi;
        store_hw(p + i, pi);
    };
    uint32_t r2 = 0, r4 = 0;
    bool have2 = false, have4 = false, ok = true;
    ad_phase(p, sizeof(P), r2, r4, have2, have4, ok);
    ad_phase(g, sizeof(G), r2, r4, have2, have4, ok);
    ad_phase(m, 4, r2, r4, have2, have4, ok);
    ad_phase(v, 4, r2, r4, have2, have4, ok);
    if constexpr (MASTER) ad_phase(ms, 4, r2, r4, have2, have4, ok);
    ok = ok && (!have2 || !have4 || (r2 & 3u) == r4);
    if (!ok) { // the streams' phases disagree: element by element
        const int64_t e0 = ch * kAdamChunk, e1 = std::min<int64_t>(n, e0 + kAdamChunk);
        for (int64_t i = e0 + tid; i < e1; i += kAdamBlock) one(i);
        return;
    }
    const int64_t head = std::min<int64_t>(n, have2 ? r2 : r4);
    const int64_t nb = (n - head) / kAdamPack, t0 = head + nb * kAdamPack;
    if (ch == 0) {
        if (tid < head) one(tid);
        if (t0 + tid < n) one(t0 + tid);
    }
    constexpr int64_t CP = kAdamChunk / kAdamPack; // packs per chunk: 2 per thread
    const int64_t k0 = ch * CP, k1 = std::min<int64_t>(nb, k0 + CP);
    P *pp = p + head;
    const G *gp = g + head;
    float *mp = m + head, *vp = v + head, *sp = MASTER ? ms + head : nullptr;
    constexpr int U = (int)(CP / kAdamBlock);
    float fp[U][kAdamPack], fg[U][kAdamPack], fm[U][kAdamPack], fv[U][kAdamPack];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t k = k0 + tid + (int64_t)u * kAdamBlock;
        live[u] = k < k1;
        if (live[u]) {
            if constexpr (MASTER) ad_ldv(sp, k, fp[u]); else ad_ldv(pp, k, fp[u]);
            ad_ldv(gp, k, fg[u]);
            ad_ldv(mp, k, fm[u]);
            ad_ldv(vp, k, fv[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!live[u]) continue;
        const int64_t k = k0 + tid + (int64_t)u * kAdamBlock;
#pragma unroll
        for (int i = 0; i < kAdamPack; ++i) fp[u][i] = ad_elem(fp[u][i], fg[u][i] * c.gmul * clip, fm[u][i], fv[u][i], c);
        ad_stv(mp, k, fm[u]);
        ad_stv(vp, k, fv[u]);
        if constexpr (MASTER) ad_stv(sp, k, fp[u]);
        ad_stv(pp, k, fp[u]);
    }
}

__global__ __launch_bounds__(kAdamBlock) void adamw_update(const AdamwArgs a) {
    const int32_t q = (int32_t)blockIdx.x;
    if (q >= a.chunk0[a.count]) return; // a launch whose tensors are all empty still has one block
    const int t = ad_find(a, q);
    const int64_t ch = q - a.chunk0[t];
    const float clip = a.coef ? *a.coef : 1.f;
    const int pd = a.pdt[t], gd = a.gdt[t];
    const bool master = a.master[t] != nullptr;
    if (pd == AD_F32) ad_update_chunk<float, float, false>(a, t, ch, clip);
    else if (pd == AD_BF16) {
        if (gd == AD_F32) { if (master) ad_update_chunk<bf16_t, float, true>(a, t, ch, clip); else ad_update_chunk<bf16_t, float, false>(a, t, ch, clip); }
        else { if (master) ad_update_chunk<bf16_t, bf16_t, true>(a, t, ch, clip); else ad_update_chunk<bf16_t, bf16_t, false>(a, t, ch, clip); }
    } else {
        if (gd == AD_F32) { if (master) ad_update_chunk<f16_t, float, true>(a, t, ch, clip); else ad_update_chunk<f16_t, float, false>(a, t, ch, clip); }
        else { if (master) ad_update_chunk<f16_t, f16_t, true>(a, t, ch, clip); else ad_update_chunk<f16_t, f16_t, false>(a, t, ch, clip); }
    }
}

// the steps of a group advance by one, before its update reads them (stream order: no block of the update can see the old count)
__device__ __forceinline__ void ad_advance(const AdamwArgs &a) {
    if ((int)threadIdx.x < a.count) *a.step[threadIdx.x] += 1.f;
}

__global__ __launch_bounds__(64) void adamw_advance(const AdamwArgs a) { ad_advance(a); }

// sum of (grad * grad_scale)^2 over chunk ch of tensor t, this thread's share
template <typename G>
__device__ __forceinline__ float ad_norm_chunk(const AdamwArgs &a, int t, int64_t ch) {
    const G *g = (const G *)a.grad[t];
    const int64_t n = a.numel[t];
    const float gs = a.gscale;
    const int tid = threadIdx.x;
    float s = 0.f;
    const int64_t head = std::min<int64_t>(n, (int64_t)(((16u - ((uint32_t)(uintptr_t)g & 15u)) & 15u) / (uint32_t)sizeof(G)));
    const int64_t nb = (n - head) / kAdamPack, t0 = head + nb * kAdamPack;
    if (ch == 0) {
        if (tid < head) { const float x = load_f32(g + tid) * gs; s += x * x; }
        if (t0 + tid < n) { const float x = load_f32(g + t0 + tid) * gs; s += x * x; }
    }
    constexpr int64_t CP = kAdamChunk / kAdamPack;
    constexpr int U = (int)(CP / kAdamBlock);
    const int64_t k0 = ch * CP, k1 = std::min<int64_t>(nb, k0 + CP);
    float f[U][kAdamPack];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t k = k0 + tid + (int64_t)u * kAdamBlock;
        if (k < k1) ad_ldv(g + head, k, f[u]);
        else {
#pragma unroll
            for (int i = 0; i < kAdamPack; ++i) f[u][i] = 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int i = 0; i < kAdamPack; ++i) { const float x = f[u][i] * gs; s += x * x; }
    }
    return s;
}

// block b sums the chunks b, b + grid, ... of the group, folds its 256 lanes in a fixed order and writes partial[b]; block 0 also
// advances the group's steps (nothing reads them before the update, which runs after the fold)
__global__ __launch_bounds__(kAdamBlock) void adamw_norm(const AdamwArgs a) {
    __shared__ float red[kAdamBlock / 64];
    float s = 0.f;
    for (int32_t q = blockIdx.x; q < a.chunk0[a.count]; q += gridDim.x) {
        const int t = ad_find(a, q);
        const int64_t ch = q - a.chunk0[t];
        const int gd = a.gdt[t];
        s += gd == AD_F32 ? ad_norm_chunk<float>(a, t, ch) : gd == AD_BF16 ? ad_norm_chunk<bf16_t>(a, t, ch) : ad_norm_chunk<f16_t>(a, t, ch);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float b = red[0];
#pragma unroll
        for (int w = 1; w < kAdamBlock / 64; ++w) b += red[w];
        a.partial[blockIdx.x] = b;
    }
    if (blockIdx.x == 0) ad_advance(a);
}

// one block: the n partial sums in a fixed order (thread i takes i, i + 1024, ... in double; then a tree), the norm and clip_coef
__global__ __launch_bounds__(kAdamFoldThreads) void adamw_fold(const float *partial, int64_t n, float max_norm, float *coef, float *norm_out) {
    __shared__ double rs[kAdamFoldThreads];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kAdamFoldThreads) s += (double)partial[i];
    rs[threadIdx.x] = s;
    __syncthreads();
    for (int w = kAdamFoldThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) rs[threadIdx.x] += rs[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(rs[0]);
        const float c = max_norm / (norm + 1e-6f);
        coef[0] = c > 1.f ? 1.f : c; // a NaN norm gives a NaN coefficient, as torch's clamp does (fminf would return 1)
        if (norm_out) norm_out[0] = norm;
    }
}

int ad_dt(int dtype) { return dtype == KF_F32 ? AD_F32 : dtype == KF_BF16 ? AD_BF16 : AD_F16; }
int64_t ad_chunks(int64_t n) { return (n + kAdamChunk - 1) / kAdamChunk; }
int64_t ad_groups(int64_t n) { return (n + kAdamK - 1) / kAdamK; }

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_adamw_workspace_bytes(int64_t n, float max_grad_norm, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_adamw_workspace_bytes: null out pointer");
    *bytes = 0;
    KF_REQUIRE(n >= 0, KF_ERR_INVALID, "kf_adamw_workspace_bytes: tensor count %lld < 0", (long long)n);
    KF_REQUIRE(!(max_grad_norm != max_grad_norm), KF_ERR_INVALID, "kf_adamw_workspace_bytes: max_grad_norm is NaN");
    if (max_grad_norm > 0.f) *bytes = kAdamHeader + (size_t)ad_groups(n) * kAdamNormGrid * sizeof(float);
    return KF_OK;
}

extern "C" int kf_adamw_step(const kf_adamw_tensor *tensors, int64_t n, double beta1, double beta2, double eps, const float *lr,
                             float grad_scale, float max_grad_norm, float *grad_norm, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_adamw_step";
    KF_REQUIRE(n >= 0, KF_ERR_INVALID, "%s: tensor count %lld < 0", who, (long long)n);
    KF_REQUIRE(n == 0 || tensors, KF_ERR_INVALID, "%s: null tensors", who);
    KF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0, KF_ERR_INVALID, "%s: beta1 %g outside [0, 1)", who, beta1);
    KF_REQUIRE(beta2 >= 0.0 && beta2 < 1.0, KF_ERR_INVALID, "%s: beta2 %g outside [0, 1)", who, beta2);
    KF_REQUIRE(eps >= 0.0 && eps < INFINITY, KF_ERR_INVALID, "%s: eps %g outside [0, inf)", who, eps);
    KF_REQUIRE(lr, KF_ERR_INVALID, "%s: null lr (a device float [1])", who);
    KF_REQUIRE(isfinite(grad_scale), KF_ERR_INVALID, "%s: grad_scale %g is not finite", who, (double)grad_scale);
    KF_REQUIRE(!(max_grad_norm != max_grad_norm), KF_ERR_INVALID, "%s: max_grad_norm is NaN", who);
    const bool clip = max_grad_norm > 0.f;
    KF_REQUIRE(clip || !grad_norm, KF_ERR_INVALID, "%s: grad_norm needs max_grad_norm > 0 (INFINITY: the norm without clipping)", who);
    for (int64_t i = 0; i < n; ++i) {
        const kf_adamw_tensor &t = tensors[i];
        const int pd = t.param_dtype, gd = t.grad_dtype;
        KF_REQUIRE(pd == KF_F32 || pd == KF_BF16 || pd == KF_F16, KF_ERR_INVALID, "%s: tensor %lld: param dtype %d not supported (float, half, bfloat16)",
                   who, (long long)i, pd);
        KF_REQUIRE(gd == KF_F32 || gd == pd, KF_ERR_INVALID, "%s: tensor %lld: grad dtype %d is neither float nor the param's dtype %d", who,
                   (long long)i, gd, pd);
        KF_REQUIRE(t.numel >= 0, KF_ERR_INVALID, "%s: tensor %lld: numel %lld < 0", who, (long long)i, (long long)t.numel);
        KF_REQUIRE(ad_chunks(t.numel) < (1LL << 30), KF_ERR_INVALID, "%s: tensor %lld: numel %lld too large", who, (long long)i, (long long)t.numel);
        KF_REQUIRE(!t.master || pd != KF_F32, KF_ERR_INVALID, "%s: tensor %lld: a master copy is for 16-bit params only", who, (long long)i);
        KF_REQUIRE(t.weight_decay >= 0.f && t.weight_decay < INFINITY, KF_ERR_INVALID, "%s: tensor %lld: weight_decay %g outside [0, inf)", who,
                   (long long)i, (double)t.weight_decay);
        KF_REQUIRE(t.step, KF_ERR_INVALID, "%s: tensor %lld: null step", who, (long long)i);
        KF_REQUIRE(t.numel == 0 || (t.param && t.grad && t.exp_avg && t.exp_avg_sq), KF_ERR_INVALID, "%s: tensor %lld: null param, grad, exp_avg or exp_avg_sq",
                   who, (long long)i);
        const uintptr_t ps = (uintptr_t)dtype_size(pd), gs = (uintptr_t)dtype_size(gd);
        KF_REQUIRE((uintptr_t)t.param % ps == 0 && (uintptr_t)t.grad % gs == 0 && (uintptr_t)t.master % 4 == 0 && (uintptr_t)t.exp_avg % 4 == 0 &&
                       (uintptr_t)t.exp_avg_sq % 4 == 0 && (uintptr_t)t.step % 4 == 0,
                   KF_ERR_INVALID, "%s: tensor %lld: a pointer not aligned to its element size", who, (long long)i);
    }
    size_t need = 0;
    kf_adamw_workspace_bytes(n, max_grad_norm, &need);
    KF_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), KF_ERR_INVALID, "%s: workspace of %zu bytes required, got %zu", who, need,
               workspace ? workspace_bytes : (size_t)0);
    KF_REQUIRE((uintptr_t)workspace % 4 == 0, KF_ERR_INVALID, "%s: workspace not 4-byte aligned", who);

    hipStream_t st = as_stream(stream);
    const int64_t ng = ad_groups(n);
    float *coef = clip ? (float *)workspace : nullptr, *partial = clip ? (float *)((char *)workspace + kAdamHeader) : nullptr;
    auto group = [&](int64_t gi, AdamwArgs &a) {
        memset(&a, 0, sizeof(a));
        const int64_t i0 = gi * kAdamK;
        a.count = (int)std::min<int64_t>(kAdamK, n - i0);
        int32_t c = 0;
        for (int j = 0; j < a.count; ++j) {
            const kf_adamw_tensor &t = tensors[i0 + j];
            a.param[j] = t.param;
            a.grad[j] = t.grad;
            a.master[j] = t.master;
            a.m[j] = t.exp_avg;
            a.v[j] = t.exp_avg_sq;
            a.step[j] = t.step;
            a.numel[j] = t.numel;
            a.wd[j] = t.weight_decay;
            a.pdt[j] = (uint8_t)ad_dt(t.param_dtype);
            a.gdt[j] = (uint8_t)ad_dt(t.grad_dtype);
            a.chunk0[j] = c;
            c += (int32_t)ad_chunks(t.numel);
        }
        a.chunk0[a.count] = c;
        a.b1 = beta1; a.b2 = beta2;
        a.b1f = (float)beta1; a.omb1 = (float)(1.0 - beta1); a.b2f = (float)beta2; a.omb2 = (float)(1.0 - beta2);
        a.eps = (float)eps; a.gscale = grad_scale;
        a.lr = lr;
        a.coef = coef;
        a.partial = partial ? partial + gi * kAdamNormGrid : nullptr;
        return c;
    };
    // chunk prefix sums of one launch stay below 2^31 (48 tensors below 2^30 chunks each would not): checked before the first launch
    for (int64_t gi = 0; gi < ng; ++gi) {
        int64_t c = 0;
        for (int64_t i = gi * kAdamK; i < std::min<int64_t>(n, (gi + 1) * kAdamK); ++i) c += ad_chunks(tensors[i].numel);
        KF_REQUIRE(c < 0x7fffffffLL, KF_ERR_INVALID, "%s: tensors %lld.. hold %lld chunks of %lld elements, above 2^31", who, (long long)(gi * kAdamK),
                   (long long)c, (long long)kAdamChunk);
    }
    AdamwArgs a;
    if (clip) {
        {
            KF_PROF("adamw_norm", st);
            for (int64_t gi = 0; gi < ng; ++gi) {
                group(gi, a);
                const int rc = launch(adamw_norm, kAdamNormGrid, kAdamBlock, 0, st, a);
                if (rc != KF_OK) return rc;
            }
        }
        KF_PROF("adamw_fold", st);
        const int rc = launch(adamw_fold, 1, kAdamFoldThreads, 0, st, partial, ng * kAdamNormGrid, max_grad_norm, coef, grad_norm);
        if (rc != KF_OK) return rc;
    }
    KF_PROF("adamw_update", st);
    for (int64_t gi = 0; gi < ng; ++gi) {
        const int32_t chunks = group(gi, a);
        int rc = clip ? KF_OK : launch(adamw_advance, 1, 64, 0, st, a);
        if (rc == KF_OK) rc = launch(adamw_update, (unsigned)std::max<int32_t>(1, chunks), kAdamBlock, 0, st, a);
        if (rc != KF_OK) return rc;
    }
    return KF_OK;
}
