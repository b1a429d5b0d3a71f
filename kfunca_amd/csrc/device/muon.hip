// The memory-bound ends of a Muon step for gfx950; the Newton-Schulz iteration between them runs on kf_gemm_sym and kf_gemm.
//
//   kf_muon_prepare   buf = mu buf + g (g = grad * grad_scale, buf the f32 momentum); u = g + mu buf (Nesterov) or buf;
//                     X = bf16(u / (|u|_F + 1e-7)) in the WIDE orientation [min(rows, cols), max(rows, cols)], zero-extended to [xm, xn]
//   kf_muon_apply     p = p (1 - lr wd) - lr scale O, with O in the wide orientation; on the f32 master when there is one
//
// prepare is two launches. muon_momentum updates the buffer and writes one partial sum of u^2 per block into the caller's workspace
// (each thread its elements in index order, a wave by shuffles, the four waves in order). muon_scale cuts X into 64 x 64 tiles; every
// block folds the partial sums itself in one fixed order (double), forms 1 / (sqrt(sum) + 1e-7) and writes its tile - u is formed again
// from grad and the new buffer, 6 to 8 bytes read per element instead of an f32 copy of u written and read. When rows > cols the tile goes
// through LDS, so both the reads of grad / buf and the stores of X are contiguous. apply reads O the same way. No atomics, no host read,
// no allocation: two calls give the same bits and both entries can be captured.
#include <math.h>

#include <algorithm>

#include "float_pack.h"

namespace kf {
namespace {

constexpr int kMuonBlock = 256;
constexpr int kMuonPartials = 1024; // blocks of muon_momentum at most: the workspace is this many floats
constexpr int kMuonTile = 64;

template <typename G> __device__ __forceinline__ void mu_load4(const G *p, float (&f)[4]) {
    if constexpr (sizeof(G) == 4) {
        const float4 q = *(const float4 *)p;
        f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
    } else {
        const uint2 q = *(const uint2 *)p;
        const uint16_t h[4] = {(uint16_t)q.x, (uint16_t)(q.x >> 16), (uint16_t)q.y, (uint16_t)(q.y >> 16)};
#pragma unroll
        for (int i = 0; i < 4; ++i) { const G e{h[i]}; f[i] = load_f32(&e); }
    }
}

// b = mu b + grad gs, formed in double and rounded once (in f32 a cancelling pair would leave the rounding of one product in the
// state for good; the kernel is bound by memory either way); no buffer: mu is 0 and b = grad gs. Returns u.
__device__ __forceinline__ float mu_step(float grad, float &b, float mu, float gs, int nesterov) {
    b = (float)((double)mu * (double)b + (double)grad * (double)gs);
    return nesterov ? grad * gs + mu * b : b;
}

template <typename G>
__global__ __launch_bounds__(kMuonBlock) void muon_momentum(const G *grad, float *buf, int64_t n, float mu, float gs, int nesterov, float *partial) {
    __shared__ float red[kMuonBlock / 64];
    const int64_t gid = (int64_t)blockIdx.x * kMuonBlock + threadIdx.x, nthr = (int64_t)gridDim.x * kMuonBlock;
    const bool vec = ((uintptr_t)grad % (4 * sizeof(G))) == 0 && (!buf || (uintptr_t)buf % 16 == 0);
    const int64_t n4 = vec ? n / 4 : 0;
    float s = 0.f;
    for (int64_t i = gid; i < n4; i += nthr) {
        float g[4], b[4] = {0.f, 0.f, 0.f, 0.f};
        mu_load4<G>(grad + 4 * i, g);
        if (buf) mu_load4<float>(buf + 4 * i, b);
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float u = mu_step(g[e], b[e], mu, gs, nesterov); s += u * u; }
        if (buf) *(float4 *)(buf + 4 * i) = float4{b[0], b[1], b[2], b[3]};
    }
    for (int64_t i = 4 * n4 + gid; i < n; i += nthr) {
        float b = buf ? buf[i] : 0.f;
        const float u = mu_step(load_f32(grad + i), b, mu, gs, nesterov);
        s += u * u;
        if (buf) buf[i] = b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the np partial sums in one fixed order (thread t takes t, t + 256, ... in double; then a tree): 1 / (sqrt(sum) + 1e-7)
__device__ __forceinline__ float mu_inv_norm(const float *partial, int np, double *rs) {
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += kMuonBlock) s += (double)partial[i];
    rs[threadIdx.x] = s;
    __syncthreads();
    for (int w = kMuonBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) rs[threadIdx.x] += rs[threadIdx.x + w];
        __syncthreads();
    }
    return (float)(1.0 / (sqrt(rs[0]) + 1e-7));
}

// One 64 x 64 tile of X [xm, xn] (pitch ldx): X[a, b] = u(r, c) / (|u| + 1e-7) with (r, c) = (a, b), or (b, a) when TR (rows > cols);
// +0 outside the wide matrix. Lanes run along c when reading and along b when writing.
template <typename G, bool TR>
__global__ __launch_bounds__(kMuonBlock) void muon_scale(const G *grad, const float *buf, int64_t rows, int64_t cols, float mu, float gs, int nesterov,
                                                        const float *partial, int np, bf16_t *X, int64_t xm, int64_t xn, int64_t ldx) {
    __shared__ double rs[kMuonBlock];
    __shared__ float tile[kMuonTile][kMuonTile + 1];
    const float inv = mu_inv_norm(partial, np, rs);
    const int64_t tb = (xn + kMuonTile - 1) / kMuonTile;
    const int64_t a0 = (int64_t)(blockIdx.x / tb) * kMuonTile, b0 = (int64_t)(blockIdx.x % tb) * kMuonTile;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    auto u_at = [&](int64_t r, int64_t c) -> float {
        if (r >= rows || c >= cols) return 0.f;
        const int64_t i = r * cols + c;
        const float g = load_f32(grad + i) * gs;
        return (buf ? (nesterov ? g + mu * buf[i] : buf[i]) : g) * inv;
    };
    if constexpr (TR) {
        for (int y = ty; y < kMuonTile; y += kMuonBlock / 64) tile[y][tx] = u_at(b0 + y, a0 + tx);
        __syncthreads();
    }
    for (int y = ty; y < kMuonTile; y += kMuonBlock / 64) {
        const int64_t a = a0 + y, b = b0 + tx;
        if (a >= xm || b >= xn) continue;
        X[a * ldx + b] = f32_to_bf16(TR ? tile[tx][y] : u_at(a, b));
    }
}

// One 64 x 64 tile of the param [rows, cols]: p = p decay - step O, O[r, c] or, when TR, O[c, r]
template <typename P, bool TR>
__global__ __launch_bounds__(kMuonBlock) void muon_apply(P *param, float *master, int64_t rows, int64_t cols, const bf16_t *O, int64_t ldo, const float *lr,
                                                        float wd, float scale) {
    __shared__ float tile[kMuonTile][kMuonTile + 1];
    const int64_t tc = (cols + kMuonTile - 1) / kMuonTile;
    const int64_t r0 = (int64_t)(blockIdx.x / tc) * kMuonTile, c0 = (int64_t)(blockIdx.x % tc) * kMuonTile;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const double l = (double)*lr, decay = 1.0 - l * (double)wd, step = l * (double)scale; // the update in double, rounded once
    if constexpr (TR) {
        for (int y = ty; y < kMuonTile; y += kMuonBlock / 64) {
            const int64_t c = c0 + y, r = r0 + tx;
            tile[y][tx] = c < cols && r < rows ? bf16_to_f32(O[c * ldo + r]) : 0.f;
        }
        __syncthreads();
    }
    for (int y = ty; y < kMuonTile; y += kMuonBlock / 64) {
        const int64_t r = r0 + y, c = c0 + tx;
        if (r >= rows || c >= cols) continue;
        const int64_t i = r * cols + c;
        const float o = TR ? tile[tx][y] : bf16_to_f32(O[r * ldo + c]);
        const float p = (float)((double)(master ? master[i] : load_f32(param + i)) * decay - step * (double)o);
        if (master) master[i] = p;
        store_hw(param + i, p);
    }
}

bool mu_dtype_ok(int dt) { return dt == KF_F32 || dt == KF_BF16 || dt == KF_F16; }

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_muon_prepare_workspace_bytes(int64_t rows, int64_t cols, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_muon_prepare_workspace_bytes: null out pointer");
    *bytes = 0;
    KF_REQUIRE(rows >= 0 && cols >= 0, KF_ERR_INVALID, "kf_muon_prepare_workspace_bytes: bad extents %lld x %lld", (long long)rows, (long long)cols);
    *bytes = (size_t)kMuonPartials * sizeof(float);
    return KF_OK;
}

extern "C" int kf_muon_prepare(int grad_dtype, int64_t rows, int64_t cols, const void *grad, float *momentum, float mu, int nesterov, float grad_scale,
                               void *X, int64_t xm, int64_t xn, int64_t ldx, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_muon_prepare";
    KF_REQUIRE(mu_dtype_ok(grad_dtype), KF_ERR_INVALID, "%s: grad dtype %d not supported (float, half, bfloat16)", who, grad_dtype);
    KF_REQUIRE(rows >= 0 && cols >= 0 && rows < ((int64_t)1 << 31) && cols < ((int64_t)1 << 31), KF_ERR_INVALID, "%s: bad extents %lld x %lld", who,
               (long long)rows, (long long)cols);
    const int64_t wm = rows < cols ? rows : cols, wn = rows < cols ? cols : rows;
    KF_REQUIRE(xm >= wm && xn >= wn && ldx >= xn && xn < ((int64_t)1 << 31), KF_ERR_INVALID,
               "%s: X [%lld, %lld] pitch %lld does not hold the wide matrix [%lld, %lld]", who, (long long)xm, (long long)xn, (long long)ldx, (long long)wm,
               (long long)wn);
    KF_REQUIRE(mu >= 0.f && mu < 1.f, KF_ERR_INVALID, "%s: momentum %g outside [0, 1)", who, (double)mu);
    KF_REQUIRE(momentum || mu == 0.f, KF_ERR_INVALID, "%s: momentum %g without a momentum buffer", who, (double)mu);
    KF_REQUIRE(nesterov == 0 || nesterov == 1, KF_ERR_INVALID, "%s: nesterov %d is not 0 or 1", who, nesterov);
    KF_REQUIRE(isfinite(grad_scale), KF_ERR_INVALID, "%s: grad_scale %g is not finite", who, (double)grad_scale);
    KF_REQUIRE((grad || rows * cols == 0) && (X || xm * xn == 0), KF_ERR_INVALID, "%s: null grad or X", who);
    KF_REQUIRE((uintptr_t)grad % dtype_size(grad_dtype) == 0 && (uintptr_t)momentum % 4 == 0 && (uintptr_t)X % 2 == 0 && (uintptr_t)workspace % 4 == 0,
               KF_ERR_INVALID, "%s: a pointer not aligned to its element size", who);
    KF_REQUIRE(workspace && workspace_bytes >= kMuonPartials * sizeof(float), KF_ERR_INVALID, "%s: workspace of %zu bytes required, got %zu", who,
               kMuonPartials * sizeof(float), workspace ? workspace_bytes : (size_t)0);
    const int64_t tiles = ((xm + kMuonTile - 1) / kMuonTile) * ((xn + kMuonTile - 1) / kMuonTile);
    KF_REQUIRE(tiles < ((int64_t)1 << 31), KF_ERR_UNSUPPORTED, "%s: %lld tiles exceed one grid", who, (long long)tiles);
    if (tiles == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    const int64_t n = rows * cols;
    const int np = (int)std::max<int64_t>(1, std::min<int64_t>(kMuonPartials, (n + 4 * kMuonBlock - 1) / (4 * kMuonBlock)));
    float *partial = (float *)workspace;
    const bool tr = rows > cols;
    KF_PROF("muon_prepare", st);
    return with_dtype(grad_dtype, [&](auto t) {
        using G = decltype(t);
        const int rc = launch(muon_momentum<G>, dim3(np), dim3(kMuonBlock), 0, st, (const G *)grad, momentum, n, mu, grad_scale, nesterov, partial);
        if (rc != KF_OK) return rc;
        return with_flags([&](auto TR) {
            return launch(muon_scale<G, TR>, dim3((unsigned)tiles), dim3(kMuonBlock), 0, st, (const G *)grad, (const float *)momentum, rows, cols, mu, grad_scale,
                          nesterov, (const float *)partial, np, (bf16_t *)X, xm, xn, ldx);
        }, tr);
    });
}

extern "C" int kf_muon_apply(int param_dtype, int64_t rows, int64_t cols, void *param, float *master, const void *O, int64_t ldo, const float *lr,
                             float weight_decay, float scale, void *stream) {
    const char *who = "kf_muon_apply";
    KF_REQUIRE(mu_dtype_ok(param_dtype), KF_ERR_INVALID, "%s: param dtype %d not supported (float, half, bfloat16)", who, param_dtype);
    KF_REQUIRE(rows >= 0 && cols >= 0 && rows < ((int64_t)1 << 31) && cols < ((int64_t)1 << 31), KF_ERR_INVALID, "%s: bad extents %lld x %lld", who,
               (long long)rows, (long long)cols);
    KF_REQUIRE(ldo >= (rows < cols ? cols : rows), KF_ERR_INVALID, "%s: pitch of O %lld < %lld", who, (long long)ldo, (long long)(rows < cols ? cols : rows));
    KF_REQUIRE(lr, KF_ERR_INVALID, "%s: null lr (a device float [1])", who);
    KF_REQUIRE(weight_decay >= 0.f && weight_decay < INFINITY && isfinite(scale), KF_ERR_INVALID, "%s: weight_decay %g outside [0, inf) or scale %g not finite",
               who, (double)weight_decay, (double)scale);
    KF_REQUIRE(!master || param_dtype != KF_F32, KF_ERR_INVALID, "%s: a master copy is for 16-bit params only", who);
    KF_REQUIRE((param && O) || rows * cols == 0, KF_ERR_INVALID, "%s: null param or O", who);
    KF_REQUIRE((uintptr_t)param % dtype_size(param_dtype) == 0 && (uintptr_t)master % 4 == 0 && (uintptr_t)O % 2 == 0 && (uintptr_t)lr % 4 == 0, KF_ERR_INVALID,
               "%s: a pointer not aligned to its element size", who);
    const int64_t tiles = ((rows + kMuonTile - 1) / kMuonTile) * ((cols + kMuonTile - 1) / kMuonTile);
    KF_REQUIRE(tiles < ((int64_t)1 << 31), KF_ERR_UNSUPPORTED, "%s: %lld tiles exceed one grid", who, (long long)tiles);
    if (tiles == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    KF_PROF("muon_apply", st);
    return with_dtype(param_dtype, [&](auto t) {
        using P = decltype(t);
        return with_flags([&](auto TR) {
            return launch(muon_apply<P, TR>, dim3((unsigned)tiles), dim3(kMuonBlock), 0, st, (P *)param, master, rows, cols, (const bf16_t *)O, ldo, lr,
                          weight_decay, scale);
        }, rows > cols);
    });
}
