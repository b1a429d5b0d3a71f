// Causal depthwise conv1d with a carried state for gfx950, forward and backward (kf_causal_conv1d_*): the short convolution in front
// of a linear-time sequence mixer, channel-last on rows addressed by a leading dimension.
//
//   pre[b, t, c] = bias[c] + sum_{j < K} w[j, c] z[b, t + j, c]     z[b] = h0[b] (K - 1 rows) then x[b] (S rows),  y = act(pre)
//   dz[b, m]     = sum_j w[j] dpre[b, m - j] + d_hT[b, m - S]       dpre = dy act'(pre);  dx = dz rows K - 1 .., d_h0 = dz rows 0 .. K - 2
//   dw[j, c]     = sum_{b, t} dpre[b, t, c] z[b, t + j, c]          dbias[c] = sum_{b, t} dpre[b, t, c]
//
// The split. A lane owns one 16-byte pack of channels (V = 8 elements of 16 bits, 4 floats) and never needs another lane's data: a wave
// spans 64 packs of a row (1 KiB of 16-bit elements) and walks kConvRows = 64 consecutive rows of them, the previous K - 1 rows a sliding
// window in registers (widened to f32, like the weights and the bias). A workgroup is 4 waves on 4 consecutive row tiles; the grid is
// (channel blocks) x ceil(S / 256) x B. Every x row is loaded once, plus a halo of K - 1 rows per wave (from h0, or zeros, in the first
// tile of a batch row). Loads are issued in unrolled batches ahead of use (8 rows forward, 4 rows of x and of dy backward).
//
// Forward: K fused multiply-adds per output from the bias up, in the order of the taps, whatever the tile - so a sequence cut into
// segments chained through hT -> h0, and the decode step, give the bits of one call. The wave that holds a batch row's last rows
// writes hT from the packs it loaded (copies, exact). With S <= 64 one lane reads and writes everything of its channels: hT may then be
// h0 and y may be x.
//
// Backward: one ascending walk per wave. At row s it recomputes pre[s] (the forward's expression), forms dpre[s], adds it to the
// (K + 1) x V weight partials when the row is the tile's own, and emits dz[s] = sum_j w[j] dpre[s - j] from a window of K dpre rows:
// d_h0 for s < K - 1, else dx[s - (K - 1)] - a lag of K - 1, so the walk runs K - 1 rows past the tile (rows of the next tile are
// recomputed for dx only; rows past S are zero and take d_hT). The sum starts from d_hT (or 0) and takes the taps in ascending order,
// skipping the rows outside [0, S): in f32 a segment's d_h0 is then exactly the head of the chain the whole sequence runs, and dx of two
// chained segments has the bits of one call. The four waves' partials are summed through LDS in the order 0..3 and one [K + 1, C] f32
// row per workgroup goes to the workspace; conv_wgrad_reduce_kernel sums the workgroups ascending and rounds once. No atomics.
//
// SiLU is glu.hip's: e = exp2(-|x| log2 e), r = rcp(1 + e), sigma = r or e r - no overflow, every finite input gives a finite result.
// All offsets are 64-bit. No scratch, no host synchronisation: every call can be captured in a graph.
#include <math.h>

#include <type_traits>

#include "float_pack.h"

// every copy of a row's arithmetic (whole batches, the last rows, the step) must round alike, bit for bit
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kConvRows = KF_CONV1D_STEP_MAX;   // rows a wave walks
constexpr int kConvWaves = 4, kConvBlock = kConvWaves * kWave;
constexpr int kConvTile = kConvWaves * kConvRows;   // rows of a workgroup
constexpr int kConvFwdBatch = 8, kConvBwdBatch = 4;  // rows whose loads are issued together
constexpr int kConvReduceBlock = 256;
constexpr float kConvLog2e = 1.44269504088896340736f;

struct ConvArgs {
    const void *x, *w, *bias, *h0, *dy, *d_hT;
    void *y, *hT, *dx, *d_h0;
    float *part;                        // [B * tiles, K + 1, C]
    int64_t S, C, P;                    // P = packs per row (C / V)
    int64_t ldx, ldy, lddy, lddx;       // leading dimensions in elements
};

__device__ __forceinline__ uint4 conv_ld(const void *p) { return *(const uint4 *)p; }

// a = SiLU(v) and, with GRAD, d = SiLU'(v) = s (1 + v (1 - s))
template <bool GRAD>
__device__ __forceinline__ void conv_silu(float v, float &a, float &d) {
    const float e = __builtin_exp2f(-fabsf(v) * kConvLog2e);
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float er = e * r;
    const float s = v >= 0.f ? r : er;
    a = v * s;
    if constexpr (GRAD) d = s * fmaf(v, v >= 0.f ? er : r, 1.f);
}

// what both walks start from: the lane's weights and bias in f32 and the K - 1 rows in front of row t0 (h0 or zeros before row 0)
template <typename T, int K, int V>
__device__ __forceinline__ void conv_prologue(const ConvArgs &a, int64_t b, int64_t c, int64_t t0, const T *x, float (&w)[K][V], float (&bias)[V],
                                              uint4 (&raw)[K - 1], float (&win)[K - 1][V]) {
#pragma unroll
    for (int j = 0; j < K; ++j) unpack16<T>(conv_ld((const T *)a.w + j * a.C + c), w[j]);
    if (a.bias) {
        unpack16<T>(conv_ld((const T *)a.bias + c), bias);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) bias[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < K - 1; ++i) {
        if (t0 > 0) raw[i] = conv_ld(x + (t0 - (K - 1) + i) * a.ldx);   // t0 >= kConvRows > K - 1
        else if (a.h0) raw[i] = conv_ld((const T *)a.h0 + (b * (K - 1) + i) * a.C + c);
        else raw[i] = make_uint4(0, 0, 0, 0);
        unpack16<T>(raw[i], win[i]);
    }
}

// pre of one row from the window and the current row: K fused multiply-adds from the bias up, in the order of the taps
template <int K, int V>
__device__ __forceinline__ void conv_pre(const float (&w)[K][V], const float (&bias)[V], const float (&win)[K - 1][V], const float (&cur)[V],
                                         float (&pre)[V]) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        float acc = bias[i];
#pragma unroll
        for (int j = 0; j < K - 1; ++j) acc = fmaf(w[j][i], win[j][i], acc);
        pre[i] = fmaf(w[K - 1][i], cur[i], acc);
    }
}

template <typename T, int K, bool SILU>
__global__ __launch_bounds__(kConvBlock) void conv_fwd_kernel(const ConvArgs a) {
    constexpr int V = kPack16<T>, NB = kConvFwdBatch;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t p = (int64_t)blockIdx.x * kWave + lane;
    const int64_t t0 = ((int64_t)blockIdx.y * kConvWaves + wave) * kConvRows;
    if (p >= a.P || t0 >= a.S) return;
    const int64_t b = blockIdx.z, c = p * V, tend = t0 + kConvRows < a.S ? t0 + kConvRows : a.S;
    const T *x = (const T *)a.x + b * a.S * a.ldx + c;
    T *y = (T *)a.y + b * a.S * a.ldy + c;
    float w[K][V], bias[V], win[K - 1][V];
    uint4 raw[K - 1];
    conv_prologue<T, K, V>(a, b, c, t0, x, w, bias, raw, win);

    auto row = [&](const uint4 &in, int64_t t) {
        float cur[V], pre[V];
        unpack16<T>(in, cur);
        conv_pre<K, V>(w, bias, win, cur, pre);
        if constexpr (SILU) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float unused;
                conv_silu<false>(pre[i], pre[i], unused);
            }
        }
        *(uint4 *)(y + t * a.ldy) = pack16<T>(pre);
#pragma unroll
        for (int j = 0; j + 1 < K - 1; ++j) {
            raw[j] = raw[j + 1];
#pragma unroll
            for (int i = 0; i < V; ++i) win[j][i] = win[j + 1][i];
        }
        raw[K - 2] = in;
#pragma unroll
        for (int i = 0; i < V; ++i) win[K - 2][i] = cur[i];
    };

    int64_t t = t0;
    for (; t + NB <= tend; t += NB) {
        uint4 in[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) in[i] = conv_ld(x + (t + i) * a.ldx);
#pragma unroll
        for (int i = 0; i < NB; ++i) row(in[i], t + i);
    }
    if (t < tend) {   // the last rows of a sequence: the loads still go first (y may be x)
        uint4 in[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) in[i] = t + i < tend ? conv_ld(x + (t + i) * a.ldx) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (t + i < tend) row(in[i], t + i);
    }
    if (tend == a.S && a.hT) {   // the window is now z rows S .. S + K - 2
#pragma unroll
        for (int i = 0; i < K - 1; ++i) *(uint4 *)((T *)a.hT + (b * (K - 1) + i) * a.C + c) = raw[i];
    }
}

template <typename T, int K, bool SILU>
__global__ __launch_bounds__(kConvBlock, 2) void conv_bwd_kernel(const ConvArgs a) {
    constexpr int V = kPack16<T>, NB = K == 4 && V == 8 ? kConvBwdBatch / 2 : kConvBwdBatch;   // (4 taps of 8 channels spill at 4)
    __shared__ float red[kConvWaves - 1][K + 1][V][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int64_t p = (int64_t)blockIdx.x * kWave + lane;
    const int64_t t0 = ((int64_t)blockIdx.y * kConvWaves + wave) * kConvRows;
    const int64_t b = blockIdx.z, c = p * V, S = a.S;
    float acc[K + 1][V];   // dw taps 0 .. K - 1, then dbias
#pragma unroll
    for (int j = 0; j <= K; ++j)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[j][i] = 0.f;

    if (p < a.P && t0 < S) {
        const int64_t tend = t0 + kConvRows < S ? t0 + kConvRows : S, wend = tend + (K - 1), emit_from = t0 == 0 ? 0 : t0 + (K - 1);
        const T *x = (const T *)a.x + b * S * a.ldx + c, *dy = (const T *)a.dy + b * S * a.lddy + c;
        T *dx = (T *)a.dx + b * S * a.lddx + c;
        float w[K][V], bias[V], dp[K][V];   // dp[K - 1 - j] = dpre[s - j]
        uint4 raw[K - 1];
        {
            float win[K - 1][V];
            conv_prologue<T, K, V>(a, b, c, t0, x, w, bias, raw, win);
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int i = 0; i < V; ++i) dp[j][i] = 0.f;

        auto row = [&](const uint4 &xin, const uint4 &gin, int64_t s) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j)
#pragma unroll
                for (int i = 0; i < V; ++i) dp[j][i] = dp[j + 1][i];
            if (s < S) {
                float cur[V], pre[V], g[V], win[K - 1][V];   // the window stays packed between rows: (K - 1) x 4 registers, not x V
#pragma unroll
                for (int j = 0; j < K - 1; ++j) unpack16<T>(raw[j], win[j]);
                unpack16<T>(xin, cur);
                unpack16<T>(gin, g);
                conv_pre<K, V>(w, bias, win, cur, pre);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if constexpr (SILU) {
                        float unused, der;
                        conv_silu<true>(pre[i], unused, der);
                        g[i] *= der;
                    }
                    dp[K - 1][i] = g[i];
                }
                if (s < tend) {   // the tile's own row: its weight partials
#pragma unroll
                    for (int i = 0; i < V; ++i) {
#pragma unroll
                        for (int j = 0; j < K - 1; ++j) acc[j][i] = fmaf(g[i], win[j][i], acc[j][i]);
                        acc[K - 1][i] = fmaf(g[i], cur[i], acc[K - 1][i]);
                        acc[K][i] += g[i];
                    }
                }
#pragma unroll
                for (int j = 0; j + 1 < K - 1; ++j) raw[j] = raw[j + 1];
                raw[K - 2] = xin;
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) dp[K - 1][i] = 0.f;
            }
            if (s < emit_from) return;
            float dz[V];
            if (s >= S && a.d_hT) {
                unpack16<T>(conv_ld((const T *)a.d_hT + (b * (K - 1) + (s - S)) * a.C + c), dz);
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i) dz[i] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (s - j >= 0 && s - j < S) {
#pragma unroll
                    for (int i = 0; i < V; ++i) dz[i] = fmaf(w[j][i], dp[K - 1 - j][i], dz[i]);
                }
            }
            if (s >= K - 1) *(uint4 *)(dx + (s - (K - 1)) * a.lddx) = pack16<T>(dz);
            else if (a.d_h0) *(uint4 *)((T *)a.d_h0 + (b * (K - 1) + s) * a.C + c) = pack16<T>(dz);
        };

        for (int64_t s = t0; s < wend; s += NB) {
            uint4 xin[NB], gin[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const bool in = s + i < S;   // (wend <= S + K - 1: rows past S are not loaded)
                xin[i] = in ? conv_ld(x + (s + i) * a.ldx) : make_uint4(0, 0, 0, 0);
                gin[i] = in ? conv_ld(dy + (s + i) * a.lddy) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (s + i < wend) row(xin[i], gin[i], s + i);
        }
    }

    // the four waves' partials in the order 0..3 (a wave past S holds zeros), one row per workgroup
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j <= K; ++j)
#pragma unroll
            for (int i = 0; i < V; ++i) red[wave - 1][j][i][lane] = acc[j][i];
    }
    __syncthreads();
    if (wave == 0 && p < a.P) {
        float *part = a.part + (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * (K + 1)) * a.C + c;
#pragma unroll
        for (int j = 0; j <= K; ++j)
#pragma unroll
            for (int i = 0; i < V; i += 4) {
                float4 v;
                v.x = ((acc[j][i] + red[0][j][i][lane]) + red[1][j][i][lane]) + red[2][j][i][lane];
                v.y = ((acc[j][i + 1] + red[0][j][i + 1][lane]) + red[1][j][i + 1][lane]) + red[2][j][i + 1][lane];
                v.z = ((acc[j][i + 2] + red[0][j][i + 2][lane]) + red[1][j][i + 2][lane]) + red[2][j][i + 2][lane];
                v.w = ((acc[j][i + 3] + red[0][j][i + 3][lane]) + red[1][j][i + 3][lane]) + red[2][j][i + 3][lane];
                *(float4 *)(part + j * a.C + i) = v;
            }
    }
}

// dw[j, c] (j < K) and dbias[c] (j == K) = the workgroups' partials summed ascending, rounded once; one thread per (j, c)
template <typename T>
__global__ __launch_bounds__(kConvReduceBlock) void conv_wgrad_reduce_kernel(const float *part, int64_t nparts, int64_t K, int64_t C, T *dw, T *dbias) {
    const int64_t idx = (int64_t)blockIdx.x * kConvReduceBlock + threadIdx.x, row = (K + 1) * C;
    if (idx >= row) return;
    float v = part[idx];
    int64_t q = 1;
    for (; q + 8 <= nparts; q += 8) {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = part[(q + i) * row + idx];
#pragma unroll
        for (int i = 0; i < 8; ++i) v += f[i];
    }
    for (; q < nparts; ++q) v += part[q * row + idx];
    if (idx < K * C) store_hw(dw + idx, v);
    else if (dbias) store_hw(dbias + (idx - K * C), v);
}

bool conv_al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// byte ranges [p, p + n) and [q, q + m) share a byte (a null pointer has no range)
bool conv_overlap(const void *p, int64_t n, const void *q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}
int64_t conv_tiles(int64_t S) { return (S + kConvTile - 1) / kConvTile; }

// the checks of the three entries that need no pointer
int conv_check(const char *who, int dtype, int64_t B, int64_t S, int64_t C, int64_t K) {
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_UNSUPPORTED, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(B > 0 && S > 0 && C > 0, KF_ERR_INVALID, "%s: bad extents B %lld S %lld C %lld", who, (long long)B, (long long)S, (long long)C);
    KF_REQUIRE(K >= 2 && K <= 4, KF_ERR_UNSUPPORTED, "%s: K %lld not supported (2, 3, 4)", who, (long long)K);
    KF_REQUIRE(C % (16 / dtype_size(dtype)) == 0, KF_ERR_UNSUPPORTED, "%s: C %lld is not a multiple of the 16-byte pack", who, (long long)C);
    KF_REQUIRE(B <= 65535 && conv_tiles(S) <= 65535, KF_ERR_UNSUPPORTED, "%s: B %lld or S %lld beyond the grid", who, (long long)B, (long long)S);
    return KF_OK;
}

int conv_check_act(const char *who, int act) {
    KF_REQUIRE(act == KF_CONV1D_ACT_NONE || act == KF_CONV1D_ACT_SILU, KF_ERR_INVALID, "%s: act %d is not KF_CONV1D_ACT_NONE or KF_CONV1D_ACT_SILU", who, act);
    return KF_OK;
}

int conv_check_rows(const char *who, int dtype, int64_t C, const char *name, const void *p, int64_t ld) {
    KF_REQUIRE(ld >= C, KF_ERR_INVALID, "%s: leading dimension of %s %lld < C = %lld", who, name, (long long)ld, (long long)C);
    KF_REQUIRE(ld % (16 / dtype_size(dtype)) == 0, KF_ERR_UNSUPPORTED, "%s: leading dimension of %s %lld is not a multiple of the 16-byte pack", who, name,
               (long long)ld);
    KF_REQUIRE(conv_al16(p), KF_ERR_INVALID, "%s: %s is not aligned to 16 bytes", who, name);
    return KF_OK;
}

// bytes from the first to past the last element of [B * S, C] rows of leading dimension ld
int64_t conv_span(int64_t rows, int64_t C, int64_t ld, int es) { return ((rows - 1) * ld + C) * es; }

// two row operands share an element: their spans meet and, on one row pitch, so do their column windows
bool conv_rows_overlap(const void *p, int64_t ldp, const void *q, int64_t ldq, int64_t rows, int64_t C, int es) {
    if (!conv_overlap(p, conv_span(rows, C, ldp, es), q, conv_span(rows, C, ldq, es))) return false;
    if (ldp != ldq) return true;
    const int64_t pitch = ldp * es, width = C * es;
    const int64_t d = (int64_t)(((uintptr_t)q > (uintptr_t)p ? (uintptr_t)q - (uintptr_t)p : (uintptr_t)p - (uintptr_t)q) % (uintptr_t)pitch);
    return d < width || d > pitch - width;
}

template <typename F> int conv_with_k(int64_t K, F &&f) {
    return K == 2 ? f(std::integral_constant<int, 2>{}) : K == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 4>{});
}

const char *conv_label(int dtype, const char *const (&names)[3]) { return names[dtype == KF_BF16 ? 0 : dtype == KF_F16 ? 1 : 2]; }

}   // namespace
}   // namespace kf

using namespace kf;

extern "C" int kf_causal_conv1d_fwd(int dtype, int act, int64_t B, int64_t S, int64_t C, int64_t K, const void *x, int64_t ldx, const void *weight,
                                    const void *bias, const void *h0, void *y, int64_t ldy, void *hT, void *stream) {
    const char *who = "kf_causal_conv1d_fwd";
    KF_REQUIRE(x && weight && y, KF_ERR_INVALID, "%s: null x, weight or y", who);
    int rc = conv_check(who, dtype, B, S, C, K);
    if (rc == KF_OK) rc = conv_check_act(who, act);
    if (rc == KF_OK) rc = conv_check_rows(who, dtype, C, "x", x, ldx);
    if (rc == KF_OK) rc = conv_check_rows(who, dtype, C, "y", y, ldy);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(conv_al16(weight) && conv_al16(bias) && conv_al16(h0) && conv_al16(hT), KF_ERR_INVALID,
               "%s: weight, bias, h0 or hT is not aligned to 16 bytes", who);
    const int es = dtype_size(dtype);
    const int64_t rows = B * S, wb = K * C * es, bb = C * es, sb = B * (K - 1) * C * es, yb = conv_span(rows, C, ldy, es), xb = conv_span(rows, C, ldx, es);
    const bool step = S <= KF_CONV1D_STEP_MAX;
    KF_REQUIRE(y == x ? step && ldy == ldx : !conv_rows_overlap(x, ldx, y, ldy, rows, C, es), KF_ERR_INVALID,
               "%s: y overlaps x (y == x with ldy == ldx is allowed for S <= %d)", who, KF_CONV1D_STEP_MAX);
    KF_REQUIRE(hT == h0 ? !hT || step : !conv_overlap(hT, sb, h0, sb), KF_ERR_INVALID, "%s: hT overlaps h0 (hT == h0 is allowed for S <= %d)", who,
               KF_CONV1D_STEP_MAX);
    KF_REQUIRE(!conv_overlap(y, yb, weight, wb) && !conv_overlap(y, yb, bias, bb) && !conv_overlap(y, yb, h0, sb) && !conv_overlap(y, yb, hT, sb) &&
                   !conv_overlap(hT, sb, weight, wb) && !conv_overlap(hT, sb, bias, bb) && !conv_overlap(hT, sb, x, xb),
               KF_ERR_INVALID, "%s: an output overlaps another operand", who);
    ConvArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.h0 = h0; a.y = y; a.hT = hT;
    a.S = S; a.C = C; a.P = C / (16 / es); a.ldx = ldx; a.ldy = ldy;
    const dim3 grid((unsigned)((a.P + kWave - 1) / kWave), (unsigned)conv_tiles(S), (unsigned)B);
    hipStream_t st = as_stream(stream);
    static const char *const names[3] = {"causal_conv1d_fwd_bf16", "causal_conv1d_fwd_f16", "causal_conv1d_fwd_f32"};
    KF_PROF(conv_label(dtype, names), st);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return conv_with_k(K, [&](auto KK) {
            return with_flags([&](auto SILU) { return launch(conv_fwd_kernel<T, decltype(KK)::value, decltype(SILU)::value>, grid, kConvBlock, 0, st, a); },
                              act == KF_CONV1D_ACT_SILU);
        });
    });
}

extern "C" int kf_causal_conv1d_bwd_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t C, int64_t K, size_t *bytes) {
    const char *who = "kf_causal_conv1d_bwd_workspace_bytes";
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null bytes", who);
    const int rc = conv_check(who, dtype, B, S, C, K);
    if (rc != KF_OK) return rc;
    *bytes = (size_t)(B * conv_tiles(S) * (K + 1) * C) * sizeof(float);
    return KF_OK;
}

extern "C" int kf_causal_conv1d_bwd(int dtype, int act, int64_t B, int64_t S, int64_t C, int64_t K, const void *x, int64_t ldx, const void *weight,
                                    const void *bias, const void *h0, const void *dy, int64_t lddy, const void *d_hT, void *dx, int64_t lddx, void *dw,
                                    void *dbias, void *d_h0, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_causal_conv1d_bwd";
    KF_REQUIRE(x && weight && dy && dx && dw, KF_ERR_INVALID, "%s: null x, weight, dy, dx or dw", who);
    int rc = conv_check(who, dtype, B, S, C, K);
    if (rc == KF_OK) rc = conv_check_act(who, act);
    if (rc == KF_OK) rc = conv_check_rows(who, dtype, C, "x", x, ldx);
    if (rc == KF_OK) rc = conv_check_rows(who, dtype, C, "dy", dy, lddy);
    if (rc == KF_OK) rc = conv_check_rows(who, dtype, C, "dx", dx, lddx);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(conv_al16(weight) && conv_al16(bias) && conv_al16(h0) && conv_al16(d_hT) && conv_al16(dw) && conv_al16(dbias) && conv_al16(d_h0),
               KF_ERR_INVALID, "%s: weight, bias, h0, d_hT, dw, dbias or d_h0 is not aligned to 16 bytes", who);
    const int es = dtype_size(dtype);
    const int64_t rows = B * S, wb = K * C * es, bb = C * es, sb = B * (K - 1) * C * es;
    const size_t need = (size_t)(B * conv_tiles(S) * (K + 1) * C) * sizeof(float);
    KF_REQUIRE(workspace && workspace_bytes >= need && conv_al16(workspace), KF_ERR_WORKSPACE,
               "%s: workspace missing, not aligned to 16 bytes or too small (%zu < %zu bytes)", who, workspace ? workspace_bytes : (size_t)0, need);
    // every output against every input and every other output
    const void *in[6] = {x, dy, weight, bias, h0, d_hT};
    const int64_t in_b[6] = {conv_span(rows, C, ldx, es), conv_span(rows, C, lddy, es), wb, bb, sb, sb};
    const void *out[5] = {dx, dw, dbias, d_h0, workspace};
    const int64_t out_b[5] = {conv_span(rows, C, lddx, es), wb, bb, sb, (int64_t)need};
    bool clash = conv_rows_overlap(x, ldx, dx, lddx, rows, C, es) || conv_rows_overlap(dy, lddy, dx, lddx, rows, C, es);
    for (int o = 0; o < 5; ++o) {
        for (int i = o == 0 ? 2 : 0; i < 6; ++i) clash = clash || conv_overlap(out[o], out_b[o], in[i], in_b[i]);
        for (int q = o + 1; q < 5; ++q) clash = clash || conv_overlap(out[o], out_b[o], out[q], out_b[q]);
    }
    KF_REQUIRE(!clash, KF_ERR_INVALID, "%s: an output or the workspace overlaps another operand", who);
    ConvArgs a{};
    a.x = x; a.w = weight; a.bias = bias; a.h0 = h0; a.dy = dy; a.d_hT = d_hT; a.dx = dx; a.d_h0 = d_h0; a.part = (float *)workspace;
    a.S = S; a.C = C; a.P = C / (16 / es); a.ldx = ldx; a.lddy = lddy; a.lddx = lddx;
    const int64_t tiles = conv_tiles(S);
    const dim3 grid((unsigned)((a.P + kWave - 1) / kWave), (unsigned)tiles, (unsigned)B);
    hipStream_t st = as_stream(stream);
    {
        static const char *const names[3] = {"causal_conv1d_bwd_bf16", "causal_conv1d_bwd_f16", "causal_conv1d_bwd_f32"};
        KF_PROF(conv_label(dtype, names), st);
        rc = with_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            return conv_with_k(K, [&](auto KK) {
                return with_flags([&](auto SILU) { return launch(conv_bwd_kernel<T, decltype(KK)::value, decltype(SILU)::value>, grid, kConvBlock, 0, st, a); },
                                  act == KF_CONV1D_ACT_SILU);
            });
        });
        if (rc != KF_OK) return rc;
    }
    KF_PROF("causal_conv1d_wgrad_reduce", st);
    const unsigned rgrid = (unsigned)(((K + 1) * C + kConvReduceBlock - 1) / kConvReduceBlock);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch(conv_wgrad_reduce_kernel<T>, rgrid, kConvReduceBlock, 0, st, (const float *)workspace, B * tiles, K, C, (T *)dw, (T *)dbias);
    });
}
