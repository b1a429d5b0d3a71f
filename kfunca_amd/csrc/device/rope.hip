// Rotary position embeddings (RoPE) for gfx950, forward and backward, on any [B, H, S, D] operand addressed by element strides -
// in particular q | k | v in place in the packed [B*S, (Hq + 2 Hkv) D] projection output that the strided attention kernels read.
//
//   pairs (a, b):  rotate-half (Llama / NeoX) (i, i + R/2), interleaved (GPT-J) (2i, 2i + 1), i < R/2
//   y_a = x_a c - x_b s        y_b = x_b c + x_a s        c = cos[p, i], s = sin[p, i] (s -> -s for the inverse = the transpose)
//   dims d >= R and heads h >= h_rot are copied (not written at all in place)
//
// An HBM stream: one read and one write of every element, plus a table slice per token that stays in L2 / the Infinity Cache.
// One wave per token (grid-stride over tokens). In the packed path a lane owns pair slot j < L = R / (2V) (V elements per 16-byte
// pack): for rotate-half pack j of each half of a head, interleaved packs 2j and 2j + 1 - V pairs either way, whose cos / sin it
// loads once per token and keeps in registers. The 64 / L head slots of the wave walk the token's rotated heads with kRopeU heads'
// loads in flight before the first use, then (out of place) the copied packs, kRopeU per lane in flight. The position is read once per
// token. The packed path needs every head start and both tables 16-byte aligned and R/2 a multiple of V with L <= 64; anything else
// (odd strides or bases, R = 2, D = 2048 bf16) takes the element path, which walks the same pairs one at a time. Dims beyond the
// last whole pack of a head (D % V) are copied element by element in both paths.
//
// A position outside [0, table_rows) reads table row 0 in its place (never outside the table) and replaces those values with NaN,
// so exactly that token's rotated elements become NaN.
// All offsets are 64-bit. No atomics, no scratch, no host synchronisation: a call can be captured in a graph.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// rope_rot's FMAs are written out, and nothing else may be fused: the packed and the element path must round alike, bit for bit
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kRopeBlock = 256;   // four waves = four tokens in flight per block
constexpr int kRopeU = 4;         // heads (rotation) / packs (copy) per lane with loads in flight before the first use
constexpr int64_t kRopeMaxGrid = 1 << 20;

// stores: pack16 and store_hw, one rounding per element; the hardware bf16 converter keeps a NaN a NaN (a bad position must show)

// y_a = x_a c - x_b s, y_b = x_b c + x_a s: the same expression in both paths, so the element path and the packed path agree bitwise
__device__ __forceinline__ void rope_rot(float xa, float xb, float c, float s, float &ya, float &yb) {
    ya = fmaf(xa, c, -(xb * s));
    yb = fmaf(xb, c, xa * s);
}

struct RopeArgs {
    const float *cos, *sin;
    const int64_t *positions;
    const void *x;
    void *y;
    int64_t tokens, S, H, D, h_rot, R, table_rows;
    int64_t xb, xh, xr, yb, yh, yr;   // element strides of B, H, S
    float sign;                       // +1 forward, -1 inverse
    int copy;                         // y is not x: copied parts are written
};

// the token's position and its table row (row 0 for a position outside [0, table_rows), whose values the callers replace with NaN)
__device__ __forceinline__ int64_t rope_token(const RopeArgs &a, int64_t tok, int64_t &xo, int64_t &yo, bool &ok) {
    const int64_t b = tok / a.S, s = tok - b * a.S;
    const int64_t p = a.positions ? a.positions[tok] : s;
    ok = p >= 0 && p < a.table_rows;
    xo = b * a.xb + s * a.xr;
    yo = b * a.yb + s * a.yr;
    return ok ? p : 0;
}

// the packed path: 16-byte packs (see the file comment for the lane map)
template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(kRopeBlock) void rope_packed(const RopeArgs a) {
    constexpr int V = kPack16<T>;
    const T *x = (const T *)a.x;
    T *y = (T *)a.y;
    const int lane = threadIdx.x & 63;
    const int L = (int)(a.R / (2 * V)), HP = 64 / L;   // pair slots per head, head slots per wave
    const int j = lane % L, hs = lane / L;
    const int64_t half = a.R / 2;
    const int64_t P0 = (a.D - a.R) / V, P1 = a.D / V;   // whole packs per rotated head beyond R, per copied head
    const int64_t ncopy = a.copy ? a.h_rot * P0 + (a.H - a.h_rot) * P1 : 0;
    const int64_t tr = a.D - P1 * V;                    // elements past the last whole pack of a head
    for (int64_t tok = (int64_t)blockIdx.x * (kRopeBlock / 64) + (threadIdx.x >> 6); tok < a.tokens; tok += (int64_t)gridDim.x * (kRopeBlock / 64)) {
        int64_t xo, yo;
        bool ok;
        const int64_t p = rope_token(a, tok, xo, yo, ok);
        // the lane's V (cos, sin) of this token, kept across its heads
        float c[V], s[V];
        {
            const uint4 *cp = (const uint4 *)(a.cos + p * half + (int64_t)j * V), *sp = (const uint4 *)(a.sin + p * half + (int64_t)j * V);
#pragma unroll
            for (int q = 0; q < V / 4; ++q) {
                const uint4 cv = cp[q], sv = sp[q];
                c[4 * q] = __uint_as_float(cv.x); c[4 * q + 1] = __uint_as_float(cv.y); c[4 * q + 2] = __uint_as_float(cv.z); c[4 * q + 3] = __uint_as_float(cv.w);
                s[4 * q] = __uint_as_float(sv.x); s[4 * q + 1] = __uint_as_float(sv.y); s[4 * q + 2] = __uint_as_float(sv.z); s[4 * q + 3] = __uint_as_float(sv.w);
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                c[i] = ok ? c[i] : __builtin_nanf("");
                s[i] = ok ? s[i] * a.sign : __builtin_nanf("");
            }
        }
        // element offsets of the lane's two packs inside a head
        const int64_t ea = INTERLEAVED ? (int64_t)j * 2 * V : (int64_t)j * V, eb = INTERLEAVED ? ea + V : ea + half;
        if (hs < HP) {
            for (int64_t h0 = hs; h0 < a.h_rot; h0 += (int64_t)HP * kRopeU) {
                uint4 ra[kRopeU], rb[kRopeU];
#pragma unroll
                for (int u = 0; u < kRopeU; ++u) {
                    const int64_t h = h0 + (int64_t)u * HP;
                    if (h < a.h_rot) {
                        const T *xh = x + xo + h * a.xh;
                        ra[u] = *(const uint4 *)(xh + ea);
                        rb[u] = *(const uint4 *)(xh + eb);
                    }
                }
#pragma unroll
                for (int u = 0; u < kRopeU; ++u) {
                    const int64_t h = h0 + (int64_t)u * HP;
                    if (h < a.h_rot) {
                        float fa[V], fb[V], ga[V], gb[V];
                        unpack16<T>(ra[u], fa);
                        unpack16<T>(rb[u], fb);
                        if constexpr (INTERLEAVED) {
                            // pairs (2i, 2i + 1): pack a holds pairs 0 .. V/2 - 1 of the slot, pack b the rest
#pragma unroll
                            for (int k = 0; k < V / 2; ++k) {
                                rope_rot(fa[2 * k], fa[2 * k + 1], c[k], s[k], ga[2 * k], ga[2 * k + 1]);
                                rope_rot(fb[2 * k], fb[2 * k + 1], c[V / 2 + k], s[V / 2 + k], gb[2 * k], gb[2 * k + 1]);
                            }
                        } else {
#pragma unroll
                            for (int k = 0; k < V; ++k) rope_rot(fa[k], fb[k], c[k], s[k], ga[k], gb[k]);
                        }
                        T *yh = y + yo + h * a.yh;
                        *(uint4 *)(yh + ea) = pack16<T>(ga);
                        *(uint4 *)(yh + eb) = pack16<T>(gb);
                    }
                }
            }
        }
        if (!a.copy) continue;
        // the copied packs: dims [R, R + P0 V) of each rotated head, then [0, P1 V) of each copied head, flattened over the wave
        for (int64_t k0 = lane; k0 < ncopy; k0 += 64 * kRopeU) {
            uint4 r[kRopeU];
            int64_t oxs[kRopeU], oys[kRopeU];
#pragma unroll
            for (int u = 0; u < kRopeU; ++u) {
                const int64_t k = k0 + (int64_t)u * 64;
                if (k < ncopy) {
                    int64_t h, e;
                    if (k < a.h_rot * P0) { h = k / P0; e = a.R + (k - h * P0) * V; }
                    else { const int64_t kk = k - a.h_rot * P0; h = a.h_rot + kk / P1; e = (kk - (h - a.h_rot) * P1) * V; }
                    oxs[u] = xo + h * a.xh + e;
                    oys[u] = yo + h * a.yh + e;
                    r[u] = *(const uint4 *)(x + oxs[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kRopeU; ++u)
                if (k0 + (int64_t)u * 64 < ncopy) *(uint4 *)(y + oys[u]) = r[u];
        }
        // the last D % V elements of every head (R is a multiple of V here, so they follow the last whole pack of both kinds of head)
        for (int64_t k = lane; k < a.H * tr; k += 64) {
            const int64_t h = k / tr, e = a.D - tr + (k - h * tr);
            y[yo + h * a.yh + e] = x[xo + h * a.xh + e];
        }
    }
}

// the element path: any element-aligned base and strides, any even R. Lane k of the wave takes pair k, k + 64, ... of the token's
// rotated heads (cos / sin from the table each time: L1 / L2 hits), then, out of place, copied element k, k + 64, ...
template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(kRopeBlock) void rope_elem(const RopeArgs a) {
    const T *x = (const T *)a.x;
    T *y = (T *)a.y;
    const int lane = threadIdx.x & 63;
    const int64_t half = a.R / 2, npair = a.h_rot * half, cr = a.D - a.R;
    const int64_t ncopy = a.copy ? a.h_rot * cr + (a.H - a.h_rot) * a.D : 0;
    for (int64_t tok = (int64_t)blockIdx.x * (kRopeBlock / 64) + (threadIdx.x >> 6); tok < a.tokens; tok += (int64_t)gridDim.x * (kRopeBlock / 64)) {
        int64_t xo, yo;
        bool ok;
        const int64_t p = rope_token(a, tok, xo, yo, ok);
        for (int64_t k = lane; k < npair; k += 64) {
            const int64_t h = k / half, i = k - h * half;
            const int64_t ia = INTERLEAVED ? 2 * i : i, ib = INTERLEAVED ? 2 * i + 1 : i + half;
            const float c = ok ? a.cos[p * half + i] : __builtin_nanf(""), s = ok ? a.sin[p * half + i] * a.sign : __builtin_nanf("");
            const T *xh = x + xo + h * a.xh;
            float ya, yb;
            rope_rot(load_f32(xh + ia), load_f32(xh + ib), c, s, ya, yb);
            T *yh = y + yo + h * a.yh;
            store_hw(yh + ia, ya);
            store_hw(yh + ib, yb);
        }
        for (int64_t k = lane; k < ncopy; k += 64) {
            int64_t h, e;
            if (k < a.h_rot * cr) { h = k / cr; e = a.R + (k - h * cr); }
            else { const int64_t kk = k - a.h_rot * cr; h = a.h_rot + kk / a.D; e = kk - (h - a.h_rot) * a.D; }
            y[yo + h * a.yh + e] = x[xo + h * a.xh + e];
        }
    }
}

__global__ __launch_bounds__(kRopeBlock) void rope_table_kernel(double base, int64_t R, int64_t rows, float *cos_out, float *sin_out) {
    const int64_t half = R / 2, n = rows * half;
    for (int64_t k = (int64_t)blockIdx.x * kRopeBlock + threadIdx.x; k < n; k += (int64_t)gridDim.x * kRopeBlock) {
        const int64_t p = k / half, i = k - p * half;
        const double theta = (double)p * pow(base, -(double)(2 * i) / (double)R);
        cos_out[k] = (float)cos(theta);
        sin_out[k] = (float)sin(theta);
    }
}

bool rope_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_rope(int dtype, int64_t B, int64_t H, int64_t S, int64_t D, int64_t h_rot, int64_t rotary_dim, int interleaved, int inverse,
                       const float *cos, const float *sin, int64_t table_rows, const int64_t *positions, const void *x, const kf_attn_layout *lx,
                       void *y, const kf_attn_layout *ly, void *stream) {
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "kf_rope: dtype %d not supported (float, half, bfloat16)", dtype);
    KF_REQUIRE(B >= 0 && H >= 0 && S >= 0 && D >= 1, KF_ERR_INVALID, "kf_rope: bad extents B %lld H %lld S %lld D %lld", (long long)B, (long long)H,
               (long long)S, (long long)D);
    KF_REQUIRE(rotary_dim >= 2 && rotary_dim % 2 == 0 && rotary_dim <= D, KF_ERR_INVALID, "kf_rope: rotary_dim %lld must be even and in [2, D = %lld]",
               (long long)rotary_dim, (long long)D);
    KF_REQUIRE(h_rot >= 0 && h_rot <= H, KF_ERR_INVALID, "kf_rope: h_rot %lld outside [0, H = %lld]", (long long)h_rot, (long long)H);
    KF_REQUIRE(interleaved == 0 || interleaved == 1, KF_ERR_INVALID, "kf_rope: interleaved must be 0 or 1, got %d", interleaved);
    KF_REQUIRE(inverse == 0 || inverse == 1, KF_ERR_INVALID, "kf_rope: inverse must be 0 or 1, got %d", inverse);
    KF_REQUIRE(cos && sin && x && y && lx && ly, KF_ERR_INVALID, "kf_rope: null table, operand or layout");
    KF_REQUIRE(table_rows >= 1, KF_ERR_INVALID, "kf_rope: table_rows %lld < 1", (long long)table_rows);
    KF_REQUIRE(positions || S <= table_rows, KF_ERR_INVALID, "kf_rope: without positions the table needs S = %lld rows, it has %lld", (long long)S,
               (long long)table_rows);
    KF_REQUIRE(x != y || (lx->batch == ly->batch && lx->head == ly->head && lx->row == ly->row), KF_ERR_INVALID,
               "kf_rope: in place (y == x) needs y's layout to equal x's");
    const int es = dtype_size(dtype);
    KF_REQUIRE((uintptr_t)x % es == 0 && (uintptr_t)y % es == 0, KF_ERR_INVALID, "kf_rope: x or y not aligned to its element size");
    const int64_t tokens = B * S;
    if (tokens == 0 || H == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    RopeArgs a{cos, sin, positions, x, y, tokens, S, H, D, h_rot, rotary_dim, table_rows, lx->batch, lx->head, lx->row, ly->batch, ly->head, ly->row,
               inverse ? -1.f : 1.f, x != y};
    const int V = 16 / es;
    const int64_t b16 = 16 / es; // strides in elements that keep 16-byte alignment
    const bool packed = (rotary_dim / 2) % V == 0 && rotary_dim / (2 * V) <= 64 && rope_aligned16(x) && rope_aligned16(y) && rope_aligned16(cos) &&
                        rope_aligned16(sin) && lx->batch % b16 == 0 && lx->head % b16 == 0 && lx->row % b16 == 0 && ly->batch % b16 == 0 &&
                        ly->head % b16 == 0 && ly->row % b16 == 0;
    const unsigned grid = (unsigned)std::min<int64_t>((tokens + kRopeBlock / 64 - 1) / (kRopeBlock / 64), kRopeMaxGrid);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_flags([&](auto IL) {
            if (packed) {
                KF_PROF("rope_packed", st);
                return launch(rope_packed<T, IL>, grid, kRopeBlock, 0, st, a);
            }
            KF_PROF("rope_elem", st);
            return launch(rope_elem<T, IL>, grid, kRopeBlock, 0, st, a);
        }, interleaved != 0);
    });
}

extern "C" int kf_rope_table(double base, int64_t rotary_dim, int64_t rows, float *cos, float *sin, void *stream) {
    KF_REQUIRE(base > 0.0 && isfinite(base), KF_ERR_INVALID, "kf_rope_table: base %g must be positive and finite", base);
    KF_REQUIRE(rotary_dim >= 2 && rotary_dim % 2 == 0, KF_ERR_INVALID, "kf_rope_table: rotary_dim %lld must be even and >= 2", (long long)rotary_dim);
    KF_REQUIRE(rows >= 1, KF_ERR_INVALID, "kf_rope_table: rows %lld < 1", (long long)rows);
    KF_REQUIRE(cos && sin, KF_ERR_INVALID, "kf_rope_table: null cos or sin");
    hipStream_t st = as_stream(stream);
    const int64_t n = rows * (rotary_dim / 2);
    const unsigned grid = (unsigned)std::min<int64_t>((n + kRopeBlock - 1) / kRopeBlock, kRopeMaxGrid);
    KF_PROF("rope_table", st);
    return launch(rope_table_kernel, grid, kRopeBlock, 0, st, base, rotary_dim, rows, cos, sin);
}
