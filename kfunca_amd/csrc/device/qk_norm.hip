// Per-head RMS norm of q and k (QK-norm: Chameleon, Qwen3, Gemma-3, OLMo-2) fused with the rotary embedding, for gfx950, forward and
// backward, in place in the packed [B*S, (Hq + Hk + Hv) D] projection (heads of a token in the order q | k | v).
//
//   forward    rstd = 1 / sqrt(mean_d x_d^2 + eps)      n_d = x_d rstd w_d      y = rope(n) over the leading R dims (rope.hip's pairs)
//   backward   g = rope^T(dy)    xhat = x rstd    gw = g w    m = mean_d(gw_d xhat_d)
//              dx_d = rstd (gw_d - xhat_d m)            dw_d = sum over tokens and heads of g_d xhat_d   (wq over q heads, wk over k heads)
//
// all in f32 on the stored values with ONE rounding, at the store. The backward recomputes rstd and xhat from x: nothing but the
// input is kept. Its rotation carries the products' rounding residuals (qkn_rot_exact): g is accurate relative to |g|, not to the pair. v heads are copied (not written at all in place).
//
// An HBM stream: the forward reads the projection once and writes it once, the backward reads x and dy once and writes dx once.
// The packed path, one wave per token (grid-stride over tokens), starts from rope.hip's lane map: with V elements in a 16-byte pack a
// head is L = D / 2V slots of two packs, and slot j < R / 2V holds pack j of each half of the rotated dims (rotate-half; packs 2j and
// 2j + 1 interleaved) so that a pair never leaves its lane, slot j >= R / 2V two packs of the dims beyond R. The G = 2^ceil(log2 L)
// lanes of a group own the slots of one head, the 64 / G groups of a wave walk the token's q heads and then its k heads with kQknU*
// heads' loads in flight before the first use. cos and sin are loaded once per token, the weights once per kernel; a head's values
// stay in the registers that loaded them between the sums and the store. The sum of squares (and the backward's sum of gw x) of a
// head is a lane's sequential sum over its two packs followed by a fixed-order __shfl_xor tree over the G lanes of the group.
// The backward's weight sums stay in registers over all the tokens a wave walks; at the end the groups of a wave are combined by
// shuffles, the waves of a block through LDS in wave order, and the block writes ONE f32 row [2][D] (dwq | dwk) to the workspace. A
// second kernel adds the rows in a fixed order. No atomics: bitwise reproducible; the workspace needs no initialisation.
//
// The packed path needs D a multiple of two packs with D / 2V <= 64, and R = 0 or R / 2 a multiple of the pack. With every head start,
// both tables and the weights 16-byte aligned it moves packs; otherwise (an odd leading dimension, a base shifted by an element) the
// same lanes own the same elements and do the same arithmetic with element loads and stores: the same bits. Any other geometry
// (D = 80 in f32, R = 2, an odd D) takes the element kernel: one wave per head, lane k owning pair k, k + 64, ... and then the dims
// beyond R, in two passes over the head (the sums, then the result), with the same expressions (qkn_*) and the weight sums kept in
// the wave's own workspace row.
//
// A position outside [0, table_rows) reads table row 0 in its place (never outside the table) and replaces cos and sin with NaN:
// the token's rotated elements of y are NaN; in the backward g is NaN there, so is m, hence all of dx of the token's q and k heads.
// All offsets are 64-bit. No host synchronisation, no allocation: calls can be captured in a graph.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

// every FMA is written out and nothing else may be fused: the pack and the element access must round alike, bit for bit
#pragma clang fp contract(off)

namespace kf {

namespace {

constexpr int kQknBlock = 256;       // four waves = four tokens in flight per block
constexpr int kQknUF = 4;            // forward: heads per lane group with loads in flight before the first use
constexpr int kQknUB = 2;            // backward (two operands per head)
constexpr int kQknCopyU = 4;         // copied packs per lane in flight
constexpr int64_t kQknMaxGrid = 1 << 20;
constexpr int kQknMaxParts = 1024;   // the backward's grid = rows of the workspace, at most
constexpr int kQknFoldCols = 64;

struct QknArgs {
    const float *cos, *sin;
    const int64_t *positions;
    const void *wq, *wk;
    const void *x, *dy;   // forward: x, -; backward: x, dy
    void *o;              // forward: y; backward: dx
    float *part;          // backward: [grid][2][D] partial weight sums, or null (no weight gradient wanted)
    int64_t tokens, S, Hq, Hk, Hv, D, R, table_rows, ldx, lddy, ldo;
    float eps;
    int copy;             // o is not the source of the v heads: they are written
};

// ---- the arithmetic, written once for both kernels ----------------------------------------------------------------------------------
__device__ __forceinline__ void qkn_rot(float xa, float xb, float c, float s, float &ya, float &yb) {
    ya = fmaf(xa, c, -(xb * s));
    yb = fmaf(xb, c, xa * s);
}
// the backward's rotation, g = rope^T(dy): where the two products cancel, the rounding of the first one (relative to |x_b s|, not to
// |g|) would be all that is left of g, and dx is held to a bound on |g w|. The product's exact residual is carried along, so g is
// within two roundings of its own magnitude.
__device__ __forceinline__ void qkn_rot_exact(float xa, float xb, float c, float s, float &ya, float &yb) {
    const float p = xb * s, q = xa * s;
    ya = fmaf(xa, c, -p) - fmaf(xb, s, -p);
    yb = fmaf(xb, c, q) + fmaf(xa, s, -q);
}
__device__ __forceinline__ float qkn_sq(float acc, float x) { return fmaf(x, x, acc); }
__device__ __forceinline__ float qkn_rstd(float ss, float d, float eps) { return 1.0f / sqrtf(ss / d + eps); }
__device__ __forceinline__ float qkn_n(float x, float rstd, float w) { return x * rstd * w; }
// backward: the term of sum_d gw_d x_d (m = rstd * that / D), dx and the weight term
__device__ __forceinline__ float qkn_dot(float acc, float g, float w, float x) { return fmaf(g * w, x, acc); }
__device__ __forceinline__ float qkn_m(float dot, float rstd, float d) { return dot * rstd / d; }
__device__ __forceinline__ float qkn_dx(float g, float w, float x, float rstd, float m) { return rstd * fmaf(-(x * rstd), m, g * w); }
__device__ __forceinline__ float qkn_dw(float acc, float g, float x, float rstd) { return fmaf(g, x * rstd, acc); }

// f32 -> f16 of values the compiler cannot see through: left to itself it folds the last multiply into the conversion in one path only
// (see glu.hip)
template <typename T> __device__ __forceinline__ float qkn_opaque(float v) {
    if constexpr (std::is_same<T, f16_t>::value) asm("" : "+v"(v));
    return v;
}
template <typename T> __device__ __forceinline__ void qkn_store1(T *p, float v) { store_hw(p, qkn_opaque<T>(v)); }

// the table row of a token (row 0 for a position outside [0, table_rows), whose cos and sin the callers replace with NaN)
__device__ __forceinline__ int64_t qkn_pos(const QknArgs &a, int64_t tok, bool &ok) {
    ok = true;
    if (a.R == 0) return 0;
    const int64_t p = a.positions ? a.positions[tok] : tok % a.S;
    ok = p >= 0 && p < a.table_rows;
    return ok ? p : 0;
}

// 16 bytes as they were loaded (a native vector: arrays of these stay in registers)
typedef uint32_t qkn_u32x4 __attribute__((ext_vector_type(4)));

// V elements at p as they were loaded: one 16-byte pack, or V single elements
template <typename T, bool VEC> struct QknRaw {
    static constexpr int V = kPack16<T>;
    qkn_u32x4 r;
    __device__ __forceinline__ void load(const T *p) { r = *(const qkn_u32x4 *)p; }
    __device__ __forceinline__ void get(float (&f)[V]) const { unpack16<T>(make_uint4(r.x, r.y, r.z, r.w), f); }
};
template <typename T> struct QknRaw<T, false> {
    static constexpr int V = kPack16<T>;
    float r[V];
    __device__ __forceinline__ void load(const T *p) {
#pragma unroll
        for (int i = 0; i < V; ++i) r[i] = load_f32(p + i);
    }
    __device__ __forceinline__ void get(float (&f)[V]) const {
#pragma unroll
        for (int i = 0; i < V; ++i) f[i] = r[i];
    }
};
template <typename T, bool VEC, int V> __device__ __forceinline__ void qkn_load(const T *p, float (&f)[V]) {
    QknRaw<T, VEC> r;
    r.load(p);
    r.get(f);
}
template <typename T, bool VEC, int V> __device__ __forceinline__ void qkn_store(T *p, const float (&f)[V]) {
    float r[V];
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = qkn_opaque<T>(f[i]);
    if constexpr (VEC) {
        *(uint4 *)p = pack16<T>(r);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) store_hw(p + i, r[i]);
    }
}
template <bool VEC, int V> __device__ __forceinline__ void qkn_load_table(const float *p, float (&f)[V]) {
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
            const uint4 v = ((const uint4 *)p)[q];
            f[4 * q] = __uint_as_float(v.x); f[4 * q + 1] = __uint_as_float(v.y); f[4 * q + 2] = __uint_as_float(v.z); f[4 * q + 3] = __uint_as_float(v.w);
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) f[i] = p[i];
    }
}

// the lane's place in the packed map
struct QknLane {
    int G, hs;            // lanes per head group (a power of two), the lane's group in the wave
    bool own, rot;        // the lane holds a slot of the head; a rotated one
    int64_t ea, eb;       // element offsets of its two packs inside a head
};

// the two packs of a head as the arithmetic sees them: x, and in the backward g = rope^T(dy)
template <typename T, bool IL, bool VEC, bool BWD, int V>
__device__ __forceinline__ void qkn_unpack(const QknLane &ln, const QknRaw<T, VEC> &xa, const QknRaw<T, VEC> &xb, const QknRaw<T, VEC> &da,
                                           const QknRaw<T, VEC> &db, const float (&c)[V], const float (&s)[V], float (&fa)[V], float (&fb)[V],
                                           float (&ga)[V], float (&gb)[V]) {
    xa.get(fa);
    xb.get(fb);
    if constexpr (BWD) {
        float ta[V], tb[V];
        da.get(ta);
        db.get(tb);
        if (ln.rot) {
            if constexpr (IL) {
#pragma unroll
                for (int k = 0; k < V / 2; ++k) {
                    qkn_rot_exact(ta[2 * k], ta[2 * k + 1], c[k], s[k], ga[2 * k], ga[2 * k + 1]);
                    qkn_rot_exact(tb[2 * k], tb[2 * k + 1], c[V / 2 + k], s[V / 2 + k], gb[2 * k], gb[2 * k + 1]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) qkn_rot_exact(ta[k], tb[k], c[k], s[k], ga[k], gb[k]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) { ga[k] = ta[k]; gb[k] = tb[k]; }
        }
    }
}

// heads [hbeg, hend) of one token, all with the weight (wa | wb): the groups of the wave take heads hbeg + hs, + 64 / G, ...
template <typename T, bool IL, bool VEC, bool BWD, int V>
__device__ __forceinline__ void qkn_heads(const QknArgs &a, const QknLane &ln, int64_t hbeg, int64_t hend, const float (&wa)[V], const float (&wb)[V],
                                          const float (&c)[V], const float (&s)[V], int64_t xo, int64_t go, int64_t oo, float (&dwa)[V],
                                          float (&dwb)[V]) {
    constexpr int U = BWD ? kQknUB : kQknUF;
    const T *x = (const T *)a.x, *dy = (const T *)a.dy;
    T *o = (T *)a.o;
    const int HP = 64 / ln.G;
    const float d = (float)a.D;
    for (int64_t h0 = hbeg; h0 < hend; h0 += (int64_t)HP * U) {   // (uniform over the wave: the shuffles below are reached by every lane)
        QknRaw<T, VEC> xa[U], xb[U], da[U], db[U];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t h = h0 + (int64_t)u * HP + ln.hs;
            live[u] = ln.own && h < hend;
            if (live[u]) {
                const T *xh = x + xo + h * a.D;
                xa[u].load(xh + ln.ea);
                xb[u].load(xh + ln.eb);
                if constexpr (BWD) {
                    const T *gh = dy + go + h * a.D;
                    da[u].load(gh + ln.ea);
                    db[u].load(gh + ln.eb);
                }
            }
        }
        // the lane's share of the sums of its U heads, then all the trees side by side
        float ss[U], dot[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ss[u] = dot[u] = 0.f;
            if (live[u]) {
                float fa[V], fb[V], ga[V], gb[V];
                qkn_unpack<T, IL, VEC, BWD, V>(ln, xa[u], xb[u], da[u], db[u], c, s, fa, fb, ga, gb);
#pragma unroll
                for (int k = 0; k < V; ++k) ss[u] = qkn_sq(ss[u], fa[k]);
#pragma unroll
                for (int k = 0; k < V; ++k) ss[u] = qkn_sq(ss[u], fb[k]);
                if constexpr (BWD) {
#pragma unroll
                    for (int k = 0; k < V; ++k) dot[u] = qkn_dot(dot[u], ga[k], wa[k], fa[k]);
#pragma unroll
                    for (int k = 0; k < V; ++k) dot[u] = qkn_dot(dot[u], gb[k], wb[k], fb[k]);
                }
            }
        }
        for (int off = ln.G >> 1; off > 0; off >>= 1) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ss[u] += __shfl_xor(ss[u], off, 64);
                if constexpr (BWD) dot[u] += __shfl_xor(dot[u], off, 64);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;
            const int64_t h = h0 + (int64_t)u * HP + ln.hs;
            const float rstd = qkn_rstd(ss[u], d, a.eps);
            float fa[V], fb[V], ga[V], gb[V], ra[V], rb[V];
            qkn_unpack<T, IL, VEC, BWD, V>(ln, xa[u], xb[u], da[u], db[u], c, s, fa, fb, ga, gb);
            if constexpr (BWD) {
                const float m = qkn_m(dot[u], rstd, d);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    ra[k] = qkn_dx(ga[k], wa[k], fa[k], rstd, m);
                    rb[k] = qkn_dx(gb[k], wb[k], fb[k], rstd, m);
                    dwa[k] = qkn_dw(dwa[k], ga[k], fa[k], rstd);
                    dwb[k] = qkn_dw(dwb[k], gb[k], fb[k], rstd);
                }
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    fa[k] = qkn_n(fa[k], rstd, wa[k]);
                    fb[k] = qkn_n(fb[k], rstd, wb[k]);
                }
                if (ln.rot) {
                    if constexpr (IL) {
#pragma unroll
                        for (int k = 0; k < V / 2; ++k) {
                            qkn_rot(fa[2 * k], fa[2 * k + 1], c[k], s[k], ra[2 * k], ra[2 * k + 1]);
                            qkn_rot(fb[2 * k], fb[2 * k + 1], c[V / 2 + k], s[V / 2 + k], rb[2 * k], rb[2 * k + 1]);
                        }
                    } else {
#pragma unroll
                        for (int k = 0; k < V; ++k) qkn_rot(fa[k], fb[k], c[k], s[k], ra[k], rb[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) { ra[k] = fa[k]; rb[k] = fb[k]; }
                }
            }
            T *oh = o + oo + h * a.D;
            qkn_store<T, VEC>(oh + ln.ea, ra);
            qkn_store<T, VEC>(oh + ln.eb, rb);
        }
    }
}

template <typename T, bool VEC, int V> __device__ __forceinline__ void qkn_load_weight(const void *w, const QknLane &ln, float (&wa)[V], float (&wb)[V]) {
#pragma unroll
    for (int k = 0; k < V; ++k) wa[k] = wb[k] = 1.f;
    if (w && ln.own) {
        qkn_load<T, VEC>((const T *)w + ln.ea, wa);
        qkn_load<T, VEC>((const T *)w + ln.eb, wb);
    }
}

// ---- the packed map (see the file comment) ---------------------------------------------------------------------------------------------
template <typename T, bool IL, bool VEC, bool BWD>
__global__ __launch_bounds__(kQknBlock) void qkn_packed(const QknArgs a) {
    constexpr int V = kPack16<T>;
    extern __shared__ __align__(16) float qkn_lds[];   // backward: [waves][2][D]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = (int)(a.D / (2 * V)), Lr = (int)(a.R / (2 * V));
    QknLane ln;
    int lg = 0;
    while ((1 << lg) < L) ++lg;
    ln.G = 1 << lg;
    const int j = lane & (ln.G - 1);
    ln.hs = lane >> lg;
    ln.own = j < L;
    ln.rot = j < Lr;
    const int64_t half = a.R / 2;
    if (ln.rot) {
        ln.ea = IL ? (int64_t)j * 2 * V : (int64_t)j * V;
        ln.eb = IL ? ln.ea + V : ln.ea + half;
    } else {
        ln.ea = a.R + (int64_t)(j - Lr) * V;
        ln.eb = ln.ea + (a.D - a.R) / 2;
    }
    float wqa[V], wqb[V], wka[V], wkb[V];
    qkn_load_weight<T, VEC>(a.wq, ln, wqa, wqb);
    qkn_load_weight<T, VEC>(a.wk, ln, wka, wkb);
    float dqa[V], dqb[V], dka[V], dkb[V];
#pragma unroll
    for (int k = 0; k < V; ++k) dqa[k] = dqb[k] = dka[k] = dkb[k] = 0.f;
    const int64_t nh = a.Hq + a.Hk;
    for (int64_t tok = (int64_t)blockIdx.x * (kQknBlock / 64) + wave; tok < a.tokens; tok += (int64_t)gridDim.x * (kQknBlock / 64)) {
        bool ok;
        const int64_t p = qkn_pos(a, tok, ok);
        // the lane's V (cos, sin) of this token, kept across its heads; the backward rotates by the transpose
        float c[V], s[V];
#pragma unroll
        for (int k = 0; k < V; ++k) { c[k] = 1.f; s[k] = 0.f; }
        if (ln.rot) {
            qkn_load_table<VEC>(a.cos + p * half + (int64_t)j * V, c);
            qkn_load_table<VEC>(a.sin + p * half + (int64_t)j * V, s);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                c[k] = ok ? c[k] : __builtin_nanf("");
                s[k] = ok ? (BWD ? -s[k] : s[k]) : __builtin_nanf("");
            }
        }
        const int64_t xo = tok * a.ldx, go = tok * a.lddy, oo = tok * a.ldo;
        qkn_heads<T, IL, VEC, BWD, V>(a, ln, 0, a.Hq, wqa, wqb, c, s, xo, go, oo, dqa, dqb);
        qkn_heads<T, IL, VEC, BWD, V>(a, ln, a.Hq, nh, wka, wkb, c, s, xo, go, oo, dka, dkb);
        if (!a.copy) continue;
        // the v heads: one contiguous run of Hv D elements per token
        const T *src = (BWD ? (const T *)a.dy + go : (const T *)a.x + xo) + nh * a.D;
        T *dst = (T *)a.o + oo + nh * a.D;
        const int64_t n = a.Hv * a.D;
        if constexpr (VEC) {
            const int64_t np = n / V;
            int64_t k0 = lane;
            for (; k0 + 64 * (kQknCopyU - 1) < np; k0 += 64 * kQknCopyU) {
                qkn_u32x4 r[kQknCopyU];
#pragma unroll
                for (int u = 0; u < kQknCopyU; ++u) r[u] = *(const qkn_u32x4 *)(src + (k0 + (int64_t)u * 64) * V);
#pragma unroll
                for (int u = 0; u < kQknCopyU; ++u) *(qkn_u32x4 *)(dst + (k0 + (int64_t)u * 64) * V) = r[u];
            }
            for (; k0 < np; k0 += 64) *(qkn_u32x4 *)(dst + k0 * V) = *(const qkn_u32x4 *)(src + k0 * V);
        } else {
            for (int64_t k = lane; k < n; k += 64) dst[k] = src[k];
        }
    }
    if constexpr (BWD) {
        if (a.part) {   // (uniform over the block)
            // the groups of the wave (lanes of one slot j), then the waves in wave order, then one row of the workspace
            for (int off = ln.G; off < 64; off <<= 1) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    dqa[k] += __shfl_xor(dqa[k], off, 64);
                    dqb[k] += __shfl_xor(dqb[k], off, 64);
                    dka[k] += __shfl_xor(dka[k], off, 64);
                    dkb[k] += __shfl_xor(dkb[k], off, 64);
                }
            }
            float *red = qkn_lds + (int64_t)wave * 2 * a.D;
            if (ln.hs == 0 && ln.own) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    red[ln.ea + k] = dqa[k];
                    red[ln.eb + k] = dqb[k];
                    red[a.D + ln.ea + k] = dka[k];
                    red[a.D + ln.eb + k] = dkb[k];
                }
            }
            __syncthreads();
            float *row = a.part + (int64_t)blockIdx.x * 2 * a.D;
            for (int64_t i = threadIdx.x; i < 2 * a.D; i += kQknBlock) {
                float v = qkn_lds[i];
#pragma unroll
                for (int w = 1; w < kQknBlock / 64; ++w) v += qkn_lds[(int64_t)w * 2 * a.D + i];
                row[i] = v;
            }
        }
    }
}

// ---- the element kernel: any element-aligned base and leading dimension, any D, any even R. One wave per block and per token
// (grid-stride); its 64 lanes take one head at a time. Item i < R/2 is the pair i, item i >= R/2 the single dim R + (i - R/2); lane k
// owns items k, k + 64, ... in both passes, so in place every element is read and written by one lane. The wave's weight sums live
// in its own workspace row, each dim with the lane that owns it.
template <typename T, bool IL, bool BWD>
__global__ __launch_bounds__(64) void qkn_elem(const QknArgs a) {
    const T *x = (const T *)a.x, *dy = (const T *)a.dy;
    T *o = (T *)a.o;
    const int lane = threadIdx.x;
    const int64_t half = a.R / 2, items = half + (a.D - a.R), nh = a.Hq + a.Hk;
    const float d = (float)a.D;
    float *part = BWD && a.part ? a.part + (int64_t)blockIdx.x * 2 * a.D : nullptr;
    // the dims of item i
    auto dims = [&](int64_t i, int64_t &ia, int64_t &ib) {
        if (i < half) { ia = IL ? 2 * i : i; ib = IL ? 2 * i + 1 : i + half; return true; }
        ia = ib = a.R + (i - half);
        return false;
    };
    if (part) {
        for (int64_t i = lane; i < items; i += 64) {
            int64_t ia, ib;
            dims(i, ia, ib);
            part[ia] = part[ib] = part[a.D + ia] = part[a.D + ib] = 0.f;
        }
    }
    for (int64_t tok = blockIdx.x; tok < a.tokens; tok += gridDim.x) {
        bool ok;
        const int64_t p = qkn_pos(a, tok, ok);
        const int64_t xo = tok * a.ldx, go = tok * a.lddy, oo = tok * a.ldo;
        for (int64_t h = 0; h < nh; ++h) {
            const bool isq = h < a.Hq;
            const T *w = (const T *)(isq ? a.wq : a.wk);
            const T *xh = x + xo + h * a.D, *gh = BWD ? dy + go + h * a.D : nullptr;
            T *oh = o + oo + h * a.D;
            // x (and in the backward g = rope^T(dy)) and the weights of item i
            auto item = [&](int64_t i, int64_t &ia, int64_t &ib, float &xa, float &xb, float &ga, float &gb, float &wa, float &wb, float &c, float &s) {
                const bool pair = dims(i, ia, ib);
                xa = load_f32(xh + ia);
                xb = pair ? load_f32(xh + ib) : 0.f;
                wa = w ? load_f32(w + ia) : 1.f;
                wb = w ? load_f32(w + ib) : 1.f;
                c = 1.f;
                s = 0.f;
                if (pair) {
                    c = ok ? a.cos[p * half + i] : __builtin_nanf("");
                    s = ok ? (BWD ? -a.sin[p * half + i] : a.sin[p * half + i]) : __builtin_nanf("");
                }
                ga = gb = 0.f;
                if constexpr (BWD) {
                    ga = load_f32(gh + ia);
                    if (pair) {
                        const float ta = ga, tb = load_f32(gh + ib);
                        qkn_rot_exact(ta, tb, c, s, ga, gb);
                    }
                }
                return pair;
            };
            float ss = 0.f, dot = 0.f;
            for (int64_t i = lane; i < items; i += 64) {
                int64_t ia, ib;
                float xa, xb, ga, gb, wa, wb, c, s;
                const bool pair = item(i, ia, ib, xa, xb, ga, gb, wa, wb, c, s);
                ss = qkn_sq(ss, xa);
                if (pair) ss = qkn_sq(ss, xb);
                if constexpr (BWD) {
                    dot = qkn_dot(dot, ga, wa, xa);
                    if (pair) dot = qkn_dot(dot, gb, wb, xb);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                ss += __shfl_xor(ss, off, 64);
                if constexpr (BWD) dot += __shfl_xor(dot, off, 64);
            }
            const float rstd = qkn_rstd(ss, d, a.eps);
            const float m = qkn_m(dot, rstd, d);
            float *pw = part ? part + (isq ? 0 : a.D) : nullptr;
            for (int64_t i = lane; i < items; i += 64) {
                int64_t ia, ib;
                float xa, xb, ga, gb, wa, wb, c, s;
                const bool pair = item(i, ia, ib, xa, xb, ga, gb, wa, wb, c, s);
                if constexpr (BWD) {
                    qkn_store1(oh + ia, qkn_dx(ga, wa, xa, rstd, m));
                    if (pair) qkn_store1(oh + ib, qkn_dx(gb, wb, xb, rstd, m));
                    if (pw) {
                        pw[ia] = qkn_dw(pw[ia], ga, xa, rstd);
                        if (pair) pw[ib] = qkn_dw(pw[ib], gb, xb, rstd);
                    }
                } else {
                    const float na = qkn_n(xa, rstd, wa), nb = qkn_n(xb, rstd, wb);
                    if (pair) {
                        float ya, yb;
                        qkn_rot(na, nb, c, s, ya, yb);
                        qkn_store1(oh + ia, ya);
                        qkn_store1(oh + ib, yb);
                    } else {
                        qkn_store1(oh + ia, na);
                    }
                }
            }
        }
        if (a.copy) {
            const T *src = (BWD ? dy + go : x + xo) + nh * a.D;
            T *dst = o + oo + nh * a.D;
            for (int64_t k = lane; k < a.Hv * a.D; k += 64) dst[k] = src[k];
        }
    }
}

// ---- the fold: dwq | dwk = the workspace rows added up, four interleaved runs of rows per column combined in a fixed order ------------
template <typename T>
__global__ __launch_bounds__(kQknBlock) void qkn_fold(const float *part, int64_t rows, int64_t D, T *dwq, T *dwk) {
    __shared__ float red[kQknBlock / 64][kQknFoldCols];
    const int cl = threadIdx.x & (kQknFoldCols - 1), rg = threadIdx.x / kQknFoldCols;
    const int64_t col = (int64_t)blockIdx.x * kQknFoldCols + cl;
    float v = 0.f;
    if (col < 2 * D)
        for (int64_t r = rg; r < rows; r += kQknBlock / kQknFoldCols) v += part[r * 2 * D + col];
    red[rg][cl] = v;
    __syncthreads();
    if (rg == 0 && col < 2 * D) {
#pragma unroll
        for (int w = 1; w < kQknBlock / kQknFoldCols; ++w) v += red[w][cl];
        T *dst = col < D ? dwq : dwk;
        if (dst) qkn_store1(dst + (col < D ? col : col - D), v);
    }
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------------
struct QknOperand { const char *name; const void *p; int64_t ld; };

struct QknGeom {
    int dtype;
    int64_t B, S, Hq, Hk, Hv, D, R;
    int interleaved;
    double eps;
    const void *wq, *wk;
    const float *cos, *sin;
    int64_t table_rows;
    const int64_t *positions;
    int64_t W() const { return (Hq + Hk + Hv) * D; }
    int64_t tokens() const { return B * S; }
};

int qkn_check_extents(const char *who, int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D) {
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(B >= 0 && S >= 0 && Hq >= 0 && Hk >= 0 && Hv >= 0 && D >= 0, KF_ERR_INVALID,
               "%s: negative extents B %lld S %lld Hq %lld Hk %lld Hv %lld D %lld", who, (long long)B, (long long)S, (long long)Hq, (long long)Hk,
               (long long)Hv, (long long)D);
    KF_REQUIRE(Hq + Hk >= 1, KF_ERR_INVALID, "%s: Hq + Hk = %lld < 1: no head to normalise", who, (long long)(Hq + Hk));
    return KF_OK;
}

int qkn_check(const char *who, const QknGeom &g, const QknOperand *ops, int n) {
    const int rc = qkn_check_extents(who, g.dtype, g.B, g.S, g.Hq, g.Hk, g.Hv, g.D);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(g.R >= 0 && g.R % 2 == 0 && g.R <= g.D, KF_ERR_INVALID, "%s: rotary_dim %lld must be even and in [0, D = %lld]", who, (long long)g.R,
               (long long)g.D);
    KF_REQUIRE(g.interleaved == 0 || g.interleaved == 1, KF_ERR_INVALID, "%s: interleaved must be 0 or 1, got %d", who, g.interleaved);
    KF_REQUIRE(g.eps >= 0.0 && g.eps <= 3.402823466e38, KF_ERR_INVALID, "%s: eps %g is negative or not finite", who, g.eps);
    const int es = dtype_size(g.dtype);
    for (int i = 0; i < n; ++i) {
        KF_REQUIRE(ops[i].p, KF_ERR_INVALID, "%s: null %s", who, ops[i].name);
        KF_REQUIRE(ops[i].ld >= g.W(), KF_ERR_INVALID, "%s: leading dimension of %s %lld < W = %lld", who, ops[i].name, (long long)ops[i].ld,
                   (long long)g.W());
    }
    if (g.R > 0) {
        KF_REQUIRE(g.cos && g.sin, KF_ERR_INVALID, "%s: rotary_dim %lld > 0 needs the cos and sin tables, got a null one", who, (long long)g.R);
        KF_REQUIRE(g.table_rows >= 1, KF_ERR_INVALID, "%s: table_rows %lld < 1", who, (long long)g.table_rows);
        KF_REQUIRE(g.positions || g.S <= g.table_rows, KF_ERR_INVALID, "%s: without positions the table needs S = %lld rows, it has %lld", who,
                   (long long)g.S, (long long)g.table_rows);
        KF_REQUIRE((uintptr_t)g.cos % 4 == 0 && (uintptr_t)g.sin % 4 == 0 && (!g.positions || (uintptr_t)g.positions % 8 == 0), KF_ERR_INVALID,
                   "%s: cos, sin or positions not aligned to its element size", who);
    }
    for (int i = 0; i < n; ++i)
        KF_REQUIRE((uintptr_t)ops[i].p % es == 0, KF_ERR_INVALID, "%s: %s not aligned to its element size", who, ops[i].name);
    KF_REQUIRE((uintptr_t)g.wq % es == 0 && (uintptr_t)g.wk % es == 0, KF_ERR_INVALID, "%s: wq or wk not aligned to its element size", who);
    return KF_OK;
}

// [p, p + (T - 1) ld + W) of two operands share no byte
bool qkn_disjoint(const QknOperand &u, const QknOperand &v, int64_t T, int64_t W, int es) {
    if (T == 0 || W == 0) return true;
    const uintptr_t a = (uintptr_t)u.p, b = (uintptr_t)v.p;
    const uintptr_t ea = a + (uintptr_t)((T - 1) * u.ld + W) * es, eb = b + (uintptr_t)((T - 1) * v.ld + W) * es;
    return ea <= b || eb <= a;
}

bool qkn_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the packed map fits the geometry; with `vec` it moves 16-byte packs
void qkn_plan(const QknGeom &g, const QknOperand *ops, int n, bool &packed, bool &vec) {
    const int V = 16 / dtype_size(g.dtype);
    packed = g.D % (2 * V) == 0 && g.D / (2 * V) <= 64 && (g.R / 2) % V == 0;
    vec = packed && qkn_aligned16(g.wq) && qkn_aligned16(g.wk) && (g.R == 0 || (qkn_aligned16(g.cos) && qkn_aligned16(g.sin)));
    for (int i = 0; i < n; ++i) vec = vec && qkn_aligned16(ops[i].p) && ops[i].ld % V == 0;
}

int64_t qkn_bwd_rows(int64_t tokens) { return std::min<int64_t>(tokens, kQknMaxParts); }
size_t qkn_bwd_bytes(int64_t tokens, int64_t D) { return (size_t)qkn_bwd_rows(tokens) * 2 * (size_t)D * sizeof(float); }

unsigned qkn_grid(bool bwd, bool packed, int64_t tokens) {
    return (unsigned)std::min<int64_t>(packed ? (tokens + kQknBlock / 64 - 1) / (kQknBlock / 64) : tokens, bwd ? kQknMaxParts : kQknMaxGrid);
}

template <bool BWD>
int qkn_run(const QknGeom &g, const QknArgs &a, bool packed, bool vec, unsigned grid, void *stream) {
    // elem: the element kernel; lanes: the packed map with element loads and stores; packed: the packed map moving 16-byte packs
    static const char *const labels[2][3] = {{"qk_norm_rope_fwd_elem", "qk_norm_rope_fwd_lanes", "qk_norm_rope_fwd_packed"},
                                             {"qk_norm_rope_bwd_elem", "qk_norm_rope_bwd_lanes", "qk_norm_rope_bwd_packed"}};
    hipStream_t st = as_stream(stream);
    KF_PROF(labels[BWD][packed ? (vec ? 2 : 1) : 0], st);
    return with_dtype(g.dtype, [&](auto t) {
        using T = decltype(t);
        return with_flags([&](auto IL, auto VEC) {
            if (packed) {
                const size_t lds = BWD && a.part ? (size_t)(kQknBlock / 64) * 2 * (size_t)a.D * sizeof(float) : 0;
                return launch(qkn_packed<T, IL, VEC, BWD>, grid, kQknBlock, lds, st, a);
            }
            return launch(qkn_elem<T, IL, BWD>, grid, 64, 0, st, a);
        }, g.interleaved != 0, vec);
    });
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_qk_norm_rope_fwd(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, int64_t rotary_dim, int interleaved,
                                   double eps, const void *wq, const void *wk, const float *cos, const float *sin, int64_t table_rows,
                                   const int64_t *positions, const void *x, int64_t ldx, void *y, int64_t ldy, void *stream) {
    const char *who = "kf_qk_norm_rope_fwd";
    const QknGeom g{dtype, B, S, Hq, Hk, Hv, D, rotary_dim, interleaved, eps, wq, wk, cos, sin, table_rows, positions};
    const QknOperand ops[2] = {{"x", x, ldx}, {"y", y, ldy}};
    const int rc = qkn_check(who, g, ops, 2);
    if (rc != KF_OK) return rc;
    const int es = dtype_size(dtype);
    KF_REQUIRE((y == x && ldy == ldx) || qkn_disjoint(ops[1], ops[0], g.tokens(), g.W(), es), KF_ERR_INVALID,
               "%s: y overlaps x (the only alias allowed is y == x with ldy == ldx)", who);
    if (g.tokens() == 0 || D == 0) return KF_OK;
    bool packed, vec;
    qkn_plan(g, ops, 2, packed, vec);
    const QknArgs a{cos, sin, positions, wq, wk, x, nullptr, y, nullptr, g.tokens(), S, Hq, Hk, Hv, D, rotary_dim, table_rows, ldx, 0, ldy, (float)eps,
                    y != x && Hv > 0};
    return qkn_run<false>(g, a, packed, vec, qkn_grid(false, packed, g.tokens()), stream);
}

extern "C" int kf_qk_norm_rope_bwd_workspace_bytes(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, size_t *bytes) {
    const char *who = "kf_qk_norm_rope_bwd_workspace_bytes";
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null out pointer", who);
    *bytes = 0;
    const int rc = qkn_check_extents(who, dtype, B, S, Hq, Hk, Hv, D);
    if (rc != KF_OK) return rc;
    *bytes = qkn_bwd_bytes(B * S, D);
    return KF_OK;
}

extern "C" int kf_qk_norm_rope_bwd(int dtype, int64_t B, int64_t S, int64_t Hq, int64_t Hk, int64_t Hv, int64_t D, int64_t rotary_dim, int interleaved,
                                   double eps, const void *wq, const void *wk, const float *cos, const float *sin, int64_t table_rows,
                                   const int64_t *positions, const void *x, int64_t ldx, const void *dy, int64_t lddy, void *dx, int64_t lddx,
                                   void *dwq, void *dwk, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "kf_qk_norm_rope_bwd";
    const QknGeom g{dtype, B, S, Hq, Hk, Hv, D, rotary_dim, interleaved, eps, wq, wk, cos, sin, table_rows, positions};
    const QknOperand ops[3] = {{"x", x, ldx}, {"dy", dy, lddy}, {"dx", dx, lddx}};
    const int rc = qkn_check(who, g, ops, 3);
    if (rc != KF_OK) return rc;
    const int es = dtype_size(dtype);
    KF_REQUIRE((uintptr_t)dwq % es == 0 && (uintptr_t)dwk % es == 0, KF_ERR_INVALID, "%s: dwq or dwk not aligned to its element size", who);
    KF_REQUIRE(qkn_disjoint(ops[2], ops[0], g.tokens(), g.W(), es), KF_ERR_INVALID, "%s: dx overlaps x (no alias of dx and x is allowed)", who);
    KF_REQUIRE((dx == dy && lddx == lddy) || qkn_disjoint(ops[2], ops[1], g.tokens(), g.W(), es), KF_ERR_INVALID,
               "%s: dx overlaps dy (the only alias allowed is dx == dy with lddx == lddy)", who);
    const bool want_dw = dwq || dwk;
    const size_t need = want_dw ? qkn_bwd_bytes(g.tokens(), D) : 0;
    KF_REQUIRE(!need || (workspace && workspace_bytes >= need && (uintptr_t)workspace % 4 == 0), KF_ERR_INVALID,
               "%s: workspace of %zu bytes (4-byte aligned) required for dwq / dwk, got %zu", who, need, workspace_bytes);
    if (g.tokens() == 0 || D == 0) return KF_OK;
    bool packed, vec;
    qkn_plan(g, ops, 3, packed, vec);
    const QknArgs a{cos, sin, positions, wq, wk, x, dy, dx, want_dw ? (float *)workspace : nullptr, g.tokens(), S, Hq, Hk, Hv, D, rotary_dim, table_rows,
                    ldx, lddy, lddx, (float)eps, dx != dy && Hv > 0};
    const unsigned rows = qkn_grid(true, packed, g.tokens());   // one workspace row per block
    const int rc2 = qkn_run<true>(g, a, packed, vec, rows, stream);
    if (rc2 != KF_OK || !want_dw) return rc2;
    hipStream_t st = as_stream(stream);
    KF_PROF("qk_norm_rope_bwd_fold", st);
    const unsigned grid = (unsigned)((2 * D + kQknFoldCols - 1) / kQknFoldCols);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return launch(qkn_fold<T>, grid, kQknBlock, 0, st, (const float *)workspace, (int64_t)rows, D, (T *)dwq, (T *)dwk);
    });
}
