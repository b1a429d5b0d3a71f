// Full (non-causal) softmax attention with an optional per-batch key length and grouped K/V heads, forward + backward, for gfx950
// (include/kfunca_hip.h: kf_attn_full_*). No reference counterpart: the reference has the causal kernel only
// (src/device/causal_attention_kernel.cu); this is the attention of an encoder, of a cross-attention layer and of a padded batch.
//
//   len_b  = clamp(kv_len[b], 0, Skv)   (kv_len == NULL: Skv)
//   s[m,n] = scale <q[b,h,m], k[b,h/G,n]>  for n < len_b;  o = softmax_n(s) v;  lse = log sum_n exp s  (len_b == 0: o = 0, lse = -inf)
//
// Two implementations behind one ABI:
//  * matrix-core path (bf16 / f16, D = 64 | 128, any Sq, Skv >= 1, strided operands): v_mfma_f32_32x32x16 in the operands' type, in
//    the orientation of attention.hip ("query on the lane" for the forward and dQ, "key on the lane" for dK/dV), with its LDS image
//    (256-byte rows, XOR swizzle, conflict-free for row reads and for ds_read_b64_tr_b16). The fragment types, the swizzle, the
//    transposed reads, the per-wave epilogue slab and the unmasked tile bodies are COPIES of attention.hip's (attn_fwd_v3_kernel,
//    attn_bwd_dq_v2_kernel): that file is part of the benchmark path and stays untouched.
//      forward  one 128-query block per workgroup (4 waves x 32 queries), 64-key tiles, K | V double-buffered in LDS
//      delta    rowsum(dO o O)
//      dQ       one 128-query block per workgroup, 64-key tiles; S and dP recomputed
//      dK/dV    one (batch, K/V head, 128-key block) per workgroup (4 waves x 32 keys, K and V fragments in registers); loops over the
//               group's G query heads in ascending order and over 64-query tiles of Q | dO, f32 accumulators: the group sum needs
//               no partial arrays, no second kernel and no atomics
//    Tiles are staged global -> registers -> LDS with a row predicate, not by LDS-DMA: a K / V row at n >= len_b (and a Q / dO row at
//    m >= Sq) is never LOADED - its LDS image is zeros - so padding that holds NaN or Inf cannot enter an MFMA operand, and the tile
//    loops stop at ceil(len_b / 64). Only the last key tile of a batch runs the masked tile body.
//  * generic path (f32; 16-bit with D <= 256 other than 64 and 128; bases that are not 16-byte aligned): plain vector-ALU kernels,
//    one workgroup per output row, f32 accumulation, the same semantics. They are meant to be correct, not fast; an f32 matrix-core
//    tier is out of scope.
//
// The prefix-LM variant (kf_attn_prefix_*: full inside a per-batch prefix, causal after it; no prefix: causal over a padded batch) is
// the same kernels compiled with CAUSAL:
//   pre_b = clamp(prefix_len[b], 0, Skv)   (prefix_len == NULL: 0);   query m sees key n  <=>  n < len_b and (n < pre_b or n <= m)
// top-left aligned with absolute indices, Sq and Skv in either size order. The mask enters a kernel as a loop bound or tile skip
// (key_bound, the per-wave skips, the dK/dV start tile t0), as the choice of the masked tile body, and as one compare-and-select per
// score inside it; besides that only the assignment of blocks to workgroups differs (block_of), which no result depends on. With
// pre_b >= len_b every choice is kf_attn_full_*'s and the results have its bits. The instantiations without CAUSAL are the code they
// were before the variant existed.
//
// The window variant (kf_attn_window_*: a band around the diagonal, either side optionally unbounded) is a third compile-time MODE of
// the same kernels:
//   query m sees key n  <=>  n < len_b and (wl < 0 or n >= m - wl) and (wr < 0 or n <= m + wr)
// top-left aligned with absolute indices. The keys a query sees are an interval that need not start at key 0, so the mask enters in
// the same three places with a lower edge as well: the key tiles of a query block are first .. last (first_tile, key_bound), not 0 .. last, and
// the query tiles of a key block likewise; a wave skips a tile outside the band of its 32 rows; the masked body selects on
// lo <= r < hi per lane (win_lim). A row may see no key of the first tile its block visits, or no key at all: the masked forward body
// carries such a row with a stand-in for its maximum (f_qk_sm), and the backward bodies select its p to 0 before anything is
// multiplied by it (its lse is -inf). (-1, -1) and (-1, 0) are dispatched to the two older families on the host.
// The document variant (kf_attn_doc_*: several independent sequences packed end to end in one row, self-attention, Sq = Skv = S) is a
// fourth MODE of the same kernels:
//   query m sees key n  <=>  n < len_b and doc_start[b, m] <= n < doc_end[b, m] and (causal == 0 or n <= m)
// The interval of the window variant, read from a per-token table (kf_attn_doc_table writes it from the documents' cumulative lengths)
// instead of computed from m: each lane loads its row's (start, end) once, the block's first and last row give its tile range, the
// wave's first and last row the tile skip and the choice of body, and the lane's own pair goes to the masked bodies of the window
// variant (MASK 3) unchanged. The tables describe a partition of the tokens into consecutive intervals, so both columns are
// nondecreasing along a row - which is what makes the first and last row of a block or wave its extremes - and the relation is
// symmetric: the dK/dV kernel reads the same two arrays at the KEY index to learn which queries see a key. Every entry is clamped on
// load, so no table content moves an access outside an operand; a table that is no partition gives an unspecified mask, nothing worse.
// No kernel uses atomics; every result is bitwise reproducible run to run.
//
// Two modifiers of the scores (kf_attn_ext_*) are compile-time switches of the same kernels; the
// instantiations without them are the code they were before the modifiers existed:
//   CAP   logit soft-capping, s = cap tanh(scale <q, k> / cap): the tile bodies turn each raw score into t = tanh(.) right after the
//         MFMAs (cap_tanh, built from v_exp_f32 and v_rcp_f32) and carry t where they carried the raw score, with c = cap log2(e) in
//         place of scale log2(e) - the running maximum, the deferred rescale, the mask selects and lse need nothing else. The
//         backward bodies multiply dS by 1 - t^2.
//   sink  one logit per query head that joins the softmax denominator and owns no value row: the forward EPILOGUE folds it into
//         1 / l and lse against max(m_i c, sink log2(e)) (fold_sink). The backward bodies are unchanged - P is formed from lse, which
//         holds the sink - and attn_sink_grad_kernel sums dsink from lse and the delta of the pre-pass in a fixed order.
// This header is the whole family but its C entries: the kernels and, below the `host` banner, the one host path - a kf_attn_mask
// checked once (mask_check), the call in four bundles, full_fwd<X> and full_bwd<CAP>. attn_full.hip holds the per-family entries and
// the instantiations without modifiers (plain_fwd, plain_bwd); attn_ext.hip holds kf_attn_ext_* and every modified instantiation, and
// calls plain_fwd / plain_bwd when the modifiers are off (two translation units, so the modified instantiations compile beside the
// others, not after them).
#pragma once

#include <math.h>

#include <algorithm>
#include <type_traits>

#include "float_pack.h"

namespace kf {
namespace full {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

struct Lay { int64_t sb, sh, sr; }; // byte strides of batch, head and row (the last dim is contiguous)

struct FullArgs {
    const char *q, *k, *v, *o, *d_o;
    char *out, *dq, *dk, *dv;
    float *lse;          // forward: written (may be null)
    const float *lse_r;  // backward: read
    float *delta;        // backward: rowsum(dO o O), [B, Hq, Sq]
    const int64_t *kv_len; // [B] on the device, or null
    int64_t B, H, Hkv, Sq, Skv, D;
    int G;               // query heads per K/V head
    float scale;
    Lay lq, lk, lv, lo, ldo, ldq, ldk, ldv;
    const int64_t *prefix_len; // [B] on the device, or null (the prefix-LM variant only; last, so no other member moves)
    int64_t wl, wr;            // the window variant only: keys m - wl .. m + wr; an unbounded side is kNoEdge
    const int32_t *doc_start, *doc_end; // the document variant only: [B, S] on the device, the keys start <= n < end of each token
    int causal;                         // the document variant only: 1 adds n <= m
    float softcap;                      // kf_attn_ext_* only: the cap of the instantiations compiled with CAP (positive and finite there)
    const float *sink;                  // kf_attn_ext_* only: [Hq] on the device, or null; read by the forward epilogues compiled for it
};

enum Mode { M_FULL = 0, M_PREFIX = 1, M_WINDOW = 2, M_DOC = 3 }; // the mask a kernel is compiled with
constexpr int64_t kNoEdge = (int64_t)1 << 40;         // a window side no index reaches (extents are at most 2^31): m - wl < 0, m + wr >= Skv

__device__ __forceinline__ int64_t key_len(const FullArgs &a, int64_t b) {
    if (!a.kv_len) return a.Skv;
    const int64_t l = a.kv_len[b];
    return l < 0 ? 0 : (l > a.Skv ? a.Skv : l);
}

// the prefix-LM variant (kf_attn_prefix_*): keys n < pre_b are visible to every query, the others to queries m >= n
__device__ __forceinline__ int64_t prefix_of(const FullArgs &a, int64_t b) {
    if (!a.prefix_len) return 0;
    const int64_t l = a.prefix_len[b];
    return l < 0 ? 0 : (l > a.Skv ? a.Skv : l);
}
__device__ __forceinline__ int clamp_i(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// Soft-capping. gfx950 has no tanh instruction: tanh(y) = sign(y) (1 - 2 / (exp(2 |y|) + 1)) from v_exp_f32 and v_rcp_f32. The |y| form
// has no cancellation at either end - exp2 overflows to +inf, whose reciprocal is 0, so a large |y| gives exactly 1 - and its absolute
// error is about 3 2^-23 with 1-ulp exp2 and rcp. x is the raw score <q, k>, k2 = 2 log2(e) scale / cap.
__device__ __forceinline__ float cap_tanh(float x, float k2) {
    const float e = __builtin_amdgcn_exp2f(fabsf(x) * k2);
    return copysignf(__builtin_fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f), x);
}
__device__ __forceinline__ float cap_k2(const FullArgs &a) { return 2.f * kLog2e * a.scale / a.softcap; }

// The sink in the matrix-core forward epilogue. In: l = sum_n exp2(s_n c - m c) over the visible keys, m the maximum in use (m c in
// exponent units of base 2; -inf with l = 0 for a row that saw no key), sk = sink log2(e). Out: the row's 1 / Z factor for o (inv) and
// lse / ln 2 (lg2). The maximum in use may trail the true one (the deferred rescale) and the sink may be of any size, so the sink is
// folded in against max(m c, sk): every exponent below is <= 0. sink = -inf adds exp2(-inf) = 0: the call without a sink, exactly, and
// a sink too small to move l leaves that call's expressions, hence its bits.
__device__ __forceinline__ void fold_sink(float l, float m, float c, float sk, float &inv, float &lg2) {
    if (sk > m * c) { // the sink is the row's maximum (always, for a row that saw no key and a finite sink)
        const float w = l > 0.f ? __builtin_amdgcn_exp2f(m * c - sk) : 0.f;
        const float z = __builtin_fmaf(l, w, 1.f);
        inv = w / z;
        lg2 = sk + __builtin_amdgcn_logf(z);
    } else if (l > 0.f) {
        const float z = l + __builtin_amdgcn_exp2f(sk - m * c);
        inv = 1.f / z;
        lg2 = __builtin_fmaf(m, c, __builtin_amdgcn_logf(z)); // (the fused form the epilogue without a sink compiles to: its bits)
    } else { // no visible key and sink = -inf
        inv = 0.f;
        lg2 = -INFINITY;
    }
}

// ==========================================================================================
// matrix-core path (idioms of attention.hip; the LDS images are laid out for D = 128 at both head sizes)
// ==========================================================================================
constexpr int AD = 128;
constexpr int AROW = AD * 2;       // bytes per row of a 16-bit tile
constexpr int OPAD = AROW + 8;     // epilogue staging row stride (bytes)
constexpr int TQ = 128;            // forward / dQ: queries per workgroup; dK/dV: keys per workgroup
constexpr int TK = 64;             // forward / dQ: keys per tile; dK/dV: queries per tile
constexpr int NT = 256;            // threads per workgroup (4 waves, one per SIMD)
constexpr int TILE = TK * AROW;    // bytes of one 64-row tile (16 KiB)
constexpr int SLOT = 2 * TILE;     // K | V   (dK/dV: Q | dO)
constexpr float kDeferMax = 8.0f;
constexpr float kPShiftLog2 = 14.f, kPShiftF16 = 16384.f; // f16 dK/dV: P is carried as P 2^14 into the dV product (attention.hip: kPShiftF16)

template <bool BF> struct AFrag { using type = f16x8; };
template <> struct AFrag<true> { using type = bf16x8; };

template <bool BF>
__device__ __forceinline__ f32x16 a_mfma(typename AFrag<BF>::type a, typename AFrag<BF>::type b, f32x16 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// 16-B chunk `ch` of row `row` lives at chunk position ch ^ (((row & 3) << 2) | ((row >> 2) & 3))
__device__ __forceinline__ int a_off(int row, int ch) { return row * AROW + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4); }

// registers 8s..8s+7 of an accumulator -> 16-bit B fragment of k-step s
template <bool BF>
__device__ __forceinline__ typename AFrag<BF>::type a_pack(const f32x16 &x, int s) {
    typename AFrag<BF>::type r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if constexpr (BF)
            r[j] = (__bf16)x[8 * s + j];
        else
            r[j] = (_Float16)x[8 * s + j];
    }
    return r;
}

// accumulator row index of register e for lane half h
__device__ __forceinline__ int a_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <bool BF>
__device__ __forceinline__ uint32_t a_cvt16(float v) { return BF ? f32_to_bf16(v).x : f32_to_f16(v).x; }

// a wave's 32 x D result held as X^T accumulators (lane = row, registers = columns) -> 16-bit rows of dst, via a per-wave LDS slab
template <bool BF, int DB>
__device__ __forceinline__ void a_store_rows(char *slab, char *dst, const f32x16 (&acc)[DB], float mul, int64_t rs, int nrows) {
    const int lane = threadIdx.x & 63, xl = lane & 31, hl = lane >> 5;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const uint32_t h0 = a_cvt16<BF>(acc[db][4 * gq + 0] * mul), h1 = a_cvt16<BF>(acc[db][4 * gq + 1] * mul);
            const uint32_t h2 = a_cvt16<BF>(acc[db][4 * gq + 2] * mul), h3 = a_cvt16<BF>(acc[db][4 * gq + 3] * mul);
            uint2 w;
            w.x = h0 | (h1 << 16);
            w.y = h2 | (h3 << 16);
            const int col = db * 32 + 8 * gq + 4 * hl;
            *(uint2 *)(slab + xl * OPAD + col * 2) = w;
        }
    // same wave reads back what it wrote: LDS ops of one wave complete in order
#pragma unroll
    for (int i = 0; i < 4 * DB; ++i) {
        const int id = lane + 64 * i;
        const int row = id / (8 * DB), piece = id % (8 * DB);
        const uint2 w = *(const uint2 *)(slab + row * OPAD + piece * 8);
        if (row < nrows) *(uint2 *)(dst + (int64_t)row * rs + piece * 8) = w;
    }
}

// per-lane byte offset (relative to the tile, for a 16-row-aligned r0) of the two transposed reads
__device__ __forceinline__ int a_tr_lane_off(int col0, int second) {
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, i = lane & 15, qq = i >> 2, p = i & 3, h = g >> 1;
    const int ch = ((col0 + 16 * (g & 1)) >> 3) + (p >> 1);
    return a_off(4 * h + qq + 8 * second, ch) + 8 * (p & 1);
}

// transposed reads issued from inline asm (attention.hip: tr4_issue / tr4_wait1 / tr4_wait_next)
template <int DB> struct TrN { s16x4 lo[DB], hi[DB]; };
using Tr4 = TrN<4>;
using Tr2 = TrN<2>;
template <int ROFF>
__device__ __forceinline__ void tr4_issue(const char *tile, const int (&vo)[2][2], Tr2 &t) {
    const unsigned base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)tile;
    asm volatile("ds_read_b64_tr_b16 %0, %4 offset:%c8\n\tds_read_b64_tr_b16 %1, %5 offset:%c8\n\t"
                 "ds_read_b64_tr_b16 %2, %6 offset:%c8\n\tds_read_b64_tr_b16 %3, %7 offset:%c8"
                 : "=&v"(t.lo[0]), "=&v"(t.hi[0]), "=&v"(t.lo[1]), "=&v"(t.hi[1])
                 : "v"(base + vo[0][0]), "v"(base + vo[0][1]), "v"(base + vo[1][0]), "v"(base + vo[1][1]), "i"(ROFF)
                 : "memory");
}
__device__ __forceinline__ void tr4_wait1(Tr2 &a) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a.lo[0]), "+v"(a.hi[0]), "+v"(a.lo[1]), "+v"(a.hi[1]) : : "memory");
}
template <int ROFF>
__device__ __forceinline__ void tr4_issue(const char *tile, const int (&vo)[4][2], Tr4 &t) {
    const unsigned base = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)tile;
    asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%c16\n\tds_read_b64_tr_b16 %1, %9 offset:%c16\n\t"
                 "ds_read_b64_tr_b16 %2, %10 offset:%c16\n\tds_read_b64_tr_b16 %3, %11 offset:%c16\n\t"
                 "ds_read_b64_tr_b16 %4, %12 offset:%c16\n\tds_read_b64_tr_b16 %5, %13 offset:%c16\n\t"
                 "ds_read_b64_tr_b16 %6, %14 offset:%c16\n\tds_read_b64_tr_b16 %7, %15 offset:%c16"
                 : "=&v"(t.lo[0]), "=&v"(t.hi[0]), "=&v"(t.lo[1]), "=&v"(t.hi[1]), "=&v"(t.lo[2]), "=&v"(t.hi[2]), "=&v"(t.lo[3]), "=&v"(t.hi[3])
                 : "v"(base + vo[0][0]), "v"(base + vo[0][1]), "v"(base + vo[1][0]), "v"(base + vo[1][1]), "v"(base + vo[2][0]),
                   "v"(base + vo[2][1]), "v"(base + vo[3][0]), "v"(base + vo[3][1]), "i"(ROFF)
                 : "memory");
}
__device__ __forceinline__ void tr4_wait1(Tr4 &a) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a.lo[0]), "+v"(a.hi[0]), "+v"(a.lo[1]), "+v"(a.hi[1]), "+v"(a.lo[2]), "+v"(a.hi[2]), "+v"(a.lo[3]), "+v"(a.hi[3])
                 :
                 : "memory");
}
__device__ __forceinline__ void tr4_wait_next(Tr2 &a) {
    asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(a.lo[0]), "+v"(a.hi[0]), "+v"(a.lo[1]), "+v"(a.hi[1]) : : "memory");
}
__device__ __forceinline__ void tr4_wait_next(Tr4 &a) {
    asm volatile("s_waitcnt lgkmcnt(8)"
                 : "+v"(a.lo[0]), "+v"(a.hi[0]), "+v"(a.lo[1]), "+v"(a.hi[1]), "+v"(a.lo[2]), "+v"(a.hi[2]), "+v"(a.lo[3]), "+v"(a.hi[3])
                 :
                 : "memory");
}
template <bool BF, int DB>
__device__ __forceinline__ typename AFrag<BF>::type tr4_frag(const TrN<DB> &t, int d) {
    s16x8 r;
    r[0] = t.lo[d][0]; r[1] = t.lo[d][1]; r[2] = t.lo[d][2]; r[3] = t.lo[d][3];
    r[4] = t.hi[d][0]; r[5] = t.hi[d][1]; r[6] = t.hi[d][2]; r[7] = t.hi[d][3];
    return __builtin_bit_cast(typename AFrag<BF>::type, r);
}

__device__ __forceinline__ float a_half_max(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
}
__device__ __forceinline__ float a_half_sum(float x) {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// Staging of one 64-row tile pair (K | V, or Q | dO): global -> registers (t_load, issued a tile ahead) -> swizzled LDS image (t_store).
// 64 rows x D / 8 pieces of 16 bytes over 256 threads: D / 32 pieces of each tensor per thread. A row at or beyond `nrows` is NOT
// loaded: its image is zeros (the key-length bound and the ragged last tile in one predicate).
template <int D> struct TileRegs { uint4 x[D / 32], y[D / 32]; };
template <int D>
__device__ __forceinline__ void t_load(TileRegs<D> &r, const char *xg, const char *yg, int64_t xrs, int64_t yrs, int64_t nrows) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int id = threadIdx.x + NT * i, row = id / (D / 8), ch = id % (D / 8);
        r.x[i] = r.y[i] = uint4{0, 0, 0, 0};
        if (row < nrows) {
            r.x[i] = *(const uint4 *)(xg + row * xrs + ch * 16);
            r.y[i] = *(const uint4 *)(yg + row * yrs + ch * 16);
        }
    }
}
template <int D>
__device__ __forceinline__ void t_store(const TileRegs<D> &r, char *slot) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int id = threadIdx.x + NT * i, row = id / (D / 8), ch = id % (D / 8);
        *(uint4 *)(slot + a_off(row, ch)) = r.x[i];
        *(uint4 *)(slot + TILE + a_off(row, ch)) = r.y[i];
    }
}

// forward / dQ: keys the workgroup of query block xb walks (tiles 0 .. ceil(bound / 64) - 1, ascending). The prefix-LM variant stops
// at the last key one of its queries can see: min(len, max(pre, min(Sq, xb 128 + 128)))
// Which block of its (batch, head) a workgroup takes. Under the causal mask a block's work grows (forward, dQ) or shrinks (dK/dV)
// with its index, and the hardware deals consecutive workgroup ids round-robin to XCDs and shader engines: with block = id % n the
// heavy blocks of every head land on the same engines and the light ones on the others, and the kernel takes as long as without the
// mask. Rotating the blocks of each (batch, head) by a hash of its index gives every engine every block size. The results do not
// depend on which workgroup computes a block.
// Under a window the work of a block does not depend on its index while every key exists, but a key length makes it so again: the
// blocks beyond len_b + wl walk no tile at all, and with block = id % n those of every head of the batch share their engines. Measured
// both ways: the rotation costs nothing where the work is uniform and takes a padded batch from 1.6 - 1.9 to
// 1.2 - 1.4 times the time its tiles account for, so the window variant rotates as the causal one does.
template <int MODE>
__device__ __forceinline__ int64_t block_of(int64_t pos, int64_t group, int64_t n) {
    if constexpr (MODE == M_FULL) return pos;
    return (pos + (int64_t)(((uint32_t)group * 2654435761u) >> 16)) % n;
}

// rows of the tile at kv0 that the query of lane xl of the wave at qw sees: min(len, max(pre, qw + xl + 1)) - kv0, clamped to the tile.
// Everything but the last step is wave-uniform (scalar); the clamp of qw + 1 - kv0 keeps it in 32 bits without changing the result.
__device__ __forceinline__ int tile_lim(int64_t len, int64_t pre, int64_t qw, int64_t kv0, int xl) {
    const int nl = clamp_i(len - kv0, 0, TK), np = clamp_i(pre - kv0, 0, TK), dq1 = clamp_i(qw + 1 - kv0, -32, TK);
    const int dm1 = dq1 + xl;
    return min(nl, max(np, dm1));
}

// lo <= r < lo + n as one compare (n >= 0: win_lim and the dK/dV kernel hand over the interval as first row and row count)
__device__ __forceinline__ bool win_in(int r, int lo, int n) { return (unsigned)(r - lo) < (unsigned)n; }

template <int MODE>
__device__ __forceinline__ int64_t key_bound(const FullArgs &a, int64_t len, int64_t pre, int64_t xb) {
    if constexpr (MODE == M_FULL) return len;
    const int64_t qe = a.Sq < xb * TQ + TQ ? a.Sq : xb * TQ + TQ;
    if constexpr (MODE == M_WINDOW) return len < qe + a.wr ? len : qe + a.wr; // the last query qe - 1 sees up to key qe - 1 + wr
    const int64_t vis = pre > qe ? pre : qe;
    return len < vis ? len : vis;
}
// window variant: the first key tile of query block xb - the one that holds key max(0, xb 128 - wl), the first its first query sees
template <int MODE>
__device__ __forceinline__ int first_tile(const FullArgs &a, int64_t xb) {
    if constexpr (MODE != M_WINDOW) return 0;
    const int64_t lo = xb * TQ - a.wl;
    return lo > 0 ? (int)(lo / TK) : 0;
}
// window variant: the rows lo <= r < hi of the tile at kv0 that the query of lane xl of the wave at qw sees, i.e. the keys
// max(0, m - wl) <= n < min(len, m + wr + 1) relative to kv0. As in tile_lim everything but the last addition is wave-uniform, and the
// clamps keep it in 32 bits without changing which rows 0 .. 63 pass: below -32 every lane's bound is negative, above 64 none's is.
// Handed over as the first row and the row count (0 when the interval is empty), for win_in.
__device__ __forceinline__ void win_lim(const FullArgs &a, int64_t len, int64_t qw, int64_t kv0, int xl, int &lo, int &cnt) {
    const int nl = clamp_i(len - kv0, 0, TK);
    lo = clamp_i(qw - a.wl - kv0, -32, TK) + xl;
    cnt = max(min(nl, clamp_i(qw + a.wr + 1 - kv0, -32, TK) + xl) - lo, 0);
}

// document variant, forward and dQ: the keys lo <= n < hi that query m of batch b sees, clamped into [0, len] (the key tiles walked and
// the rows loaded follow from these alone); with causal the interval ends at the query itself. m < Sq.
__device__ __forceinline__ int doc_lo(const FullArgs &a, int64_t b, int64_t m, int64_t len) { return clamp_i(a.doc_start[b * a.Sq + m], 0, (int)len); }
__device__ __forceinline__ int doc_hi(const FullArgs &a, int64_t b, int64_t m, int64_t len) {
    const int e = clamp_i(a.doc_end[b * a.Sq + m], 0, (int)len);
    return a.causal && e > m + 1 ? (int)(m + 1) : e;
}
// document variant, dK/dV: the queries lo <= m < hi that see key n of batch b - the same two arrays read at the key (the relation is
// symmetric), clamped into [0, Sq]; with causal the interval starts at the key itself. n < Skv = Sq.
__device__ __forceinline__ int doc_qlo(const FullArgs &a, int64_t b, int64_t n) {
    const int s = clamp_i(a.doc_start[b * a.Sq + n], 0, (int)a.Sq);
    return a.causal && s < n ? (int)n : s;
}
__device__ __forceinline__ int doc_qhi(const FullArgs &a, int64_t b, int64_t n) { return clamp_i(a.doc_end[b * a.Sq + n], 0, (int)a.Sq); }
// the rows of the tile at t0 inside lo <= r < hi, as win_in takes them: first row and row count
__device__ __forceinline__ void doc_lim(int lo_abs, int hi_abs, int64_t t0, int &lo, int &cnt) {
    lo = clamp_i(lo_abs - t0, 0, TK);
    cnt = max(clamp_i(hi_abs - t0, 0, TK) - lo, 0);
}
// forward / dQ: the key tiles of query block xb, from the tile of the first key its first row sees to the tile of the last key its last
// row (below Sq) sees; doc_lo and doc_hi lie in [0, len], so both tiles lie in [0, ceil(len / 64)]
__device__ __forceinline__ int doc_first_tile(const FullArgs &a, int64_t b, int64_t len, int64_t xb) { return doc_lo(a, b, xb * TQ, len) / TK; }
__device__ __forceinline__ int doc_last_tile(const FullArgs &a, int64_t b, int64_t len, int64_t xb) {
    const int64_t last = (a.Sq < xb * TQ + TQ ? a.Sq : xb * TQ + TQ) - 1;
    return (doc_hi(a, b, last, len) + TK - 1) / TK;
}
// forward / dQ: the interval of the lane's own row (empty for a row beyond Sq) and, wave-uniform, those of the wave's first row and of
// its last row below Sq. Both columns are nondecreasing along a row, so the wave sees the keys lo_first .. hi_last - 1 and nothing else,
// and every row of it sees every key of lo_last .. hi_first - 1.
struct DocRows { int lo, hi, lo_first, lo_last, hi_first, hi_last; };
template <bool DOC>
__device__ __forceinline__ DocRows doc_rows(const FullArgs &a, int64_t b, int64_t len, int64_t qw, int64_t m, bool active) {
    DocRows r{0, 0, 0, 0, 0, 0};
    if constexpr (DOC) {
        if (m < a.Sq) {
            r.lo = doc_lo(a, b, m, len);
            r.hi = doc_hi(a, b, m, len);
        }
        if (active) {
            const int64_t last = (a.Sq < qw + 32 ? a.Sq : qw + 32) - 1;
            r.lo_first = __builtin_amdgcn_readfirstlane(doc_lo(a, b, qw, len));
            r.lo_last = __builtin_amdgcn_readfirstlane(doc_lo(a, b, last, len));
            r.hi_first = __builtin_amdgcn_readfirstlane(doc_hi(a, b, qw, len));
            r.hi_last = __builtin_amdgcn_readfirstlane(doc_hi(a, b, last, len));
        }
    }
    return r;
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
// S^T = K Q^T (A = K rows from LDS, B = Q fragments in registers), online softmax with a deferred running maximum. MASK 1: the last
// tile of a batch whose key count is no multiple of 64 - keys at kv0 + row >= len get -inf (their K rows are zeros in LDS). MASK 2
// (prefix-LM variant): the keys a query sees are a leading interval, n < min(len, max(pre, m + 1)), so tile row r is visible to this
// lane's query iff r < lim, that bound relative to the tile (tile_lim). MASK 3 (window variant): the keys a query sees are an interval
// that starts anywhere: tile row r is visible iff lo <= r < lo + lim (win_lim: first row and row count)
// CAP (soft-capping): each raw score becomes t = tanh(scale <q, k> / cap) before the mask selects, c is cap log2(e), and m_i is a
// maximum of t; a zero K row gives t = 0, which the select then replaces like any other score.
template <bool BF, int MASK, int D, bool CAP = false>
__device__ __forceinline__ void f_qk_sm(const char *buf, const typename AFrag<BF>::type (&qf)[D / 16], const int (&ko)[D / 16], f32x16 (&o)[D / 32],
                                        typename AFrag<BF>::type (&pf)[4], float &m_i, float &l_i, float c, float k2, int64_t kv0, int64_t len, int hl,
                                        int lim = 0, int lo = 0) {
    using frag_t = typename AFrag<BF>::type;
    f32x16 s[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[sub][e] = 0.f;
#pragma unroll
        for (int kg = 0; kg < D / 64; ++kg) {
#pragma unroll
            for (int kk = 4 * kg; kk < 4 * kg + 4; ++kk)
                s[sub] = a_mfma<BF>(*(const frag_t *)(buf + sub * 32 * AROW + ko[kk]), qf[kk], s[sub]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if constexpr (CAP) s[sub][e] = cap_tanh(s[sub][e], k2);
            if constexpr (MASK == 1) {
                if (kv0 + sub * 32 + a_row(e, hl) >= len) s[sub][e] = -INFINITY;
            } else if constexpr (MASK == 2) {
                if (sub * 32 + a_row(e, hl) >= lim) s[sub][e] = -INFINITY;
            } else if constexpr (MASK == 3) {
                if (!win_in(sub * 32 + a_row(e, hl), lo, lim)) s[sub][e] = -INFINITY;
            }
            mx = fmaxf(mx, s[sub][e]);
        }
    // Without the causal mask mx is finite: key kv0 of every visited tile is visible. With it a row may see no key of this tile
    // (mx = -inf), but never in tile 0, which is visited first and holds key 0, visible to every row (rows m >= Sq included): m_i is
    // finite from there on, so m_i - fmaxf(m_i, -inf) = 0 and exp2(-inf - m_i c) = 0 - no (-inf) - (-inf) arises.
    // Under a window (MASK 3) that argument is gone: the first tile a block visits is seen by its earliest queries only, and a row
    // beyond the keys' end sees none at all, so a row can be EMPTY so far: m_i = -inf, l_i = 0, o = 0. m_i stays -inf as the row's
    // state - the first finite mx then exceeds it by +inf and is adopted with alpha = exp2(-inf) = 0 on l_i = 0 and o = 0, exactly as in
    // tile 0 of the other variants - and only the two places where (-inf) - (-inf) would arise use a finite stand-in, 0, for it:
    //   mx = -inf too, adoption forced by another row of the wave: (mx - m_i) c is NaN and compares false, so this row never asks; there
    //     m_new = -inf and alpha is set to 1 (l_i and o are zeros; nothing to rescale);
    //   the exponent: mc = 0 in place of -inf c, so p = exp2(fma(-inf, c, -0)) = 0 for each of its scores, all of which are -inf.
    // A row that is not empty has a finite m_i and takes neither select. The unmasked body needs nothing: its mx is finite.
    mx = a_half_max(mx);
    // deferred running maximum (attention.hip: s_qk_sm): a larger one is adopted, and O and l rescaled, only when some query of the
    // wave exceeds the maximum in use by more than kDeferMax exponent units
    if (__builtin_amdgcn_ballot_w64((mx - m_i) * c > kDeferMax) != 0) {
        const float m_new = fmaxf(m_i, mx);
        float alpha = __builtin_amdgcn_exp2f((m_i - m_new) * c);
        if constexpr (MASK == 3) alpha = m_new == -INFINITY ? 1.f : alpha;
        l_i *= alpha;
#pragma unroll
        for (int d = 0; d < D / 32; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[d][e] *= alpha;
        m_i = m_new;
    }
    const float mc = MASK == 3 && m_i == -INFINITY ? 0.f : m_i * c;
    float rs = 0.f;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[sub][e], c, -mc));
            s[sub][e] = p;
            rs += p;
        }
    rs = a_half_sum(rs);
    l_i += rs;
    pf[0] = a_pack<BF>(s[0], 0);
    pf[1] = a_pack<BF>(s[0], 1);
    pf[2] = a_pack<BF>(s[1], 0);
    pf[3] = a_pack<BF>(s[1], 1);
}

// acc^T += T^T X^T over the 64 rows of the row-major LDS tile `vt` (A = T^T through transposed reads, B = the four packed k-steps)
template <bool BF, int DB>
__device__ __forceinline__ void f_pv(const char *vt, const int (&vo)[DB][2], const typename AFrag<BF>::type (&pf)[4], f32x16 (&o)[DB]) {
    TrN<DB> ta, tb;
    tr4_issue<0>(vt, vo, ta);
    tr4_issue<16 * AROW>(vt, vo, tb);
    tr4_wait_next(ta);
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = a_mfma<BF>(tr4_frag<BF, DB>(ta, d), pf[0], o[d]);
    __builtin_amdgcn_sched_barrier(0);
    tr4_issue<32 * AROW>(vt, vo, ta);
    tr4_wait_next(tb);
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = a_mfma<BF>(tr4_frag<BF, DB>(tb, d), pf[1], o[d]);
    __builtin_amdgcn_sched_barrier(0);
    tr4_issue<48 * AROW>(vt, vo, tb);
    tr4_wait_next(ta);
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = a_mfma<BF>(tr4_frag<BF, DB>(ta, d), pf[2], o[d]);
    __builtin_amdgcn_sched_barrier(0);
    tr4_wait1(tb);
#pragma unroll
    for (int d = 0; d < DB; ++d) o[d] = a_mfma<BF>(tr4_frag<BF, DB>(tb, d), pf[3], o[d]);
    __builtin_amdgcn_sched_barrier(0);
}

// CAUSAL (the prefix-LM variant) enters in three places only: the tile bound / per-wave tile skip, the choice of the masked body,
// and the select on the scores inside it. WIN (the window variant) enters in the same three, with a first tile besides the bound.
// X (kf_attn_ext_*): X_SINK compiles the sink into the epilogue, X_CAP the soft-cap into the tile bodies and the sink (read when
// a.sink is given) into the epilogue; X_NONE is the kernel without modifiers.
enum Ext { X_NONE = 0, X_SINK = 1, X_CAP = 2 };
template <bool BF, int D, int MODE, int X = X_NONE>
__global__ __launch_bounds__(NT, MODE != M_FULL && D == 64 ? 2 : 1) void attn_full_fwd_kernel(const FullArgs a) {
    using frag_t = typename AFrag<BF>::type;
    constexpr bool CAUSAL = MODE == M_PREFIX, WIN = MODE == M_WINDOW, DOC = MODE == M_DOC, CAP = X == X_CAP;
    constexpr int KS = D / 16, DB = D / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, xl = lane & 31, hl = lane >> 5;
    const int64_t nxb = (a.Sq + TQ - 1) / TQ;
    const int64_t bh = blockIdx.x / nxb, xb = block_of<MODE>(blockIdx.x % nxb, bh, nxb), b = bh / a.H, h = bh % a.H, g = h / a.G;
    const int64_t len = key_len(a, b);
    const int64_t pre = CAUSAL ? prefix_of(a, b) : 0;
    const int nt = DOC ? doc_last_tile(a, b, len, xb) : (int)((key_bound<MODE>(a, len, pre, xb) + TK - 1) / TK);
    const int tf = DOC ? doc_first_tile(a, b, len, xb) : first_tile<MODE>(a, xb); // 0 but under a window or a document mask; there nt <= tf when no query of the block sees a key
    const char *Kg = a.k + b * a.lk.sb + g * a.lk.sh;
    const char *Vg = a.v + b * a.lv.sb + g * a.lv.sh;
    int ko[KS], vo[DB][2];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) ko[kk] = a_off(xl, kk * 2 + hl);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        vo[d][0] = a_tr_lane_off(d * 32, 0);
        vo[d][1] = a_tr_lane_off(d * 32, 1);
    }
    const float c = (CAP ? a.softcap : a.scale) * kLog2e, k2 = CAP ? cap_k2(a) : 0.f;
    const int64_t qw = xb * TQ + wid * 32, m = qw + xl;
    const bool active = qw < a.Sq; // wave-uniform
    const DocRows dr = doc_rows<DOC>(a, b, len, qw, m, active);

    frag_t qf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[kk][j] = 0;
    if (m < a.Sq) { // a query row beyond Sq is neither read nor stored
        const char *Qg = a.q + b * a.lq.sb + h * a.lq.sh + m * a.lq.sr;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = *(const frag_t *)(Qg + (kk * 16 + 8 * hl) * 2);
    }
    f32x16 o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[d][e] = 0.f;
    float m_i = -INFINITY, l_i = 0.f;
    frag_t pf[4];

    TileRegs<D> tr;
    if (nt > tf) {
        t_load<D>(tr, Kg + (int64_t)tf * TK * a.lk.sr, Vg + (int64_t)tf * TK * a.lv.sr, a.lk.sr, a.lv.sr, len - (int64_t)tf * TK);
        t_store<D>(tr, smem);
    }
    for (int t = tf; t < nt; ++t) {
        const int64_t kv0 = (int64_t)t * TK;
        if (t + 1 < nt) t_load<D>(tr, Kg + (kv0 + TK) * a.lk.sr, Vg + (kv0 + TK) * a.lv.sr, a.lk.sr, a.lv.sr, len - kv0 - TK);
        __syncthreads(); // tile t is in its slot; slot (t + 1) & 1 is no longer read
        const char *cur = smem + ((t - tf) & 1) * SLOT;
        if constexpr (CAUSAL) {
            // (wave-uniform) no query of the wave sees a key of a tile at or beyond both the prefix and the wave's last query; tile 0 is
            // never skipped (qw + 32 > 0). A skipping wave still stages and synchronises.
            if (active && kv0 < (pre > qw + 32 ? pre : qw + 32)) {
                if (kv0 + TK > len || (kv0 + TK - 1 > qw && kv0 + TK - 1 >= pre)) {
                    f_qk_sm<BF, 2, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl, tile_lim(len, pre, qw, kv0, xl));
                } else f_qk_sm<BF, 0, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl);
                f_pv<BF, DB>(cur + TILE, vo, pf, o);
            }
        } else if constexpr (WIN) {
            // (wave-uniform) skip a tile that lies wholly outside the keys qw - wl .. qw + 31 + wr of the wave's 32 rows; the masked body
            // where the length, the lower edge (of the wave's last row) or the upper edge (of its first) cuts the tile
            if (active && kv0 + TK > qw - a.wl && kv0 <= qw + 31 + a.wr) {
                if (kv0 + TK > len || qw + 31 - a.wl > kv0 || qw + a.wr < kv0 + TK - 1) {
                    int lo, cnt;
                    win_lim(a, len, qw, kv0, xl, lo, cnt);
                    f_qk_sm<BF, 3, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl, cnt, lo);
                } else f_qk_sm<BF, 0, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl);
                f_pv<BF, DB>(cur + TILE, vo, pf, o);
            }
        } else if constexpr (DOC) {
            // (wave-uniform) skip a tile that lies wholly outside the keys of the wave's rows; the masked body (the window variant's:
            // an interval per lane) unless every row sees all 64 keys - a tile the length cuts has hi_first <= len < kv0 + 64
            if (active && kv0 + TK > dr.lo_first && kv0 < dr.hi_last) {
                if (dr.lo_last > kv0 || dr.hi_first < kv0 + TK) {
                    int lo, cnt;
                    doc_lim(dr.lo, dr.hi, kv0, lo, cnt);
                    f_qk_sm<BF, 3, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl, cnt, lo);
                } else f_qk_sm<BF, 0, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl);
                f_pv<BF, DB>(cur + TILE, vo, pf, o);
            }
        } else if (active) {
            if (kv0 + TK > len) f_qk_sm<BF, 1, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl);
            else f_qk_sm<BF, 0, D, CAP>(cur, qf, ko, o, pf, m_i, l_i, c, k2, kv0, len, hl);
            f_pv<BF, DB>(cur + TILE, vo, pf, o);
        }
        if (t + 1 < nt) t_store<D>(tr, smem + ((t + 1 - tf) & 1) * SLOT);
    }
    __syncthreads();
    if (active) {
        const int64_t left = a.Sq - qw;
        if constexpr (X != X_NONE) {
            if (a.sink) { // (workgroup-uniform) a row that saw no key: inv = 0 whatever the sink, so o = 0 as zero bits, and lse = sink
                float inv, lg2;
                const float sink = a.sink[h];
                fold_sink(l_i, m_i, c, sink * kLog2e, inv, lg2);
                a_store_rows<BF, DB>(smem + wid * 32 * OPAD, a.out + b * a.lo.sb + h * a.lo.sh + qw * a.lo.sr, o, inv, a.lo.sr, left < 32 ? (int)left : 32);
                if (a.lse && hl == 0 && m < a.Sq) a.lse[bh * a.Sq + m] = l_i > 0.f ? lg2 * kLn2 : sink; // (no key: the stored value itself)
                return;
            }
        }
        const float inv = l_i > 0.f ? 1.f / l_i : 0.f; // no visible key: o = 0, lse = -inf
        a_store_rows<BF, DB>(smem + wid * 32 * OPAD, a.out + b * a.lo.sb + h * a.lo.sh + qw * a.lo.sr, o, inv, a.lo.sr, left < 32 ? (int)left : 32);
        if (a.lse && hl == 0 && m < a.Sq) a.lse[bh * a.Sq + m] = l_i > 0.f ? (m_i * c + __builtin_amdgcn_logf(l_i)) * kLn2 : -INFINITY;
    }
}

// ------------------------------------------------------------------------------------------
// backward pre-pass: delta[q] = sum_d dO[q][d] * O[q][d]   (16 lanes per row, 16-B loads)
// ------------------------------------------------------------------------------------------
template <bool BF>
__global__ __launch_bounds__(NT) void attn_full_delta_kernel(const char *o, const char *d_o, float *delta, int64_t nrows, Lay lo, Lay ldo, int64_t S, int64_t H,
                                                             int nparts) {
    const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int part = threadIdx.x & 15;
    uint4 x = uint4{0, 0, 0, 0}, y = x;
    if (row < nrows && part < nparts) {
        const int64_t bh = row / S, sq = row - bh * S, bb = bh / H, hh = bh % H;
        x = *(const uint4 *)(o + bb * lo.sb + hh * lo.sh + sq * lo.sr + part * 16);
        y = *(const uint4 *)(d_o + bb * ldo.sb + hh * ldo.sh + sq * ldo.sr + part * 16);
    }
    float acc = 0.f;
    const uint32_t xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float a0, a1, b0, b1;
        if constexpr (BF) {
            a0 = __uint_as_float(xw[j] << 16); a1 = __uint_as_float(xw[j] & 0xffff0000u);
            b0 = __uint_as_float(yw[j] << 16); b1 = __uint_as_float(yw[j] & 0xffff0000u);
        } else {
            a0 = f16_to_f32(f16_t{(uint16_t)(xw[j] & 0xffff)}); a1 = f16_to_f32(f16_t{(uint16_t)(xw[j] >> 16)});
            b0 = f16_to_f32(f16_t{(uint16_t)(yw[j] & 0xffff)}); b1 = f16_to_f32(f16_t{(uint16_t)(yw[j] >> 16)});
        }
        acc += a0 * b0 + a1 * b1;
    }
    for (int msk = 8; msk > 0; msk >>= 1) acc += __shfl_xor(acc, msk, 64);
    if (row < nrows && part == 0) delta[row] = acc;
}

// ------------------------------------------------------------------------------------------
// backward: dQ. Per 32-key sub-tile: S^T = K Q^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T
// ------------------------------------------------------------------------------------------
// CAP: P = exp2(t c - lse log2 e) from t = tanh(scale <q, k> / cap), c = cap log2(e), and dS carries the factor ds/dx = 1 - t^2; a row's
// p is still selected to 0 before any product.
template <bool BF, int MASK, int D, bool CAP = false>
__device__ __forceinline__ void q_tile(const char *buf, const char *doslab, const typename AFrag<BF>::type (&qf)[D / 16], const int (&ko)[D / 16],
                                       const int (&vo)[D / 32][2], f32x16 (&dq)[D / 32], float c, float k2, float lse2, float dlt, int64_t kv0, int64_t len,
                                       int hl, int lim = 0, int lo = 0) {
    using frag_t = typename AFrag<BF>::type;
    constexpr int DB = D / 32;
    const char *vt = buf + TILE;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
        for (int kg = 0; kg < D / 64; ++kg) {
#pragma unroll
            for (int kk = 4 * kg; kk < 4 * kg + 4; ++kk) s = a_mfma<BF>(*(const frag_t *)(buf + sub * 32 * AROW + ko[kk]), qf[kk], s);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int kg = 0; kg < D / 64; ++kg) {
#pragma unroll
            for (int kk = 4 * kg; kk < 4 * kg + 4; ++kk)
                dp = a_mfma<BF>(*(const frag_t *)(vt + sub * 32 * AROW + ko[kk]), *(const frag_t *)(doslab + ko[kk]), dp);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if constexpr (CAP) s[e] = cap_tanh(s[e], k2);
            const float dt = CAP ? __builtin_fmaf(-s[e], s[e], 1.f) : 1.f;
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[e], c, -lse2));
            if constexpr (MASK == 1) {
                if (kv0 + sub * 32 + a_row(e, hl) >= len) p = 0.f;
            } else if constexpr (MASK == 2) { // f_qk_sm's predicate
                if (sub * 32 + a_row(e, hl) >= lim) p = 0.f;
            } else if constexpr (MASK == 3) { // a row that sees no key has lse = -inf and p = +inf here: the select, before the product
                if (!win_in(sub * 32 + a_row(e, hl), lo, lim)) p = 0.f;
            }
            s[e] = CAP ? p * ((dp[e] - dlt) * dt) : p * (dp[e] - dlt);
        }
        TrN<DB> ta;
        if (sub == 0) tr4_issue<0>(buf, vo, ta); else tr4_issue<32 * AROW>(buf, vo, ta);
        tr4_wait1(ta);
        { const frag_t df = a_pack<BF>(s, 0);
#pragma unroll
          for (int d = 0; d < DB; ++d) dq[d] = a_mfma<BF>(tr4_frag<BF, DB>(ta, d), df, dq[d]); }
        __builtin_amdgcn_sched_barrier(0);
        if (sub == 0) tr4_issue<16 * AROW>(buf, vo, ta); else tr4_issue<48 * AROW>(buf, vo, ta);
        tr4_wait1(ta);
        { const frag_t df = a_pack<BF>(s, 1);
#pragma unroll
          for (int d = 0; d < DB; ++d) dq[d] = a_mfma<BF>(tr4_frag<BF, DB>(ta, d), df, dq[d]); }
        __builtin_amdgcn_sched_barrier(0);
    }
}

constexpr int QSLAB = 32 * AROW;              // one wave's dO rows (8 KiB)
constexpr int DQ_LDS = 2 * SLOT + 4 * QSLAB;  // two K | V slots + four dO slabs = 96 KiB

template <bool BF, int D, int MODE, bool CAP = false>
__global__ __launch_bounds__(NT) void attn_full_bwd_dq_kernel(const FullArgs a) {
    using frag_t = typename AFrag<BF>::type;
    constexpr bool CAUSAL = MODE == M_PREFIX, WIN = MODE == M_WINDOW, DOC = MODE == M_DOC;
    constexpr int KS = D / 16, DB = D / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, xl = lane & 31, hl = lane >> 5;
    const int64_t nxb = (a.Sq + TQ - 1) / TQ;
    const int64_t bh = blockIdx.x / nxb, xb = block_of<MODE>(blockIdx.x % nxb, bh, nxb), b = bh / a.H, h = bh % a.H, g = h / a.G;
    const int64_t len = key_len(a, b);
    const int64_t pre = CAUSAL ? prefix_of(a, b) : 0;
    const int nt = DOC ? doc_last_tile(a, b, len, xb) : (int)((key_bound<MODE>(a, len, pre, xb) + TK - 1) / TK);
    const int tf = DOC ? doc_first_tile(a, b, len, xb) : first_tile<MODE>(a, xb); // 0 but under a window or a document mask; there nt <= tf when no query of the block sees a key
    const char *Kg = a.k + b * a.lk.sb + g * a.lk.sh;
    const char *Vg = a.v + b * a.lv.sb + g * a.lv.sh;
    char *doslab = smem + 2 * SLOT + wid * QSLAB; // this wave's dO rows, same swizzled image as a K tile (B operand of dP^T)
    int ko[KS], vo[DB][2];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) ko[kk] = a_off(xl, kk * 2 + hl);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        vo[d][0] = a_tr_lane_off(d * 32, 0);
        vo[d][1] = a_tr_lane_off(d * 32, 1);
    }
    const float c = (CAP ? a.softcap : a.scale) * kLog2e, k2 = CAP ? cap_k2(a) : 0.f;
    const int64_t qw = xb * TQ + wid * 32, m = qw + xl;
    const bool active = qw < a.Sq;
    const DocRows dr = doc_rows<DOC>(a, b, len, qw, m, active);

    frag_t qf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[kk][j] = 0;
    float lse2 = 0.f, dlt = 0.f;
    if (m < a.Sq) {
        const char *Qg = a.q + b * a.lq.sb + h * a.lq.sh + m * a.lq.sr;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = *(const frag_t *)(Qg + (kk * 16 + 8 * hl) * 2);
        lse2 = a.lse_r[bh * a.Sq + m] * kLog2e;
        dlt = a.delta[bh * a.Sq + m];
    }
    if (active) {
        const char *dOw = a.d_o + b * a.ldo.sb + h * a.ldo.sh + qw * a.ldo.sr;
#pragma unroll
        for (int i = 0; i < D / 16; ++i) { // 32 rows x D / 8 pieces of 16 B; a row beyond Sq is zeros
            const int id = lane + 64 * i, row = id / (D / 8), ch = id % (D / 8);
            uint4 w = uint4{0, 0, 0, 0};
            if (qw + row < a.Sq) w = *(const uint4 *)(dOw + row * a.ldo.sr + ch * 16);
            *(uint4 *)(doslab + a_off(row, ch)) = w;
        }
    }
    f32x16 dq[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) dq[d][e] = 0.f;

    TileRegs<D> tr;
    if (nt > tf) {
        t_load<D>(tr, Kg + (int64_t)tf * TK * a.lk.sr, Vg + (int64_t)tf * TK * a.lv.sr, a.lk.sr, a.lv.sr, len - (int64_t)tf * TK);
        t_store<D>(tr, smem);
    }
    for (int t = tf; t < nt; ++t) {
        const int64_t kv0 = (int64_t)t * TK;
        if (t + 1 < nt) t_load<D>(tr, Kg + (kv0 + TK) * a.lk.sr, Vg + (kv0 + TK) * a.lv.sr, a.lk.sr, a.lv.sr, len - kv0 - TK);
        __syncthreads();
        const char *cur = smem + ((t - tf) & 1) * SLOT;
        if constexpr (CAUSAL) { // the forward's skip and body choice
            if (active && kv0 < (pre > qw + 32 ? pre : qw + 32)) {
                if (kv0 + TK > len || (kv0 + TK - 1 > qw && kv0 + TK - 1 >= pre)) {
                    q_tile<BF, 2, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl, tile_lim(len, pre, qw, kv0, xl));
                } else q_tile<BF, 0, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl);
            }
        } else if constexpr (WIN) { // the forward's skip and body choice; the unmasked body runs where every row sees all 64 keys, so
                                    // a row with lse = -inf never meets it
            if (active && kv0 + TK > qw - a.wl && kv0 <= qw + 31 + a.wr) {
                if (kv0 + TK > len || qw + 31 - a.wl > kv0 || qw + a.wr < kv0 + TK - 1) {
                    int lo, cnt;
                    win_lim(a, len, qw, kv0, xl, lo, cnt);
                    q_tile<BF, 3, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl, cnt, lo);
                } else q_tile<BF, 0, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl);
            }
        } else if constexpr (DOC) { // the forward's skip and body choice; a row with lse = -inf sees no key, so it never meets the unmasked body
            if (active && kv0 + TK > dr.lo_first && kv0 < dr.hi_last) {
                if (dr.lo_last > kv0 || dr.hi_first < kv0 + TK) {
                    int lo, cnt;
                    doc_lim(dr.lo, dr.hi, kv0, lo, cnt);
                    q_tile<BF, 3, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl, cnt, lo);
                } else q_tile<BF, 0, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl);
            }
        } else if (active) {
            if (kv0 + TK > len) q_tile<BF, 1, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl);
            else q_tile<BF, 0, D, CAP>(cur, doslab, qf, ko, vo, dq, c, k2, lse2, dlt, kv0, len, hl);
        }
        if (t + 1 < nt) t_store<D>(tr, smem + ((t + 1 - tf) & 1) * SLOT);
    }
    __syncthreads();
    if (active) {
        const int64_t left = a.Sq - qw;
        a_store_rows<BF, DB>(smem + wid * 32 * OPAD, a.dq + b * a.ldq.sb + h * a.ldq.sh + qw * a.ldq.sr, dq, a.scale, a.ldq.sr, left < 32 ? (int)left : 32);
    }
}

// ------------------------------------------------------------------------------------------
// backward: dK / dV, key on the lane. A wave owns 32 keys: their K and V rows are B fragments in registers for the whole kernel.
// Per 64-query tile (Q | dO in LDS, the K | V image and offsets of the forward):
//   S = Q K^T and dP = dO V^T   (A = Q / dO rows from LDS)        P = exp2(c S - lse log2 e),  dS = P o (dP - delta)
//   dV^T += dO^T P,  dK^T += Q^T dS   (A = dO^T / Q^T through transposed reads, B = P / dS packed from the accumulators)
// The row constants of the tile's 64 queries travel with it (two float[64] per slot). A query row beyond Sq has Q = dO = 0 and
// lse = +inf, so P = 0 there. MASK: this wave holds keys at or beyond len (their K / V fragments are zeros): P = 0 on those lanes.
// ------------------------------------------------------------------------------------------
constexpr int KV_SLOT = SLOT + 512;       // Q | dO | lse log2(e) [64] | delta [64]
constexpr int KV_LDS = 2 * KV_SLOT;

// MASK 2 (prefix-LM variant): P = 0 for the tile's queries r < cut - every one (64) when the lane's key is dead, those before the key
// when it lies beyond the prefix, none otherwise. MASK 3 (window variant): P = 0 for the tile's queries outside cut <= r < cut + hi, the
// queries n - wr .. n + wl that see the lane's key (none, hi = 0, when it is dead); a query that sees no key (lse = -inf, P = +inf) is
// outside it.
// CAP: as in q_tile - t = tanh(.) in place of the raw score, c = cap log2(e), and the factor 1 - t^2 on dS (not on the P of dV).
template <bool BF, int MASK, int D, bool CAP = false>
__device__ __forceinline__ void kv_tile(const char *buf, const typename AFrag<BF>::type (&kf)[D / 16], const typename AFrag<BF>::type (&vf)[D / 16],
                                        const int (&ko)[D / 16], const int (&vo)[D / 32][2], f32x16 (&dk)[D / 32], f32x16 (&dv)[D / 32], float c, float k2,
                                        bool dead, int hl, int cut = 0, int hi = 0) {
    using frag_t = typename AFrag<BF>::type;
    constexpr int DB = D / 32;
    const char *dot = buf + TILE;
    const float *rc = (const float *)(buf + SLOT);
    frag_t pf[4], df[4];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        f32x16 s, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
        for (int kg = 0; kg < D / 64; ++kg) {
#pragma unroll
            for (int kk = 4 * kg; kk < 4 * kg + 4; ++kk) s = a_mfma<BF>(*(const frag_t *)(buf + sub * 32 * AROW + ko[kk]), kf[kk], s);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int kg = 0; kg < D / 64; ++kg) {
#pragma unroll
            for (int kk = 4 * kg; kk < 4 * kg + 4; ++kk) dp = a_mfma<BF>(*(const frag_t *)(dot + sub * 32 * AROW + ko[kk]), vf[kk], dp);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { // registers 4 j .. 4 j + 3 <-> queries sub 32 + 8 j + 4 hl + 0..3
            const float4 l4 = *(const float4 *)(rc + sub * 32 + 8 * j + 4 * hl);
            const float4 d4 = *(const float4 *)(rc + 64 + sub * 32 + 8 * j + 4 * hl);
            const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = 4 * j + i;
                // f16: P travels as P 2^14 into the dV product (small weights would be subnormal f16 values), dS at its own scale
                if constexpr (CAP) s[e] = cap_tanh(s[e], k2);
                const float dt = CAP ? __builtin_fmaf(-s[e], s[e], 1.f) : 1.f;
                float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[e], c, (BF ? 0.f : kPShiftLog2) - lv[i]));
                if constexpr (MASK == 1) {
                    if (dead) p = 0.f;
                } else if constexpr (MASK == 2) {
                    if (sub * 32 + 8 * j + 4 * hl + i < cut) p = 0.f;
                } else if constexpr (MASK == 3) {
                    if (!win_in(sub * 32 + 8 * j + 4 * hl + i, cut, hi)) p = 0.f;
                }
                s[e] = p;
                if constexpr (CAP) dp[e] = BF ? p * ((dp[e] - dl[i]) * dt) : p * ((dp[e] - dl[i]) * (dt * (1.f / kPShiftF16)));
                else dp[e] = BF ? p * (dp[e] - dl[i]) : p * ((dp[e] - dl[i]) * (1.f / kPShiftF16));
            }
        }
        pf[2 * sub] = a_pack<BF>(s, 0);
        pf[2 * sub + 1] = a_pack<BF>(s, 1);
        df[2 * sub] = a_pack<BF>(dp, 0);
        df[2 * sub + 1] = a_pack<BF>(dp, 1);
    }
    f_pv<BF, DB>(dot, vo, pf, dv);
    f_pv<BF, DB>(buf, vo, df, dk);
}

template <bool BF, int D, int MODE, bool CAP = false>
__global__ __launch_bounds__(NT) void attn_full_bwd_dkv_kernel(const FullArgs a) {
    using frag_t = typename AFrag<BF>::type;
    constexpr bool CAUSAL = MODE == M_PREFIX, WIN = MODE == M_WINDOW, DOC = MODE == M_DOC;
    constexpr int KS = D / 16, DB = D / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, xl = lane & 31, hl = lane >> 5;
    const int64_t nkb = (a.Skv + TQ - 1) / TQ;
    const int64_t bg = blockIdx.x / nkb, kb = block_of<MODE>(blockIdx.x % nkb, bg, nkb), b = bg / a.Hkv, g = bg % a.Hkv;
    const int64_t len = key_len(a, b);
    const int64_t k0 = kb * TQ, kw = k0 + wid * 32, n = kw + xl;
    char *dKg = a.dk + b * a.ldk.sb + g * a.ldk.sh;
    char *dVg = a.dv + b * a.ldv.sb + g * a.ldv.sh;
    // prefix-LM variant: a key block beyond the prefix is seen by queries m >= k0 only, so its query tiles start at t0 = k0 / 64; with
    // no tile left (the block lies beyond Sq too) no query sees it
    const int nqt = (int)((a.Sq + TK - 1) / TK);
    const int64_t pre = CAUSAL ? prefix_of(a, b) : 0;
    // window variant: the keys k0 .. k0 + 127 are seen by the queries k0 - wr .. k0 + 127 + wl: query tiles t0 .. tl, none when tl < t0
    const int64_t wlo = k0 - a.wr, whi = k0 + TQ - 1 + a.wl; // (read under WIN only)
    const int64_t tl = (whi < a.Sq - 1 ? whi : a.Sq - 1) / TK;
    // document variant: the keys k0 .. min(k0 + 128, len) - 1 are seen by the queries from the first one of key k0 to the last one of the
    // last of them (both columns are nondecreasing): query tiles dlo / 64 .. (dhi - 1) / 64, none when the interval is empty
    int dlo = 0, dhi = 0;
    if constexpr (DOC) {
        if (k0 < len) {
            dlo = doc_qlo(a, b, k0);
            dhi = doc_qhi(a, b, (k0 + TQ < len ? k0 + TQ : len) - 1);
        }
    }
    const int64_t t0 = DOC ? dlo / TK : (WIN ? (wlo > 0 ? wlo / TK : 0) : (CAUSAL && k0 >= pre ? k0 / TK : 0));
    const int64_t nq = DOC ? (dhi > dlo ? (dhi - 1) / TK - t0 + 1 : 0) : (WIN ? tl - t0 + 1 : nqt - t0); // query tiles per head
    if (k0 >= len || ((CAUSAL || WIN || DOC) && nq <= 0)) { // (workgroup-uniform) a key block beyond the batch's length, or unseen: its dK and dV rows are zeros
        const int64_t rows = a.Skv - k0 < TQ ? a.Skv - k0 : TQ;
        for (int id = threadIdx.x; id < rows * (D / 8); id += NT) {
            const int row = id / (D / 8), ch = id % (D / 8);
            *(uint4 *)(dKg + (k0 + row) * a.ldk.sr + ch * 16) = uint4{0, 0, 0, 0};
            *(uint4 *)(dVg + (k0 + row) * a.ldv.sr + ch * 16) = uint4{0, 0, 0, 0};
        }
        return;
    }
    int ko[KS], vo[DB][2];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) ko[kk] = a_off(xl, kk * 2 + hl);
#pragma unroll
    for (int d = 0; d < DB; ++d) {
        vo[d][0] = a_tr_lane_off(d * 32, 0);
        vo[d][1] = a_tr_lane_off(d * 32, 1);
    }
    const float c = (CAP ? a.softcap : a.scale) * kLog2e, k2 = CAP ? cap_k2(a) : 0.f;
    const bool dead = n >= len;       // this lane's key does not exist
    const bool work = kw < len;        // wave-uniform: the wave has a visible key
    const bool ragged = kw + 32 > len; // wave-uniform: some lane's key is beyond len
    // document variant: the queries that see the lane's own key (none when it is dead) and, wave-uniform, those of the wave's first key
    // and of its last key below len
    int qlo = 0, qhi = 0, qlo_first = 0, qlo_last = 0, qhi_first = 0, qhi_last = 0;
    if constexpr (DOC) {
        if (!dead) {
            qlo = doc_qlo(a, b, n);
            qhi = doc_qhi(a, b, n);
        }
        if (work) {
            const int64_t last = (kw + 32 < len ? kw + 32 : len) - 1;
            qlo_first = __builtin_amdgcn_readfirstlane(doc_qlo(a, b, kw));
            qlo_last = __builtin_amdgcn_readfirstlane(doc_qlo(a, b, last));
            qhi_first = __builtin_amdgcn_readfirstlane(doc_qhi(a, b, kw));
            qhi_last = __builtin_amdgcn_readfirstlane(doc_qhi(a, b, last));
        }
    }

    frag_t kf[KS], vf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) { kf[kk][j] = 0; vf[kk][j] = 0; }
    if (!dead) { // K / V rows at n >= len are never read
        const char *Kr = a.k + b * a.lk.sb + g * a.lk.sh + n * a.lk.sr;
        const char *Vr = a.v + b * a.lv.sb + g * a.lv.sh + n * a.lv.sr;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            kf[kk] = *(const frag_t *)(Kr + (kk * 16 + 8 * hl) * 2);
            vf[kk] = *(const frag_t *)(Vr + (kk * 16 + 8 * hl) * 2);
        }
    }
    f32x16 dk[DB], dv[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) { dk[d][e] = 0.f; dv[d][e] = 0.f; }

    const int64_t nit = (int64_t)a.G * nq; // query heads g G .. g G + G - 1 in ascending order, each over its query tiles t0 .. nqt - 1
    TileRegs<D> tr;
    float rcv = 0.f;
    int64_t q0n = 0, q0 = t0 * TK; // first query of the tile just loaded / of the tile in LDS (read by the masked variants only)
    auto load = [&](int64_t it) {
        const int64_t hh = g * a.G + it / nq, q0 = (t0 + it % nq) * TK, bh = b * a.H + hh;
        q0n = q0;
        t_load<D>(tr, a.q + b * a.lq.sb + hh * a.lq.sh + q0 * a.lq.sr, a.d_o + b * a.ldo.sb + hh * a.ldo.sh + q0 * a.ldo.sr, a.lq.sr, a.ldo.sr, a.Sq - q0);
        if (threadIdx.x < 128) {
            const int64_t mq = q0 + (threadIdx.x & 63);
            if (threadIdx.x < 64) rcv = mq < a.Sq ? a.lse_r[bh * a.Sq + mq] * kLog2e : INFINITY;
            else rcv = mq < a.Sq ? a.delta[bh * a.Sq + mq] : 0.f;
        }
    };
    auto store = [&](char *slot) {
        t_store<D>(tr, slot);
        if (threadIdx.x < 128) ((float *)(slot + SLOT))[threadIdx.x] = rcv;
    };
    load(0);
    store(smem);
    for (int64_t it = 0; it < nit; ++it) {
        if (it + 1 < nit) load(it + 1);
        __syncthreads();
        const char *cur = smem + (it & 1) * KV_SLOT;
        if constexpr (CAUSAL) {
            if (work && !(kw >= pre && q0 + TK - 1 < kw)) { // (wave-uniform) skip: every key of the wave is causal and after the tile's last query
                if (ragged || (kw + 31 >= pre && kw + 31 > q0))
                    kv_tile<BF, 2, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl, dead ? TK : (n >= pre ? clamp_i(n - q0, 0, TK) : 0));
                else kv_tile<BF, 0, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl);
            }
        } else if constexpr (WIN) {
            // (wave-uniform) skip a tile none of the wave's keys kw .. kw + 31 is seen from; the masked body where a key is dead or the
            // tile is cut by the first query of the wave's last key (n - wr) or by the last query of its first key (n + wl)
            if (work && q0 + TK > kw - a.wr && q0 <= kw + 31 + a.wl) {
                if (ragged || kw + 31 - a.wr > q0 || kw + a.wl < q0 + TK - 1) {
                    const int lo = clamp_i(n - a.wr - q0, 0, TK), hi = clamp_i(n + a.wl + 1 - q0, 0, TK);
                    kv_tile<BF, 3, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl, lo, dead ? 0 : max(hi - lo, 0));
                } else kv_tile<BF, 0, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl);
            }
        } else if constexpr (DOC) {
            // (wave-uniform) the window variant's skip and body choice with the table's intervals: skip a tile none of the wave's keys is
            // seen from; the unmasked body only where every key of the wave exists and is seen by all 64 queries (whose lse is finite then)
            if (work && q0 + TK > qlo_first && q0 < qhi_last) {
                if (ragged || qlo_last > q0 || qhi_first < q0 + TK) {
                    int lo, cnt;
                    doc_lim(qlo, qhi, q0, lo, cnt);
                    kv_tile<BF, 3, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl, lo, cnt);
                } else kv_tile<BF, 0, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl);
            }
        } else if (work) {
            if (ragged) kv_tile<BF, 1, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl);
            else kv_tile<BF, 0, D, CAP>(cur, kf, vf, ko, vo, dk, dv, c, k2, dead, hl);
        }
        if (it + 1 < nit) store(smem + ((it + 1) & 1) * KV_SLOT);
        q0 = q0n;
    }
    __syncthreads();
    if (kw < a.Skv) { // a wave without a visible key stores its zeros: rows n >= len of dK and dV are zeros
        const int64_t left = a.Skv - kw;
        const int nrows = left < 32 ? (int)left : 32;
        a_store_rows<BF, DB>(smem + wid * 32 * OPAD, dKg + kw * a.ldk.sr, dk, a.scale, a.ldk.sr, nrows);
        a_store_rows<BF, DB>(smem + wid * 32 * OPAD, dVg + kw * a.ldv.sr, dv, BF ? 1.f : 1.f / kPShiftF16, a.ldv.sr, nrows);
    }
}

// ==========================================================================================
// generic path: contiguous tensors, one workgroup of 256 threads per output row, 256 partners per step
// ==========================================================================================
template <bool MAX>
__device__ __forceinline__ float g_block_reduce(float v, float *red) { // every thread gets the result; red: 4 floats, reusable after return
    for (int msk = 32; msk > 0; msk >>= 1) {
        const float w = __shfl_xor(v, msk, 64);
        v = MAX ? fmaxf(v, w) : v + w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// CAUSAL (prefix-LM variant): query m sees the keys n < min(len, max(pre, m + 1)) - a plain bound in the forward and dQ, a predicate
// on the query in dK/dV
// WIN (window variant): the keys max(0, m - wl) <= n < min(len, m + wr + 1) - a first key besides the bound in the forward and dQ (an
// empty interval leaves o = 0, lse = -inf and dq = 0), the predicate n - wr <= m <= n + wl in dK/dV
// DOC (document variant): the same with the interval read from the table - doc_lo .. doc_hi of the query, doc_qlo .. doc_qhi of the key
template <int MODE>
__device__ __forceinline__ int64_t g_key_bound(const FullArgs &a, int64_t b, int64_t m) {
    const int64_t len = key_len(a, b);
    if constexpr (MODE == M_FULL) return len;
    if constexpr (MODE == M_WINDOW) return len < m + a.wr + 1 ? len : m + a.wr + 1;
    if constexpr (MODE == M_DOC) return doc_hi(a, b, m, len);
    const int64_t pre = prefix_of(a, b), vis = pre > m + 1 ? pre : m + 1;
    return len < vis ? len : vis;
}
template <int MODE>
__device__ __forceinline__ int64_t g_key_first(const FullArgs &a, int64_t b, int64_t m) {
    if constexpr (MODE == M_DOC) return doc_lo(a, b, m, key_len(a, b));
    if constexpr (MODE != M_WINDOW) return 0;
    return m > a.wl ? m - a.wl : 0;
}

// X, CAP (kf_attn_ext_*): the modifiers of the matrix-core kernels - s = cap tanh(scale <q, k> / cap) where a score is formed, the factor
// 1 - t^2 on dS, the sink folded into the forward's last step against max(mrun, sink)
__device__ __forceinline__ float g_cap(float dot, const FullArgs &a) { return a.softcap * cap_tanh(dot, cap_k2(a)); }

template <typename T, int MODE, int X = X_NONE>
__global__ __launch_bounds__(NT) void attn_full_fwd_generic_kernel(const FullArgs a) {
    __shared__ float qs[256], ps[256], red[4];
    const int tid = threadIdx.x, D = (int)a.D;
    const int64_t bh = blockIdx.x / a.Sq, m = blockIdx.x % a.Sq, b = bh / a.H, h = bh % a.H, g = h / a.G;
    const int64_t len = g_key_bound<MODE>(a, b, m);
    const T *Q = (const T *)a.q + (bh * a.Sq + m) * D;
    const T *K = (const T *)a.k + (b * a.Hkv + g) * a.Skv * D;
    const T *V = (const T *)a.v + (b * a.Hkv + g) * a.Skv * D;
    if (tid < D) qs[tid] = load_f32(Q + tid);
    __syncthreads();
    float acc = 0.f, mrun = -INFINITY, lrun = 0.f;
    for (int64_t c0 = g_key_first<MODE>(a, b, m); c0 < len; c0 += NT) {
        const int64_t n = c0 + tid;
        float s = -INFINITY;
        if (n < len) {
            float dot = 0.f;
            for (int d = 0; d < D; ++d) dot += qs[d] * load_f32(K + n * D + d);
            s = X == X_CAP ? g_cap(dot, a) : dot * a.scale;
        }
        const float mnew = fmaxf(mrun, g_block_reduce<true>(s, red)); // finite: key c0 exists
        const float alpha = expf(mrun - mnew), p = n < len ? expf(s - mnew) : 0.f;
        ps[tid] = p;
        lrun = lrun * alpha + g_block_reduce<false>(p, red); // (its barriers publish ps)
        if (tid < D) {
            const int cnt = (int)(len - c0 < NT ? len - c0 : NT);
            float t = 0.f;
            for (int j = 0; j < cnt; ++j) t += ps[j] * load_f32(V + (c0 + j) * D + tid);
            acc = acc * alpha + t;
        }
        mrun = mnew;
        __syncthreads();
    }
    if constexpr (X != X_NONE) {
        if (a.sink) { // (workgroup-uniform) fold_sink in natural units; a row without a key keeps acc = 0 and gets lse = sink
            const float sk = a.sink[h];
            if (sk > mrun) {
                const float w = lrun > 0.f ? expf(mrun - sk) : 0.f;
                acc *= w;
                lrun = lrun * w + 1.f;
                mrun = sk;
            } else if (lrun > 0.f) lrun += expf(sk - mrun);
        }
    }
    if (tid < D) store_canonical((T *)a.out + (bh * a.Sq + m) * D + tid, lrun > 0.f ? acc / lrun : 0.f);
    if (tid == 0 && a.lse) a.lse[bh * a.Sq + m] = lrun > 0.f ? mrun + logf(lrun) : -INFINITY;
}

template <typename T>
__global__ __launch_bounds__(NT) void attn_full_delta_generic_kernel(const T *o, const T *d_o, float *delta, int64_t nrows, int D) {
    const int64_t row = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (row >= nrows) return;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc += load_f32(o + row * D + d) * load_f32(d_o + row * D + d);
    delta[row] = acc;
}

template <typename T, int MODE, bool CAP = false>
__global__ __launch_bounds__(NT) void attn_full_bwd_dq_generic_kernel(const FullArgs a) {
    __shared__ float qs[256], dos[256], dss[256];
    const int tid = threadIdx.x, D = (int)a.D;
    const int64_t bh = blockIdx.x / a.Sq, m = blockIdx.x % a.Sq, b = bh / a.H, h = bh % a.H, g = h / a.G;
    const int64_t len = g_key_bound<MODE>(a, b, m);
    const T *K = (const T *)a.k + (b * a.Hkv + g) * a.Skv * D;
    const T *V = (const T *)a.v + (b * a.Hkv + g) * a.Skv * D;
    if (tid < D) {
        qs[tid] = load_f32((const T *)a.q + (bh * a.Sq + m) * D + tid);
        dos[tid] = load_f32((const T *)a.d_o + (bh * a.Sq + m) * D + tid);
    }
    const float lse = a.lse_r[bh * a.Sq + m], dlt = a.delta[bh * a.Sq + m];
    __syncthreads();
    float acc = 0.f;
    for (int64_t c0 = g_key_first<MODE>(a, b, m); c0 < len; c0 += NT) {
        const int64_t n = c0 + tid;
        float ds = 0.f;
        if (n < len) {
            float dot = 0.f, dp = 0.f;
            for (int d = 0; d < D; ++d) {
                dot += qs[d] * load_f32(K + n * D + d);
                dp += dos[d] * load_f32(V + n * D + d);
            }
            if constexpr (CAP) {
                const float s = g_cap(dot, a), t = s / a.softcap;
                ds = expf(s - lse) * ((dp - dlt) * (1.f - t * t));
            } else ds = expf(dot * a.scale - lse) * (dp - dlt);
        }
        dss[tid] = ds;
        __syncthreads();
        if (tid < D) {
            const int cnt = (int)(len - c0 < NT ? len - c0 : NT);
            for (int j = 0; j < cnt; ++j) acc += dss[j] * load_f32(K + (c0 + j) * D + tid);
        }
        __syncthreads();
    }
    if (tid < D) store_canonical((T *)a.dq + (bh * a.Sq + m) * D + tid, acc * a.scale);
}

template <typename T, int MODE, bool CAP = false>
__global__ __launch_bounds__(NT) void attn_full_bwd_dkv_generic_kernel(const FullArgs a) {
    __shared__ float ks[256], vs[256], ps[256], dss[256];
    const int tid = threadIdx.x, D = (int)a.D;
    const int64_t bg = blockIdx.x / a.Skv, n = blockIdx.x % a.Skv, b = bg / a.Hkv, g = bg % a.Hkv;
    const int64_t len = key_len(a, b);
    T *dK = (T *)a.dk + (bg * a.Skv + n) * D, *dV = (T *)a.dv + (bg * a.Skv + n) * D;
    if (n >= len) { // (workgroup-uniform)
        if (tid < D) { store_canonical(dK + tid, 0.f); store_canonical(dV + tid, 0.f); }
        return;
    }
    if (tid < D) {
        ks[tid] = load_f32((const T *)a.k + (bg * a.Skv + n) * D + tid);
        vs[tid] = load_f32((const T *)a.v + (bg * a.Skv + n) * D + tid);
    }
    __syncthreads();
    constexpr bool CAUSAL = MODE == M_PREFIX, WIN = MODE == M_WINDOW, DOC = MODE == M_DOC;
    const bool in_prefix = !CAUSAL || n < prefix_of(a, b); // else only queries m >= n see this key
    int64_t dlo = 0, dhi = 0; // document variant: the queries dlo <= m < dhi see this key
    if constexpr (DOC) {
        dlo = doc_qlo(a, b, n);
        dhi = doc_qhi(a, b, n);
    }
    float ak = 0.f, av = 0.f;
    for (int hh = 0; hh < a.G; ++hh) {
        const int64_t bh = b * a.H + g * a.G + hh;
        const T *Q = (const T *)a.q + bh * a.Sq * D, *dO = (const T *)a.d_o + bh * a.Sq * D;
        for (int64_t c0 = 0; c0 < a.Sq; c0 += NT) {
            const int64_t m = c0 + tid;
            float p = 0.f, ds = 0.f;
            if (m < a.Sq && (in_prefix || m >= n) && (!WIN || (m >= n - a.wr && m <= n + a.wl)) && (!DOC || (m >= dlo && m < dhi))) {
                float dot = 0.f, dp = 0.f;
                for (int d = 0; d < D; ++d) {
                    dot += ks[d] * load_f32(Q + m * D + d);
                    dp += vs[d] * load_f32(dO + m * D + d);
                }
                if constexpr (CAP) {
                    const float s = g_cap(dot, a), t = s / a.softcap;
                    p = expf(s - a.lse_r[bh * a.Sq + m]);
                    ds = p * ((dp - a.delta[bh * a.Sq + m]) * (1.f - t * t));
                } else {
                    p = expf(dot * a.scale - a.lse_r[bh * a.Sq + m]);
                    ds = p * (dp - a.delta[bh * a.Sq + m]);
                }
            }
            ps[tid] = p;
            dss[tid] = ds;
            __syncthreads();
            if (tid < D) {
                const int cnt = (int)(a.Sq - c0 < NT ? a.Sq - c0 : NT);
                for (int j = 0; j < cnt; ++j) {
                    av += ps[j] * load_f32(dO + (c0 + j) * D + tid);
                    ak += dss[j] * load_f32(Q + (c0 + j) * D + tid);
                }
            }
            __syncthreads();
        }
    }
    if (tid < D) { store_canonical(dK + tid, ak * a.scale); store_canonical(dV + tid, av); }
}

// ==========================================================================================
// document table (kf_attn_doc_table): one thread per token, a binary search over its row's cumulative lengths
// ==========================================================================================
// c_j = clamp(cu[b, j], 0, S), c_0 = 0 whatever it holds; token m < c_n belongs to the LAST document j with c_j <= m (a zero-length
// document owns nothing). The search keeps c_lo <= m < c_hi, so whatever the row holds the pair written has 0 <= start <= end <= S.
static __global__ __launch_bounds__(NT) void attn_doc_table_kernel(const int64_t *cu, int64_t B, int64_t S, int64_t n_docs, int64_t *kv_len, int32_t *doc_start,
                                                            int32_t *doc_end) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= B * S) return;
    const int64_t b = idx / S, m = idx - b * S;
    const int64_t *row = cu + b * (n_docs + 1);
    auto c = [&](int64_t j) -> int64_t {
        if (j == 0) return 0;
        const int64_t x = row[j];
        return x < 0 ? 0 : (x > S ? S : x);
    };
    const int64_t len = c(n_docs);
    if (m == 0) kv_len[b] = len;
    int64_t s = len, e = len;
    if (m < len) {
        int64_t lo = 0, hi = n_docs;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (c(mid) <= m) lo = mid;
            else hi = mid;
        }
        s = c(lo);
        e = c(hi);
    }
    doc_start[idx] = (int32_t)s;
    doc_end[idx] = (int32_t)e;
}

// ==========================================================================================
// span table (kf_attn_span_table): the document mask with a causal rule, per-document prefixes and a window baked into the intervals
// ==========================================================================================
// The search and the clamps of attn_doc_table_kernel; token m of document j = [cs, ce) with P = cs + clamp(prefix[b, j], 0, ce - cs)
// (P = cs without prefixes) gets the keys it sees as a query and the queries that see it as a key, each one interval (DESIGN.md section
// 4.9.6). wl and wr arrive as -1 or clamped to [0, S] (the host), so m - wl and m + wr + 1 stay far inside 64 bits; every value written
// lies in [cs, ce], hence in [0, S], with lo <= hi.
static __global__ __launch_bounds__(NT) void attn_span_table_kernel(const int64_t *cu, const int64_t *prefix, int64_t B, int64_t S, int64_t n_docs, int causal,
                                                             int64_t wl, int64_t wr, int64_t *kv_len, int32_t *key_lo, int32_t *key_hi, int32_t *query_lo,
                                                             int32_t *query_hi) {
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (idx >= B * S) return;
    const int64_t b = idx / S, m = idx - b * S;
    const int64_t *row = cu + b * (n_docs + 1);
    auto c = [&](int64_t j) -> int64_t {
        if (j == 0) return 0;
        const int64_t x = row[j];
        return x < 0 ? 0 : (x > S ? S : x);
    };
    auto lower = [](int64_t x, int64_t y) { return x < y ? x : y; };
    auto upper = [](int64_t x, int64_t y) { return x > y ? x : y; };
    const int64_t len = c(n_docs);
    if (m == 0) kv_len[b] = len;
    int64_t klo = len, khi = len, qlo = len, qhi = len;
    if (m < len) {
        int64_t lo = 0, hi = n_docs;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (c(mid) <= m) lo = mid;
            else hi = mid;
        }
        const int64_t cs = c(lo), ce = c(hi);
        int64_t P = cs;
        if (prefix) {
            const int64_t x = prefix[b * n_docs + lo];
            P = cs + (x < 0 ? 0 : lower(x, ce - cs));
        }
        klo = wl < 0 ? cs : upper(cs, m - wl);
        khi = causal ? lower(ce, upper(m + 1, P)) : ce;
        if (wr >= 0) khi = lower(khi, m + wr + 1);
        qlo = causal && m >= P ? upper(cs, m) : cs;
        if (wr >= 0) qlo = upper(qlo, m - wr);
        qhi = wl < 0 ? ce : lower(ce, m + wl + 1);
        khi = upper(khi, klo);
        qhi = upper(qhi, qlo);
    }
    key_lo[idx] = (int32_t)klo;
    key_hi[idx] = (int32_t)khi;
    query_lo[idx] = (int32_t)qlo;
    query_hi[idx] = (int32_t)qhi;
}

// ==========================================================================================
// sink gradient (kf_attn_ext_bwd): dsink[h] = - sum_{b, m < Sq} exp(sink[h] - lse[b,h,m]) delta[b,h,m]
// ==========================================================================================
// One workgroup per query head. Thread t adds the terms i = t, t + 256, ... of the head's B Sq rows (b-major) in ascending order, then
// the 256 partial sums meet in a fixed tree (g_block_reduce): no atomics, the same bits every run. lse >= sink wherever a sink is, so
// every weight is <= 1; a row with lse = -inf can only belong to sink = -inf, and its weight is 0, not exp(-inf + inf).
static __global__ __launch_bounds__(NT) void attn_sink_grad_kernel(const float *sink, const float *lse, const float *delta, float *dsink, int64_t B, int64_t H, int64_t Sq) {
    __shared__ float red[4];
    const int64_t h = blockIdx.x, n = B * Sq;
    const float sk = sink[h];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += NT) {
        const int64_t b = i / Sq, m = i - b * Sq, at = (b * H + h) * Sq + m;
        const float l = lse[at];
        acc += l == -INFINITY ? 0.f : expf(sk - l) * delta[at];
    }
    acc = g_block_reduce<false>(acc, red);
    if (threadIdx.x == 0) dsink[h] = -acc;
}

// ==========================================================================================
// host
// ==========================================================================================
static inline size_t a_align(size_t v) { return (v + 255) / 256 * 256; }
static size_t ws_bytes(int64_t B, int64_t Hq, int64_t Sq) { return a_align((size_t)B * Hq * Sq * sizeof(float)); } // delta [B, Hq, Sq]

static Lay lay_contig(int64_t H, int64_t S, int64_t D, int es) { return {H * S * D * es, S * D * es, D * es}; }
static bool lay_from(const kf_attn_layout *l, int es, Lay &out) {
    if (!l || l->batch < 0 || l->head < 0 || l->row < 0) return false;
    out = {l->batch * es, l->head * es, l->row * es};
    return l->batch % 8 == 0 && l->head % 8 == 0 && l->row % 8 == 0;
}

enum Plan { PLAN_NONE, PLAN_MFMA, PLAN_GENERIC };

// A call as the C entries take it, in four bundles. The operands are in the order of the prototypes, each pointer beside its layout
// (NULL: contiguous), so an entry fills them by name and reads like the prototype it implements.
struct Problem {
    int dtype;
    int64_t B, Hq, Hkv, Sq, Skv, D;
    float scale;
};
struct FwdOps {
    const void *q; const kf_attn_layout *lq;
    const void *k; const kf_attn_layout *lk;
    const void *v; const kf_attn_layout *lv;
    void *o; const kf_attn_layout *lo;
    float *lse; // written; may be null
};
struct BwdOps {
    const void *q; const kf_attn_layout *lq;
    const void *k; const kf_attn_layout *lk;
    const void *v; const kf_attn_layout *lv;
    const void *o; const kf_attn_layout *lo;
    const float *lse;
    const void *d_o; const kf_attn_layout *ldo;
    void *dq; const kf_attn_layout *ldq;
    void *dk; const kf_attn_layout *ldk;
    void *dv; const kf_attn_layout *ldv;
    void *workspace; size_t workspace_bytes;
};
struct Mods { // the score modifiers of kf_attn_ext_*; the entries of attn_full.hip have none
    float softcap;     // 0: off
    const float *sink; // [Hq] on the device, or null
};

// Everything about the problem and its operands that can be refused, in one place and before any device call. `ops`: the operand
// pointers in the order of `lay` (forward: q k v o; backward: + dO dQ dK dV). plan == PLAN_NONE with KF_OK: nothing to do (B, Hq or Sq is 0).
static int full_check(const char *who, const Problem &pr, const void *const *ops, const kf_attn_layout *const *lay, int nlay, FullArgs &a, Plan &plan) {
    const int dtype = pr.dtype;
    const int64_t B = pr.B, Hq = pr.Hq, Hkv = pr.Hkv, Sq = pr.Sq, Skv = pr.Skv, D = pr.D;
    const float scale = pr.scale;
    plan = PLAN_NONE;
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d is not f32, bf16 or f16", who, dtype);
    KF_REQUIRE(B >= 0 && Hq >= 0 && Sq >= 0 && Skv >= 0, KF_ERR_INVALID, "%s: negative extent", who);
    KF_REQUIRE(D >= 1 && D <= 256, KF_ERR_INVALID, "%s: head size %lld outside [1, 256]", who, (long long)D);
    KF_REQUIRE(Skv >= 1, KF_ERR_INVALID, "%s: Skv must be positive", who);
    KF_REQUIRE(scale > 0.f && scale < INFINITY, KF_ERR_INVALID, "%s: the softmax scale must be positive and finite", who);
    if (Hq == 0) return KF_OK;
    KF_REQUIRE(Hkv >= 1 && Hkv <= Hq && Hq % Hkv == 0, KF_ERR_INVALID, "%s: Hkv %lld must divide Hq %lld (1 <= Hkv <= Hq)", who, (long long)Hkv,
               (long long)Hq);
    int given = 0;
    for (int i = 0; i < nlay; ++i) given += lay[i] != nullptr;
    KF_REQUIRE(given == 0 || given == nlay, KF_ERR_INVALID, "%s: the layouts are all NULL (contiguous tensors) or all given, not %d of %d", who, given, nlay);
    const bool strided = nlay > 0 && given == nlay;
    Lay L[8];
    const int es = dtype_size(dtype);
    uintptr_t bits = 0;
    for (int i = 0; i < nlay; ++i) {
        const bool key_rows = i == 1 || i == 2 || i >= 6; // k, v, dK, dV: Hkv heads of Skv rows
        if (strided) KF_REQUIRE(lay_from(lay[i], es, L[i]), KF_ERR_INVALID, "%s: strides must be non-negative multiples of 8 elements", who);
        else L[i] = lay_contig(key_rows ? Hkv : Hq, key_rows ? Skv : Sq, D, es);
    }
    if (B == 0 || Sq == 0) return KF_OK;
    for (int i = 0; i < nlay; ++i) {
        KF_REQUIRE(ops[i], KF_ERR_INVALID, "%s: null operand", who);
        bits |= (uintptr_t)ops[i];
    }
    const bool mfma_shape = (dtype == KF_BF16 || dtype == KF_F16) && (D == 64 || D == 128);
    if (strided) {
        KF_REQUIRE(bits % 16 == 0, KF_ERR_INVALID, "%s: strided operands must be 16-byte aligned", who);
        KF_REQUIRE(mfma_shape, KF_ERR_UNSUPPORTED, "%s: strided layouts are served by the 16-bit matrix-core kernels only (D = 64 or 128)", who);
    }
    KF_REQUIRE(bits % es == 0, KF_ERR_INVALID, "%s: an operand is not aligned to its element", who);
    plan = mfma_shape && bits % 16 == 0 ? PLAN_MFMA : PLAN_GENERIC;
    const int64_t blocks = plan == PLAN_MFMA ? (B * Hq * Sq + 15) / 16 /* the delta kernel: 16 rows per workgroup */ : B * Hq * Sq, kblocks = plan == PLAN_MFMA ? B * Hkv * ((Skv + TQ - 1) / TQ) : B * Hkv * Skv;
    KF_REQUIRE(B * Hq <= (1ll << 24) && Sq <= (1ll << 31) && Skv <= (1ll << 31) && blocks < (1ll << 31) && kblocks < (1ll << 31), KF_ERR_UNSUPPORTED,
               "%s: the problem needs more than 2^31 workgroups", who);
    memset(&a, 0, sizeof(a));
    a.B = B; a.H = Hq; a.Hkv = Hkv; a.Sq = Sq; a.Skv = Skv; a.D = D;
    a.G = (int)(Hq / Hkv);
    a.scale = scale;
    Lay *const out[8] = {&a.lq, &a.lk, &a.lv, &a.lo, &a.ldo, &a.ldq, &a.ldk, &a.ldv};
    for (int i = 0; i < nlay; ++i) *out[i] = L[i];
    return KF_OK;
}

} // namespace full
} // namespace kf

using namespace kf;
using namespace kf::full;

// The four families and kf_attn_ext_* share their host path. A mask is the ABI's kf_attn_mask from the C entry on - a per-family entry
// builds one from its own arguments - and mask_check turns it into a MaskPlan: the `mode` that selects the instantiations and labels
// (M_PREFIX the prefix-LM ones, M_WINDOW the window ones, M_DOC the document ones; with M_FULL the launches are kf_attn_full_*'s own)
// and what the kernels of that mode read.
template <typename F> static inline int with_mode(Mode mode, F &&f) {
    return mode == M_FULL ? f(std::integral_constant<int, M_FULL>{})
                          : mode == M_PREFIX ? f(std::integral_constant<int, M_PREFIX>{})
                                             : mode == M_WINDOW ? f(std::integral_constant<int, M_WINDOW>{}) : f(std::integral_constant<int, M_DOC>{});
}
struct Window { int64_t left, right; };
// The document variant's tables ([B, S] on the device) and its causal flag. A partition is symmetric, so kf_attn_doc_* hands over one
// pair that the dK/dV kernels read at the key index too (keyed = false, qstart and qend null). kf_attn_span_* bakes a causal rule, a
// prefix and a window into the intervals, which are then no longer symmetric: keyed = true, and the dK/dV launches take (qstart, qend),
// the queries that see each key, in place of (start, end), the keys each query sees.
struct DocTables { const int32_t *start, *end; int causal; const int32_t *qstart, *qend; bool keyed; };
struct MaskPlan {
    Mode mode;
    const int64_t *kv_len, *prefix_len; // [B] on the device, or null; prefix_len of KF_ATTN_MASK_PREFIX only
    Window win;                         // of KF_ATTN_MASK_WINDOW, else (-1, -1)
    DocTables doc;                      // of KF_ATTN_MASK_DOC, else nulls and 0
};

// The two windows an older family already is take its kernels, so their results have its bits: (-1, -1) is full attention, (-1, 0)
// padded-causal (kf_attn_prefix_* without a prefix). The refusals still carry the calling entry's name.
static Mode window_mode(int64_t wl, int64_t wr) { return wl < 0 && wr < 0 ? M_FULL : (wl < 0 && wr == 0 ? M_PREFIX : M_WINDOW); }

// The one validation of a mask: its kind and the fields that belong to it. A field of another kind must hold its neutral value (NULL,
// -1, 0); the per-family entries have no such argument at all, and the masks they build hold those values.
static int mask_check(const char *who, const kf_attn_mask *m, int64_t Sq, int64_t Skv, MaskPlan &p) {
    KF_REQUIRE(m, KF_ERR_INVALID, "%s: null mask", who);
    KF_REQUIRE(m->kind >= KF_ATTN_MASK_FULL && m->kind <= KF_ATTN_MASK_DOC, KF_ERR_INVALID, "%s: unknown mask kind %d", who, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_PREFIX || !m->prefix_len, KF_ERR_INVALID, "%s: prefix_len belongs to KF_ATTN_MASK_PREFIX, the kind is %d", who, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_WINDOW || (m->window_left == -1 && m->window_right == -1), KF_ERR_INVALID,
               "%s: a window (%lld, %lld) belongs to KF_ATTN_MASK_WINDOW, the kind is %d (other kinds: -1, -1)", who, (long long)m->window_left,
               (long long)m->window_right, m->kind);
    KF_REQUIRE(m->kind == KF_ATTN_MASK_DOC || (!m->doc_start && !m->doc_end && m->causal == 0), KF_ERR_INVALID,
               "%s: doc_start, doc_end and causal belong to KF_ATTN_MASK_DOC, the kind is %d", who, m->kind);
    p = MaskPlan{(Mode)m->kind, m->kv_len, m->prefix_len, Window{-1, -1}, DocTables{nullptr, nullptr, 0, nullptr, nullptr, false}};
    if (m->kind == KF_ATTN_MASK_WINDOW) {
        KF_REQUIRE(m->window_left >= -1 && m->window_right >= -1, KF_ERR_INVALID, "%s: a window side is a key count >= 0 or -1 (unbounded), not (%lld, %lld)", who,
                   (long long)m->window_left, (long long)m->window_right);
        p.win = Window{m->window_left, m->window_right};
        p.mode = window_mode(m->window_left, m->window_right);
    } else if (m->kind == KF_ATTN_MASK_DOC) {
        KF_REQUIRE(m->causal == 0 || m->causal == 1, KF_ERR_INVALID, "%s: causal is 0 or 1, not %d", who, m->causal);
        KF_REQUIRE(Sq == Skv, KF_ERR_INVALID, "%s: a document mask is self-attention, Sq %lld must equal Skv %lld", who, (long long)Sq, (long long)Skv);
        p.doc = DocTables{m->doc_start, m->doc_end, m->causal, nullptr, nullptr, false};
    }
    return KF_OK;
}

// The plan as the kernels carry it; fields of another mode stay zero. An unbounded window side, or one wider than any extent, is
// kNoEdge. The document tables are required once there is something to launch (as the operands are), and 32-bit, so S stays below 2^31.
static int set_mask(const char *who, FullArgs &a, const MaskPlan &p) {
    a.kv_len = p.kv_len;
    a.prefix_len = p.prefix_len;
    if (p.mode == M_WINDOW) {
        a.wl = p.win.left < 0 || p.win.left > kNoEdge ? kNoEdge : p.win.left;
        a.wr = p.win.right < 0 || p.win.right > kNoEdge ? kNoEdge : p.win.right;
    }
    if (p.mode != M_DOC) return KF_OK;
    KF_REQUIRE(p.doc.start && p.doc.end, KF_ERR_INVALID, "%s: null %s writes them)", who,
               p.doc.keyed ? "key_lo or key_hi (kf_attn_span_table" : "doc_start or doc_end (kf_attn_doc_table");
    KF_REQUIRE(a.Sq < (1ll << 31), KF_ERR_UNSUPPORTED, "%s: the document tables are 32-bit, S must be below 2^31", who);
    a.doc_start = p.doc.start;
    a.doc_end = p.doc.end;
    a.causal = p.doc.causal;
    return KF_OK;
}

// The profile labels of one family, without (cap = "") or with (cap = "_cap") the soft-cap: string literals, KF_PROF keeps the pointer.
struct Labels { const char *fwd[2], *dq[2], *dkv[2], *generic[3]; }; // [d64]; generic: fwd, dQ, dK/dV
#define KF_ATTN_LABELS(family, cap)                                                                                      \
    {{"attn_" family cap "_fwd_mfma_d128", "attn_" family cap "_fwd_mfma_d64"},                                          \
     {"attn_" family cap "_bwd_dq_mfma_d128", "attn_" family cap "_bwd_dq_mfma_d64"},                                    \
     {"attn_" family cap "_bwd_dkv_mfma_d128", "attn_" family cap "_bwd_dkv_mfma_d64"},                                  \
     {"attn_" family cap "_fwd_generic", "attn_" family cap "_bwd_dq_generic", "attn_" family cap "_bwd_dkv_generic"}}
static const Labels kLabels[2][4] = { // [with the soft-cap: kf_attn_ext_* with softcap > 0][mode]
    {KF_ATTN_LABELS("full", ""), KF_ATTN_LABELS("prefix", ""), KF_ATTN_LABELS("window", ""), KF_ATTN_LABELS("doc", "")},
    {KF_ATTN_LABELS("full", "_cap"), KF_ATTN_LABELS("prefix", "_cap"), KF_ATTN_LABELS("window", "_cap"), KF_ATTN_LABELS("doc", "_cap")}};
#undef KF_ATTN_LABELS

// X, CAP: the modifiers of kf_attn_ext_* (attn_ext.hip), which instantiates the modified kernels; attn_full.hip instantiates the others
// (plain_fwd, plain_bwd). X_SINK keeps the labels of the kernels without modifiers, X_CAP and CAP take the _cap_ ones.
template <int X> static int full_fwd(const char *who, const Problem &pr, const MaskPlan &p, Mods mod, const FwdOps &x, void *stream) {
    const void *ops[4] = {x.q, x.k, x.v, x.o};
    const kf_attn_layout *lay[4] = {x.lq, x.lk, x.lv, x.lo};
    FullArgs a;
    Plan plan;
    int rc = full_check(who, pr, ops, lay, 4, a, plan);
    if (rc != KF_OK || plan == PLAN_NONE) return rc;
    a.q = (const char *)x.q; a.k = (const char *)x.k; a.v = (const char *)x.v; a.out = (char *)x.o; a.lse = x.lse;
    rc = set_mask(who, a, p);
    if (rc != KF_OK) return rc;
    a.softcap = mod.softcap;
    a.sink = mod.sink;
    hipStream_t st = as_stream(stream);
    const Mode mode = p.mode;
    const Labels &label = kLabels[X == X_CAP][mode];
    const int64_t B = pr.B, Hq = pr.Hq, Sq = pr.Sq;
    const bool bf = pr.dtype == KF_BF16, d64 = pr.D == 64;
    if (plan == PLAN_MFMA) {
        const unsigned grid = (unsigned)(B * Hq * ((Sq + TQ - 1) / TQ));
        KF_PROF(label.fwd[d64], st);
        return with_mode(mode, [&](auto M) {
            return with_flags([&](auto BF, auto D64) { return launch(attn_full_fwd_kernel<BF, D64 ? 64 : 128, M, X>, grid, NT, 2 * SLOT, st, a); }, bf, d64);
        });
    }
    KF_PROF(label.generic[0], st);
    return with_dtype(pr.dtype, [&](auto t) {
        return with_mode(mode, [&](auto M) { return launch(attn_full_fwd_generic_kernel<decltype(t), M, X>, (unsigned)(B * Hq * Sq), NT, 0, st, a); });
    });
}

// size_query: the workspace query of the calling family, which the workspace refusal names. mod.sink is not read: the backward kernels
// form P from lse, which holds the sink (kf_attn_ext_bwd launches attn_sink_grad after this).
template <bool CAP>
static int full_bwd(const char *who, const char *size_query, const Problem &pr, const MaskPlan &p, Mods mod, const BwdOps &x, void *stream) {
    const void *ops[8] = {x.q, x.k, x.v, x.o, x.d_o, x.dq, x.dk, x.dv};
    const kf_attn_layout *lay[8] = {x.lq, x.lk, x.lv, x.lo, x.ldo, x.ldq, x.ldk, x.ldv};
    FullArgs a;
    Plan plan;
    int rc = full_check(who, pr, ops, lay, 8, a, plan);
    if (rc != KF_OK || plan == PLAN_NONE) return rc;
    const int64_t B = pr.B, Hq = pr.Hq, Hkv = pr.Hkv, Sq = pr.Sq, Skv = pr.Skv, D = pr.D;
    KF_REQUIRE(x.lse, KF_ERR_INVALID, "%s: null operand", who);
    const size_t need = ws_bytes(B, Hq, Sq);
    KF_REQUIRE(x.workspace && x.workspace_bytes >= need && (uintptr_t)x.workspace % sizeof(float) == 0, KF_ERR_INVALID,
               "%s: workspace of at least %zu bytes required (%s), got %zu", who, need, size_query, x.workspace_bytes);
    a.q = (const char *)x.q; a.k = (const char *)x.k; a.v = (const char *)x.v; a.o = (const char *)x.o; a.d_o = (const char *)x.d_o;
    a.dq = (char *)x.dq; a.dk = (char *)x.dk; a.dv = (char *)x.dv;
    a.lse_r = x.lse; a.delta = (float *)x.workspace;
    rc = set_mask(who, a, p);
    if (rc != KF_OK) return rc;
    a.softcap = mod.softcap;
    FullArgs akv = a; // what the two dK/dV launches take: they read the tables at the key index, a keyed mask has a pair of its own for that
    if (p.mode == M_DOC && p.doc.keyed) {
        KF_REQUIRE(p.doc.qstart && p.doc.qend, KF_ERR_INVALID, "%s: null query_lo or query_hi (kf_attn_span_table writes them)", who);
        akv.doc_start = p.doc.qstart;
        akv.doc_end = p.doc.qend;
    }
    hipStream_t st = as_stream(stream);
    const Mode mode = p.mode;
    const Labels &label = kLabels[CAP][mode];
    const bool bf = pr.dtype == KF_BF16, d64 = D == 64;
    const int64_t nrows = B * Hq * Sq;
    if (plan == PLAN_MFMA) {
        { // the delta pre-pass knows no mask: one kernel and one label for every family
            KF_PROF("attn_full_bwd_delta", st);
            rc = with_flags([&](auto BF) { return launch(attn_full_delta_kernel<BF>, (unsigned)((nrows + 15) / 16), NT, 0, st, a.o, a.d_o, a.delta, nrows, a.lo, a.ldo, Sq, Hq, (int)(D / 8)); }, bf);
            if (rc != KF_OK) return rc;
        }
        {
            KF_PROF(label.dq[d64], st);
            const unsigned grid = (unsigned)(B * Hq * ((Sq + TQ - 1) / TQ));
            rc = with_mode(mode, [&](auto M) {
                return with_flags([&](auto BF, auto D64) { return launch(attn_full_bwd_dq_kernel<BF, D64 ? 64 : 128, M, CAP>, grid, NT, DQ_LDS, st, a); }, bf, d64);
            });
            if (rc != KF_OK) return rc;
        }
        KF_PROF(label.dkv[d64], st);
        const unsigned grid = (unsigned)(B * Hkv * ((Skv + TQ - 1) / TQ));
        return with_mode(mode, [&](auto M) {
            return with_flags([&](auto BF, auto D64) { return launch(attn_full_bwd_dkv_kernel<BF, D64 ? 64 : 128, M, CAP>, grid, NT, KV_LDS, st, akv); }, bf, d64);
        });
    }
    return with_dtype(pr.dtype, [&](auto t) {
        using T = decltype(t);
        {
            KF_PROF("attn_full_bwd_delta_generic", st);
            rc = launch(attn_full_delta_generic_kernel<T>, (unsigned)((nrows + NT - 1) / NT), NT, 0, st, (const T *)x.o, (const T *)x.d_o, a.delta, nrows, (int)D);
            if (rc != KF_OK) return rc;
        }
        {
            KF_PROF(label.generic[1], st);
            rc = with_mode(mode, [&](auto M) { return launch(attn_full_bwd_dq_generic_kernel<T, M, CAP>, (unsigned)nrows, NT, 0, st, a); });
            if (rc != KF_OK) return rc;
        }
        KF_PROF(label.generic[2], st);
        return with_mode(mode, [&](auto M) { return launch(attn_full_bwd_dkv_generic_kernel<T, M, CAP>, (unsigned)(B * Hkv * Skv), NT, 0, st, akv); });
    });
}

// kf_attn_full_bwd_workspace_bytes and kf_attn_ext_bwd_workspace_bytes: one size (delta), the checks of the problem under the query's name
static int ws_query(const char *who, const Problem &pr, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "%s: null out pointer", who);
    FullArgs a;
    Plan plan;
    int rc = full_check(who, pr, nullptr, nullptr, 0, a, plan);
    if (rc != KF_OK) return rc;
    *bytes = ws_bytes(pr.B, pr.Hq, pr.Sq);
    return KF_OK;
}

// The host path without modifiers, full_fwd<X_NONE> and full_bwd<false>: defined in attn_full.hip, whose translation unit alone holds
// those instantiations, and called from attn_ext.hip when the modifiers are off (library-internal, as kf::set_error is). `who` is the
// C entry that was called: every refusal carries its name.
namespace kf {
namespace full {
int plain_fwd(const char *who, const Problem &pr, const MaskPlan &p, const FwdOps &x, void *stream);
int plain_bwd(const char *who, const char *size_query, const Problem &pr, const MaskPlan &p, const BwdOps &x, void *stream);
} // namespace full
} // namespace kf

