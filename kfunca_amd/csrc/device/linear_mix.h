// What the chunked linear-time mixers share (linear_attn.hip; delta_rule.hip, 4.15): the 64-row tiles of 16-bit values in
// LDS with an XOR swizzle on the 16-byte chunk, their LDS-DMA staging through buffer descriptors that end with the sequence, the two MFMA
// fragment readers, the chunk's prefix sum of g with its decay vectors, the carried state's 16-bit copy, update and way in and out, and
// the argument checks of the C entries. Everything lives in the including file's unnamed namespace.
#pragma once

#include <math.h>

#include "common.h"

namespace kf {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 l_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 l_f16x8;
typedef __attribute__((ext_vector_type(16))) float l_f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t l_u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t l_u32x2;

constexpr int L_C = 64;           // chunk length
constexpr int L_PT = L_C * 128;   // bytes of a [64][64] 16-bit tile (P, M, a V slice)
constexpr int L_G = 2 * 3 * L_C * 4; // two parities of {G, kd, qd}, 64 floats each

template <bool BF>
__device__ __forceinline__ l_f32x16 l_mma(l_u32x4 a, l_u32x4 b, l_f32x16 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(l_bf16x8, a), __builtin_bit_cast(l_bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(l_f16x8, a), __builtin_bit_cast(l_f16x8, b), c, 0, 0, 0);
}
template <bool BF> __device__ __forceinline__ uint32_t l_cvt16(float v) { return BF ? f32_to_bf16(v).x : f32_to_f16(v).x; }
template <bool BF> __device__ __forceinline__ float l_f32(uint32_t h) { return BF ? bf16_to_f32(bf16_t{(uint16_t)h}) : f16_to_f32(f16_t{(uint16_t)h}); }

// LDS image of a tile with RB-byte rows: the 16-B chunk ch of row r at chunk position ch ^ f(r) (gemm.hip's f for 128-B rows,
// attention.hip's for 256-B rows: both conflict-free for row reads and for the 4-row x 16-column blocks of the transposed read)
template <int RB> __device__ __forceinline__ int l_off(int row, int ch) {
    if constexpr (RB == 128) return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4);
    else return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
// accumulator register e of lane half h <-> row of the 32 x 32 block (the column is lane & 31)
__device__ __forceinline__ int l_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// MFMA operand whose 32 rows are the tile's rows row0 .. row0 + 31 and whose 16 k are the tile's columns k0 .. k0 + 15
template <int RB> __device__ __forceinline__ l_u32x4 l_frag_row(unsigned tile, int row0, int k0) {
    const int lane = threadIdx.x & 63;
    l_u32x4 r;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(tile + (unsigned)l_off<RB>(row0 + (lane & 31), (k0 >> 3) + (lane >> 5))) : "memory");
    return r;
}
// MFMA operand whose 32 rows are the tile's COLUMNS col0 .. col0 + 31 and whose 16 k are the tile's rows r0 .. r0 + 15. Each group of 16
// lanes hands the transposed read a 4-row x 16-column block (lane i: row i >> 2, columns 4 (i & 3) ..) and lane i gets column i of it:
// lane half h reads rows r0 + 8 h + 0..3, then + 4..7 - the k order of l_frag_row.
template <int RB> __device__ __forceinline__ l_u32x4 l_frag_col(unsigned tile, int col0, int r0) {
    const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
    const int row = r0 + 8 * (g >> 1) + (i >> 2), col = col0 + 16 * (g & 1) + 4 * (i & 3);
    const unsigned a0 = tile + (unsigned)(l_off<RB>(row, col >> 3) + (col & 7) * 2), a1 = tile + (unsigned)(l_off<RB>(row + 4, col >> 3) + (col & 7) * 2);
    l_u32x2 lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %2\n\tds_read_b64_tr_b16 %1, %3\n\ts_waitcnt lgkmcnt(0)" : "=&v"(lo), "=&v"(hi) : "v"(a0), "v"(a1) : "memory");
    return l_u32x4{lo[0], lo[1], hi[0], hi[1]};
}
// element j of the fragment times w[j], in f32, one rounding
template <bool BF> __device__ __forceinline__ l_u32x4 l_scale_frag(l_u32x4 f, const float (&w)[8]) {
    l_u32x4 r;
#pragma unroll
    for (int p = 0; p < 4; ++p)
        r[p] = l_cvt16<BF>(l_f32<BF>(f[p] & 0xffffu) * w[2 * p]) | (l_cvt16<BF>(l_f32<BF>(f[p] >> 16) * w[2 * p + 1]) << 16);
    return r;
}

// the descriptor of `bytes` bytes at base; its inputs through readfirstlane (gemm_fp8.hip): block-uniform to the compiler too
__device__ __forceinline__ __amdgpu_buffer_rsrc_t l_rsrc(const char *base, uint32_t bytes) {
    const uint64_t p = (uint64_t)(uintptr_t)base;
    const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p) |
                       ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32)) << 32);
    return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)u, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}
// rows 0 .. 63 of a chunk (RB bytes of each, from byte cb of rows ld bytes apart) -> tile. One wave-instruction moves 1 KiB to consecutive
// LDS bytes, so the swizzle is on the SOURCE chunk; a row at or past `valid` asks for the descriptor's end and gets 16 zero bytes.
template <int RB> __device__ __forceinline__ void l_stage(const char *chunk, int valid, uint32_t ld, uint32_t cb, char *tile) {
    const uint32_t end = (uint32_t)valid * ld;
    const __amdgpu_buffer_rsrc_t rs = l_rsrc(chunk, end);
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int CPR = RB / 16, ROWS = 64 / CPR, OPW = RB / 64; // chunks per row, rows per instruction, instructions per wave
#pragma unroll
    for (int i = 0; i < OPW; ++i) {
        const int row0 = (wid * OPW + i) * ROWS, row = row0 + lane / CPR, pos = lane % CPR;
        const uint32_t src = (uint32_t)(l_off<RB>(row, pos) - row * RB); // the chunk that belongs at position pos: pos ^ f(row)
        const uint32_t voff = row < valid ? (uint32_t)row * ld + cb + src : end;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(tile + row0 * RB), 16, (int)voff, 0, 0, 0);
    }
}
__device__ __forceinline__ void l_landed() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// wave 0: the chunk's inclusive prefix sum of g in f32 (a wave scan over 64 values; steps past the sequence count as 0) and the two
// decay vectors every product of the chunk takes: G[t] = G_t - G_start, kd[s] = exp(G_end - G_s), qd[t] = scale exp(G_t - G_start)
__device__ __forceinline__ void l_scan(const float *g, int valid, float scale, float *out) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    float x = lane < valid ? g[lane] : 0.f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    const float total = __shfl(x, 63);
    out[lane] = x;
    out[64 + lane] = expf(total - x);
    out[128 + lane] = scale * expf(x);
}

// acc (t, s) of block (tb, sb) -> scale acc exp(G_t - G_s) for s <= t, else 0 -> one rounding -> the [t][s] tile
template <bool BF> __device__ __forceinline__ void l_mask_store(const l_f32x16 &acc, char *tile, int tb, int sb, const float (&gt)[16], float gs, float scale) {
    const int lane = threadIdx.x & 63, xl = lane & 31, hl = lane >> 5, s = 32 * sb + xl;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int t = 32 * tb + l_row(e, hl);
        const float v = s <= t ? acc[e] * scale * expf(gt[e] - gs) : 0.f;
        *(uint16_t *)(tile + l_off<128>(t, s >> 3) + (s & 7) * 2) = (uint16_t)l_cvt16<BF>(v);
    }
}
// a state block (rows d of block db in the registers, column dv = lane & 31 of block dvb) -> the 16-bit copy [dv][d], 8-byte stores
template <bool BF, int RB> __device__ __forceinline__ void l_state_store(const l_f32x16 &s, char *tile, int db, int dvb) {
    const int lane = threadIdx.x & 63, xl = lane & 31, hl = lane >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int d = 32 * db + 8 * q + 4 * hl;
        uint2 w;
        w.x = l_cvt16<BF>(s[4 * q]) | (l_cvt16<BF>(s[4 * q + 1]) << 16);
        w.y = l_cvt16<BF>(s[4 * q + 2]) | (l_cvt16<BF>(s[4 * q + 3]) << 16);
        *(uint2 *)(tile + l_off<RB>(32 * dvb + xl, d >> 3) + (d & 7) * 2) = w;
    }
}
// state <- decay state + (rows of tile A)^T (diag(w) rows of tile B): blocks (db[i], dvb), k = the chunk's 64 steps. The 16-bit rounding
// of w B is the one rounding an operand takes on its way into the state.
template <bool BF, int RBA, int RBB, int N>
__device__ __forceinline__ void l_state_update(l_f32x16 (&st)[N], unsigned tA, unsigned tB, const int (&db)[N], int dvb, float decay, const float (&w)[4][8]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) st[i][e] *= decay;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const l_u32x4 b = l_scale_frag<BF>(l_frag_col<RBB>(tB, 32 * dvb, 16 * ks), w[ks]);
#pragma unroll
        for (int i = 0; i < N; ++i) st[i] = l_mma<BF>(l_frag_col<RBA>(tA, 32 * db[i], 16 * ks), b, st[i]);
    }
}
// per lane: w[ks][j] = vec[16 ks + 8 h + j], the k order of a fragment
__device__ __forceinline__ void l_kvec(const float *vec, float (&w)[4][8]) {
    const int hl = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) w[ks][j] = vec[16 * ks + 8 * hl + j];
}
__device__ __forceinline__ void l_rows(const float *vec, int blk, float (&r)[16]) {
    const int hl = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int e = 0; e < 16; ++e) r[e] = vec[32 * blk + l_row(e, hl)];
}
// sum over the 32 lanes of a half wave (the 32 columns of a block), every lane gets it
__device__ __forceinline__ float l_half_sum(float x) {
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// state variants: the f32 state [D][ld] in memory (null: zeros) -> the accumulator blocks (db[i], dvb), each lane its own elements
template <int N> __device__ __forceinline__ void l_state_in(l_f32x16 (&st)[N], const int (&db)[N], int dvb, const float *src, int ld) {
    const int lane = threadIdx.x & 63, xl = lane & 31, hl = lane >> 5;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) st[i][e] = src ? src[(32 * db[i] + l_row(e, hl)) * ld + 32 * dvb + xl] : 0.f;
}
// the accumulator blocks -> an LDS image [rows][W] f32 over tiles nobody reads any more -> memory, 16 bytes a lane along whole rows
template <int N, int W> __device__ __forceinline__ void l_state_out(const l_f32x16 (&st)[N], const int (&db)[N], int dvb, float *img, int rows, float *dst, int ld) {
    const int lane = threadIdx.x & 63, xl = lane & 31, hl = lane >> 5;
    __syncthreads(); // the last reads of the tiles under the image
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) img[(32 * db[i] + l_row(e, hl)) * W + 32 * dvb + xl] = st[i][e];
    __syncthreads();
    for (int at = threadIdx.x; at < rows * (W / 4); at += 256) {
        const int r = at / (W / 4), c4 = at % (W / 4);
        *(float4 *)(dst + (int64_t)r * ld + 4 * c4) = *(const float4 *)(img + r * W + 4 * c4);
    }
}

// ---- the C entries' checks ---------------------------------------------------------------------------------------------------------------
int lin_check(const char *who,int dtype, int64_t B, int64_t H, int64_t S, int64_t Dk, int64_t Dv, float scale) {
    KF_REQUIRE(B > 0 && H > 0 && S > 0 && Dk > 0 && Dv > 0, KF_ERR_INVALID, "%s: bad extents B %lld H %lld S %lld Dk %lld Dv %lld", who, (long long)B,
               (long long)H, (long long)S, (long long)Dk, (long long)Dv);
    KF_REQUIRE(isfinite(scale) && scale != 0.f, KF_ERR_INVALID, "%s: scale must be finite and not zero", who);
    KF_REQUIRE(dtype == KF_BF16 || dtype == KF_F16, KF_ERR_UNSUPPORTED, "%s: dtype %d not supported (half, bfloat16)", who, dtype);
    KF_REQUIRE(Dk == Dv, KF_ERR_UNSUPPORTED, "%s: Dk %lld != Dv %lld is not supported", who, (long long)Dk, (long long)Dv);
    KF_REQUIRE(Dk == 64 || Dk == 128, KF_ERR_UNSUPPORTED, "%s: head size %lld not supported (64, 128)", who, (long long)Dk);
    KF_REQUIRE(B * H < (int64_t)1 << 30 && S < (int64_t)1 << 40, KF_ERR_UNSUPPORTED, "%s: B * H %lld or S %lld above one grid", who, (long long)(B * H), (long long)S);
    return KF_OK;
}
bool al16(const void *p) { return p && ((uintptr_t)p & 15u) == 0; }
bool al16_or_null(const void *p) { return ((uintptr_t)p & 15u) == 0; }

} // namespace
} // namespace kf
