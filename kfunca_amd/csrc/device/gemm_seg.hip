// Segmented (expert) GEMM for gfx950: row segments of one [T, K] operand, each multiplied by its own weight matrix, with the segment
// boundaries in DEVICE memory - the product of a mixture-of-experts layer, and both of its backward products.
//
//   kf_segment_offsets       sorted expert ids -> offsets[E + 1] (a lower bound per entry)
//   kf_gemm_segmented        C[r, :] = alpha A[r, :] op(W_e) + beta C[r, :] for offsets[e] <= r < offsets[e + 1]   (forward, and dX with trans_b)
//   kf_gemm_segmented_wgrad  dW_e = alpha A[seg_e, :]^T B[seg_e, :] + beta dW_e
//
// No entry reads an extent back to the host, synchronises, allocates or uses atomics: a plan kernel (one workgroup) sanitises the offsets
// into the caller's workspace and writes a table of row tiles - each tile inside ONE segment - and the product kernels are launched on a
// host-known bound of tiles; surplus workgroups find an empty table entry and leave. Every output element belongs to exactly one
// workgroup and every sum runs in an order fixed by the arguments: results are bitwise reproducible, and the launches can be captured.
//
// 16-bit fast path: the structure of gemm.hip's 128-tile kernel (128x128x64 tiles, v_mfma_f32_32x32x16, LDS-DMA staging with the same two
// swizzles, the four-stage ring, the LDS-staged 16-byte epilogue); the staging helpers are restated here because gemm.hip is pinned
// to its measured profiles. Ragged rows (forward / dX): the staged row index is clamped to the tile's last row - mapped memory, and the
// product of such a row is never stored. Ragged contraction (wgrad): whole K tiles run through the ring; the one boundary tile is staged
// through registers with explicit zeros past the segment's end, so a neighbour's Inf / NaN never meets a multiplier and nothing past T
// is addressed. Everything else (f32, any extents, any pitch) takes one plain FMA kernel per entry with the same semantics.
#include <limits.h>

#include <type_traits>

#include "common.h"

namespace kf {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 sg_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 sg_f16x8;
typedef __attribute__((ext_vector_type(16))) float sg_f32x16;
typedef __attribute__((ext_vector_type(4))) short sg_s16x4;
typedef __attribute__((ext_vector_type(8))) short sg_s16x8;

constexpr int S_BM = 128, S_BN = 128, S_BK = 64;
constexpr int S_TILE_BYTES = S_BM * S_BK * 2; // 16 KiB per operand tile
constexpr int S_STAGES = 4;                   // ring of [A tile | B tile] buffers: 128 KiB
constexpr int64_t SEG_SURPLUS = -1, SEG_UNCOVERED = -2;

// one row tile of the plan: rows [row0, rend) of segment seg (an expert, or SEG_UNCOVERED: beta only; SEG_SURPLUS: no tile)
struct SegTile {
    int64_t row0, rend, seg, pad;
};

static inline size_t plan_offsets_bytes(int64_t E) { return ((size_t)(E + 1) * 8 + 31) / 32 * 32; }
static inline int64_t plan_tiles(int64_t T, int64_t E) { return T / S_BM + E + 2; }

struct SegArgs {
    const void *A, *B; // forward: A [T, K], B = W; wgrad: A [T, M], B [T, N]
    void *C;           // forward: C [T, N]; wgrad: dW
    int64_t T, M, N, K, E, lda, ldb, ldc, stride; // stride: w_stride / dw_stride (elements)
    float alpha, beta;
    const int64_t *so;  // sanitised offsets [E + 1] (workspace)
    const SegTile *tab; // row tiles (workspace)
    int64_t ntab;       // table entries: the host-known bound T / 128 + E + 2
};

// ---- the plan: o'_j = min(max(0, o_0 .. o_j), T), the row tiles of head | experts | tail, the surplus entries -------------------------
// One workgroup walks the offsets 256 at a time: an inclusive max scan gives the sanitised offsets, an exclusive sum scan of the
// segments' tile counts gives every segment its first table entry; the thread that owns a segment writes its tiles.
template <typename Op>
__device__ __forceinline__ int64_t block_scan_incl(int64_t v, int64_t *sm, Op op) {
    const int t = threadIdx.x;
    sm[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int64_t o = t >= d ? sm[t - d] : v;
        __syncthreads();
        if (t >= d) v = op(v, o);
        sm[t] = v;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(256) void seg_plan_kernel(const int64_t *off, int64_t T, int64_t E, int64_t *so, SegTile *tab, int64_t ntab) {
    __shared__ int64_t sm[256];
    __shared__ int64_t shift[257];
    const int t = threadIdx.x;
    int64_t run_max = 0, run_tiles = 0, prev_last = 0; // the clamp's lower bound, tiles so far, the previous chunk's last boundary
    for (int64_t base = 0; base <= E; base += 256) {
        const int64_t j = base + t;
        const bool live = j <= E;
        int64_t m = block_scan_incl(live ? off[j] : (int64_t)0, sm, [](int64_t a, int64_t b) { return a > b ? a : b; });
        m = m > run_max ? m : run_max;
        const int64_t s = m < T ? m : T; // o'_j
        if (live) so[j] = s;
        shift[t + 1] = s;
        if (t == 0) shift[0] = prev_last;
        __syncthreads();
        const int64_t lo = shift[t]; // segment j: [o'_{j-1}, o'_j); j = 0 is the uncovered head [0, o'_0)
        const int64_t nt = live ? (s - lo + S_BM - 1) / S_BM : 0;
        const int64_t incl = block_scan_incl(nt, sm, [](int64_t a, int64_t b) { return a + b; });
        int64_t at = run_tiles + incl - nt;
        for (int64_t i = 0; i < nt; ++i, ++at) {
            const int64_t r0 = lo + i * S_BM, r1 = r0 + S_BM < s ? r0 + S_BM : s;
            if (at < ntab) tab[at] = SegTile{r0, r1, j == 0 ? SEG_UNCOVERED : j - 1, 0};
        }
        run_tiles += sm[255]; // (sm holds the tile sums now; the maxima travel through shift)
        const int64_t last = shift[256];
        __syncthreads(); // shift and sm are rewritten by the next chunk
        run_max = last > run_max ? last : run_max; // o' is monotone: the chunk's last value is its maximum (T-clamped: so is every later one)
        prev_last = last;
    }
    // the uncovered tail [o'_E, T), then the surplus entries
    const int64_t ntail = (T - prev_last + S_BM - 1) / S_BM;
    for (int64_t i = t; i < ntail; i += 256) {
        const int64_t r0 = prev_last + i * S_BM, r1 = r0 + S_BM < T ? r0 + S_BM : T;
        if (run_tiles + i < ntab) tab[run_tiles + i] = SegTile{r0, r1, SEG_UNCOVERED, 0};
    }
    for (int64_t i = run_tiles + ntail + t; i < ntab; i += 256) tab[i] = SegTile{0, 0, SEG_SURPLUS, 0};
}

__global__ __launch_bounds__(256) void segment_offsets_kernel(const int64_t *ids, int64_t n, int64_t E, int64_t *offsets) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > E) return;
    int64_t lo = 0, hi = n; // the number of ids < e
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (ids[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    offsets[e] = lo;
}

// ---- element access of the plain kernels ---------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float s_load(const T *p) { return (float)*p; }
template <> __device__ __forceinline__ float s_load<bf16_t>(const bf16_t *p) { return bf16_to_f32(*p); }
template <> __device__ __forceinline__ float s_load<f16_t>(const f16_t *p) { return f16_to_f32(*p); }
template <typename T> __device__ __forceinline__ void s_store(T *p, float v) { *p = (T)v; }
template <> __device__ __forceinline__ void s_store<bf16_t>(bf16_t *p, float v) { *p = f32_to_bf16(v); }
template <> __device__ __forceinline__ void s_store<f16_t>(f16_t *p, float v) { *p = f32_to_f16(v); }

// the segment of row r in the sanitised offsets: the number of entries <= r, minus one (-1: the head; E: the tail)
__device__ __forceinline__ int64_t seg_of_row(const int64_t *so, int64_t E, int64_t r) {
    int64_t lo = 0, hi = E + 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (so[mid] <= r) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// plain forward / dX: one thread per output element, a 16 x 16 block of C per workgroup
template <typename T>
__global__ __launch_bounds__(256) void seg_generic_kernel(const SegArgs g, int tb) {
    const int64_t ntn = (g.N + 15) / 16;
    const int64_t r = (int64_t)(blockIdx.x / ntn) * 16 + threadIdx.x / 16, n = (int64_t)(blockIdx.x % ntn) * 16 + threadIdx.x % 16;
    if (r >= g.T || n >= g.N) return;
    const int64_t e = seg_of_row(g.so, g.E, r);
    T *c = (T *)g.C + r * g.ldc + n;
    float v = 0.f;
    if (e >= 0 && e < g.E) {
        const T *a = (const T *)g.A + r * g.lda, *w = (const T *)g.B + e * g.stride;
        float acc = 0.f;
        for (int64_t k = 0; k < g.K; ++k) acc = fmaf(s_load<T>(a + k), s_load<T>(tb ? w + n * g.ldb + k : w + k * g.ldb + n), acc);
        v = g.alpha * acc;
    }
    if (g.beta != 0.f) v += g.beta * s_load<T>(c);
    s_store<T>(c, v);
}

// plain wgrad: one thread per element of dW_e, the segment's rows in order
template <typename T>
__global__ __launch_bounds__(256) void seg_wgrad_generic_kernel(const SegArgs g) {
    const int64_t ntn = (g.N + 15) / 16, ntm = (g.M + 15) / 16, per = ntn * ntm;
    const int64_t e = blockIdx.x / per, in = blockIdx.x % per;
    const int64_t m = (in / ntn) * 16 + threadIdx.x / 16, n = (in % ntn) * 16 + threadIdx.x % 16;
    if (m >= g.M || n >= g.N) return;
    const int64_t r0 = g.so[e], r1 = g.so[e + 1];
    T *c = (T *)g.C + e * g.stride + m * g.ldc + n;
    float v = 0.f;
    if (r1 > r0) {
        float acc = 0.f;
        for (int64_t r = r0; r < r1; ++r) acc = fmaf(s_load<T>((const T *)g.A + r * g.lda + m), s_load<T>((const T *)g.B + r * g.ldb + n), acc);
        v = g.alpha * acc;
    }
    if (g.beta != 0.f) v += g.beta * s_load<T>(c);
    s_store<T>(c, v);
}

// ---- 16-bit fast path: the staging of gemm.hip's 128-tile kernel, restated -----------------------------------------------------------
__device__ __forceinline__ uint32_t s_xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t nx = 8, xcd = bid % nx, q = nwg / nx, r = nwg % nx;
    const uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / nx;
}

// Grouped tile order (gemm.hip's): logical ids walk groups of gm tile rows column by column, so the consecutive ids one XCD owns cover a
// gm x (q / gm) rectangle of the output - gm row panels and q / gm column panels through that XCD's L2 instead of one row panel and a
// whole row of column panels. Bijective for any extents.
constexpr uint32_t S_GROUP = 8;
__device__ __forceinline__ void s_grouped_tile(uint32_t id, uint32_t tiles_m, uint32_t tiles_n, uint32_t &tm, uint32_t &tn) {
    const uint32_t per = S_GROUP * tiles_n, grp = id / per, first = grp * S_GROUP;
    const uint32_t rows = min(S_GROUP, tiles_m - first), in = id - grp * per;
    tm = first + in % rows;
    tn = in / rows;
}

template <bool BF> struct SFrag { using type = sg_f16x8; };
template <> struct SFrag<true> { using type = sg_bf16x8; };

template <bool BF>
__device__ __forceinline__ sg_f32x16 s_mfma(typename SFrag<BF>::type a, typename SFrag<BF>::type b, sg_f32x16 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// [128 rows][64 k] image, 128-B rows, 16-B chunk c of row r at chunk position c ^ ((r >> 1) & 7)
__device__ __forceinline__ int s_lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// rows x0 .. x0 + 127 of a k-contiguous operand; a row past xlast is fetched from row xlast (mapped; its product is never stored)
__device__ __forceinline__ void s_stage(const char *gbase, int64_t ld_bytes, int64_t x0, int64_t xlast, int64_t k0_bytes, char *lds_tile) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row0 = (wid * 4 + i) * 8;
        const int row = row0 + (lane >> 3), pos = lane & 7;
        const int chunk = pos ^ ((row >> 1) & 7);
        const int64_t x = x0 + row < xlast ? x0 + row : xlast;
        const char *src = gbase + x * ld_bytes + k0_bytes + chunk * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + row0 * 128), 16, 0, 0);
    }
}
// [64 k][128 rows / columns] image of an operand whose contraction dim is the strided one: 256-B rows, chunk ch of k-row r at chunk
// position ch ^ (((r & 3) << 2) | ((r >> 2) & 3)), read with ds_read_b64_tr_b16
__device__ __forceinline__ int s_tr_off(int row, int ch) { return row * 256 + ((ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4); }
__device__ __forceinline__ void s_stage_tr(const char *gbase, int64_t ld_bytes, int64_t x0, int64_t k0, char *lds_tile) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row0 = (wid * 4 + i) * 4;
        const int row = row0 + (lane >> 4), pos = lane & 15;
        const int chunk = pos ^ (((row & 3) << 2) | ((row >> 2) & 3));
        const char *src = gbase + (k0 + row) * ld_bytes + (x0 + chunk * 8) * 2;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + row0 * 256), 16, 0, 0);
    }
}
// the same image through registers, k-rows at or past `valid` written as zeros and never addressed (the boundary K tile of a segment)
__device__ __forceinline__ void s_stage_tr_zero(const char *gbase, int64_t ld_bytes, int64_t x0, int64_t k0, int valid, char *lds_tile) {
    uint4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = i * 256 + (int)threadIdx.x, row = idx >> 4, ch = idx & 15;
        v[i] = uint4{0u, 0u, 0u, 0u};
        if (row < valid) v[i] = *(const uint4 *)(gbase + (k0 + row) * ld_bytes + (x0 + ch * 8) * 2);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = i * 256 + (int)threadIdx.x, row = idx >> 4, ch = idx & 15;
        *(uint4 *)(lds_tile + s_tr_off(row, ch)) = v[i];
    }
}
__device__ __forceinline__ void s_tr_lane_off(int cb, int (&off)[2]) {
    const int lane = threadIdx.x & 63;
    const int gq = lane >> 4, ii = lane & 15, qq = ii >> 2, p = ii & 3, h = gq >> 1;
    const int ch = ((cb + 16 * (gq & 1)) >> 3) + (p >> 1);
#pragma unroll
    for (int second = 0; second < 2; ++second) off[second] = s_tr_off(8 * h + qq + 4 * second, ch) + 8 * (p & 1);
}
template <bool BF, int OFF>
__device__ __forceinline__ typename SFrag<BF>::type s_tr_frag(unsigned a0, unsigned a1) {
    sg_s16x4 lo, hi;
    asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%c4\n\tds_read_b64_tr_b16 %1, %3 offset:%c4"
                 : "=&v"(lo), "=&v"(hi)
                 : "v"(a0), "v"(a1), "n"(OFF)
                 : "memory");
    sg_s16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return __builtin_bit_cast(typename SFrag<BF>::type, r);
}

// The per-lane read addresses of one workgroup's fragments and the four k-steps of one staged tile.
template <bool BF, bool TRA, bool TRB>
struct SReader {
    using frag_t = typename SFrag<BF>::type;
    int toffA[2][2], toffB[2][2], offA[2], offB[2];
    __device__ __forceinline__ SReader() {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        const int wr = wid >> 1, wc = wid & 1, xl = lane & 31, hl = lane >> 5;
        if constexpr (TRA) { s_tr_lane_off(wr * 64, toffA[0]); s_tr_lane_off(wr * 64 + 32, toffA[1]); }
        if constexpr (TRB) { s_tr_lane_off(wc * 64, toffB[0]); s_tr_lane_off(wc * 64 + 32, toffB[1]); }
        offA[0] = s_lds_off(wr * 64 + xl, hl); offA[1] = s_lds_off(wr * 64 + 32 + xl, hl);
        offB[0] = s_lds_off(wc * 64 + xl, hl); offB[1] = s_lds_off(wc * 64 + 32 + xl, hl);
    }
    static __device__ __forceinline__ void rd(frag_t &dst, unsigned addr) { asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr) : "memory"); }
    template <int KS>
    __device__ __forceinline__ void read_step(unsigned cur_u, frag_t (&a)[2], frag_t (&b)[2]) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (TRA) a[i] = s_tr_frag<BF, KS * 16 * 256>(cur_u + toffA[i][0], cur_u + toffA[i][1]);
            else rd(a[i], cur_u + (unsigned)(offA[i] ^ (KS * 32)));
            if constexpr (TRB) b[i] = s_tr_frag<BF, KS * 16 * 256>(cur_u + S_TILE_BYTES + toffB[i][0], cur_u + S_TILE_BYTES + toffB[i][1]);
            else rd(b[i], cur_u + S_TILE_BYTES + (unsigned)(offB[i] ^ (KS * 32)));
        }
    }
    static __device__ __forceinline__ void landed(frag_t (&a)[2], frag_t (&b)[2]) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : : "memory");
    }
    static __device__ __forceinline__ void mma(frag_t (&a)[2], frag_t (&b)[2], sg_f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = s_mfma<BF>(a[i], b[j], acc[i][j]);
    }
};

// nt >= 1 K tiles through the four-stage ring (gemm.hip's loop: three to four tiles in flight, a wave issues 8 LDS-DMA operations per
// tile, so vmcnt(16) = "everything but the two youngest tiles has landed"; past the end the last tile is fetched again and never read;
// one barrier per tile, in front of its last k-step). stage(t, buf) issues tile t's 8 operations. Returns with nothing in flight.
template <bool BF, bool TRA, bool TRB, typename Stage>
__device__ __forceinline__ void s_ring(const SReader<BF, TRA, TRB> &R, Stage stage, int nt, char *smem, sg_f32x16 (&acc)[2][2]) {
    using frag_t = typename SFrag<BF>::type;
    const unsigned smem_u = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    auto clampt = [&](int t) { return t < nt ? t : nt - 1; };
#pragma unroll
    for (int t = 0; t < S_STAGES; ++t) stage(clampt(t), smem + t * 2 * S_TILE_BYTES);
    frag_t fa[2][2], fb[2][2];
    asm volatile("s_waitcnt vmcnt(24)\n\ts_barrier" ::: "memory"); // tile 0 has landed for everyone
    R.template read_step<0>(smem_u, fa[0], fb[0]);
    R.landed(fa[0], fb[0]);
    for (int t = 0; t < nt; ++t) {
        const unsigned cur_u = smem_u + (unsigned)((t % S_STAGES) * 2 * S_TILE_BYTES), nxt_u = smem_u + (unsigned)(((t + 1) % S_STAGES) * 2 * S_TILE_BYTES);
        R.template read_step<1>(cur_u, fa[1], fb[1]);
        R.mma(fa[0], fb[0], acc);
        R.landed(fa[1], fb[1]);
        R.template read_step<2>(cur_u, fa[0], fb[0]);
        R.mma(fa[1], fb[1], acc);
        R.landed(fa[0], fb[0]);
        R.template read_step<3>(cur_u, fa[1], fb[1]);
        R.mma(fa[0], fb[0], acc);
        R.landed(fa[1], fb[1]);
        asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory"); // tile t + 1 has landed for everyone; nobody reads tile t any more
        stage(clampt(t + S_STAGES), smem + (t % S_STAGES) * 2 * S_TILE_BYTES);
        R.template read_step<0>(nxt_u, fa[0], fb[0]);
        R.mma(fa[1], fb[1], acc);
        R.landed(fa[0], fb[0]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the re-fetched tail tiles: nothing may still be writing LDS afterwards
}

template <bool BF>
__device__ __forceinline__ uint32_t s_pack2(float lo, float hi) {
    if constexpr (BF) return f32x2_to_bf16x2_hw(lo, hi);
    else return (uint32_t)f32_to_f16(lo).x | ((uint32_t)f32_to_f16(hi).x << 16);
}
template <bool BF>
__device__ __forceinline__ void s_unpack8(const uint4 q, float (&f)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint16_t o = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
        f[e] = BF ? bf16_to_f32(bf16_t{o}) : f16_to_f32(f16_t{o});
    }
}

// Eight consecutive columns of one row per lane and step, one 16-byte access each way: rows [0, rows) of the 128 x 128 tile at C
// (16-byte aligned, ldc a multiple of 8) become scale * value + beta * C. beta == 0 never reads C.
template <bool BF, typename Value>
__device__ __forceinline__ void s_store_rows(uint16_t *C, int64_t ldc, int rows, float beta, Value value) {
#pragma unroll
    for (int r = 0; r < S_BM * S_BN / 8 / 256; ++r) {
        const int gi = (int)threadIdx.x + 256 * r, row = gi >> 4, c8 = (gi & 15) * 8;
        if (row >= rows) continue;
        float v[8];
        value(row, c8, v);
        uint4 *p = (uint4 *)(C + (int64_t)row * ldc + c8);
        if (beta != 0.f) {
            float old[8];
            s_unpack8<BF>(*p, old);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += beta * old[e];
        }
        *p = uint4{s_pack2<BF>(v[0], v[1]), s_pack2<BF>(v[2], v[3]), s_pack2<BF>(v[4], v[5]), s_pack2<BF>(v[6], v[7])};
    }
}

// the accumulators through LDS (the ring is free), then s_store_rows; `product` false: the tile has no product (an empty segment)
template <bool BF>
__device__ __forceinline__ void s_epilogue(const sg_f32x16 (&acc)[2][2], char *smem, uint16_t *C, int64_t ldc, int rows, float alpha, float beta,
                                           bool product) {
    constexpr int EROW = S_BN + 4;
    static_assert(S_BM * EROW * 4 <= S_STAGES * 2 * S_TILE_BYTES, "the staged tile must fit into the ring");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr = wid >> 1, wc = wid & 1, xl = lane & 31, hl = lane >> 5;
    float *stg = (float *)smem;
    __syncthreads(); // nobody reads the ring any more
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stg[(wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl) * EROW + wc * 64 + j * 32 + xl] = acc[i][j][e];
    __syncthreads();
    s_store_rows<BF>(C, ldc, rows, beta, [&](int row, int c8, float (&v)[8]) {
        const float4 lo = *(const float4 *)(stg + row * EROW + c8), hi = *(const float4 *)(stg + row * EROW + c8 + 4);
        const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = product ? alpha * x[e] : 0.f;
    });
}

// forward / dX. A [T, K] k-contiguous; W_e [K, N] (TRB: the contraction is its strided dim) or [N, K].
template <bool BF, bool TRB>
__global__ __launch_bounds__(256) void seg_h_kernel(const SegArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t tiles_n = (uint32_t)(g.N / S_BN);
    // row tiles in table order, eight at a time: the tiles of one expert are neighbours on one XCD and share W_e's column panels there
    uint32_t rt, tn;
    s_grouped_tile(s_xcd_remap(blockIdx.x, gridDim.x), (uint32_t)g.ntab, tiles_n, rt, tn);
    const SegTile tl = g.tab[rt];
    if (tl.seg == SEG_SURPLUS) return;
    const int64_t n0 = (int64_t)tn * S_BN;
    const int rows = (int)(tl.rend - tl.row0);
    uint16_t *C = (uint16_t *)g.C + tl.row0 * g.ldc + n0;
    if (tl.seg == SEG_UNCOVERED) { // rows no segment covers: beta C, which is +0 when beta == 0
        s_store_rows<BF>(C, g.ldc, rows, g.beta, [](int, int, float (&v)[8]) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = 0.f;
        });
        return;
    }
    const char *A = (const char *)g.A, *W = (const char *)g.B + tl.seg * g.stride * 2;
    const int64_t lda_b = g.lda * 2, ldw_b = g.ldb * 2;
    sg_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const SReader<BF, false, TRB> R;
    s_ring<BF, false, TRB>(R, [&](int t, char *buf) __attribute__((always_inline)) {
        s_stage(A, lda_b, tl.row0, tl.rend - 1, (int64_t)t * S_BK * 2, buf);
        if constexpr (TRB) s_stage_tr(W, ldw_b, n0, (int64_t)t * S_BK, buf + S_TILE_BYTES);
        else s_stage(W, ldw_b, n0, n0 + S_BN - 1, (int64_t)t * S_BK * 2, buf + S_TILE_BYTES);
    }, (int)(g.K / S_BK), smem, acc);
    s_epilogue<BF>(acc, smem, C, g.ldc, rows, g.alpha, g.beta, true);
}

// wgrad: both operands are contracted along their strided dim (the segment's rows). K tiles start at the segment's first row.
template <bool BF>
__global__ __launch_bounds__(256) void seg_wgrad_h_kernel(const SegArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const uint32_t tiles_n = (uint32_t)(g.N / S_BN), per = (uint32_t)(g.M / S_BM) * tiles_n;
    // A workgroup's work is its segment's length, so the experts are walked in launch order - every XCD takes its share of each expert,
    // long or empty - and the XCD remap runs inside one expert: the tiles an XCD owns there are neighbours that share A and B panels.
    // (Remapping the whole grid hands the first experts to one XCD: 3.4 x the balanced time under a Zipf skew.)
    const int64_t e = blockIdx.x / per;
    uint32_t tm, tn;
    s_grouped_tile(s_xcd_remap(blockIdx.x % per, per), per / tiles_n, tiles_n, tm, tn);
    const int64_t m0 = (int64_t)tm * S_BM, n0 = (int64_t)tn * S_BN;
    const int64_t r0 = g.so[e], len = g.so[e + 1] - r0;
    const int nfull = (int)(len / S_BK), rem = (int)(len % S_BK);
    const int64_t lda_b = g.lda * 2, ldb_b = g.ldb * 2;
    const char *A = (const char *)g.A + r0 * lda_b, *B = (const char *)g.B + r0 * ldb_b;
    sg_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e2 = 0; e2 < 16; ++e2) acc[i][j][e2] = 0.f;
    const SReader<BF, true, true> R;
    if (nfull > 0)
        s_ring<BF, true, true>(R, [&](int t, char *buf) __attribute__((always_inline)) {
            s_stage_tr(A, lda_b, m0, (int64_t)t * S_BK, buf);
            s_stage_tr(B, ldb_b, n0, (int64_t)t * S_BK, buf + S_TILE_BYTES);
        }, nfull, smem, acc);
    if (rem > 0) { // the boundary tile: rows past the segment's end enter as zeros
        using frag_t = typename SFrag<BF>::type;
        __syncthreads(); // (no LDS-DMA is in flight: s_ring waited for all of it)
        s_stage_tr_zero(A, lda_b, m0, (int64_t)nfull * S_BK, rem, smem);
        s_stage_tr_zero(B, ldb_b, n0, (int64_t)nfull * S_BK, rem, smem + S_TILE_BYTES);
        __syncthreads();
        const unsigned smem_u = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
        frag_t fa[2], fb[2];
        R.template read_step<0>(smem_u, fa, fb); R.landed(fa, fb); R.mma(fa, fb, acc);
        if (rem > 16) { R.template read_step<1>(smem_u, fa, fb); R.landed(fa, fb); R.mma(fa, fb, acc); }
        if (rem > 32) { R.template read_step<2>(smem_u, fa, fb); R.landed(fa, fb); R.mma(fa, fb, acc); }
        if (rem > 48) { R.template read_step<3>(smem_u, fa, fb); R.landed(fa, fb); R.mma(fa, fb, acc); }
    }
    s_epilogue<BF>(acc, smem, (uint16_t *)g.C + e * g.stride + m0 * g.ldc + n0, g.ldc, S_BM, g.alpha, g.beta, len > 0);
}

template <typename F> int with_seg_dtype(int dtype, F &&f) {
    return dtype == KF_F32 ? f(float{}) : dtype == KF_BF16 ? f(bf16_t{}) : f(f16_t{});
}
bool seg_dtype_ok(int dtype) { return dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16; }
bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int check_workspace(const char *who, int64_t T, int64_t E, const void *workspace, size_t workspace_bytes) {
    const size_t need = plan_offsets_bytes(E) + (size_t)plan_tiles(T, E) * sizeof(SegTile);
    KF_REQUIRE(workspace != nullptr, KF_ERR_INVALID, "%s: null workspace (%zu bytes needed)", who, need);
    KF_REQUIRE(workspace_bytes >= need, KF_ERR_INVALID, "%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, need);
    KF_REQUIRE(al16(workspace), KF_ERR_INVALID, "%s: workspace not 16-byte aligned", who);
    return KF_OK;
}

int run_plan(const int64_t *offsets, int64_t T, int64_t E, void *workspace, hipStream_t st) {
    int64_t *so = (int64_t *)workspace;
    SegTile *tab = (SegTile *)((char *)workspace + plan_offsets_bytes(E));
    return launch(seg_plan_kernel, dim3(1), dim3(256), 0, st, offsets, T, E, so, tab, plan_tiles(T, E));
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_segment_offsets(const int64_t *sorted_ids, int64_t n, int64_t E, int64_t *offsets, void *stream) {
    KF_REQUIRE(n >= 0 && E >= 1, KF_ERR_INVALID, "kf_segment_offsets: bad extents n %lld E %lld (n >= 0, E >= 1)", (long long)n, (long long)E);
    KF_REQUIRE(offsets && (sorted_ids || n == 0), KF_ERR_INVALID, "kf_segment_offsets: null sorted_ids or offsets");
    KF_REQUIRE((uintptr_t)offsets % 8 == 0 && (uintptr_t)sorted_ids % 8 == 0, KF_ERR_INVALID, "kf_segment_offsets: operands not aligned to 8 bytes");
    KF_REQUIRE(E < ((int64_t)1 << 31) * 256 - 1, KF_ERR_INVALID, "kf_segment_offsets: E %lld too large", (long long)E);
    hipStream_t st = as_stream(stream);
    KF_PROF("segment_offsets", st);
    return launch(segment_offsets_kernel, dim3((unsigned)((E + 1 + 255) / 256)), dim3(256), 0, st, sorted_ids, n, E, offsets);
}

extern "C" int kf_gemm_segmented_workspace_bytes(int dtype, int64_t T, int64_t E, size_t *bytes) {
    KF_REQUIRE(bytes, KF_ERR_INVALID, "kf_gemm_segmented_workspace_bytes: null bytes");
    KF_REQUIRE(seg_dtype_ok(dtype), KF_ERR_INVALID, "kf_gemm_segmented_workspace_bytes: dtype %d not supported (float, half, bfloat16)", dtype);
    KF_REQUIRE(T >= 0 && E >= 1, KF_ERR_INVALID, "kf_gemm_segmented_workspace_bytes: bad extents T %lld E %lld (T >= 0, E >= 1)", (long long)T, (long long)E);
    *bytes = plan_offsets_bytes(E) + (size_t)plan_tiles(T, E) * sizeof(SegTile);
    return KF_OK;
}

extern "C" int kf_gemm_segmented(int dtype, int trans_b, int64_t T, int64_t N, int64_t K, int64_t E, const int64_t *offsets, float alpha, const void *A,
                                 int64_t lda, const void *W, int64_t ldw, int64_t w_stride, float beta, void *C, int64_t ldc, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    const char *who = "kf_gemm_segmented";
    KF_REQUIRE(seg_dtype_ok(dtype), KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(trans_b == 0 || trans_b == 1, KF_ERR_INVALID, "%s: trans_b %d is not 0 or 1", who, trans_b);
    KF_REQUIRE(T >= 0 && N >= 0 && K >= 0 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld N %lld K %lld E %lld (E >= 1)", who, (long long)T,
               (long long)N, (long long)K, (long long)E);
    KF_REQUIRE(offsets && A && W && C, KF_ERR_INVALID, "%s: null offsets, A, W or C", who);
    const int64_t wr = trans_b ? N : K, wc = trans_b ? K : N; // W_e as stored: [wr, wc]
    KF_REQUIRE(lda >= K, KF_ERR_INVALID, "%s: pitch of A %lld < K = %lld", who, (long long)lda, (long long)K);
    KF_REQUIRE(ldw >= wc, KF_ERR_INVALID, "%s: pitch of W %lld < %lld", who, (long long)ldw, (long long)wc);
    KF_REQUIRE(ldc >= N, KF_ERR_INVALID, "%s: pitch of C %lld < N = %lld", who, (long long)ldc, (long long)N);
    KF_REQUIRE(E == 1 || wr == 0 || wc == 0 || w_stride >= (wr - 1) * ldw + wc, KF_ERR_INVALID, "%s: w_stride %lld < one expert's extent %lld", who, (long long)w_stride,
               (long long)((wr - 1) * ldw + wc));
    const int es = dtype_size(dtype);
    KF_REQUIRE((uintptr_t)A % es == 0 && (uintptr_t)W % es == 0 && (uintptr_t)C % es == 0 && (uintptr_t)offsets % 8 == 0, KF_ERR_INVALID,
               "%s: an operand is not aligned to its element size", who);
    const int rc = check_workspace(who, T, E, workspace, workspace_bytes);
    if (rc != KF_OK) return rc;
    if (T == 0 || N == 0 || K == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    SegArgs g{};
    g.A = A; g.B = W; g.C = C;
    g.T = T; g.N = N; g.K = K; g.E = E; g.lda = lda; g.ldb = ldw; g.ldc = ldc; g.stride = w_stride;
    g.alpha = alpha; g.beta = beta;
    g.so = (const int64_t *)workspace;
    g.tab = (const SegTile *)((const char *)workspace + plan_offsets_bytes(E));
    g.ntab = plan_tiles(T, E);
    const bool fast = es == 2 && N % S_BN == 0 && K % S_BK == 0 && lda % 8 == 0 && ldw % 8 == 0 && ldc % 8 == 0 && w_stride % 8 == 0 && al16(A) && al16(W) &&
                      al16(C) && plan_tiles(T, E) * (N / S_BN) < ((int64_t)1 << 31);
    const int64_t blocks = fast ? plan_tiles(T, E) * (N / S_BN) : ((T + 15) / 16) * ((N + 15) / 16);
    KF_REQUIRE(blocks < ((int64_t)1 << 31), KF_ERR_UNSUPPORTED, "%s: %lld workgroups exceed one grid", who, (long long)blocks);
    const bool bf = dtype == KF_BF16;
    KF_PROF(fast ? (bf ? "gemm_seg_bf16_mfma" : "gemm_seg_f16_mfma") : "gemm_seg_generic", st);
    const int prc = run_plan(offsets, T, E, workspace, st);
    if (prc != KF_OK) return prc;
    if (fast)
        return with_flags([&](auto BF, auto TRB) { return launch(seg_h_kernel<BF, TRB>, dim3((unsigned)blocks), dim3(256), (size_t)S_STAGES * 2 * S_TILE_BYTES, st, g); },
                          bf, trans_b == 0);
    return with_seg_dtype(dtype, [&](auto t) { return launch(seg_generic_kernel<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, st, g, trans_b); });
}

extern "C" int kf_gemm_segmented_wgrad(int dtype, int64_t T, int64_t M, int64_t N, int64_t E, const int64_t *offsets, float alpha, const void *A,
                                       int64_t lda, const void *B, int64_t ldb, float beta, void *dW, int64_t lddw, int64_t dw_stride, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    const char *who = "kf_gemm_segmented_wgrad";
    KF_REQUIRE(seg_dtype_ok(dtype), KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(T >= 0 && M >= 0 && N >= 0 && E >= 1, KF_ERR_INVALID, "%s: bad extents T %lld M %lld N %lld E %lld (E >= 1)", who, (long long)T, (long long)M,
               (long long)N, (long long)E);
    KF_REQUIRE(offsets && A && B && dW, KF_ERR_INVALID, "%s: null offsets, A, B or dW", who);
    KF_REQUIRE(lda >= M, KF_ERR_INVALID, "%s: pitch of A %lld < M = %lld", who, (long long)lda, (long long)M);
    KF_REQUIRE(ldb >= N, KF_ERR_INVALID, "%s: pitch of B %lld < N = %lld", who, (long long)ldb, (long long)N);
    KF_REQUIRE(lddw >= N, KF_ERR_INVALID, "%s: pitch of dW %lld < N = %lld", who, (long long)lddw, (long long)N);
    KF_REQUIRE(E == 1 || M == 0 || N == 0 || dw_stride >= (M - 1) * lddw + N, KF_ERR_INVALID, "%s: dw_stride %lld < one expert's extent %lld", who, (long long)dw_stride,
               (long long)((M - 1) * lddw + N));
    const int es = dtype_size(dtype);
    KF_REQUIRE((uintptr_t)A % es == 0 && (uintptr_t)B % es == 0 && (uintptr_t)dW % es == 0 && (uintptr_t)offsets % 8 == 0, KF_ERR_INVALID,
               "%s: an operand is not aligned to its element size", who);
    const int rc = check_workspace(who, T, E, workspace, workspace_bytes);
    if (rc != KF_OK) return rc;
    if (T == 0 || M == 0 || N == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    SegArgs g{};
    g.A = A; g.B = B; g.C = dW;
    g.T = T; g.M = M; g.N = N; g.E = E; g.lda = lda; g.ldb = ldb; g.ldc = lddw; g.stride = dw_stride;
    g.alpha = alpha; g.beta = beta;
    g.so = (const int64_t *)workspace;
    g.tab = (const SegTile *)((const char *)workspace + plan_offsets_bytes(E));
    g.ntab = plan_tiles(T, E);
    const bool fast = es == 2 && M % S_BM == 0 && N % S_BN == 0 && lda % 8 == 0 && ldb % 8 == 0 && lddw % 8 == 0 && dw_stride % 8 == 0 && al16(A) && al16(B) &&
                      al16(dW) && (double)E * (double)(M / S_BM) * (double)(N / S_BN) < 2147483648.0;
    const double blocks_d = fast ? (double)E * (double)(M / S_BM) * (double)(N / S_BN) : (double)E * (double)((M + 15) / 16) * (double)((N + 15) / 16);
    KF_REQUIRE(blocks_d < 2147483648.0, KF_ERR_UNSUPPORTED, "%s: %.0f workgroups exceed one grid", who, blocks_d);
    const unsigned blocks = (unsigned)blocks_d;
    const bool bf = dtype == KF_BF16;
    KF_PROF(fast ? (bf ? "gemm_seg_wgrad_bf16_mfma" : "gemm_seg_wgrad_f16_mfma") : "gemm_seg_wgrad_generic", st);
    const int prc = run_plan(offsets, T, E, workspace, st);
    if (prc != KF_OK) return prc;
    if (fast)
        return with_flags([&](auto BF) { return launch(seg_wgrad_h_kernel<BF>, dim3(blocks), dim3(256), (size_t)S_STAGES * 2 * S_TILE_BYTES, st, g); }, bf);
    return with_seg_dtype(dtype, [&](auto t) { return launch(seg_wgrad_generic_kernel<decltype(t)>, dim3(blocks), dim3(256), 0, st, g); });
}
