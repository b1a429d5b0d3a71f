// Symmetric rank-K product for gfx950: C[M, M] = alpha X X^T + beta D + gamma I with X [M, K] row-major, D (optional) symmetric - the two
// symmetric products of a Newton-Schulz iteration (A = X X^T, then c A A + b A + a I with X = D = A).
//
//   kf_gemm_sym   only the tiles on and below the diagonal are computed; every tile below it is stored twice, once transposed
//
// Guarantee: C is BITWISE symmetric - element (r, c) and element (c, r) are two stores of one rounded value, never two computations.
// Every element of C is written by exactly one workgroup, there are no atomics, no workspace, no allocation and no synchronisation:
// results are reproducible to the bit and the call can be captured. Only the values of D at and below the diagonal enter the result.
//
// 16-bit fast path (M a multiple of 128, K of 64, pitches of 8, 16-byte bases): 128 x 128 x 64 tiles on v_mfma_f32_32x32x16, both operands
// of a tile being rows of the same X (the NT form, k-contiguous), staged by LDS-DMA into a four-stage ring - the structure of
// gemm_seg.hip's forward kernel, whose staging helpers are restated here (gemm.hip and gemm_seg.hip are pinned to their measured
// profiles). What is this kernel's own:
//   grid      nt (nt + 1) / 2 workgroups for nt = M / 128; the linear id is decoded to a tile (i >= j) in integers (y_tile). Tile rows are
//             walked in groups of eight, column by column inside a group, so the consecutive ids one XCD owns cover an 8 x (q / 8) block:
//             eight row panels of X and q / 8 column panels pass through that XCD's L2, not one row panel and q column panels.
//   diagonal  a tile with i == j stages its one row panel once per K step (four LDS-DMA operations a wave, not eight) and feeds both MFMA
//             operands from it.
//   epilogue  accumulators -> an f32 image in LDS -> the tail (alpha, beta D from tile (i, j) of D, gamma on the diagonal) and ONE rounding;
//             the rounded 16-bit values go to C(i, j) as 16-byte row stores and, transposed, into a second LDS image whose rows leave as
//             the 16-byte row stores of C(j, i). A diagonal tile writes the values at and below its diagonal to both places of that
//             image and stores the image alone. (The accumulators of (r, c) and (c, r) of a diagonal tile are the same products summed
//             in the same K order; storing one of them twice makes the symmetry independent of that.)
// Everything else (f32, any extents, any pitch, unaligned bases) takes one plain FMA kernel with the same semantics and the same bitwise
// symmetry: the thread of (r >= c) stores both elements.
#include <limits.h>

#include <type_traits>

#include "common.h"

namespace kf {
namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 y_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 y_f16x8;
typedef __attribute__((ext_vector_type(16))) float y_f32x16;

constexpr int Y_BM = 128, Y_BN = 128, Y_BK = 64;
constexpr int Y_TILE_BYTES = Y_BM * Y_BK * 2; // 16 KiB per operand tile
constexpr int Y_STAGES = 4;                   // ring of [row panel tile | column panel tile] buffers: 128 KiB
constexpr int Y_EROW = Y_BN + 4;              // f32 image of the accumulators: 128 rows of 132 floats
constexpr int Y_F32_IMAGE = Y_BM * Y_EROW * 4;
constexpr int Y_LDS = Y_STAGES * 2 * Y_TILE_BYTES;
static_assert(Y_F32_IMAGE % 16 == 0 && Y_F32_IMAGE + Y_BM * Y_BN * 2 <= Y_LDS, "both epilogue images must fit into the ring");

struct SymArgs {
    const void *X, *D; // D null: no beta term
    void *C;
    int64_t M, K, ldx, ldd, ldc;
    float alpha, beta, gamma;
    uint32_t nt; // tile rows: M / 128 (fast path), ceil(M / 16) (plain path)
};

// ---- the triangular grid -------------------------------------------------------------------------------------------------------------
// Tile rows in groups of eight. 32 g^2 + 4 g tiles lie before group g (a whole group g has 64 g + 36); inside a group the ids walk the
// 8 g full columns top to bottom, then the columns of the group's own triangle. g comes from a float square root corrected by
// comparison in integers, so the decode is exact for every id of a grid (ids < 2^31). Bijective onto {(i, j): nt > i >= j >= 0}.
constexpr int64_t Y_GROUP = 8;
__host__ __device__ __forceinline__ void y_tile(uint32_t id, uint32_t nt, uint32_t &ti, uint32_t &tj) {
    int64_t g = (int64_t)sqrtf((float)id * (1.f / 32.f));
    while (32 * g * g + 4 * g > (int64_t)id) --g;
    while (32 * (g + 1) * (g + 1) + 4 * (g + 1) <= (int64_t)id) ++g;
    const int64_t first = g * Y_GROUP, rows = (int64_t)nt - first < Y_GROUP ? (int64_t)nt - first : Y_GROUP;
    int64_t in = (int64_t)id - (32 * g * g + 4 * g);
    if (in < rows * first) {
        ti = (uint32_t)(first + in % rows);
        tj = (uint32_t)(in / rows);
        return;
    }
    in -= rows * first;
    int64_t c = 0;
    while (in >= rows - c) { in -= rows - c; ++c; }
    ti = (uint32_t)(first + c + in);
    tj = (uint32_t)(first + c);
}

__device__ __forceinline__ uint32_t y_xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t nx = 8, xcd = bid % nx, q = nwg / nx, r = nwg % nx;
    const uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / nx;
}

// ---- element access of the plain kernel ------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float y_load(const T *p) { return (float)*p; }
template <> __device__ __forceinline__ float y_load<bf16_t>(const bf16_t *p) { return bf16_to_f32(*p); }
template <> __device__ __forceinline__ float y_load<f16_t>(const f16_t *p) { return f16_to_f32(*p); }
template <typename T> __device__ __forceinline__ void y_store(T *p, float v) { *p = (T)v; }
template <> __device__ __forceinline__ void y_store<bf16_t>(bf16_t *p, float v) { *p = f32_to_bf16(v); }
template <> __device__ __forceinline__ void y_store<f16_t>(f16_t *p, float v) { *p = f32_to_f16(v); }

// plain path: a 16 x 16 block of C per workgroup, the blocks on and below the diagonal; the thread of (r >= c) stores (r, c) and (c, r)
template <typename T>
__global__ __launch_bounds__(256) void sym_generic_kernel(const SymArgs g) {
    uint32_t bi, bj;
    y_tile(blockIdx.x, g.nt, bi, bj);
    const int64_t r = (int64_t)bi * 16 + threadIdx.x / 16, c = (int64_t)bj * 16 + threadIdx.x % 16;
    if (r >= g.M || c > r) return;
    const T *xr = (const T *)g.X + r * g.ldx, *xc = (const T *)g.X + c * g.ldx;
    float acc = 0.f;
    for (int64_t k = 0; k < g.K; ++k) acc = fmaf(y_load<T>(xr + k), y_load<T>(xc + k), acc);
    float v = g.alpha * acc;
    if (g.D && g.beta != 0.f) v += g.beta * y_load<T>((const T *)g.D + r * g.ldd + c);
    if (r == c) v += g.gamma;
    y_store<T>((T *)g.C + r * g.ldc + c, v);
    if (r != c) y_store<T>((T *)g.C + c * g.ldc + r, v);
}

// ---- 16-bit fast path: the staging of gemm_seg.hip's forward kernel, restated -----------------------------------------------------------
template <bool BF> struct YFrag { using type = y_f16x8; };
template <> struct YFrag<true> { using type = y_bf16x8; };

template <bool BF>
__device__ __forceinline__ y_f32x16 y_mfma(typename YFrag<BF>::type a, typename YFrag<BF>::type b, y_f32x16 c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// [128 rows][64 k] image, 128-B rows, 16-B chunk c of row r at chunk position c ^ ((r >> 1) & 7)
__device__ __forceinline__ int y_lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// rows x0 .. x0 + 127 of X, k bytes k0_bytes .. + 127: four LDS-DMA operations a wave
__device__ __forceinline__ void y_stage(const char *gbase, int64_t ld_bytes, int64_t x0, int64_t k0_bytes, char *lds_tile) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row0 = (wid * 4 + i) * 8;
        const int row = row0 + (lane >> 3), pos = lane & 7;
        const int chunk = pos ^ ((row >> 1) & 7);
        const char *src = gbase + (x0 + row) * ld_bytes + k0_bytes + chunk * 16;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(lds_tile + row0 * 128), 16, 0, 0);
    }
}

// The per-lane read addresses of one workgroup's fragments and the four k-steps of one staged tile. BOFF: where the column panel's tile
// lies behind the row panel's - 0 for a diagonal tile, whose two operands are one staged tile.
template <bool BF, int BOFF>
struct YReader {
    using frag_t = typename YFrag<BF>::type;
    int offA[2], offB[2];
    __device__ __forceinline__ YReader() {
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        const int wr = wid >> 1, wc = wid & 1, xl = lane & 31, hl = lane >> 5;
        offA[0] = y_lds_off(wr * 64 + xl, hl); offA[1] = y_lds_off(wr * 64 + 32 + xl, hl);
        offB[0] = y_lds_off(wc * 64 + xl, hl); offB[1] = y_lds_off(wc * 64 + 32 + xl, hl);
    }
    static __device__ __forceinline__ void rd(frag_t &dst, unsigned addr) { asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr) : "memory"); }
    template <int KS>
    __device__ __forceinline__ void read_step(unsigned cur_u, frag_t (&a)[2], frag_t (&b)[2]) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            rd(a[i], cur_u + (unsigned)(offA[i] ^ (KS * 32)));
            rd(b[i], cur_u + BOFF + (unsigned)(offB[i] ^ (KS * 32)));
        }
    }
    static __device__ __forceinline__ void landed(frag_t (&a)[2], frag_t (&b)[2]) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : : "memory");
    }
    static __device__ __forceinline__ void mma(frag_t (&a)[2], frag_t (&b)[2], y_f32x16 (&acc)[2][2]) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = y_mfma<BF>(a[i], b[j], acc[i][j]);
    }
};

// nt >= 1 K tiles through the four-stage ring (gemm_seg.hip's loop: three to four tiles in flight; a wave issues OPS LDS-DMA operations per
// tile - 8, or 4 for a diagonal tile - so vmcnt(2 OPS) = "everything but the two youngest tiles has landed"; past the end the last tile is
// fetched again and never read; one barrier per tile, in front of its last k-step). Returns with nothing in flight.
template <bool DIAG> __device__ __forceinline__ void y_wait_first() {
    if constexpr (DIAG) asm volatile("s_waitcnt vmcnt(12)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(24)\n\ts_barrier" ::: "memory");
}
template <bool DIAG> __device__ __forceinline__ void y_wait_next() {
    if constexpr (DIAG) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(16)\n\ts_barrier" ::: "memory");
}
template <bool BF, bool DIAG, typename Stage>
__device__ __forceinline__ void y_ring(Stage stage, int nt, char *smem, y_f32x16 (&acc)[2][2]) {
    using R = YReader<BF, DIAG ? 0 : Y_TILE_BYTES>;
    using frag_t = typename YFrag<BF>::type;
    const R rd;
    const unsigned smem_u = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    auto clampt = [&](int t) { return t < nt ? t : nt - 1; };
#pragma unroll
    for (int t = 0; t < Y_STAGES; ++t) stage(clampt(t), smem + t * 2 * Y_TILE_BYTES);
    frag_t fa[2][2], fb[2][2];
    y_wait_first<DIAG>(); // tile 0 has landed for everyone
    rd.template read_step<0>(smem_u, fa[0], fb[0]);
    R::landed(fa[0], fb[0]);
    for (int t = 0; t < nt; ++t) {
        const unsigned cur_u = smem_u + (unsigned)((t % Y_STAGES) * 2 * Y_TILE_BYTES), nxt_u = smem_u + (unsigned)(((t + 1) % Y_STAGES) * 2 * Y_TILE_BYTES);
        rd.template read_step<1>(cur_u, fa[1], fb[1]);
        R::mma(fa[0], fb[0], acc);
        R::landed(fa[1], fb[1]);
        rd.template read_step<2>(cur_u, fa[0], fb[0]);
        R::mma(fa[1], fb[1], acc);
        R::landed(fa[0], fb[0]);
        rd.template read_step<3>(cur_u, fa[1], fb[1]);
        R::mma(fa[0], fb[0], acc);
        R::landed(fa[1], fb[1]);
        y_wait_next<DIAG>(); // tile t + 1 has landed for everyone; nobody reads tile t any more
        stage(clampt(t + Y_STAGES), smem + (t % Y_STAGES) * 2 * Y_TILE_BYTES);
        rd.template read_step<0>(nxt_u, fa[0], fb[0]);
        R::mma(fa[1], fb[1], acc);
        R::landed(fa[0], fb[0]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the re-fetched tail tiles: nothing may still be writing LDS afterwards
}

template <bool BF>
__device__ __forceinline__ uint32_t y_pack2(float lo, float hi) {
    if constexpr (BF) return f32x2_to_bf16x2_hw(lo, hi);
    else return (uint32_t)f32_to_f16(lo).x | ((uint32_t)f32_to_f16(hi).x << 16);
}
template <bool BF>
__device__ __forceinline__ void y_unpack8(const uint4 q, float (&f)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint16_t o = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
        f[e] = BF ? bf16_to_f32(bf16_t{o}) : f16_to_f32(f16_t{o});
    }
}

// The 16-bit image of the tile that leaves as rows of C(j, i): element b of row a, 256-B rows, the 16-B chunk b >> 3 at chunk position
// (b >> 3) ^ (a >> 3) - the sixteen lanes that write one element each of sixteen rows (a = 8 m + e) then hit sixteen chunk positions.
__device__ __forceinline__ int y_img_off(int a, int b) { return a * 256 + ((((b >> 3) ^ (a >> 3)) & 15) << 4) + (b & 7) * 2; }

// accumulators -> f32 image -> tail and the one rounding -> C(i, j) and the transposed 16-bit image -> C(j, i). r0 / c0: the tile's first
// row / column (equal for a diagonal tile, which fills the image from its lower triangle and stores the image only).
template <bool BF, bool DIAG>
__device__ __forceinline__ void y_epilogue(const y_f32x16 (&acc)[2][2], char *smem, const SymArgs &g, int64_t r0, int64_t c0) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr = wid >> 1, wc = wid & 1, xl = lane & 31, hl = lane >> 5;
    float *stg = (float *)smem;
    char *img = smem + Y_F32_IMAGE;
    uint16_t *C = (uint16_t *)g.C;
    const uint16_t *D = g.beta != 0.f ? (const uint16_t *)g.D : nullptr;
    __syncthreads(); // nobody reads the ring any more
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                stg[(wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl) * Y_EROW + wc * 64 + j * 32 + xl] = acc[i][j][e];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < Y_BM * Y_BN / 8 / 256; ++r) {
        const int gi = (int)threadIdx.x + 256 * r, row = gi >> 4, c8 = (gi & 15) * 8;
        const float4 lo = *(const float4 *)(stg + row * Y_EROW + c8), hi = *(const float4 *)(stg + row * Y_EROW + c8 + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= g.alpha;
        if (D) {
            float old[8];
            y_unpack8<BF>(*(const uint4 *)(D + (r0 + row) * g.ldd + c0 + c8), old);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += g.beta * old[e];
        }
        if constexpr (DIAG) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c8 + e == row) v[e] += g.gamma;
        }
        const uint32_t w[4] = {y_pack2<BF>(v[0], v[1]), y_pack2<BF>(v[2], v[3]), y_pack2<BF>(v[4], v[5]), y_pack2<BF>(v[6], v[7])};
        if constexpr (!DIAG) *(uint4 *)(C + (r0 + row) * g.ldc + c0 + c8) = uint4{w[0], w[1], w[2], w[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint16_t h = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
            const int c = c8 + e;
            if (!DIAG || c < row) *(uint16_t *)(img + y_img_off(c, row)) = h;
            if (DIAG && c <= row) *(uint16_t *)(img + y_img_off(row, c)) = h;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < Y_BM * Y_BN / 8 / 256; ++r) {
        const int gi = (int)threadIdx.x + 256 * r, row = gi >> 4, c8 = (gi & 15) * 8;
        *(uint4 *)(C + (c0 + row) * g.ldc + r0 + c8) = *(const uint4 *)(img + y_img_off(row, c8));
    }
}

template <bool BF, bool DIAG>
__device__ __forceinline__ void y_tile_product(const SymArgs &g, uint32_t ti, uint32_t tj, char *smem) {
    const int64_t r0 = (int64_t)ti * Y_BM, c0 = (int64_t)tj * Y_BN, ldx_b = g.ldx * 2;
    const char *X = (const char *)g.X;
    y_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    y_ring<BF, DIAG>([&](int t, char *buf) __attribute__((always_inline)) {
        y_stage(X, ldx_b, r0, (int64_t)t * Y_BK * 2, buf);
        if constexpr (!DIAG) y_stage(X, ldx_b, c0, (int64_t)t * Y_BK * 2, buf + Y_TILE_BYTES);
    }, (int)(g.K / Y_BK), smem, acc);
    y_epilogue<BF, DIAG>(acc, smem, g, r0, c0);
}

template <bool BF>
__global__ __launch_bounds__(256) void sym_h_kernel(const SymArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t ti, tj;
    y_tile(y_xcd_remap(blockIdx.x, gridDim.x), g.nt, ti, tj);
    if (ti == tj) y_tile_product<BF, true>(g, ti, tj, smem);
    else y_tile_product<BF, false>(g, ti, tj, smem);
}

bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// [p, p + bytes of an [M, M] matrix with pitch ld) against the same of q
bool overlap(const void *p, int64_t rows_p, int64_t cols_p, int64_t ldp, const void *q, int64_t rows_q, int64_t cols_q, int64_t ldq, int es) {
    if (!p || !q || rows_p == 0 || cols_p == 0 || rows_q == 0 || cols_q == 0) return false;
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + (uintptr_t)((rows_p - 1) * ldp + cols_p) * es;
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)((rows_q - 1) * ldq + cols_q) * es;
    return p0 < q1 && q0 < p1;
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_gemm_sym(int dtype, int64_t M, int64_t K, float alpha, const void *X, int64_t ldx, float beta, const void *D, int64_t ldd, float gamma,
                           void *C, int64_t ldc, void *stream) {
    const char *who = "kf_gemm_sym";
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_BF16 || dtype == KF_F16, KF_ERR_INVALID, "%s: dtype %d not supported (float, half, bfloat16)", who, dtype);
    KF_REQUIRE(M >= 0 && K >= 0, KF_ERR_INVALID, "%s: bad extents M %lld K %lld", who, (long long)M, (long long)K);
    KF_REQUIRE(C && (X || K == 0), KF_ERR_INVALID, "%s: null X or C", who);
    KF_REQUIRE(ldx >= K, KF_ERR_INVALID, "%s: pitch of X %lld < K = %lld", who, (long long)ldx, (long long)K);
    KF_REQUIRE(ldc >= M, KF_ERR_INVALID, "%s: pitch of C %lld < M = %lld", who, (long long)ldc, (long long)M);
    KF_REQUIRE(!D || ldd >= M, KF_ERR_INVALID, "%s: pitch of D %lld < M = %lld", who, (long long)ldd, (long long)M);
    const int es = dtype_size(dtype);
    KF_REQUIRE((uintptr_t)X % es == 0 && (uintptr_t)D % es == 0 && (uintptr_t)C % es == 0, KF_ERR_INVALID, "%s: an operand is not aligned to its element size",
               who);
    KF_REQUIRE(!overlap(C, M, M, ldc, D, M, M, ldd, es), KF_ERR_INVALID, "%s: C overlaps D", who);
    KF_REQUIRE(!overlap(C, M, M, ldc, X, M, K, ldx, es), KF_ERR_INVALID, "%s: C overlaps X", who);
    if (M == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    SymArgs g{};
    g.X = X; g.D = D; g.C = C;
    g.M = M; g.K = K; g.ldx = ldx; g.ldd = ldd; g.ldc = ldc;
    g.alpha = alpha; g.beta = beta; g.gamma = gamma;
    const bool fast = es == 2 && M % Y_BM == 0 && K >= Y_BK && K % Y_BK == 0 && ldx % 8 == 0 && ldc % 8 == 0 && (!D || ldd % 8 == 0) && al16(X) && al16(C) &&
                      al16(D) && M / Y_BM < 65536;
    const int64_t nt = fast ? M / Y_BM : (M + 15) / 16;
    KF_REQUIRE(nt < 65536, KF_ERR_UNSUPPORTED, "%s: M %lld needs %lld tile rows, above one grid", who, (long long)M, (long long)nt);
    g.nt = (uint32_t)nt;
    const unsigned blocks = (unsigned)(nt * (nt + 1) / 2);
    const bool bf = dtype == KF_BF16;
    KF_PROF(fast ? (bf ? "gemm_sym_bf16_mfma" : "gemm_sym_f16_mfma") : "gemm_sym_generic", st);
    if (fast) return with_flags([&](auto BF) { return launch(sym_h_kernel<BF>, dim3(blocks), dim3(256), (size_t)Y_LDS, st, g); }, bf);
    return dtype == KF_F32    ? launch(sym_generic_kernel<float>, dim3(blocks), dim3(256), 0, st, g)
           : dtype == KF_BF16 ? launch(sym_generic_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, g)
                              : launch(sym_generic_kernel<f16_t>, dim3(blocks), dim3(256), 0, st, g);
}
