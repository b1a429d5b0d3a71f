// kf_gemm_fp8 (include/kfunca_hip.h): C = (sa sb) A[M, K] B[N, K]^T on v_mfma_scale_f32_16x16x128_f8f6f4 with every
// E8M0 block scale 1.0 (0x7f), the two per-tensor scales applied once in the epilogue. 128 x 128 block tile, BK = 128 bytes, four waves
// of 64 x 64, both operands staged by 16-byte LDS-DMA through buffer descriptors whose range check zero-fills the K tail and the ragged
// M / N edges (FP8 zero is 0x00), two LDS buffers in one __shared__ array.
#include "common.h"

namespace kf {
namespace {

typedef __attribute__((ext_vector_type(4))) int q_i32x4;
typedef __attribute__((ext_vector_type(8))) int q_i32x8;
typedef __attribute__((ext_vector_type(4))) float q_f32x4;

constexpr int Q_BM = 128, Q_BN = 128, Q_BK = 128;
constexpr int Q_TILE = Q_BM * Q_BK;   // 16 KiB per operand tile
constexpr int Q_LDS = 2 * 2 * Q_TILE; // [2 buffers][A tile | B tile]
constexpr int Q_E8M0_ONE = 0x7f7f7f7f;
constexpr uint32_t Q_GROUP = 8;

struct Fp8GemmArgs {
    const char *A, *B;
    void *C;
    const float *sa, *sb;
    int64_t M, N, K, lda, ldb, ldc;
    int odt;
};

// gemm.hip's block order, restated: consecutive hardware ids go to different XCDs, so logical ids are dealt XCD-major (bijective for
// any count), and the logical ids walk groups of Q_GROUP tile rows column by column (an XCD's tiles share A and B panels in its L2)
__device__ __forceinline__ uint32_t q_xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t nx = 8, xcd = bid % nx, q = nwg / nx, r = nwg % nx;
    const uint32_t base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + bid / nx;
}
__device__ __forceinline__ void q_grouped_tile(uint32_t id, uint32_t tiles_m, uint32_t tiles_n, uint32_t &tm, uint32_t &tn) {
    const uint32_t per = Q_GROUP * tiles_n, grp = id / per, first = grp * Q_GROUP;
    const uint32_t rows = min(Q_GROUP, tiles_m - first), in = id - grp * per;
    tm = first + in % rows;
    tn = in / rows;
}

// LDS image of a [128 rows][128 k-bytes] tile, gemm.hip's h_lds_off: 128-B rows, the 16-B chunk c of row r at chunk position
// c ^ ((r >> 1) & 7), so the 16 rows a lane group reads at one logical chunk lie on 16 different 16-B slots of the 256-B bank row.
__device__ __forceinline__ int q_lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// One wave-instruction moves 8 rows x 128 B; 4 waves x 4 instructions cover the tile (h_stage's partition, the swizzle on the SOURCE
// chunk). The descriptor starts at the tile's first row and ends with the last valid byte of its last valid row; a lane whose row lies
// past the matrix or whose chunk starts at or past K asks for offset `oob` = num_records, and the range check writes 16 zero bytes.
__device__ __forceinline__ void q_stage(__amdgpu_buffer_rsrc_t rs, uint32_t oob, int rows_valid, uint32_t ld, uint32_t K, uint32_t k0, char *lds_tile) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave-uniform to the compiler: the LDS base goes to M0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row0 = (wid * 4 + i) * 8;
        const int row = row0 + (lane >> 3), pos = lane & 7;
        const uint32_t kb = k0 + (uint32_t)((pos ^ ((row >> 1) & 7)) << 4);
        const uint32_t voff = row < rows_valid && kb < K ? (uint32_t)row * ld + kb : oob;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(lds_tile + row0 * 128), 16, (int)voff, 0, 0, 0);
    }
}

template <int FA, int FB>
__device__ __forceinline__ q_f32x4 q_mfma(q_i32x8 b, q_i32x8 a, q_f32x4 c) {
    // D = (B fragment) x (A fragment): a C^T tile, so a lane holds four CONSECUTIVE columns of one row of C. The first operand's format
    // is cbsz, the second's blgp.
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b, a, c, FB, FA, 0, Q_E8M0_ONE, 0, Q_E8M0_ONE);
}

template <typename T> __device__ __forceinline__ void q_store4(T *p, const float (&v)[4], int n);
template <> __device__ __forceinline__ void q_store4<float>(float *p, const float (&v)[4], int n) {
    if (n == 4 && ((uintptr_t)p & 15) == 0) {
        *(float4 *)p = float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = v[e];
    }
}
template <> __device__ __forceinline__ void q_store4<bf16_t>(bf16_t *p, const float (&v)[4], int n) {
    bf16_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = f32_to_bf16(v[e]);
    if (n == 4 && ((uintptr_t)p & 7) == 0) {
        uint2 w;
        __builtin_memcpy(&w, h, 8);
        *(uint2 *)p = w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = h[e];
    }
}
template <> __device__ __forceinline__ void q_store4<f16_t>(f16_t *p, const float (&v)[4], int n) {
    f16_t h[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = f32_to_f16(v[e]);
    if (n == 4 && ((uintptr_t)p & 7) == 0) {
        uint2 w;
        __builtin_memcpy(&w, h, 8);
        *(uint2 *)p = w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = h[e];
    }
}

template <int FA, int FB>
__global__ __launch_bounds__(256) void gemm_fp8_kernel(const Fp8GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[]; // the one LDS object: [2 buffers][A tile | B tile]
    const uint32_t tiles_m = (uint32_t)((g.M + Q_BM - 1) / Q_BM), tiles_n = (uint32_t)((g.N + Q_BN - 1) / Q_BN);
    uint32_t tm, tn;
    q_grouped_tile(q_xcd_remap(blockIdx.x, gridDim.x), tiles_m, tiles_n, tm, tn);
    const int64_t m0 = (int64_t)tm * Q_BM, n0 = (int64_t)tn * Q_BN;
    const int rows_a = (int)(g.M - m0 < Q_BM ? g.M - m0 : Q_BM), rows_b = (int)(g.N - n0 < Q_BN ? g.N - n0 : Q_BN);
    const uint32_t K = (uint32_t)g.K, lda = (uint32_t)g.lda, ldb = (uint32_t)g.ldb;
    const uint32_t nrec_a = (uint32_t)(rows_a - 1) * lda + K, nrec_b = (uint32_t)(rows_b - 1) * ldb + K; // <= 2^31: the leading dimensions are at most 2^24
    // the descriptors' inputs through readfirstlane: block-uniform by construction, and this way to the compiler too (it would
    // otherwise wrap every LDS-DMA in a loop over the descriptor values it cannot prove equal)
    auto rsrc = [](const char *base, uint32_t bytes) __attribute__((always_inline)) {
        const uint64_t p = (uint64_t)(uintptr_t)base;
        const uint64_t u = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p) |
                           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32)) << 32);
        return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)u, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rs_a = rsrc(g.A + m0 * g.lda, nrec_a), rs_b = rsrc(g.B + n0 * g.ldb, nrec_b);

    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int fr = lane & 15, fg = lane >> 4;

    q_f32x4 acc[4][4]; // [n tile j][m tile i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = q_f32x4{0.f, 0.f, 0.f, 0.f};

    auto stage_tile = [&](int t, char *buf) __attribute__((always_inline)) {
        q_stage(rs_a, nrec_a, rows_a, lda, K, (uint32_t)t * Q_BK, buf);
        q_stage(rs_b, nrec_b, rows_b, ldb, K, (uint32_t)t * Q_BK, buf + Q_TILE);
    };
    // Lane (fr, fg) takes bytes 32 fg .. 32 fg + 31 of its row for BOTH operands: whatever k order the instruction gives those bytes
    // inside its 128, A and B agree on it, which is all the product needs.
    const unsigned smem_u = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char *)smem;
    unsigned offA[4][2], offB[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            offA[i][h] = (unsigned)q_lds_off(wr * 64 + i * 16 + fr, 2 * fg + h);
            offB[i][h] = (unsigned)(Q_TILE + q_lds_off(wc * 64 + i * 16 + fr, 2 * fg + h));
        }
    // The fragment reads are inline asm: a read the compiler can see gets a vmcnt(0) in front of it while the next tile's LDS-DMA is in
    // flight (it cannot tell the two buffers apart), which would put every tile's fetch in the open.
    auto rd = [&](q_i32x4 &dst, unsigned addr) __attribute__((always_inline)) { asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr) : "memory"); };

    const int nt = (int)((g.K + Q_BK - 1) / Q_BK);
    stage_tile(0, smem);
    for (int t = 0; t < nt; ++t) {
        // tile t has landed for its issuing wave (vmcnt) and then for everyone (barrier); every wave has also consumed its reads of
        // tile t - 1 (the lgkmcnt(0) in front of its MFMAs), so that buffer can take tile t + 1 now, under this tile's MFMAs
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nt) stage_tile(t + 1, smem + ((t + 1) & 1) * 2 * Q_TILE);
        const unsigned cur = smem_u + (unsigned)((t & 1) * 2 * Q_TILE);
        q_i32x4 ra[4][2], rb[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                rd(ra[i][h], cur + offA[i][h]);
                rd(rb[i][h], cur + offB[i][h]);
            }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(ra[0][0]), "+v"(ra[0][1]), "+v"(ra[1][0]), "+v"(ra[1][1]), "+v"(ra[2][0]), "+v"(ra[2][1]), "+v"(ra[3][0]), "+v"(ra[3][1]),
                       "+v"(rb[0][0]), "+v"(rb[0][1]), "+v"(rb[1][0]), "+v"(rb[1][1]), "+v"(rb[2][0]), "+v"(rb[2][1]), "+v"(rb[3][0]), "+v"(rb[3][1])
                     :
                     : "memory");
        q_i32x8 fa[4], fb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = __builtin_shufflevector(ra[i][0], ra[i][1], 0, 1, 2, 3, 4, 5, 6, 7);
            fb[i] = __builtin_shufflevector(rb[i][0], rb[i][1], 0, 1, 2, 3, 4, 5, 6, 7);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = q_mfma<FA, FB>(fb[j], fa[i], acc[j][i]);
    }

    // the scales are read here, not at the top: an ordinary load beside the LDS-DMA would have the compiler drain the pipeline for it
    const float s = *g.sa * *g.sb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + wr * 64 + i * 16 + fr;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + wc * 64 + j * 16 + 4 * fg;
            if (n >= g.N) continue;
            const int cnt = (int)(g.N - n < 4 ? g.N - n : 4);
            const float v[4] = {s * acc[j][i][0], s * acc[j][i][1], s * acc[j][i][2], s * acc[j][i][3]};
            if (g.odt == KF_F32) q_store4<float>((float *)g.C + m * g.ldc + n, v, cnt);
            else if (g.odt == KF_BF16) q_store4<bf16_t>((bf16_t *)g.C + m * g.ldc + n, v, cnt);
            else q_store4<f16_t>((f16_t *)g.C + m * g.ldc + n, v, cnt);
        }
    }
}

bool fmt_ok(int f) { return f == KF_FP8_E4M3 || f == KF_FP8_E5M2; }

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_gemm_fp8(int fmt_a, int fmt_b, int out_dtype, int64_t M, int64_t N, int64_t K, const void *A, int64_t lda, const void *B, int64_t ldb,
                           const float *scale_inv_a, const float *scale_inv_b, void *C, int64_t ldc, void *stream) {
    KF_REQUIRE(fmt_ok(fmt_a) && fmt_ok(fmt_b), KF_ERR_INVALID, "kf_gemm_fp8: format (%d, %d) is not KF_FP8_E4M3 or KF_FP8_E5M2", fmt_a, fmt_b);
    KF_REQUIRE(out_dtype == KF_F32 || out_dtype == KF_BF16 || out_dtype == KF_F16, KF_ERR_INVALID, "kf_gemm_fp8: out_dtype %d is not KF_F32, KF_BF16 or KF_F16",
               out_dtype);
    KF_REQUIRE(M >= 0 && N >= 0, KF_ERR_INVALID, "kf_gemm_fp8: negative extent: M %lld, N %lld", (long long)M, (long long)N);
    KF_REQUIRE(K > 0 && K % 16 == 0, KF_ERR_INVALID, "kf_gemm_fp8: K %lld is not a positive multiple of 16", (long long)K);
    KF_REQUIRE(lda % 16 == 0 && ldb % 16 == 0, KF_ERR_INVALID, "kf_gemm_fp8: lda %lld and ldb %lld must be multiples of 16", (long long)lda, (long long)ldb);
    KF_REQUIRE(lda >= K && ldb >= K, KF_ERR_INVALID, "kf_gemm_fp8: lda %lld or ldb %lld is below K %lld", (long long)lda, (long long)ldb, (long long)K);
    KF_REQUIRE(lda <= (1 << 24) && ldb <= (1 << 24), KF_ERR_INVALID, "kf_gemm_fp8: lda %lld or ldb %lld is beyond 2^24", (long long)lda, (long long)ldb);
    KF_REQUIRE(ldc >= N, KF_ERR_INVALID, "kf_gemm_fp8: ldc %lld is below N %lld", (long long)ldc, (long long)N);
    KF_REQUIRE(A && B && C && scale_inv_a && scale_inv_b, KF_ERR_INVALID, "kf_gemm_fp8: null A, B, C, scale_inv_a or scale_inv_b");
    KF_REQUIRE((uintptr_t)A % 16 == 0 && (uintptr_t)B % 16 == 0, KF_ERR_INVALID, "kf_gemm_fp8: A and B must be 16-byte aligned");
    KF_REQUIRE((uintptr_t)C % dtype_size(out_dtype) == 0 && (uintptr_t)scale_inv_a % 4 == 0 && (uintptr_t)scale_inv_b % 4 == 0, KF_ERR_INVALID,
               "kf_gemm_fp8: C or a scale is not aligned to its element");
    const int64_t tiles = ((M + Q_BM - 1) / Q_BM) * ((N + Q_BN - 1) / Q_BN);
    KF_REQUIRE(M < ((int64_t)1 << 38) && N < ((int64_t)1 << 38) && tiles < ((int64_t)1 << 31), KF_ERR_INVALID, "kf_gemm_fp8: %lld x %lld is beyond the grid",
               (long long)M, (long long)N);
    if (M == 0 || N == 0) return KF_OK;
    hipStream_t st = as_stream(stream);
    KF_PROF("gemm_fp8", st);
    const Fp8GemmArgs g{(const char *)A, (const char *)B, C, scale_inv_a, scale_inv_b, M, N, K, lda, ldb, ldc, out_dtype};
    const dim3 grid((unsigned)tiles), block(256);
    if (fmt_a == KF_FP8_E4M3)
        return fmt_b == KF_FP8_E4M3 ? launch(gemm_fp8_kernel<KF_FP8_E4M3, KF_FP8_E4M3>, grid, block, Q_LDS, st, g)
                                    : launch(gemm_fp8_kernel<KF_FP8_E4M3, KF_FP8_E5M2>, grid, block, Q_LDS, st, g);
    return fmt_b == KF_FP8_E4M3 ? launch(gemm_fp8_kernel<KF_FP8_E5M2, KF_FP8_E4M3>, grid, block, Q_LDS, st, g)
                                : launch(gemm_fp8_kernel<KF_FP8_E5M2, KF_FP8_E5M2>, grid, block, Q_LDS, st, g);
}
