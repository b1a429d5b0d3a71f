// Per-tensor scaled FP8 (include/kfunca_hip.h): kf_fp8_amax and kf_fp8_quantize. OCP encodings (e4m3fn, e5m2), the
// hardware converters v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 behind an explicit clamp, a power-of-two scale from the exponent of amax.
#include <algorithm>

#include "common.h"

namespace kf {
namespace {

constexpr int QT = 64;          // the quantize kernel's tile: 64 rows x 64 columns, one 16-element run per thread
constexpr int QT_PITCH = QT + 4; // bytes per row of the transposed LDS image (16-byte rows would put a column of bytes on one bank)

template <typename T> __device__ __forceinline__ float f8_ld(const T *p);
template <> __device__ __forceinline__ float f8_ld<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float f8_ld<bf16_t>(const bf16_t *p) { return bf16_to_f32(*p); }
template <> __device__ __forceinline__ float f8_ld<f16_t>(const f16_t *p) { return f16_to_f32(*p); }

// 16 consecutive elements of a row as floats: 16-byte loads when all 16 exist and the address allows, else element by element with
// zeros past n (the same values either way)
template <typename T>
__device__ __forceinline__ void f8_load16_vec(const T *p, float (&v)[16]) {
    constexpr int PER = 16 / (int)sizeof(T);
#pragma unroll
    for (int k = 0; k < 16 / PER; ++k) {
        const uint4 w = *(const uint4 *)(p + k * PER);
        T e[PER];
        __builtin_memcpy(e, &w, 16);
#pragma unroll
        for (int j = 0; j < PER; ++j) v[k * PER + j] = f8_ld<T>(e + j);
    }
}
template <typename T>
__device__ __forceinline__ void f8_load16_elem(const T *p, int n, float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = j < n ? f8_ld<T>(p + j) : 0.f;
}
template <typename T>
__device__ __forceinline__ void f8_load16(const T *p, int n, float (&v)[16]) {
    if (n >= 16 && ((uintptr_t)p & 15) == 0) f8_load16_vec<T>(p, v);
    else f8_load16_elem<T>(p, n, v);
}

// the bits of |v| order like the values, every NaN above every number; NaNs become the one quiet NaN so the maximum is one pattern
__device__ __forceinline__ uint32_t f8_abs_bits(float v) {
    const uint32_t b = __float_as_uint(v) & 0x7fffffffu;
    return b > 0x7f800000u ? 0x7fc00000u : b;
}

// *amax = 0 ahead of the partial maxima: a one-lane launch (a 4-byte memset node costs more than the whole reduction of a small matrix)
__global__ void fp8_amax_zero_kernel(unsigned *amax) { *amax = 0u; }

template <typename T>
__global__ __launch_bounds__(256) void fp8_amax_kernel(const T *x, int64_t rows, int64_t cols, int64_t ld, unsigned *amax) {
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    uint32_t m = 0;
    if (c0 < cols) {
        const int n = (int)(cols - c0 < 16 ? cols - c0 : 16);
        // four rows per trip, all their loads issued before the first is used; a row past the end reads the last row again (a maximum
        // does not mind), and the choice between 16-byte and element loads is made once, outside the loop: no load sits behind a branch
        auto walk = [&](auto vec) __attribute__((always_inline)) {
            for (int64_t r = blockIdx.y; r < rows; r += 4 * (int64_t)gridDim.y) {
                float v[4][16];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t rr = r + u * (int64_t)gridDim.y;
                    const T *p = x + (rr < rows ? rr : rows - 1) * ld + c0;
                    if constexpr (decltype(vec)::value) f8_load16_vec<T>(p, v[u]);
                    else f8_load16_elem<T>(p, n, v[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 16; ++j) m = max(m, f8_abs_bits(v[u][j]));
            }
        };
        if (n == 16 && ((uintptr_t)x & 15) == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0) walk(std::true_type{});
        else walk(std::false_type{});
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(amax, m); // one vector atomic per wave; *amax starts at 0 and 0 needs no write
}

template <int FMT> struct F8Fmt;
template <> struct F8Fmt<KF_FP8_E4M3> { static constexpr float max = 448.f; static constexpr int pow = 9; };
template <> struct F8Fmt<KF_FP8_E5M2> { static constexpr float max = 57344.f; static constexpr int pow = 16; };

// e of scale = 2^e: the largest integer with amax 2^e <= 0.875 2^pow. amax = m 2^ex with m in [0.5, 1): e = pow - ex for m <= 0.875,
// one less above it.
__device__ __forceinline__ int f8_scale_exp(float amax, int pow) {
    const uint32_t b = __float_as_uint(amax) & 0x7fffffffu;
    if (b == 0 || b >= 0x7f800000u) return 0;
    int ex;
    const float m = __builtin_frexpf(__uint_as_float(b), &ex);
    int e = pow - ex - (m > 0.875f ? 1 : 0);
    return e < -126 ? -126 : (e > 126 ? 126 : e);
}
__device__ __forceinline__ float f8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); } // e in [-126, 126]

// two values -> two bytes (the first in bits 0..7)
template <int FMT>
__device__ __forceinline__ uint32_t f8_cvt2(float x0, float x1, float scale) {
    constexpr float MAX = F8Fmt<FMT>::max;
    float s0 = x0 * scale, s1 = x1 * scale;
    s0 = s0 > MAX ? MAX : (s0 < -MAX ? -MAX : s0); // comparisons, not fmin / fmax: a NaN passes through
    s1 = s1 > MAX ? MAX : (s1 < -MAX ? -MAX : s1);
    uint32_t w;
    if constexpr (FMT == KF_FP8_E4M3) w = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(s0, s1, 0, false);
    else w = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(s0, s1, 0, false);
    w &= 0xffffu;
    if (s0 != s0) w = (w & 0xff00u) | 0x7fu | ((__float_as_uint(x0) >> 24) & 0x80u);
    if (s1 != s1) w = (w & 0x00ffu) | ((0x7fu | ((__float_as_uint(x1) >> 24) & 0x80u)) << 8);
    return w;
}

// One block: a 64 x 64 tile of x. Thread t owns row t / 4, columns 16 (t % 4) .. + 15: it reads them once, converts, stores its 16 bytes of
// q, and leaves them in the transposed LDS image; then it owns column t / 4 of the tile and rows 16 (t % 4) .. + 15 and stores those 16
// bytes of qt. A row past `rows` is zero in the image: the 16-row groups of qt end at ceil16(rows), which is its zero pad.
template <typename T, int FMT>
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const T *x, int64_t rows, int64_t cols, int64_t ld, const float *amax, uint8_t *q, int64_t ldq,
                                                           uint8_t *qt, int64_t ldqt, float *scale_inv, int64_t tiles_c) {
    __shared__ __attribute__((aligned(16))) uint8_t img[QT * QT_PITCH]; // [column][row]
    const int e = f8_scale_exp(*amax, F8Fmt<FMT>::pow);
    const float scale = f8_pow2(e);
    if (blockIdx.x == 0 && threadIdx.x == 0) *scale_inv = f8_pow2(-e);
    if (rows == 0 || cols == 0) return;
    const int64_t r0 = (int64_t)(blockIdx.x / tiles_c) * QT, c0 = (int64_t)(blockIdx.x % tiles_c) * QT;
    const int tr = threadIdx.x >> 2, tg = (threadIdx.x & 3) * 16;
    {
        const int64_t r = r0 + tr, c = c0 + tg;
        const int n = r < rows && c < cols ? (int)(cols - c < 16 ? cols - c : 16) : 0;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (n > 0) {
            float v[16];
            f8_load16<T>(x + r * ld + c, n, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = f8_cvt2<FMT>(v[4 * j], v[4 * j + 1], scale) | (f8_cvt2<FMT>(v[4 * j + 2], v[4 * j + 3], scale) << 16);
            uint8_t *dst = q + r * ldq + c;
            if (n == 16 && ((uintptr_t)dst & 15) == 0) {
                *(uint4 *)dst = uint4{w[0], w[1], w[2], w[3]};
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j < n) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
            }
        }
        if (qt) {
#pragma unroll
            for (int j = 0; j < 16; ++j) img[(tg + j) * QT_PITCH + tr] = (uint8_t)(w[j >> 2] >> (8 * (j & 3))); // columns past cols: zeros, never stored
        }
    }
    if (!qt) return;
    __syncthreads();
    const int64_t c = c0 + tr, rg = r0 + tg; // column of x = row of qt; its 16-row group
    if (c < cols && rg < rows) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = *(const uint32_t *)(img + tr * QT_PITCH + tg + 4 * j);
        uint8_t *dst = qt + c * ldqt + rg;
        if (((uintptr_t)dst & 15) == 0) {
            *(uint4 *)dst = uint4{w[0], w[1], w[2], w[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) dst[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

int fp8_in_check(const char *who, int dtype, int64_t rows, int64_t cols, int64_t ld, const void *x) {
    KF_REQUIRE(dtype == KF_F32 || dtype == KF_F16 || dtype == KF_BF16, KF_ERR_INVALID, "%s: dtype %d is not KF_F32, KF_F16 or KF_BF16", who, dtype);
    KF_REQUIRE(rows >= 0 && cols >= 0, KF_ERR_INVALID, "%s: negative extent: rows %lld, cols %lld", who, (long long)rows, (long long)cols);
    KF_REQUIRE(rows < ((int64_t)1 << 40) && cols < ((int64_t)1 << 40), KF_ERR_INVALID, "%s: extent beyond 2^40: rows %lld, cols %lld", who, (long long)rows,
               (long long)cols);
    KF_REQUIRE(ld >= cols, KF_ERR_INVALID, "%s: ld %lld is below cols %lld", who, (long long)ld, (long long)cols);
    KF_REQUIRE(x, KF_ERR_INVALID, "%s: null x", who);
    KF_REQUIRE((uintptr_t)x % dtype_size(dtype) == 0, KF_ERR_INVALID, "%s: x is not aligned to its element", who);
    return KF_OK;
}

} // namespace
} // namespace kf

using namespace kf;

extern "C" int kf_fp8_amax(int dtype, int64_t rows, int64_t cols, int64_t ld, const void *x, float *amax, void *stream) {
    const int rc = fp8_in_check("kf_fp8_amax", dtype, rows, cols, ld, x);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(amax, KF_ERR_INVALID, "kf_fp8_amax: null amax");
    KF_REQUIRE((uintptr_t)amax % 4 == 0, KF_ERR_INVALID, "kf_fp8_amax: amax is not aligned to 4 bytes");
    const int64_t gx = (cols + 256 * 16 - 1) / (256 * 16);
    KF_REQUIRE(gx < ((int64_t)1 << 31), KF_ERR_INVALID, "kf_fp8_amax: cols %lld is beyond the grid", (long long)cols);
    hipStream_t st = as_stream(stream);
    KF_PROF("fp8_amax", st);
    unsigned *out = reinterpret_cast<unsigned *>(amax);
    const int rc0 = launch(fp8_amax_zero_kernel, dim3(1), dim3(1), 0, st, out);
    if (rc0 != KF_OK || rows == 0 || cols == 0) return rc0;
    const int64_t want = (4096 + gx - 1) / gx; // about 4096 blocks in all: every block walks rows / gy rows of its column strip
    const dim3 grid((unsigned)gx, (unsigned)std::min<int64_t>(rows, std::min<int64_t>(want, 65535)));
    switch (dtype) {
    case KF_F32: return launch(fp8_amax_kernel<float>, grid, dim3(256), 0, st, (const float *)x, rows, cols, ld, out);
    case KF_F16: return launch(fp8_amax_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t *)x, rows, cols, ld, out);
    default: return launch(fp8_amax_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t *)x, rows, cols, ld, out);
    }
}

template <typename T>
static int fp8_quantize_run(int fmt, dim3 grid, hipStream_t st, const void *x, int64_t rows, int64_t cols, int64_t ld, const float *amax, void *q, int64_t ldq,
                            void *qt, int64_t ldqt, float *scale_inv, int64_t tiles_c) {
    if (fmt == KF_FP8_E4M3)
        return launch(fp8_quantize_kernel<T, KF_FP8_E4M3>, grid, dim3(256), 0, st, (const T *)x, rows, cols, ld, amax, (uint8_t *)q, ldq, (uint8_t *)qt, ldqt,
                      scale_inv, tiles_c);
    return launch(fp8_quantize_kernel<T, KF_FP8_E5M2>, grid, dim3(256), 0, st, (const T *)x, rows, cols, ld, amax, (uint8_t *)q, ldq, (uint8_t *)qt, ldqt,
                  scale_inv, tiles_c);
}

extern "C" int kf_fp8_quantize(int dtype, int fmt, int64_t rows, int64_t cols, int64_t ld, const void *x, const float *amax, void *q, int64_t ldq, void *qt,
                               int64_t ldqt, float *scale_inv, void *stream) {
    const int rc = fp8_in_check("kf_fp8_quantize", dtype, rows, cols, ld, x);
    if (rc != KF_OK) return rc;
    KF_REQUIRE(fmt == KF_FP8_E4M3 || fmt == KF_FP8_E5M2, KF_ERR_INVALID, "kf_fp8_quantize: format %d is not KF_FP8_E4M3 or KF_FP8_E5M2", fmt);
    KF_REQUIRE(amax && q && scale_inv, KF_ERR_INVALID, "kf_fp8_quantize: null amax, q or scale_inv");
    KF_REQUIRE((uintptr_t)amax % 4 == 0 && (uintptr_t)scale_inv % 4 == 0, KF_ERR_INVALID, "kf_fp8_quantize: amax or scale_inv is not aligned to 4 bytes");
    KF_REQUIRE(ldq >= cols, KF_ERR_INVALID, "kf_fp8_quantize: ldq %lld is below cols %lld", (long long)ldq, (long long)cols);
    const int64_t rows16 = (rows + 15) / 16 * 16;
    KF_REQUIRE(!qt || ldqt >= rows16, KF_ERR_INVALID, "kf_fp8_quantize: ldqt %lld is below ceil16(rows) = %lld", (long long)ldqt, (long long)rows16);
    const int64_t tiles_c = std::max<int64_t>((cols + QT - 1) / QT, 1), tiles = std::max<int64_t>((rows + QT - 1) / QT, 1) * tiles_c;
    KF_REQUIRE(tiles < ((int64_t)1 << 31), KF_ERR_INVALID, "kf_fp8_quantize: %lld tiles are beyond the grid", (long long)tiles);
    hipStream_t st = as_stream(stream);
    KF_PROF("fp8_quantize", st);
    const dim3 grid((unsigned)(rows == 0 || cols == 0 ? 1 : tiles)); // an empty matrix still has a scale: one block writes 2^0
    switch (dtype) {
    case KF_F32: return fp8_quantize_run<float>(fmt, grid, st, x, rows, cols, ld, amax, q, ldq, qt, ldqt, scale_inv, tiles_c);
    case KF_F16: return fp8_quantize_run<f16_t>(fmt, grid, st, x, rows, cols, ld, amax, q, ldq, qt, ldqt, scale_inv, tiles_c);
    default: return fp8_quantize_run<bf16_t>(fmt, grid, st, x, rows, cols, ld, amax, q, ldq, qt, ldqt, scale_inv, tiles_c);
    }
}
