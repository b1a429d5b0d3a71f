// namespace gpu: per-tensor scaled FP8 (kf_fp8_amax, kf_fp8_quantize, kf_gemm_fp8) with autograd: the Transformer-Engine recipe with
// current scaling. No reference counterpart. FP8 data live in Byte tensors (the ScalarType enum is reference API and gains no member);
// the format travels beside them as KF_FP8_E4M3 / KF_FP8_E5M2.
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

struct Fp8Quantized {
    Tensor q;         // Byte [rows, cols]
    Tensor qt;        // Byte [cols, ceil16(rows)] with zero bytes in the pad columns, or undefined
    Tensor scale_inv; // Float [1] on the device: 2^-e, what a product of q is multiplied by
};

// x [..., cols] in float, half or bfloat16, contiguous or row-pitched: amax on the device, then one pass that writes q (and qt when
// transpose) with scale 2^e, e the largest integer with amax 2^e <= the format's maximum. Nothing is read back.
Fp8Quantized fp8_quantize(const Tensor &x, int fmt, bool transpose);

// [M, N] in out_dtype (float, half, bfloat16) = (scale_inv_a scale_inv_b) a_q [M, K] b_q [N, K]^T. a_q and b_q are Byte, 2-D, unit
// stride along K, with K and their row strides multiples of 16.
Tensor gemm_fp8(const Tensor &a_q, const Tensor &b_q, const Tensor &scale_inv_a, const Tensor &scale_inv_b, int fmt_a, int fmt_b, ScalarType out_dtype);

// y [..., N] = x [..., K] weight [N, K]^T with both operands quantised to e4m3; x's dtype (float, half, bfloat16) throughout. The
// backward quantises dy to e5m2 and keeps only the transposed FP8 copies x_t [K, ceil16(T)] and w_t [K, N] and the two scales.
// K and N must be multiples of 16 (linear_fp8_check_dims raises otherwise); the token count T is any value >= 1.
Tensor linear_fp8(const Tensor &x, const Tensor &weight);
void linear_fp8_check_dims(int64_t K, int64_t N);

} // namespace gpu
