// namespace gpu: per-head QK-norm fused with the rotary embedding (kf_qk_norm_rope_*) with autograd. No reference counterpart: the
// RMS norm over every q and k head that Chameleon, Qwen3, Gemma-3 and OLMo-2 apply between the QKV projection and attention.
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// qkv: the contiguous packed projection [B*S, (H + 2 kv_heads) D] (q heads, then k, then v; kv_heads < 0 means H, 0 a lone q).
// Returns a new packed tensor: every q head (q_weight) and k head (k_weight) normalised, n = x / sqrt(mean(x^2) + eps) * w, and then
// rotated as rope_qkv does, in f32 with ONE rounding; v copied. q_weight, k_weight: [D] of qkv's dtype, or undefined (1, no gradient).
// cos, sin: f32 [P, R/2] with R <= D as for rope_qkv, or both undefined: the norm alone. Autograd to qkv and the weights in ONE launch
// plus the fold of the weight sums; the node keeps qkv, the weights, the tables and the positions - nothing the forward computed.
Tensor qk_norm_rope(const Tensor &qkv, const Tensor &q_weight, const Tensor &k_weight, const Tensor &cos, const Tensor &sin, int64_t B, int64_t S,
                    int64_t H, int64_t kv_heads, const Tensor &positions, bool interleaved, double eps);

} // namespace gpu
