// namespace gpu: rotary position embeddings (kf_rope, kf_rope_table) with autograd. No reference counterpart: the position signal
// of Llama / Mistral / Qwen / GPT-NeoX-family attention, applied to q and k between the QKV projection and attention.
#pragma once

#include <cstdint>
#include <utility>

#include "tensor.h"

namespace gpu {

// (cos, sin): f32 [max_positions, rotary_dim / 2] on `device`, cos(p base^(-2i/R)) with the angle in f64 (kf_rope_table)
std::pair<Tensor, Tensor> rope_table(int64_t max_positions, int64_t rotary_dim, double base, int device);
// qkv: the contiguous packed projection [B*S, (H + 2 kv_heads) D] (q heads, then k, then v; kv_heads < 0 means H). Returns a new packed
// tensor with the q and k heads rotated and v copied, in ONE launch; its backward is ONE inverse launch over the packed gradient.
// cos, sin: f32 [P, R/2] with R <= D (R < D rotates the leading R dims of each head); positions: undefined (p = s) or Long with B*S
// elements on qkv's device, in token order (b*S + s), any strides. The tables get no gradient.
Tensor rope_qkv(const Tensor &qkv, const Tensor &cos, const Tensor &sin, int64_t B, int64_t S, int64_t H, int64_t kv_heads,
                const Tensor &positions, bool interleaved);
// x: [B, H, S, D] with any strides and a unit D stride. Returns a contiguous [B, H, S, D] result, with autograd to x.
Tensor rope(const Tensor &x, const Tensor &cos, const Tensor &sin, const Tensor &positions, bool interleaved);

} // namespace gpu
