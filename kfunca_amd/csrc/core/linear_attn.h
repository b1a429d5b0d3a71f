// namespace gpu: chunked linear attention with a scalar per-step decay (kf_linear_attn_*) with autograd - the sequence mixer of
// Mamba-2 (SSD), RetNet, Lightning Attention and scalar-gated linear attention, the linear-time sibling of the attention operators of
// ops.h - and its token-by-token recurrence for generation. No reference counterpart.
#pragma once

#include <optional>
#include <utility>

#include "tensor.h"

namespace gpu {

// S_t = exp(g_t) S_{t-1} + k_t v_t^T,  o_t = scale q_t S_t.  q, k, v [B, H, S, D] half or bfloat16, D in {64, 128}; g [B, H, S] float,
// <= 0 (the caller applies -softplus, log sigmoid ...); scale not given: D^-0.5; a given scale goes to the kernels as it is (they refuse
// zero and non-finite values). Operands of any strides are made contiguous. S_0 is initial_state (Float [B, H, D, D]; undefined: zero);
// with return_state the second tensor is S_T (Float [B, H, D, D]), else it is undefined. A sequence cut into segments chained through
// the state gives the results and the gradients of the whole. Differentiable in q, k, v, g and initial_state; o and the returned state
// each get a node that keeps the inputs, and when both carry a gradient the backward kernels run once for each. Nothing is read back.
// Without a state on either side the call is the stateless kernels', bit for bit.
std::pair<Tensor, Tensor> linear_attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, std::optional<float> scale = std::nullopt,
                                           const Tensor &initial_state = Tensor(), bool return_state = false);

// T steps of the recurrence on `state` (Float [B, H, D, D], contiguous, updated in place): q, k, v [B, H, T, D], g [B, H, T] -> o
// [B, H, T, D]. The generation path after a prefill with return_state; not differentiable.
Tensor linear_attention_step(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, Tensor &state, std::optional<float> scale = std::nullopt);

} // namespace gpu
