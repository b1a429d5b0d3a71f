// namespace gpu: chunked linear attention with a scalar per-step decay (kf_linear_attn_fwd / kf_linear_attn_bwd) with autograd - the
// sequence mixer of Mamba-2 (SSD), RetNet, Lightning Attention and scalar-gated linear attention, the linear-time sibling of the
// attention operators of ops.h. No reference counterpart.
#pragma once

#include <optional>

#include "tensor.h"

namespace gpu {

// S_t = exp(g_t) S_{t-1} + k_t v_t^T,  o_t = scale q_t S_t.  q, k, v [B, H, S, D] half or bfloat16, D in {64, 128}; g [B, H, S] float,
// <= 0 (the caller applies -softplus, log sigmoid ...); scale not given: D^-0.5; a given scale goes to the kernels as it is (they refuse
// zero and non-finite values). Operands of any strides are made contiguous. Differentiable in q, k, v and g through one node that keeps
// the four inputs; nothing is read back, so forward and backward can be captured.
Tensor linear_attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, std::optional<float> scale = std::nullopt);

} // namespace gpu
