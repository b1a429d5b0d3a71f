// namespace gpu: the gated delta rule (kf_delta_rule_*) - the sequence mixer of Gated DeltaNet and, without the gate, DeltaNet: the
// sibling of linear_attn.h whose every step reads the state before it writes it - and its token-by-token recurrence for generation.
// Forward only: the backward is not implemented yet, so the results carry no gradient node. No reference counterpart.
#pragma once

#include <optional>
#include <utility>

#include "tensor.h"

namespace gpu {

// S' = exp(g_t) S_{t-1},  u_t = beta_t (v_t - k_t S'),  S_t = S' + k_t^T u_t,  o_t = scale q_t S_t.  q, k, v [B, H, S, D] half or
// bfloat16, D in {64, 128}; g [B, H, S] float, <= 0, or undefined (no decay); beta [B, H, S] float; the caller normalises k. scale not
// given: D^-0.5. Operands of any strides are made contiguous. S_0 is initial_state (Float [B, H, D, D]; undefined: zero); with
// return_state the second tensor is S_T, else it is undefined. The workspace comes from the caching allocator. Nothing is read back.
std::pair<Tensor, Tensor> gated_delta_rule(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &beta,
                                           std::optional<float> scale = std::nullopt, const Tensor &initial_state = Tensor(), bool return_state = false);

// T steps of the recurrence on `state` (Float [B, H, D, D], contiguous, updated in place): q, k, v [B, H, T, D], g (or undefined) and
// beta [B, H, T] -> o [B, H, T, D]. The generation path after a prefill with return_state.
Tensor gated_delta_rule_step(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &g, const Tensor &beta, Tensor &state,
                             std::optional<float> scale = std::nullopt);

} // namespace gpu
