// namespace gpu: the causal depthwise conv1d (short convolution) of kf_causal_conv1d_* with autograd and a carried state - the operator
// Mamba-2, Gated DeltaNet and their kin put in front of the recurrence of linear_attn.h - and its decode step. No reference counterpart.
#pragma once

#include <string>
#include <utility>

#include "tensor.h"

namespace gpu {

// y[b, t, c] = act(bias[c] + sum_j weight[j, c] z[b, t + j, c]), z = initial_state (K - 1 rows; undefined: zeros) then x along time.
// x [B, S, C] float, half or bfloat16; weight [K, C] tap-major with weight[K - 1] on the current token, K in {2, 3, 4}; bias [C] or
// undefined; activation "" or "silu"; C a multiple of the 16-byte pack (8 elements of 16 bits, 4 floats). x may be a last-dimension
// slice of a wider contiguous tensor: its row stride goes to the kernel and no copy is made (when the stride is whole packs and the
// base 16-byte aligned; anything else goes through dense()). With return_state the second tensor is the last K - 1 rows of z, [B, K - 1, C]
// in the dtype of x (copies: exact), else it is undefined. A sequence cut into segments chained through the state gives the bits of
// the whole. Differentiable in x, weight, bias and initial_state; y and the returned state each get a node that keeps the inputs.
std::pair<Tensor, Tensor> causal_conv1d(const Tensor &x, const Tensor &weight, const Tensor &bias = Tensor(), const std::string &activation = "",
                                        const Tensor &initial_state = Tensor(), bool return_state = false);

// The same for T <= KF_CONV1D_STEP_MAX new tokens on `state` ([B, K - 1, C], contiguous, updated in place): x [B, T, C] -> y [B, T, C].
// The generation path after a prefill with return_state; not differentiable.
Tensor causal_conv1d_step(const Tensor &x, const Tensor &weight, const Tensor &bias, Tensor &state, const std::string &activation = "");

} // namespace gpu
