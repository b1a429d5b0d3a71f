// namespace gpu: the expert product of a mixture-of-experts layer (kf_segment_offsets, kf_gemm_segmented, kf_gemm_segmented_wgrad) with
// autograd. No reference counterpart. The routing stays with the operators that exist: softmax (the router's distribution), topk (each
// token's experts), the stable sort of the flattened expert ids (its positions are the permutation), embedding (the row gather by that
// permutation, whose backward is the reproducible index-add), expert_linear, glu, expert_linear, and a gather by the inverse permutation.
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// sorted_ids: Long, ascending expert ids (the keys a stable sort returns). The result is Long [num_experts + 1] on the same device:
// offsets[e] = the number of ids < e, so expert e owns the sorted rows offsets[e] .. offsets[e + 1]; ids outside [0, num_experts) fall
// outside [offsets[0], offsets[num_experts]) and their rows are dropped by expert_linear. Nothing is read back to the host.
Tensor segment_offsets(const Tensor &sorted_ids, int64_t num_experts);

// x [T, Din] (contiguous or row-pitched), w [E, Din, Dout] contiguous, offsets Long [E + 1] on the device: y[r, :] = x[r, :] w[e] for
// offsets[e] <= r < offsets[e + 1]; a row no expert covers is zero, and so is its gradient. float, half or bfloat16. Differentiable in
// x (dx = the same product of dy with w[e]^T) and w (dw[e] = x[seg_e]^T dy[seg_e], zero for an empty expert); offsets gets no gradient.
// A bucketed weight whose gradient starts empty takes dw straight into its bucket slot, as gemm does. Scratch comes from the allocator.
Tensor expert_linear(const Tensor &x, const Tensor &w, const Tensor &offsets);

} // namespace gpu
