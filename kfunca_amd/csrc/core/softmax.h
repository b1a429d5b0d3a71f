// namespace gpu: row softmax and log_softmax (kf_softmax_fwd, kf_softmax_bwd) with autograd. No reference counterpart: the
// distribution behind an MoE router, sampling with a temperature, distillation against log-probabilities, a contrastive head.
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// softmax(scale * x) / log_softmax(scale * x) over dimension dim (negative: from the end) of a float, half or bfloat16 tensor; scale
// (1 / temperature) finite and > 0. Over the last dimension an input with a unit stride there and one uniform row stride over the
// flattened leading dims (a column slice, a split part) is read in place through its leading dimension; anything else is made dense
// first. Any other dim is moved last (permute, contiguous) and the result is permuted back. The result is a new tensor; its grad
// function keeps the RESULT, not x, and the backward is ONE kf_softmax_bwd launch.
Tensor softmax(const Tensor &x, int64_t dim = -1, float scale = 1.0f);
Tensor log_softmax(const Tensor &x, int64_t dim = -1, float scale = 1.0f);

} // namespace gpu
