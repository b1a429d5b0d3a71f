// namespace gpu: the chunked linear + cross-entropy loss (gpu::linear_cross_entropy, declared in ops.h) over kf_gemm_ex, kf_ce_fused_rows,
// kf_ce_fused_reduce and kf_scale_cast. No reference counterpart: the LM head and its loss without the [T, V] logits.
//
// The tokens are walked in chunks of chunk_rows rows. Per chunk: logits_c = x_c weight^T into an f32 buffer (the unrounded accumulators
// behind 16-bit operands), ONE kf_ce_fused_rows call that turns the buffer into the rows' losses and the UNSCALED gradient dlogits_c in the
// operands' dtype, then dX_c = dlogits_c weight into its slice of dX and dWacc += dlogits_c^T x_c into an f32 [V, d] accumulator. The two
// chunk buffers are reused by every chunk and freed before the call returns; what outlives it is dX, dWacc and the count of rows not
// ignored, held by the backward function, whose backward(g) is two kf_scale_cast calls (g / count onto dX in place and onto dWacc -> dW).
// Because they scale in place, the function refuses a second backward over the same forward. That guard is HOST state: a captured graph
// (graph_begin / graph_end around forward + backward) replays correctly because the forward's products, which rewrite dX and dWacc from
// scratch (beta = 0 on the first chunk), are replayed with the scaling - a graph that captured the backward WITHOUT its forward would
// scale the same buffers again on every launch.
#pragma once

#include <cstdint>

namespace gpu {

// chunk_rows = 0 resolves to this; otherwise chunk_rows must be a positive multiple of kLinearCeChunkQuantum (the tile kernels' row tile)
constexpr int64_t kLinearCeDefaultChunkRows = 2048;
constexpr int64_t kLinearCeChunkQuantum = 128;

// the checked chunk size of a call: the default for 0, chunk_rows itself otherwise; raises on anything that is not a positive multiple of 128
int64_t linear_ce_chunk_rows(int64_t chunk_rows);

} // namespace gpu
