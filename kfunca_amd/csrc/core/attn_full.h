// namespace gpu: full (non-causal) softmax attention with an optional per-batch key length (kf_attn_full_fwd, kf_attn_full_bwd) and its
// prefix-LM / padded-causal form (kf_attn_prefix_fwd, kf_attn_prefix_bwd) and its sliding-window form (kf_attn_window_fwd, kf_attn_window_bwd), with autograd. No reference counterpart: the self-attention of a vision / audio encoder (every token sees every token), cross-attention
// (Sq text queries over Skv image keys, in either size order) and padded batches (keys beyond a sample's own length are invisible).
#pragma once

#include <cstdint>

#include "tensor.h"

namespace gpu {

// attention(q, k, v, kv_len): q [B, Hq, Sq, D], k and v [B, Hkv, Skv, D] (Hkv divides Hq: query head h reads K/V head h / (Hq / Hkv)),
// float, half or bfloat16. kv_len: undefined (every key is visible) or Long [B] on the operands' device; batch b sees keys
// n < clamp(kv_len[b], 0, Skv), and K / V rows beyond that are never read (they may hold NaN). A batch without a visible key gives
// zeros and a zero gradient. The gradients are shaped like their inputs; dk and dv are summed over each group and are zero at the
// invisible keys. 16-bit head sizes other than 64 and 128 (D <= 128) are zero-padded to 64 or 128, with the softmax scale of the real
// head size, so they run the matrix-core kernels too.
// causal = true (kf_attn_prefix_fwd, kf_attn_prefix_bwd) adds the prefix-LM mask, top-left aligned: query m sees key n iff
// n < kv_len[b] and (n < prefix_len[b] or n <= m). prefix_len: undefined (no prefix: causal attention over a padded batch) or Long [B],
// clamped to [0, Skv]; given with causal = false it is refused. A key row no query sees (n >= prefix_len[b] and n >= Sq) has zero
// gradients. A plain causal call without lengths is faster through causal_attention / causal_attention_gqa (the generated kernels);
// this operator does not route there, the results would not have the same bits.
// window (kf_attn_window_fwd, kf_attn_window_bwd): null (the calls above, unchanged) or the sliding window {left, right}: query m sees
// key n iff n < kv_len[b], n >= m - left and n <= m + right, top-left aligned; -1 is "unbounded on that side", anything below is
// refused. causal = true with a window means right = 0 (a right side above 0 is refused); a window beside prefix_len is refused.
// A query that sees no key (m - left >= kv_len[b]) gives a zero row and zero gradients; a key no query sees has zero gradients.
struct AttentionWindow { int64_t left, right; };
Tensor attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len, bool causal = false, const Tensor &prefix_len = Tensor(),
                 const AttentionWindow *window = nullptr);
// attention_qkv(qkv, B, S, H, kv_heads, kv_len): the packed projection [B*S, (H + 2*Hkv)*D] (columns q | k | v; kv_heads < 0: Hkv = H)
// is read in place, the result is [B*S, H*D] and the backward writes one packed gradient - the layouts causal_attention_qkv builds.
// causal, prefix_len, window: as in attention (Sq = Skv = S).
Tensor attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t kv_heads, const Tensor &kv_len, bool causal = false,
                     const Tensor &prefix_len = Tensor(), const AttentionWindow *window = nullptr);

} // namespace gpu
