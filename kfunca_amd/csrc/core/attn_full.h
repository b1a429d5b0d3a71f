// namespace gpu: full (non-causal) softmax attention with an optional per-batch key length (kf_attn_full_fwd, kf_attn_full_bwd) and its
// prefix-LM / padded-causal form (kf_attn_prefix_fwd, kf_attn_prefix_bwd) and its sliding-window form (kf_attn_window_fwd, kf_attn_window_bwd) and its document-masked form for packed rows (kf_attn_doc_fwd, kf_attn_doc_bwd; with a window, a causal rule and prefixes inside the documents: kf_attn_span_fwd, kf_attn_span_bwd), with autograd. No reference counterpart: the self-attention of a vision / audio encoder (every token sees every token), cross-attention
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
// doc_mask (kf_attn_doc_table, kf_attn_doc_fwd, kf_attn_doc_bwd): null (the calls above, unchanged) or the document mask of packed rows:
// one row of [B, H, S, D] holds several independent sequences end to end, and query m sees key n iff both lie in the same document
// (and, with causal = true, n <= m). Self-attention only (Sq = Skv = S of the mask); beside kv_len, prefix_len or a window it is
// refused. A token in no document (the padded tail of a row) gives a zero row and zero gradients.
// A mask built with a window, prefixes or causal (doc_mask's second form; kf_attn_span_table, kf_attn_span_fwd, kf_attn_span_bwd) is the
// way to a sliding window or a prefix-LM mask inside packed documents: the same kernels read its tables, and the call's causal must
// equal the mask's (a mismatch is refused). kv_len, prefix_len and window beside any doc_mask stay refused.
struct AttentionWindow { int64_t left, right; };
// doc_mask(cu_doclens, S): cu_doclens Long [B, n + 1] on the device, the cumulative document lengths of each row (cu[b, 0] = 0; document
// j holds tokens cu[b, j] <= m < cu[b, j + 1]; a shorter list is padded by repeating its last value; values are clamped to [0, S]).
// Returns the tables the kernels read: kv_len Long [B] (the tokens of row b that lie in a document), doc_start and doc_end Int [B, S]
// (the interval of each token's document; both kv_len[b] beyond it). Built once per batch - one launch - and reused by every layer,
// forward and backward.
struct DocMask {
    Tensor kv_len, doc_start, doc_end;
    int64_t B = 0, S = 0;
    // the second form only (span = true): doc_start and doc_end are then the keys lo <= n < hi each token sees as a query, query_lo and
    // query_hi the queries that see it as a key, all with the mask's causal rule, prefixes and window (-1: unbounded) inside
    Tensor query_lo, query_hi;
    int64_t window_left = -1, window_right = -1;
    bool causal = false, span = false;
};
DocMask doc_mask(const Tensor &cu_doclens, int64_t S);
// doc_mask(cu_doclens, S, window, prefix_lens, causal): the document mask and, inside each document, an optional causal rule with a
// bidirectional prefix and an optional sliding window. With P_j = cu[b, j] + clamp(prefix_lens[b, j], 0, length of document j) query m of
// document j sees key n of the same document iff (not causal or n <= m or n < P_j) and m - left <= n <= m + right.
// window: null or attention's {left, right} (-1: unbounded); with causal the right side is 0 (-1 is read as 0, anything else refused)
// and, where a prefix is given, the causal rule alone: a token sees the keys of its prefix that its left side reaches.
// prefix_lens: undefined or Long [B, n_docs] on cu_doclens' device; refused without causal. One launch, built once per batch and mask.
DocMask doc_mask(const Tensor &cu_doclens, int64_t S, const AttentionWindow *window, const Tensor &prefix_lens, bool causal);
// mods (kf_attn_ext_fwd, kf_attn_ext_bwd): null (the calls above, unchanged: their path and their bits) or the modifiers of the SCORES,
// which compose with every mask: softcap (has_softcap; positive and finite, else refused) turns each visible score x = q.k / sqrt(D)
// into softcap tanh(x / softcap) (Gemma-2, Grok); sinks (defined: Float [Hq], dense, on the operands' device, else refused) adds
// exp(sinks[h]) to the softmax denominator of every query of head h - a raw logit, neither scaled nor capped, that owns no value row
// (gpt-oss, StreamingLLM). A row that sees no key is a zero row either way. sinks is a fourth differentiable input: when it requires
// grad it receives dsink[h] = - sum_{b, m} exp(sinks[h] - lse[b,h,m]) rowsum(dO o O)[b,h,m] as a Float [Hq].
struct AttentionModifiers {
    bool has_softcap = false;
    double softcap = 0.0;
    Tensor sinks;
};
Tensor attention(const Tensor &q, const Tensor &k, const Tensor &v, const Tensor &kv_len, bool causal = false, const Tensor &prefix_len = Tensor(),
                 const AttentionWindow *window = nullptr, const DocMask *doc_mask = nullptr, const AttentionModifiers *mods = nullptr);
// attention_qkv(qkv, B, S, H, kv_heads, kv_len): the packed projection [B*S, (H + 2*Hkv)*D] (columns q | k | v; kv_heads < 0: Hkv = H)
// is read in place, the result is [B*S, H*D] and the backward writes one packed gradient - the layouts causal_attention_qkv builds.
// causal, prefix_len, window, doc_mask, mods: as in attention (Sq = Skv = S; sinks is Float [H]).
Tensor attention_qkv(const Tensor &qkv, int64_t B, int64_t S, int64_t H, int64_t kv_heads, const Tensor &kv_len, bool causal = false,
                     const Tensor &prefix_len = Tensor(), const AttentionWindow *window = nullptr, const DocMask *doc_mask = nullptr,
                     const AttentionModifiers *mods = nullptr);

} // namespace gpu
