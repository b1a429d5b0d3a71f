"""Test helper (not a test): the document mask of packed rows (kf_attn_doc_table, kf_attn_doc_*), restated in numpy.

    c_j   = clamp(cu[b, j], 0, S),  c_0 = 0 whatever cu[b, 0] holds        cu: int64 [B, n + 1], nondecreasing along a row
    document j of row b holds the tokens c_j <= m < c_{j+1}; a zero-length document owns no token
    len_b = c_n

doc_table(cu, S) is what kf_attn_doc_table writes: kv_len[b] = len_b, and per token (doc_start, doc_end) = (c_j, c_{j+1}) of its
document, (len_b, len_b) for m >= len_b. doc_vis(cu, S, causal) is the visibility [B, S, S] for tests/attn_full_ref.py's
attn_ref64_vis, format_floor_vis and check_lse:

    vis[b, m, n]  <=>  n < len_b  and  doc_start[b, m] <= n < doc_end[b, m]  and  (not causal or n <= m)

A row m >= len_b is all False: attn_ref64_vis gives o = 0 and lse = -inf there."""
import numpy as np


def clamped(cu, S):
    cu = np.asarray(cu, np.int64)
    assert cu.ndim == 2 and cu.shape[1] >= 2
    c = np.clip(cu, 0, S)
    c[:, 0] = 0
    return c


def doc_table(cu, S):
    """(kv_len int64 [B], doc_start int32 [B, S], doc_end int32 [B, S]). Token m < len_b belongs to the LAST document j with c_j <= m
    (the one that is not empty when several start at the same token)."""
    c = clamped(cu, S)
    B, n = c.shape[0], c.shape[1] - 1
    kv_len = c[:, n].copy()
    start, end = np.empty((B, S), np.int32), np.empty((B, S), np.int32)
    for b in range(B):
        m = np.arange(S)
        j = np.searchsorted(c[b, :n], m, side="right") - 1        # the last j < n with c_j <= m (c_0 = 0: j >= 0)
        s, e = c[b, j], c[b, j + 1]
        tail = m >= kv_len[b]
        start[b] = np.where(tail, kv_len[b], s)
        end[b] = np.where(tail, kv_len[b], e)
    return kv_len, start, end


def doc_vis(cu, S, causal):
    kv_len, start, end = doc_table(cu, S)
    n, m = np.arange(S)[None, None, :], np.arange(S)[None, :, None]
    vis = (n < kv_len[:, None, None]) & (n >= start[:, :, None]) & (n < end[:, :, None])
    if causal:
        vis &= n <= m
    return vis


def cu_of(doc_lens, n=None):
    """cumulative lengths [B, n + 1] of per-row lists of document lengths, a shorter list padded by repeating its last value"""
    n = max(len(r) for r in doc_lens) if n is None else n
    n = max(n, 1)
    out = np.zeros((len(doc_lens), n + 1), np.int64)
    for b, r in enumerate(doc_lens):
        cs = np.concatenate([[0], np.cumsum(np.asarray(r, np.int64))]) if len(r) else np.zeros(1, np.int64)
        out[b, :len(cs)] = cs
        out[b, len(cs):] = cs[-1]
    return out
