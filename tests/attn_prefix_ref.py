"""Test helper (not a test): the visibility of the prefix-LM mask (kf_attn_prefix_*), for tests/attn_full_ref.py's attn_ref64_vis,
format_floor_vis and check_lse.

    len_b = clamp(kv_len[b], 0, Skv)        (None: Skv)
    pre_b = clamp(prefix_len[b], 0, Skv)    (None: 0)
    vis[b, m, n]  <=>  n < len_b  and  (n < pre_b  or  n <= m)

Top-left aligned, absolute indices; Sq and Skv in either size order."""
import numpy as np


def prefix_vis(kv_len, prefix_len, Sq, Skv, B):
    ln = np.full(B, Skv, np.int64) if kv_len is None else np.clip(np.asarray(kv_len, np.int64), 0, Skv)
    pre = np.zeros(B, np.int64) if prefix_len is None else np.clip(np.asarray(prefix_len, np.int64), 0, Skv)
    assert ln.shape == (B,) and pre.shape == (B,)
    n, m = np.arange(Skv)[None, None, :], np.arange(Sq)[None, :, None]
    return (n < ln[:, None, None]) & ((n < pre[:, None, None]) | (n <= m))
