"""Test helper (not a test): the visibility of the sliding-window mask (kf_attn_window_*), for tests/attn_full_ref.py's attn_ref64_vis,
format_floor_vis and check_lse.

    len_b = clamp(kv_len[b], 0, Skv)        (None: Skv)
    left, right >= 0, or None = unbounded on that side
    vis[b, m, n]  <=>  n < len_b  and  (left is None or n >= m - left)  and  (right is None or n <= m + right)

Top-left aligned, absolute indices; Sq and Skv in either size order. A row may be all False (m - left >= len_b): attn_ref64_vis gives
o = 0 and lse = -inf there."""
import numpy as np


def window_vis(kv_len, left, right, Sq, Skv, B):
    ln = np.full(B, Skv, np.int64) if kv_len is None else np.clip(np.asarray(kv_len, np.int64), 0, Skv)
    assert ln.shape == (B,) and (left is None or left >= 0) and (right is None or right >= 0)
    n, m = np.arange(Skv)[None, None, :], np.arange(Sq)[None, :, None]
    vis = np.broadcast_to(n < ln[:, None, None], (B, Sq, Skv)).copy()
    if left is not None:
        vis &= n >= m - left
    if right is not None:
        vis &= n <= m + right
    return vis


def abi(side):
    """a window side as the C ABI takes it: None -> -1"""
    return -1 if side is None else int(side)
