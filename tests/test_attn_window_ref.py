"""CPU-only: tests/attn_window_ref.py's visibility is the sliding-window mask, written out with loops. With attn_ref64_vis it equals
torch's scaled_dot_product_attention on the CPU in f64 under the same boolean mask (1e-12) on the rows that see a key, and gives o = 0 and
lse = -inf on the others; (None, 0) is the prefix-LM visibility without a prefix, (None, None) the key-length visibility."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.attn_full_ref import attn_ref64_vis, key_len_vis
from tests.attn_prefix_ref import prefix_vis
from tests.attn_window_ref import abi, window_vis

WINDOWS = [(0, 0), (2, 0), (None, 0), (0, None), (3, 1), (1, 4), (None, None), (20, 20), (0, 7)]


def loops(kv_len, left, right, Sq, Skv, B):
    vis = np.zeros((B, Sq, Skv), bool)
    for b in range(B):
        ln = Skv if kv_len is None else min(max(kv_len[b], 0), Skv)
        for m in range(Sq):
            for n in range(Skv):
                vis[b, m, n] = n < ln and (left is None or n >= m - left) and (right is None or n <= m + right)
    return vis


@pytest.mark.parametrize("Sq,Skv", [(5, 9), (9, 5), (7, 7), (1, 1)])
@pytest.mark.parametrize("left,right", WINDOWS)
def test_against_loops(left, right, Sq, Skv):
    for kv_len in (None, [Skv, 3, 0, Skv + 4, -1]):
        B = 2 if kv_len is None else len(kv_len)
        vis = window_vis(kv_len, left, right, Sq, Skv, B)
        assert vis.shape == (B, Sq, Skv) and vis.dtype == bool
        assert np.array_equal(vis, loops(kv_len, left, right, Sq, Skv, B))
    assert abi(None) == -1 and abi(left) == (-1 if left is None else left)


def test_a_window_leaves_rows_without_a_key_inside_a_live_batch():
    vis = window_vis([5], 2, 0, 12, 9, 1)[0]
    assert vis[:7].any(axis=1).all() and not vis[7:].any()      # m - 2 >= 5
    assert not window_vis(None, 1, 0, 12, 9, 1)[0, 10:].any()   # m - 1 >= Skv


@pytest.mark.parametrize("left,right", WINDOWS)
def test_against_torch_sdpa_f64(left, right):
    import torch
    B, Hq, Hkv, Sq, Skv, D = 5, 4, 2, 13, 9, 8
    kv_len = [9, 5, 13, 0, 1]
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (B, Hq, Sq, D)).astype(np.float32)
    k, v = (rng.uniform(-1, 1, (B, Hkv, Skv, D)).astype(np.float32) for _ in range(2))
    vis = window_vis(kv_len, left, right, Sq, Skv, B)
    ref = attn_ref64_vis(q, k, v, None, vis, O.F32)
    live = vis.any(axis=2)                          # [B, Sq]
    assert not live[3].any() and live[0, 0]
    safe = vis.copy()
    safe[~live, 0] = True                           # torch gives NaN for an all-False row: let those rows see key 0, then leave them out
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64) for x in (q, k, v))
    G = Hq // Hkv
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1),
                                                         attn_mask=torch.tensor(safe)[:, None]).numpy()
    rows = np.broadcast_to(live[:, None, :], (B, Hq, Sq))
    assert np.abs(ref["o"][rows] - o[rows]).max() <= 1e-12
    assert (ref["o"][~rows] == 0).all() and np.isneginf(ref["lse"][~rows]).all() and np.isfinite(ref["lse"][rows]).all()


@pytest.mark.parametrize("Sq,Skv", [(5, 9), (9, 5), (7, 7)])
def test_the_degenerate_windows_are_the_older_masks(Sq, Skv):
    for kv_len, B in ((None, 2), ([Skv, 3, 0, Skv + 2], 4)):
        assert np.array_equal(window_vis(kv_len, None, 0, Sq, Skv, B), prefix_vis(kv_len, None, Sq, Skv, B))
        assert np.array_equal(window_vis(kv_len, None, None, Sq, Skv, B), key_len_vis(kv_len, Sq, Skv, B))
