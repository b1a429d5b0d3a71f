"""CPU-only: tests/attn_prefix_ref.py's visibility is the prefix-LM mask. With attn_ref64_vis it equals torch's
scaled_dot_product_attention on the CPU in f64 under the same boolean mask written out with loops (1e-12); a prefix at or beyond the
key length is the key-length visibility; no prefix and no length is the lower triangle, rectangular when Sq != Skv."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.attn_full_ref import attn_ref64_vis, key_len_vis
from tests.attn_prefix_ref import prefix_vis


def loops(kv_len, prefix_len, Sq, Skv, B):
    vis = np.zeros((B, Sq, Skv), bool)
    for b in range(B):
        ln = Skv if kv_len is None else min(max(kv_len[b], 0), Skv)
        pre = 0 if prefix_len is None else min(max(prefix_len[b], 0), Skv)
        for m in range(Sq):
            for n in range(Skv):
                vis[b, m, n] = n < ln and (n < pre or n <= m)
    return vis


def test_against_torch_sdpa_f64():
    import torch
    B, Hq, Hkv, Sq, Skv, D = 5, 4, 2, 9, 13, 8
    kv_len, prefix_len = [13, 7, 13, 99, 1], [0, 3, 20, 5, -2]
    rng = np.random.default_rng(0)
    q = rng.uniform(-1, 1, (B, Hq, Sq, D)).astype(np.float32)
    k, v = (rng.uniform(-1, 1, (B, Hkv, Skv, D)).astype(np.float32) for _ in range(2))
    vis = prefix_vis(kv_len, prefix_len, Sq, Skv, B)
    assert np.array_equal(vis, loops(kv_len, prefix_len, Sq, Skv, B))
    assert vis[:, :, 0].all()                      # with len_b >= 1 every query sees key 0
    ref = attn_ref64_vis(q, k, v, None, vis, O.F32)
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64) for x in (q, k, v))
    G = Hq // Hkv
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1),
                                                         attn_mask=torch.tensor(vis)[:, None])
    assert np.abs(ref["o"] - o.numpy()).max() <= 1e-12


@pytest.mark.parametrize("Sq,Skv", [(5, 9), (9, 5), (7, 7)])
def test_prefix_at_or_beyond_the_length_is_the_key_length_mask(Sq, Skv):
    kv_len = [Skv, 3, 0, 4]
    for prefix_len in ([Skv, 3, 0, 4], [Skv + 5, 4, 2, Skv]):
        assert np.array_equal(prefix_vis(kv_len, prefix_len, Sq, Skv, 4), key_len_vis(kv_len, Sq, Skv))
    assert np.array_equal(prefix_vis(None, [Skv] * 2, Sq, Skv, 2), key_len_vis(None, Sq, Skv, 2))


@pytest.mark.parametrize("Sq,Skv", [(5, 9), (9, 5), (7, 7), (1, 1)])
def test_no_prefix_and_no_length_is_the_lower_triangle(Sq, Skv):
    tril = np.tril(np.ones((Sq, Skv), bool))     # top-left aligned: n <= m
    for vis in (prefix_vis(None, None, Sq, Skv, 2), prefix_vis(None, [0, 0], Sq, Skv, 2), prefix_vis([Skv, Skv + 1], None, Sq, Skv, 2)):
        assert vis.shape == (2, Sq, Skv) and all(np.array_equal(x, tril) for x in vis)
