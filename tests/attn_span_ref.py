"""Test helper (not a test): the document mask with a causal rule, per-document prefixes and a sliding window (kf_attn_span_table,
kf_attn_span_*), restated in numpy.

    c_j, len_b and document membership: tests/attn_doc_ref.py's (c_0 = 0, values clamped to [0, S], an empty document owns no token)
    P_j = c_j + clamp(doc_prefix[b, j], 0, c_{j+1} - c_j)          (doc_prefix None: P_j = c_j)

    visible(b, m, n)  <=>  m, n in the same document j
                           and (causal == 0 or n <= m or n < P_j)
                           and (wl < 0 or n >= m - wl) and (wr < 0 or n <= m + wr)

span_vis is that definition, token pair by token pair, and knows no table. span_table is what kf_attn_span_table writes: the keys
key_lo <= n < key_hi token m sees as a query, the queries query_lo <= m < query_hi that see token n as a key. A window side is the ABI's:
a key count >= 0 or -1 (unbounded).

CASES is the list tests/test_gpu_attn_span.py runs on the device and tests/test_attn_span_ref.py holds to "the mask must bite"."""
import numpy as np

from tests.attn_doc_ref import clamped, cu_of
from tests.test_gpu_attn_doc import TABLE_ROWS, mixed_rows  # noqa: F401  (the rows of the document tests: one list of them)


def doc_of(cu, S):
    """(c [B, n + 1], doc [B, S]): the document of each token (the LAST j with c_j <= m), -1 for a token in none"""
    c = clamped(cu, S)
    B, n = c.shape[0], c.shape[1] - 1
    doc = np.full((B, S), -1, np.int64)
    for b in range(B):
        for j in range(n):
            doc[b, c[b, j]:c[b, j + 1]] = j       # a later document overwrites nothing: the intervals are disjoint, an empty one is empty
    return c, doc


def prefix_ends(c, doc_prefix):
    """P [B, n]"""
    n = c.shape[1] - 1
    if doc_prefix is None:
        return c[:, :n].copy()
    p = np.asarray(doc_prefix, np.int64)
    assert p.shape == (c.shape[0], n)
    return c[:, :n] + np.clip(p, 0, c[:, 1:] - c[:, :n])


def span_vis(cu, S, causal, wl=-1, wr=-1, doc_prefix=None):
    """the brute-force definition: vis [B, S, S] (query, key)"""
    c, doc = doc_of(cu, S)
    P = prefix_ends(c, doc_prefix)
    m, n = np.arange(S)[None, :, None], np.arange(S)[None, None, :]
    vis = (doc[:, :, None] == doc[:, None, :]) & (doc[:, :, None] >= 0)                  # m, n in the same document j
    if causal:
        Pm = np.take_along_axis(P, np.maximum(doc, 0), axis=1)                           # P_j of the query's document
        vis &= (n <= m) | (n < Pm[:, :, None])
    if wl >= 0:
        vis &= n >= m - wl
    if wr >= 0:
        vis &= n <= m + wr
    return vis


def span_table(cu, S, causal, wl=-1, wr=-1, doc_prefix=None):
    """(kv_len int64 [B], key_lo, key_hi, query_lo, query_hi int32 [B, S]): the formulas of include/kfunca_hip.h"""
    c, doc = doc_of(cu, S)
    P = prefix_ends(c, doc_prefix)
    B, n = c.shape[0], c.shape[1] - 1
    kv_len = c[:, n].copy()
    out = [np.empty((B, S), np.int32) for _ in range(4)]
    for b in range(B):
        for t in range(S):
            j = doc[b, t]
            if j < 0:
                assert t >= kv_len[b]
                for x in out:
                    x[b, t] = kv_len[b]
                continue
            cs, ce, p = c[b, j], c[b, j + 1], P[b, j]
            klo = max(cs, cs if wl < 0 else t - wl)
            khi = min(ce, max(t + 1, p) if causal else ce, ce if wr < 0 else t + wr + 1)
            qlo = max(cs, t if causal and t >= p else cs, cs if wr < 0 else t - wr)
            qhi = min(ce, ce if wl < 0 else t + wl + 1)
            out[0][b, t], out[1][b, t] = klo, max(khi, klo)
            out[2][b, t], out[3][b, t] = qlo, max(qhi, qlo)
    return (kv_len,) + tuple(out)


def vis_of_tables(kv_len, lo, hi, by_key=False):
    """the visibility a pair of tables describes: [B, S, S] (query, key); by_key: the pair is indexed by the key and holds queries"""
    S = lo.shape[1]
    x = np.arange(S)[None, None, :]
    v = (x >= lo[:, :, None]) & (x < hi[:, :, None])
    return v.transpose(0, 2, 1) if by_key else v


# ---- the cases of the GPU tests ----
def off_seam_prefixes(cu, S):
    """about half of each document, moved off every multiple of 32 (the wave's rows; 64 and 128 are multiples): Long [B, n_docs]"""
    c = clamped(cu, S)
    ln = c[:, 1:] - c[:, :-1]
    p = ln // 2
    end = c[:, :-1] + p
    p = np.where((end % 32 == 0) & (p > 0), p - 1, p)
    return p.astype(np.int64)


SIZES = (1, 33, 128, 200, 257, 513)
# (name, causal, window_left, window_right, with prefixes): the causal windows, a symmetric one, a one-sided one, prefixes alone and
# prefixes under a left window (the right side is then the causal rule's: -1 in the table call)
MASKS = (("causal w(0,0)", 1, 0, 0, False), ("causal w(31,0)", 1, 31, 0, False), ("causal w(64,0)", 1, 64, 0, False), ("w(5,7)", 0, 5, 7, False),
         ("w(-1,3)", 0, -1, 3, False), ("prefix", 1, -1, -1, True), ("prefix w(31,-1)", 1, 31, -1, True))
CASES = tuple((S,) + m for S in SIZES for m in MASKS)


def case_mask(S, causal, wl, wr, with_prefix):
    """(cu, doc_prefix or None) of a case"""
    cu = cu_of(mixed_rows(S))
    return cu, off_seam_prefixes(cu, S) if with_prefix else None


def bites(S, causal, wl, wr, with_prefix):
    """whether the case's mask differs from the plain document mask with the same causal flag on mixed_rows(S), by the definition alone.
    The longest document is the whole row (S tokens): a left side bites when S - 1 > wl, a right side (non-causal) when S - 1 > wr,
    a prefix when it holds two tokens (one token is the query itself or a key before it): S // 2 >= 2, off_seam_prefixes taking at most 1."""
    if wl >= 0 and S - 1 > wl:
        return True
    if not causal and wr >= 0 and S - 1 > wr:
        return True
    return bool(with_prefix and S // 2 - 1 >= 2)
