"""CPU-only: tests/attn_doc_ref.py, the numpy restatement of the document mask, against a mask built by loops over the documents;
one document is the full family's mask (non-causal) and the prefix helper's causal one; zero-length documents, values above S, a
padded tail, a first entry that is not 0."""
import numpy as np
import pytest

from tests.attn_doc_ref import cu_of, doc_table, doc_vis
from tests.attn_full_ref import key_len_vis
from tests.attn_prefix_ref import prefix_vis


def loops(doc_lens, S, causal):
    """block-diagonal by construction: walk the documents of each row and fill their squares"""
    vis = np.zeros((len(doc_lens), S, S), bool)
    for b, row in enumerate(doc_lens):
        at = 0
        for ln in row:
            lo, hi = min(at, S), min(at + ln, S)
            for m in range(lo, hi):
                for n in range(lo, hi):
                    vis[b, m, n] = (n <= m) or not causal
            at += ln
    return vis


CASES = [
    (1, [[1]]), (7, [[3, 4], [7], [2, 2, 2], []]), (65, [[64, 1], [1, 64], [20, 0, 0, 30], [65]]),
    (200, [[100, 100], [33, 64, 31, 72], [150], [1] * 40, [0, 0, 199]]),
]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S,doc_lens", CASES)
def test_against_loops(S, doc_lens, causal):
    cu = cu_of(doc_lens)
    assert np.array_equal(doc_vis(cu, S, causal), loops(doc_lens, S, causal))
    kv_len, start, end = doc_table(cu, S)
    assert kv_len.dtype == np.int64 and start.dtype == np.int32 and end.dtype == np.int32 and start.shape == end.shape == (len(doc_lens), S)
    for b, row in enumerate(doc_lens):
        assert kv_len[b] == min(sum(row), S)
        assert (start[b, kv_len[b]:] == kv_len[b]).all() and (end[b, kv_len[b]:] == kv_len[b]).all()
        live = np.arange(S) < kv_len[b]
        assert (start[b][live] <= np.arange(S)[live]).all() and (np.arange(S)[live] < end[b][live]).all()   # a token lies in its own document
        assert (np.diff(start[b]) >= 0).all() and (np.diff(end[b]) >= 0).all()                                # a partition: both nondecreasing


@pytest.mark.parametrize("S", [1, 33, 200])
def test_one_document_is_the_older_masks(S):
    cu = np.array([[0, S], [0, S]], np.int64)
    assert np.array_equal(doc_vis(cu, S, False), key_len_vis(None, S, S, 2))
    assert np.array_equal(doc_vis(cu, S, True), prefix_vis(None, None, S, S, 2))
    short = np.array([[0, S // 2], [0, S]], np.int64)      # a padded tail is a key length (and rows beyond it see nothing)
    lens = [S // 2, S]
    want = key_len_vis(lens, S, S, 2)
    want[0, S // 2:] = False
    assert np.array_equal(doc_vis(short, S, False), want)
    wantc = prefix_vis(lens, None, S, S, 2)
    wantc[0, S // 2:] = False
    assert np.array_equal(doc_vis(short, S, True), wantc)


def test_zero_length_documents_own_nothing():
    S = 20
    a = doc_table(np.array([[0, 5, 5, 5, 12, 12, 20]], np.int64), S)
    b = doc_table(np.array([[0, 5, 12, 20, 20, 20, 20]], np.int64), S)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert list(a[1][0, [0, 4, 5, 11, 12, 19]]) == [0, 0, 5, 5, 12, 12] and list(a[2][0, [0, 4, 5, 11, 12, 19]]) == [5, 5, 12, 12, 20, 20]
    # a leading empty document, and a row of empty documents only
    kv, s, e = doc_table(np.array([[0, 0, 0, 7], [0, 0, 0, 0]], np.int64), 10)
    assert list(kv) == [7, 0] and (s[0, :7] == 0).all() and (e[0, :7] == 7).all() and (s[0, 7:] == 7).all() and (e[0, 7:] == 7).all()
    assert (s[1] == 0).all() and (e[1] == 0).all() and not doc_vis(np.array([[0, 0, 0, 0]], np.int64), 10, False).any()


def test_values_are_clamped_and_the_first_entry_is_taken_as_zero():
    S = 10
    kv, s, e = doc_table(np.array([[0, 4, 25, 99], [3, 6, 8, 8], [-7, -2, 5, 10]], np.int64), S)
    assert list(kv) == [10, 8, 10]
    assert list(s[0]) == [0] * 4 + [4] * 6 and list(e[0]) == [4] * 4 + [10] * 6          # 25 and 99 are S: the third document is empty
    assert list(s[1]) == [0] * 6 + [6, 6, 8, 8] and list(e[1]) == [6] * 6 + [8] * 4      # cu[b, 0] = 3 is read as 0
    assert list(s[2]) == [0] * 5 + [5] * 5 and list(e[2]) == [5] * 5 + [10] * 5          # negative entries are 0
    vis = doc_vis(np.array([[0, 4, 25, 99]], np.int64), S, True)
    assert vis[0, 3, :4].all() and not vis[0, 3, 4:].any() and vis[0, 9, 4:].all() and not vis[0, 9, :4].any()


def test_cu_of_pads_by_repeating_the_last_value():
    assert cu_of([[3, 4], [7], []]).tolist() == [[0, 3, 7], [0, 7, 7], [0, 0, 0]]
    assert cu_of([[2]], n=3).tolist() == [[0, 2, 2, 2]]
