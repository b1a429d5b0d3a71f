"""CPU-only: tests/attn_span_ref.py, the numpy restatement of the document mask with a causal rule, prefixes and a window.

 * span_table's two pairs both equal span_vis, the brute-force definition, and all four columns are nondecreasing along a row - what lets
   the document kernels run such a mask unchanged - on random lists and on the document tests' TABLE_ROWS (empty documents, cu[b, 0] != 0,
   out-of-range entries);
 * degenerate masks are the older references': no window and no prefix is doc_vis, one document is window_vis / prefix_vis, causal = 0
   without a window is doc_table;
 * the mask must bite: for every case of the GPU list (CASES) whose mask differs from the plain document mask at all - bites() says
   which, from the sizes alone - the f64 reference under doc_vis FAILS the GPU tests' own 16-bit check (oracle.checks.check_one with the
   floors of format_floor_vis) against the reference under span_vis, in o, dq, dk and dv. A kernel that ignored the window or the
   prefixes, or a host path that handed dK/dV the wrong pair, would therefore fail tests/test_gpu_attn_span.py."""
import functools

import numpy as np
import pytest

from oracle import checks as K
from oracle import oracle as O
from tests.attn_doc_ref import cu_of, doc_table, doc_vis
from tests.attn_full_ref import attn_ref64_vis, format_floor_vis
from tests.attn_prefix_ref import prefix_vis
from tests.attn_span_ref import CASES, MASKS, SIZES, TABLE_ROWS, bites, case_mask, span_table, span_vis, vis_of_tables
from tests.attn_window_ref import window_vis
from tests.test_gpu_attn_full import inputs

WINDOWS = [(-1, -1), (0, 0), (1, 0), (5, 3), (-1, 0), (-1, 3), (5, -1), (31, 0)]


def check_tables(cu, S, causal, wl, wr, pre):
    vis = span_vis(cu, S, causal, wl, wr, pre)
    kv, klo, khi, qlo, qhi = span_table(cu, S, causal, wl, wr, pre)
    what = f"S {S} causal {causal} window ({wl}, {wr}) prefix {None if pre is None else pre.tolist()} cu {np.asarray(cu).tolist()}"
    assert np.array_equal(vis_of_tables(kv, klo, khi), vis), f"{what}: (key_lo, key_hi) is not the definition"
    assert np.array_equal(vis_of_tables(kv, qlo, qhi, by_key=True), vis), f"{what}: (query_lo, query_hi) is not the definition"
    for name, t in zip(("key_lo", "key_hi", "query_lo", "query_hi"), (klo, khi, qlo, qhi)):
        assert t.dtype == np.int32 and t.shape == (len(cu), S)
        assert (np.diff(t, axis=1) >= 0).all(), f"{what}: {name} decreases along a row"
        assert (t >= 0).all() and (t <= S).all()
        assert (t[np.arange(S)[None, :] >= kv[:, None]] == np.broadcast_to(kv[:, None], t.shape)[np.arange(S)[None, :] >= kv[:, None]]).all()
    assert (klo <= khi).all() and (qlo <= qhi).all()
    return vis


def test_tables_are_the_definition_on_random_lists():
    rng = np.random.default_rng(0)
    for _ in range(300):
        S = int(rng.integers(1, 41))
        n = int(rng.integers(1, 6))
        lens = [[int(x) for x in rng.integers(0, max(2, 2 * S // n), n)] for _ in range(3)]   # with empty documents, some rows beyond S
        cu = cu_of(lens)
        wl, wr = WINDOWS[int(rng.integers(len(WINDOWS)))]
        for causal in (0, 1):
            check_tables(cu, S, causal, wl, wr, None)
        check_tables(cu, S, 1, wl, wr, rng.integers(-2, S + 3, (3, n)))


@pytest.mark.parametrize("S", [1, 65, 200])
def test_tables_are_the_definition_on_the_table_rows(S):
    cu = np.array(TABLE_ROWS, np.int64)
    pre = np.random.default_rng(S).integers(-3, 70, (cu.shape[0], cu.shape[1] - 1))
    for wl, wr in WINDOWS:
        check_tables(cu, S, 0, wl, wr, None)
        check_tables(cu, S, 1, wl, wr, None)
        check_tables(cu, S, 1, wl, wr, pre)


@pytest.mark.parametrize("S", [1, 33, 200])
def test_degenerate_masks_are_the_older_references(S):
    rows = [[S], [S // 3, S - S // 3 - 2], [], [1] * min(S, 9)]
    cu = cu_of(rows)
    for causal in (0, 1):       # no window, no prefix: the document mask, and a prefix of 0 or 1 token changes nothing
        assert np.array_equal(span_vis(cu, S, causal), doc_vis(cu, S, bool(causal)))
    assert np.array_equal(span_vis(cu, S, 1, doc_prefix=np.ones((4, cu.shape[1] - 1), np.int64)), doc_vis(cu, S, True))
    kv, s, e = doc_table(cu, S)     # causal = 0 without a window: both pairs are the document table
    got = span_table(cu, S, 0)
    assert np.array_equal(got[0], kv) and all(np.array_equal(x, s) for x in got[1::2]) and all(np.array_equal(x, e) for x in got[2::2])
    one = np.array([[0, S], [0, S]], np.int64)      # one document: the window family's mask and the prefix family's
    for wl, wr in ((0, 0), (5, 0), (5, 7), (-1, 3), (31, -1)):
        side = lambda w: None if w < 0 else w  # noqa: E731
        assert np.array_equal(span_vis(one, S, 0, wl, wr), window_vis(None, side(wl), side(wr), S, S, 2))
    assert np.array_equal(span_vis(one, S, 1, 7, 0), window_vis(None, 7, 0, S, S, 2))
    pre = [S // 2, 3]
    assert np.array_equal(span_vis(one, S, 1, doc_prefix=np.array(pre)[:, None]), prefix_vis(None, pre, S, S, 2))


def test_the_case_list_is_what_the_issue_asks_for():
    assert SIZES == (1, 33, 128, 200, 257, 513) and len(CASES) == len(SIZES) * len(MASKS)
    got = {(m[1], m[2], m[3]) for m in MASKS if not m[4]}
    assert {(1, 0, 0), (1, 31, 0), (1, 64, 0), (0, 5, 7), (0, -1, 3)} <= got
    assert any(m[4] for m in MASKS)
    for S in SIZES[2:]:         # from 128 on every mask of the list bites
        assert all(bites(S, *m[1:]) for m in MASKS)
    for S in SIZES[1:]:         # prefixes end off every seam of the kernels (32 rows per wave; 64 and 128 are multiples)
        cu, pre = case_mask(S, 1, -1, -1, True)
        ends = (np.clip(cu[:, :-1], 0, S) + pre)[pre > 0]
        assert len(ends) and (ends % 32 != 0).all()


# ---- the mask must bite ----
CODE, HQ, HKV, D = O.BF16, 2, 2, 64


@functools.lru_cache(maxsize=None)
def problem(S):
    return inputs(np.random.default_rng(S), CODE, 4, HQ, HKV, S, S, D)


@functools.lru_cache(maxsize=None)
def plain(S, causal):
    q, k, v, go = problem(S)
    return attn_ref64_vis(q, k, v, go, doc_vis(cu_of_case(S), S, bool(causal)), CODE)


def cu_of_case(S):
    return case_mask(S, 0, -1, -1, False)[0]


def fails(name, got, ref, fl):
    try:
        K.check_one(name, O.from_float(got.astype(np.float32), CODE), ref, CODE, floor=fl.get(name))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("S,name,causal,wl,wr,with_prefix", CASES, ids=[f"S{c[0]}-{c[1]}" for c in CASES])
def test_the_mask_bites(S, name, causal, wl, wr, with_prefix):
    cu, pre = case_mask(S, causal, wl, wr, with_prefix)
    vis = span_vis(cu, S, causal, wl, wr, pre)
    differs = not np.array_equal(vis, doc_vis(cu, S, bool(causal)))
    assert differs == bites(S, causal, wl, wr, with_prefix)
    if not differs:
        return              # the same mask: the same reference (S = 1; a window wider than the row)
    q, k, v, go = problem(S)
    ref = attn_ref64_vis(q, k, v, go, vis, CODE)
    fl = format_floor_vis(q, k, v, go, vis, CODE)
    for out in ("o", "dq", "dk", "dv"):
        assert fails(out, plain(S, causal)[out], ref, fl), f"S {S} {name}: {out} under the plain document mask passes for the one under this mask"
