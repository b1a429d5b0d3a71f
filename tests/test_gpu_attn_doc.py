"""-m gpu: document-masked attention of packed rows (kf_attn_doc_table, kf_attn_doc_fwd / kf_attn_doc_bwd, kfunca.doc_mask,
kfunca.attention(..., doc_mask=) and kfunca.attention_qkv): one row of [B, H, S, D] holds several sequences end to end, and query m sees
key n iff both lie in the same document (and, with causal, n <= m).

The reference is tests/attn_full_ref.py's float64 attention under the visibility of tests/attn_doc_ref.py. The 16-bit outputs are held
to the project's scale-aware bounds (oracle.checks.check_one with the floors of format_floor_vis), lse to check_lse's bound and to -inf
exactly where a token lies in no document. The f32 generic path is held to the rule of tests/test_gpu_attn_window.py's check_generic
(rtol 1e-4 / atol 1e-4 forward and lse, rtol 1e-3 / atol 1e-4 backward), the 16-bit generic cases (D 80, D 40) to the scale-aware 16-bit
bounds. The operator tests add that file's comparison with torch's scaled_dot_product_attention on the CPU in f32:
max |got - ref| <= TOL max |ref|, TOL = 2^-5 (bf16) and 1e-4 (f32), over the rows that lie in a document; the others must be zeros.

Where the mask is one an older family has too - one document; documents of one length, which are a batch - the results must have that
family's BITS: a tile the document kernels visit besides contributes exact zeros, so a difference is a defect in tile choice or masking.

Every call here finds its outputs (o, lse, dq, dk, dv) and its workspace pre-filled with 0xFF (tests/poison.py). Shapes sit at the
kernels' seams: 32 rows per wave, 64 per tile, 128 per workgroup. The helpers that do not name an entry are the window, prefix and full
test modules' own, through a module import."""
import numpy as np
import pytest

import kfunca_amd as kfunca
import tests.test_gpu_attn_full as F
import tests.test_gpu_attn_prefix as P
import tests.test_gpu_attn_window as W
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests import poison
from tests.attn_doc_ref import cu_of, doc_table, doc_vis

pytestmark = pytest.mark.gpu


def build_table(cu, S):
    """kf_attn_doc_table on the device: (kv_len, doc_start, doc_end) buffers, poisoned before the call"""
    cu = np.ascontiguousarray(cu, np.int64)
    B, n = cu.shape[0], cu.shape[1] - 1
    bcu = H.DevBuf.from_numpy(cu)
    sizes = (8 * B, 4 * B * S, 4 * B * S)
    bufs = tuple(H.DevBuf(max(x, 1)) for x in sizes)
    for buf, x in zip(bufs, sizes):
        poison.fill(buf.ptr, x, 0xFF)
    H.device_sync()
    return bcu, bufs, n


def run(code, q, k, v, go, cu, causal, graph=False, fill=0xFF):
    """kf_attn_doc_table + kf_attn_doc_fwd + kf_attn_doc_bwd on contiguous tensors: o, lse, dq, dk, dv. The outputs, the tables and the
    workspace are pre-filled with `fill` / 0xFF; graph: all three captured with kf_graph_* and launched once."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert k.shape[2] == S
    scale = F.scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bcu, (bkv, bs, be), n = build_table(cu, S)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    sizes = (q.nbytes, 4 * B * Hq * S, q.nbytes, k.nbytes, v.nbytes, need)
    bo, blse, dq, dk, dv, w = (H.DevBuf(x) for x in sizes)
    for buf, x in zip((bo, blse, dq, dk, dv, w), sizes):
        poison.fill(buf.ptr, x, fill)
    H.device_sync()
    kw = dict(kv_len=bkv.ptr, doc_start=bs.ptr, doc_end=be.ptr, causal=causal)

    def calls(st):
        H.attn_doc_table(B, S, n, bcu.ptr, bkv.ptr, bs.ptr, be.ptr, stream=st)
        H.attn_doc_fwd(code, B, Hq, Hkv, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, stream=st, **kw)
        H.attn_doc_bwd(code, B, Hq, Hkv, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need, stream=st, **kw)

    if graph:
        s = H.Stream()
        with H.Graph.capture(s) as g:
            calls(s.handle)
        g.launch()
        s.sync()
    else:
        calls(None)
    H.device_sync()
    return (bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), dq.to_numpy(q.shape, q.dtype), dk.to_numpy(k.shape, k.dtype),
            dv.to_numpy(v.shape, v.dtype))


# ---- the table ----
TABLE_ROWS = [
    [0, 3, 7, 7, 12, 40, 40, 64, 65, 130, 131, 200],          # ragged, with zero-length documents
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                     # no document at all
    [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],                     # one token, the list padded by repeating its last value
    [5, 9, 9, 33, 64, 64, 64, 100, 100, 100, 100, 100],       # cu[b, 0] != 0 is read as 0
    [-9, -4, 0, 2, 50, 63, 64, 66, 190, 250, 300, 10 ** 12],  # negative entries are 0, entries above S are S
    [0, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200, 200],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 199],                   # leading empty documents
    [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],                   # documents of one token
]


@pytest.mark.parametrize("S", [1, 65, 200])
def test_table_is_exact(S):
    cu = np.array(TABLE_ROWS, np.int64)
    B = cu.shape[0]
    bcu, (bkv, bs, be), n = build_table(cu, S)
    _, labels = F.profiled(lambda: H.attn_doc_table(B, S, n, bcu.ptr, bkv.ptr, bs.ptr, be.ptr))
    H.device_sync()
    kv, s, e = doc_table(cu, S)
    assert np.array_equal(bkv.to_numpy((B,), np.int64), kv)
    assert np.array_equal(bs.to_numpy((B, S), np.int32), s) and np.array_equal(be.to_numpy((B, S), np.int32), e)
    assert labels == {"attn_doc_table"}, sorted(labels)
    # one document per row (n_docs = 1)
    cu1 = np.array([[0, S], [0, S // 2], [7, S + 5]], np.int64)
    bcu, (bkv, bs, be), n = build_table(cu1, S)
    H.attn_doc_table(3, S, 1, bcu.ptr, bkv.ptr, bs.ptr, be.ptr)
    H.device_sync()
    kv, s, e = doc_table(cu1, S)
    assert np.array_equal(bkv.to_numpy((3,), np.int64), kv)
    assert np.array_equal(bs.to_numpy((3, S), np.int32), s) and np.array_equal(be.to_numpy((3, S), np.int32), e)


# ---- matrix-core forward and backward ----
MFMA_LABELS = ("attn_doc_fwd_mfma", "attn_doc_bwd_dq_mfma", "attn_doc_bwd_dkv_mfma")


def only_doc_labels(labels, D):
    for label in MFMA_LABELS:
        assert f"{label}_d{D}" in labels, (label, sorted(labels))
    assert "attn_full_bwd_delta" in labels and not any("generic" in n for n in labels), sorted(labels)
    assert all(n.startswith("attn_doc_") or n == "attn_full_bwd_delta" for n in labels), sorted(labels)


def mixed_rows(S):
    """the four rows one call carries: one document; none (len = 0); boundaries off every seam (odd cuts near S/5, S/2, 4S/5, none a
    multiple of 32); a list with a padded tail (37 tokens where S allows; its first document is empty where the row is short)"""
    cuts = sorted({c for c in (S // 5 | 1, S // 2 | 1, (4 * S) // 5 | 1) if 0 < c < S})
    edges = [0] + cuts + [S]
    total = max(1, S - 37)
    return [[S], [], [b - a for a, b in zip(edges, edges[1:])], [total // 3, total - total // 3]]


@pytest.mark.parametrize("S", [1, 33, 128, 200, 257, 513])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
def test_matrix_core_fwd_bwd(code, D, S):
    rng = np.random.default_rng(S * 7919 + D + code)
    cu = cu_of(mixed_rows(S))
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, S, S, D)
    for causal in (False, True):
        got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, causal))
        vis = doc_vis(cu, S, causal)
        W.check16(code, q, k, v, go, got, vis, f"S {S} D{D} causal {causal}")   # (with zero bits where nothing is seen)
        assert np.isneginf(got[1][1]).all() and W.zero_bits(got[0][1]) and W.zero_bits(got[2][1]) and W.zero_bits(got[3][1]) and W.zero_bits(got[4][1])
        only_doc_labels(labels, D)


# ---- a document boundary at every place where a skip, a tile range or a body choice of one of the three kernels changes ----
@pytest.mark.parametrize("causal", [False, True])
def test_seam_sweep(causal):
    code, D, S = H.BF16, 128, 200
    rng = np.random.default_rng(200)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    for p in (1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 199):
        cu = np.array([[0, p, S], [0, min(p, 150), 150]], np.int64)     # the second row is cut at 150
        got = run(code, q, k, v, go, cu, causal)
        W.check16(code, q, k, v, go, got, doc_vis(cu, S, causal), f"seam sweep p {p} causal {causal}")


# ---- the masks an older family has too: its bits ----
@pytest.mark.parametrize("S", [130, 257])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_one_document_has_the_older_families_bits(code, D, S):
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    cu = np.array([[0, S], [0, S]], np.int64)
    W.assert_same(run(code, q, k, v, go, cu, False), P.run(code, q, k, v, go, None, full=True), "one document, non-causal, is not kf_attn_full_*")
    W.assert_same(run(code, q, k, v, go, cu, True), P.run(code, q, k, v, go, None, None), "one document, causal, is not kf_attn_prefix_* without a prefix")


@pytest.mark.parametrize("L,n", [(128, 3), (256, 2)])
@pytest.mark.parametrize("code,D,Hq,Hkv", [(H.BF16, 128, 2, 2), (H.F16, 64, 4, 2), (H.BF16, 64, 2, 1)])
def test_equal_documents_have_the_bits_of_the_batched_call(code, D, Hq, Hkv, L, n):
    """documents of one length L (a multiple of the 128-row block) are a batch of B n sequences: the same family's call on the
    [B n, H, L, D] tensors walks the same tiles in the same order"""
    B, S = 2, L * n
    rng = np.random.default_rng(L + D + Hq)
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, S, S, D)
    cu = np.tile(np.arange(n + 1, dtype=np.int64) * L, (B, 1))
    split = lambda x: np.ascontiguousarray(x.reshape(B, x.shape[1], n, L, D).transpose(0, 2, 1, 3, 4).reshape(B * n, x.shape[1], L, D))  # noqa: E731
    join = lambda x: np.ascontiguousarray(x.reshape((B, n, x.shape[1], L) + x.shape[3:]).swapaxes(1, 2).reshape((B, x.shape[1], S) + x.shape[3:]))  # noqa: E731
    for causal in (False, True):
        got = run(code, q, k, v, go, cu, causal)
        want = P.run(code, split(q), split(k), split(v), split(go), None, None, full=not causal)
        W.assert_same(got, tuple(join(x) for x in want), f"documents of {L}, causal {causal}: not the bits of the batched call")


# ---- every output is written in full, whatever it held ----
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64), (H.F32, 64)])
def test_outputs_are_written_in_full(code, D):
    S = 257 if code != H.F32 else 70
    rng = np.random.default_rng(D + code)
    q, k, v, go = F.inputs(rng, code, 2, 2, 1, S, S, D)
    cu = cu_of([[S // 3, S - S // 3], [S // 4, S // 4]])     # the second row: a tail of half the row in no document
    for causal in (False, True):
        want = run(code, q, k, v, go, cu, causal, fill=0x00)
        for fill in (0xFF, 0x7F):
            got = run(code, q, k, v, go, cu, causal, fill=fill)
            W.no_nan(code, got, f"fill {fill:#x}")
            W.assert_same(got, want, f"outputs or workspace pre-filled with {fill:#x} changed the result")


# ---- K and V rows at n >= len_b are never read ----
@pytest.mark.parametrize("poison_value", [np.nan, np.inf])
@pytest.mark.parametrize("code,D,causal", [(H.BF16, 128, True), (H.F16, 64, False), (H.BF16, 80, True)])
def test_padding_never_reaches_an_output(poison_value, code, D, causal):
    S = 200
    rows = [[200], [], [1], [30, 34], [65], [100, 50]]
    lens = [sum(r) for r in rows]
    cu = cu_of(rows)
    rng = np.random.default_rng(64 + code)
    q, k, v, go = F.inputs(rng, code, len(rows), 2, 2, S, S, D)
    kz, vz = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    kp, vp = kz.copy(), vz.copy()
    for b, ln in enumerate(lens):
        kz[b, :, ln:] = 0
        vz[b, :, ln:] = 0
        kp[b, :, ln:] = poison_value
        vp[b, :, ln:] = -poison_value
    clean = run(code, q, O.from_float(kz, code), O.from_float(vz, code), go, cu, causal)
    W.check16(code, q, k, v, go, clean, doc_vis(cu, S, causal), "zero padding")
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, cu, causal)
    W.assert_same(dirty, clean, f"padding of {poison_value} changed the result")


# ---- grouped K/V heads ----
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("code,D,causal", [(H.BF16, 128, True), (H.F16, 64, False)])
def test_gqa(code, D, causal, Hkv):
    Hq, S = 8, 200
    cu = cu_of([[77, 123], [40, 33, 57], [200]])
    rng = np.random.default_rng(Hkv + D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, Hkv, S, S, D)
    got = run(code, q, k, v, go, cu, causal)
    W.check16(code, q, k, v, go, got, doc_vis(cu, S, causal), f"gqa {Hq}/{Hkv}")


# ---- strided: the packed projection read in place ----
@pytest.mark.parametrize("code,D,S,causal", [(H.BF16, 128, 200, True), (H.F16, 64, 129, False)])
def test_packed_layout_equals_contiguous(code, D, S, causal):
    B, Hq, Hkv = 2, 4, 2
    Wd, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = Wd + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = F.rnd(rng, code, (B * S, Wd)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    cu = cu_of([[S // 3, S - S // 3], [41, S - 70 - 41]])
    ref = run(code, q, k, v, go, cu, causal)
    packed, flat, gpack = (S * Wd, D, Wd), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout)
    bcu, (bkv, bs, be), n = build_table(cu, S)
    H.attn_doc_table(B, S, n, bcu.ptr, bkv.ptr, bs.ptr, be.ptr)
    ob, o = F.guarded(B * S * d * es)
    lb, lse = F.guarded(4 * B * Hq * S)
    gb, g = F.guarded(B * S * PADW * es)
    scale = F.scale_of(D)
    kw = dict(kv_len=bkv.ptr, doc_start=bs.ptr, doc_end=be.ptr, causal=causal)
    H.attn_doc_fwd(code, B, Hq, Hkv, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, layouts=(packed, packed, packed, flat), **kw)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    poison.fill(w.ptr, need, 0xFF)
    H.attn_doc_bwd(code, B, Hq, Hkv, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                   g + (d + dkv) * es, w.ptr, need, layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack), **kw)
    H.device_sync()
    assert F.same(heads(F.read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert F.same(F.read(lse, (B, Hq, S), np.float32), ref[1])
    gq = F.read(g, (B * S, PADW), qkv.dtype)
    assert F.same(heads(gq[:, :d], Hq), ref[2]) and F.same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and F.same(heads(gq[:, d + dkv:Wd], Hkv), ref[4])
    assert (gq[:, Wd:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, nb in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es)):
        assert F.guards_ok(buf, nb)


# ---- generic path ----
GENERIC_LABELS = {"attn_doc_fwd_generic", "attn_doc_bwd_dq_generic", "attn_doc_bwd_dkv_generic"}


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [33, 96, 300])
@pytest.mark.parametrize("code,D", [(H.F32, 64), (H.BF16, 80), (H.F16, 40)])
def test_generic(code, D, S, causal):
    cu = cu_of(mixed_rows(S))
    rng = np.random.default_rng(D + S + code)
    q, k, v, go = F.inputs(rng, code, 4, 4, 2, S, S, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, causal))
    vis = doc_vis(cu, S, causal)
    W.no_nan(code, got)
    if code == H.F32:
        W.check_generic(code, q, k, v, go, got, vis)
        W.zeros_where_nothing_is_seen(got, vis)
    else:
        W.check16(code, q, k, v, go, got, vis, f"generic D{D}")
    assert GENERIC_LABELS <= labels and not any("mfma" in n for n in labels), sorted(labels)
    assert all(n.startswith("attn_doc_") or n == "attn_full_bwd_delta_generic" for n in labels), sorted(labels)


# ---- determinism, graph capture ----
def test_reproducible_and_capturable():
    rng = np.random.default_rng(513)
    for code, D, Hq, Hkv, S, rows, causal in ((H.BF16, 128, 2, 2, 513, [[100, 257, 156], [300, 100]], True),
                                              (H.F16, 64, 4, 1, 200, [[64, 64, 72], [33]], False)):
        cu = cu_of(rows)
        q, k, v, go = F.inputs(rng, code, 2, Hq, Hkv, S, S, D)
        a, b, g = run(code, q, k, v, go, cu, causal), run(code, q, k, v, go, cu, causal), run(code, q, k, v, go, cu, causal, graph=True)
        W.assert_same(a, b, "two runs differ")
        W.assert_same(a, g, "the captured run differs from the eager one")


# ---- operator API ----
def dev_long(x):
    return kfunca.from_numpy(np.ascontiguousarray(x, np.int64), 0)


# every row keeps at least 3/4 of its tokens inside documents, so leaving the others out of the torch comparison cannot hide a failure
OP_ROWS = {90: [[40, 50], [33, 20, 17]], 129: [[64, 65], [50, 1, 47]]}


def test_doc_mask_object():
    S = 90
    cu = cu_of(OP_ROWS[S])
    mask = kfunca.doc_mask(dev_long(cu), S)
    kv, s, e = doc_table(cu, S)
    assert mask.B == 2 and mask.S == S
    assert np.array_equal(mask.kv_len.numpy(), kv) and np.array_equal(mask.doc_start.numpy(), s) and np.array_equal(mask.doc_end.numpy(), e)
    assert mask.doc_start.numpy().dtype == np.int32 and mask.kv_len.numpy().dtype == np.int64


@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention(code, D):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv, S = 2, 4, 2, 90
    cu = cu_of(OP_ROWS[S])
    assert (cu[:, -1] * 4 >= 3 * S).all()
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, S, S, D)
    mask = kfunca.doc_mask(dev_long(cu), S)          # one mask, reused by both calls, forward and backward
    for causal in (False, True):
        tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
        out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, causal=causal, doc_mask=mask))
        out.backward(F.value(go, code))
        got = [F.as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
        assert got[0].shape == q.shape and got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
        W.check_operator(code, q, k, v, go, doc_vis(cu, S, causal), got, f"attention D{D} doc_mask causal {causal}")
        if code == H.BF16:   # head size 40 is zero-padded to 64: the matrix-core kernels
            assert "attn_doc_fwd_mfma_d64" in labels, sorted(labels)
        else:
            assert "attn_doc_fwd_generic" in labels, sorted(labels)
        assert not any(n.startswith(("attn_full_fwd", "attn_prefix_", "attn_window_")) for n in labels), sorted(labels)


@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention_qkv(code, D):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq, Hkv = 2, 129, 4, 2
    Wd, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    cu = cu_of(OP_ROWS[S])
    assert (cu[:, -1] * 4 >= 3 * S).all()
    qkv, gout = F.rnd(rng, code, (B * S, Wd)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    mask = kfunca.doc_mask(dev_long(cu), S)
    for causal in (False, True):
        tx = F.leaf(qkv, code)
        out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=Hkv, causal=causal, doc_mask=mask)
        out.backward(F.value(gout, code))
        o2, g2 = F.as_np(out, code), F.as_np(tx.grad(), code)
        assert o2.shape == (B * S, d) and g2.shape == qkv.shape
        got = [heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv)]
        W.check_operator(code, q, k, v, go, doc_vis(cu, S, causal), got, f"attention_qkv D{D} doc_mask causal {causal}")


def test_refusals():
    rng = np.random.default_rng(1)
    q, k, v, _ = F.inputs(rng, H.BF16, 2, 2, 2, 8, 8, 64)
    tq, tk, tv = (F.value(x, H.BF16) for x in (q, k, v))
    packed = F.value(F.rnd(rng, H.BF16, (16, 6 * 64)), H.BF16)
    mask = kfunca.doc_mask(dev_long([[0, 3, 8], [0, 8, 8]]), 8)
    lens = dev_long([1, 2])
    for op, call in (("attention", lambda **kw: kfunca.attention(tq, tk, tv, doc_mask=mask, **kw)),
                     ("attention_qkv", lambda **kw: kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, doc_mask=mask, **kw))):
        for kw in (dict(kv_len=lens), dict(causal=True, prefix_len=lens), dict(window=(4, 0)), dict(kv_len=lens, window=(4, None))):
            with pytest.raises(Exception, match=f"{op}: doc_mask cannot be combined with kv_len, prefix_len or window"):
                call(**kw)
    # Sq != Skv
    k9 = F.value(F.rnd(rng, H.BF16, (2, 2, 9, 64)), H.BF16)
    with pytest.raises(Exception, match="attention: doc_mask needs self-attention"):
        kfunca.attention(tq, k9, k9, doc_mask=mask)
    # a mask of another B or S
    for other in (kfunca.doc_mask(dev_long([[0, 8]]), 8), kfunca.doc_mask(dev_long([[0, 3, 8], [0, 8, 8], [0, 1, 2]]), 8),
                  kfunca.doc_mask(dev_long([[0, 3, 9], [0, 9, 9]]), 9), kfunca.doc_mask(dev_long([[0, 3, 7], [0, 7, 7]]), 7)):
        with pytest.raises(Exception, match="attention: doc_mask was built for B = "):
            kfunca.attention(tq, tk, tv, doc_mask=other)
        with pytest.raises(Exception, match="attention_qkv: doc_mask was built for B = "):
            kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, doc_mask=other)
    if kfunca.device_count() > 1:   # a mask on another device than the operands'
        far = kfunca.doc_mask(kfunca.from_numpy(np.array([[0, 3, 8], [0, 8, 8]], np.int64), 1), 8)
        with pytest.raises(Exception, match="attention: doc_mask must be on the operands' device"):
            kfunca.attention(tq, tk, tv, doc_mask=far)
        with pytest.raises(Exception, match="attention_qkv: doc_mask must be on the operands' device"):
            kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, doc_mask=far)
    with pytest.raises(Exception, match="attention: doc_mask is a DocMask"):
        kfunca.attention(tq, tk, tv, doc_mask=(1, 2))
    with pytest.raises(Exception, match="doc_mask expects cu_doclens"):
        kfunca.doc_mask(dev_long([0, 8]), 8)
    # causal = True beside the mask is no refusal: the causal form
    a = kfunca.attention(tq, tk, tv, causal=True, doc_mask=mask)
    b = kfunca.attention(tq, tk, tv, doc_mask=mask)
    assert not F.same(F.as_np(a, H.BF16), F.as_np(b, H.BF16))


@pytest.mark.parametrize("causal,prefix_len", [(False, None), (True, None), (True, [20, 70])])
@pytest.mark.parametrize("kv_len", [None, [90, 33]])
def test_doc_mask_none_makes_the_previous_calls(kv_len, causal, prefix_len):
    """without a mask the operator launches what it launched before masks existed: the same labels, and the bits of the entry it called
    then, on the same tensors"""
    code, D = H.BF16, 64
    rng = np.random.default_rng(7)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, 70, 90, D)
    want = P.run(code, q, k, v, go, kv_len, prefix_len, full=not causal)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    opt = lambda x: None if x is None else dev_long(x)  # noqa: E731

    def call():
        out = kfunca.attention(tq, tk, tv, kv_len=opt(kv_len), causal=causal, prefix_len=opt(prefix_len), window=None, doc_mask=None)
        out.backward(F.value(go, code))
        return out

    out, labels = F.profiled(call)
    family = "prefix" if causal else "full"
    mine = {n for n in labels if n.startswith("attn_")}
    assert mine == {f"attn_{family}_fwd_mfma_d64", "attn_full_bwd_delta", f"attn_{family}_bwd_dq_mfma_d64", f"attn_{family}_bwd_dkv_mfma_d64"}, sorted(labels)
    for name, t, w in zip(("o", "dq", "dk", "dv"), (out, tq.grad(), tk.grad(), tv.grad()), (want[0], want[2], want[3], want[4])):
        assert F.same(F.as_np(t, code), w), name
