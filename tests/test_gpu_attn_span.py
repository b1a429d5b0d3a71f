"""-m gpu: the document mask with a causal rule, per-document prefixes and a sliding window at the C ABI (kf_attn_span_table,
kf_attn_span_fwd / kf_attn_span_bwd): query m sees key n iff both lie in the same document j and (not causal or n <= m or n < P_j) and
m - left <= n <= m + right.

The table is held to tests/attn_span_ref.py's span_table exactly. The attention results are held to tests/attn_full_ref.py's float64
attention under span_vis - the definition, which knows no table - with the bounds the document tests use and no other: the 16-bit
outputs to oracle.checks.check_one with the floors of format_floor_vis, lse to check_lse's bound and to -inf exactly where a token sees
nothing, zero bits on dead rows (W.check16); the generic f32 path to W.check_generic; the modifiers to tests/attn_ext_ref.py's
attn_ref64_ext with dsink at its bound (EXT.check16). tests/test_attn_span_ref.py shows on the CPU that every mask of CASES that differs
from the plain document mask fails these bounds when it is ignored.

The entries add no attention kernel: the document kernels read the tables. So where the mask is one another family has too, all five
outputs must have that family's BITS (W.assert_same): no window and no prefix is kf_attn_doc_*, one document is kf_attn_window_* /
kf_attn_prefix_*, equal documents are the batched window call, modifiers without a window are kf_attn_ext_* with KF_ATTN_MASK_DOC.

Every call finds its outputs, its tables and its workspace pre-filled with 0xFF (tests/poison.py)."""
import numpy as np
import pytest

import tests.test_gpu_attn_doc as DOC
import tests.test_gpu_attn_ext as EXT
import tests.test_gpu_attn_full as F
import tests.test_gpu_attn_prefix as P
import tests.test_gpu_attn_window as W
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests import poison
from tests.attn_doc_ref import cu_of
from tests.attn_ext_ref import sinks_for
from tests.attn_span_ref import CASES, TABLE_ROWS, case_mask, span_table, span_vis

pytestmark = pytest.mark.gpu


class Tables:
    """kf_attn_span_table's inputs and outputs on the device, the outputs poisoned; launch(stream) makes the call"""

    def __init__(self, cu, S, causal, wl, wr, pre):
        cu = np.ascontiguousarray(cu, np.int64)
        self.B, self.S, self.n = cu.shape[0], S, cu.shape[1] - 1
        self.args = (int(causal), wl, wr)
        self.cu = H.DevBuf.from_numpy(cu)
        self.pre = None if pre is None else H.DevBuf.from_numpy(np.ascontiguousarray(pre, np.int64))
        sizes = (8 * self.B,) + (4 * self.B * S,) * 4
        self.bufs = tuple(H.DevBuf(max(x, 1)) for x in sizes)
        for buf, x in zip(self.bufs, sizes):
            poison.fill(buf.ptr, x, 0xFF)
        H.device_sync()
        self.kv, self.klo, self.khi, self.qlo, self.qhi = self.bufs

    def launch(self, st=None):
        H.attn_span_table(self.B, self.S, self.n, self.cu.ptr, *(b.ptr for b in self.bufs), doc_prefix=None if self.pre is None else self.pre.ptr,
                          causal=self.args[0], window_left=self.args[1], window_right=self.args[2], stream=st)

    def read(self):
        return (self.kv.to_numpy((self.B,), np.int64),) + tuple(b.to_numpy((self.B, self.S), np.int32) for b in self.bufs[1:])

    def fwd_kw(self):
        return dict(kv_len=self.kv.ptr, key_lo=self.klo.ptr, key_hi=self.khi.ptr)

    def bwd_kw(self):
        return dict(self.fwd_kw(), query_lo=self.qlo.ptr, query_hi=self.qhi.ptr)


def run(code, q, k, v, go, cu, causal, wl=-1, wr=-1, pre=None, softcap=0.0, sink=None, graph=False, fill=0xFF):
    """kf_attn_span_table + kf_attn_span_fwd + kf_attn_span_bwd on contiguous tensors: (o, lse, dq, dk, dv, dsink or None). The outputs,
    the tables and the workspace are pre-filled; graph: all three captured with kf_graph_* and launched once."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert k.shape[2] == S
    scale = F.scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    t = Tables(cu, S, causal, wl, wr, pre)
    bsink = None if sink is None else H.DevBuf.from_numpy(np.asarray(sink, np.float32))
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    sizes = (q.nbytes, 4 * B * Hq * S, q.nbytes, k.nbytes, v.nbytes, need, 4 * Hq)
    bo, blse, dq, dk, dv, w, bds = (H.DevBuf(max(x, 1)) for x in sizes)
    for buf, x in zip((bo, blse, dq, dk, dv, w, bds), sizes):
        poison.fill(buf.ptr, x, fill)
    H.device_sync()
    mods = dict(softcap=softcap, sink=None if bsink is None else bsink.ptr)

    def calls(st):
        t.launch(st)
        H.attn_span_fwd(code, B, Hq, Hkv, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, stream=st, **t.fwd_kw(), **mods)
        H.attn_span_bwd(code, B, Hq, Hkv, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need,
                        dsink=None if bsink is None else bds.ptr, stream=st, **t.bwd_kw(), **mods)

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
            dv.to_numpy(v.shape, v.dtype), None if bsink is None else bds.to_numpy((Hq,), np.float32))


# ---- the table ----
@pytest.mark.parametrize("S", [1, 65, 200])
def test_table_is_exact(S):
    cu = np.array(TABLE_ROWS, np.int64)
    pre = np.random.default_rng(S).integers(-3, 70, (cu.shape[0], cu.shape[1] - 1))
    for wl, wr in ((-1, -1), (0, 0), (5, 7), (-1, 3), (31, 0)):
        for causal, p in ((0, None), (1, None), (1, pre)):
            t = Tables(cu, S, causal, wl, wr, p)
            _, labels = F.profiled(t.launch)
            H.device_sync()
            assert labels == {"attn_span_table"}, sorted(labels)
            for name, got, want in zip(("kv_len", "key_lo", "key_hi", "query_lo", "query_hi"), t.read(), span_table(cu, S, causal, wl, wr, p)):
                assert got.dtype == want.dtype and np.array_equal(got, want), f"S {S} window ({wl}, {wr}) causal {causal} prefixes {p is not None}: {name}"
    # one document per row (n_docs = 1), and sides no 32-bit value holds
    cu1 = np.array([[0, S], [0, S // 2], [7, S + 5]], np.int64)
    for causal, wl, wr, p in ((1, 3, 0, None), (1, 1 << 40, -1, np.array([[S // 2], [1 << 50], [-5]])), (0, (1 << 62) + 5, 1 << 62, None)):
        t = Tables(cu1, S, causal, wl, wr, p)
        t.launch()
        H.device_sync()
        for got, want in zip(t.read(), span_table(cu1, S, causal, wl, wr, p)):
            assert np.array_equal(got, want), (S, causal, wl, wr)


# ---- matrix-core forward and backward ----
def dead_rows_are_empty(got, vis):
    """a token that sees nothing: lse = -inf; its o, dq and - it is seen by nothing either - dk, dv are zero BITS"""
    dead = ~vis.any(axis=2)
    for b in range(vis.shape[0]):
        assert np.isneginf(got[1][b][:, dead[b]]).all()
        assert all(W.zero_bits(got[i][b][:, dead[b]]) for i in (0, 2, 3, 4))
    assert dead[1].all()        # (the second row of mixed_rows has no document)


@pytest.mark.parametrize("S,name,causal,wl,wr,with_prefix", CASES, ids=[f"S{c[0]}-{c[1]}" for c in CASES])
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 128), (H.F16, 64), (H.F16, 128)])
def test_matrix_core_fwd_bwd(code, D, S, name, causal, wl, wr, with_prefix):
    rng = np.random.default_rng(S * 7919 + D + code)
    cu, pre = case_mask(S, causal, wl, wr, with_prefix)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, S, S, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, causal, wl, wr, pre))
    vis = span_vis(cu, S, causal, wl, wr, pre)
    W.check16(code, q, k, v, go, got[:5], vis, f"S {S} D{D} {name}")
    dead_rows_are_empty(got, vis)
    DOC.only_doc_labels(labels - {"attn_span_table"}, D)
    assert "attn_span_table" in labels


# ---- a document boundary at every place where a skip, a tile range or a body choice of one of the three kernels changes ----
@pytest.mark.parametrize("mask", ["window", "prefix"])
def test_seam_sweep(mask):
    code, D, S = H.BF16, 128, 200
    rng = np.random.default_rng(200)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    for p in (1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 199):
        cu = np.array([[0, p, S], [0, min(p, 150), 150]], np.int64)     # the second row is cut at 150
        wl, wr, pre = (33, 0, None) if mask == "window" else (-1, -1, np.full((2, 2), p // 2, np.int64))
        got = run(code, q, k, v, go, cu, 1, wl, wr, pre)
        W.check16(code, q, k, v, go, got[:5], span_vis(cu, S, 1, wl, wr, pre), f"seam sweep p {p} {mask}")


# ---- the masks another family has too: its bits, on all five outputs ----
@pytest.mark.parametrize("S", [130, 257])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_without_window_and_prefix_it_is_the_document_call(code, D, S):
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, S, S, D)
    cu = cu_of(DOC.mixed_rows(S))
    for causal in (0, 1):
        W.assert_same(run(code, q, k, v, go, cu, causal)[:5], DOC.run(code, q, k, v, go, cu, bool(causal)), f"causal {causal}: not kf_attn_doc_*'s bits")


# A window with two bounded sides on a row whose last wave is partial (S no multiple of 32) is the one place where the two families'
# bits part, in both dtypes and head sizes: the window kernel lets the wave's rows beyond Sq (q = 0, never stored) see the keys of their
# window, the document kernel reads no table for them and gives them the empty interval. Such a row can meet its first key in the row's
# last key tile, and the deferred running maximum is adopted by the whole wave when any row asks: the real rows of that wave then
# rescale in a tile where, under the document kernel, they do not. Both results lie within the float64 bounds (test_matrix_core_fwd_bwd
# runs w(5,7) on such rows); DESIGN.md section 4.9.6 records it.
RAGGED = pytest.mark.xfail(strict=True, reason="o, lse and dq of the rows m >= 32 floor(S / 32) (the partial last wave) and dk of keys they see differ from "
                           "kf_attn_window_*: in the last key tile the window kernel's rows beyond Sq make the wave adopt a new deferred maximum")
ONE_DOC = [(code, D, S, w) for code, D, S in ((H.BF16, 128, 257), (H.F16, 64, 130)) for w in ((40, 0), (0, 0), (None, 3), (70, 70))]
ONE_DOC += [(code, D, S, w) for code, D, S in ((H.BF16, 128, 288), (H.F16, 64, 128)) for w in ((17, 5), (5, 7))]
ONE_DOC += [pytest.param(code, D, S, (17, 5), marks=RAGGED) for code, D, S in ((H.BF16, 128, 257), (H.F16, 64, 130))]


@pytest.mark.parametrize("code,D,S,window", ONE_DOC)
def test_one_document_with_a_window_is_the_window_call(code, D, S, window):
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    cu = np.array([[0, S], [0, S]], np.int64)
    wl, wr = (-1 if x is None else x for x in window)
    want = W.run(code, q, k, v, go, None, window)
    for causal in ((0, 1) if wr == 0 else (0,)):        # with right = 0 the causal rule adds nothing
        W.assert_same(run(code, q, k, v, go, cu, causal, wl, wr)[:5], want, f"one document, window {window}, causal {causal}: not kf_attn_window_*'s bits")


@pytest.mark.parametrize("code,D,S", [(H.BF16, 128, 257), (H.F16, 64, 130)])
def test_one_document_with_a_prefix_is_the_prefix_call(code, D, S):
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    cu = np.array([[0, S], [0, S]], np.int64)
    pre = [S // 2 | 1, 37]
    got = run(code, q, k, v, go, cu, 1, pre=np.array(pre, np.int64)[:, None])
    W.assert_same(got[:5], P.run(code, q, k, v, go, None, pre), "one document with a prefix: not kf_attn_prefix_*'s bits")


@pytest.mark.parametrize("L,n", [(128, 3), (256, 2)])
@pytest.mark.parametrize("code,D,Hq,Hkv", [(H.BF16, 128, 2, 2), (H.F16, 64, 4, 2)])
def test_equal_documents_with_a_window_are_the_batched_window_call(code, D, Hq, Hkv, L, n):
    """documents of one length L (a multiple of the 128-row block) are a batch of B n sequences"""
    B, S = 2, L * n
    rng = np.random.default_rng(L + D + Hq)
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, S, S, D)
    cu = np.tile(np.arange(n + 1, dtype=np.int64) * L, (B, 1))
    split = lambda x: np.ascontiguousarray(x.reshape(B, x.shape[1], n, L, D).transpose(0, 2, 1, 3, 4).reshape(B * n, x.shape[1], L, D))  # noqa: E731
    join = lambda x: np.ascontiguousarray(x.reshape((B, n, x.shape[1], L) + x.shape[3:]).swapaxes(1, 2).reshape((B, x.shape[1], S) + x.shape[3:]))  # noqa: E731
    got = run(code, q, k, v, go, cu, 1, 40, 0)
    want = W.run(code, split(q), split(k), split(v), split(go), None, (40, 0))
    W.assert_same(got[:5], tuple(join(x) for x in want), f"documents of {L}, window (40, 0): not the bits of the batched window call")


@pytest.mark.parametrize("softcap,with_sink", [(0.25, False), (0.0, True), (0.25, True)])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_modifiers_without_a_window_are_the_ext_document_call(code, D, softcap, with_sink):
    S, Hq = 200, 4
    rng = np.random.default_rng(D + int(4 * softcap))
    q, k, v, go = F.inputs(rng, code, 4, Hq, 2, S, S, D)
    cu = cu_of(DOC.mixed_rows(S))
    sink = sinks_for(Hq) if with_sink else None
    for causal in (0, 1):
        got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, causal, softcap=softcap, sink=sink))
        want = EXT.run(code, q, k, v, go, ("doc", cu, bool(causal)), softcap, sink)
        W.assert_same(got[:5], want[:5], f"cap {softcap} sink {with_sink} causal {causal}: not kf_attn_ext_*'s bits")
        if with_sink:
            assert F.same(got[5], want[5]), "dsink"
        EXT.check_labels(labels - {"attn_span_table"}, ("doc", cu, bool(causal)), D, softcap, sink)


# ---- soft-capping and sinks under a causal window ----
@pytest.mark.parametrize("softcap,with_sink", [(0.25, False), (0.0, True), (0.25, True)])
@pytest.mark.parametrize("code,D,S", [(H.BF16, 64, 200), (H.F16, 128, 257)])
def test_modifiers_under_a_causal_window(code, D, S, softcap, with_sink):
    Hq = 4
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 4, Hq, 2, S, S, D)
    cu = cu_of(DOC.mixed_rows(S))
    sink = sinks_for(Hq) if with_sink else None
    got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, 1, 31, 0, softcap=softcap, sink=sink))
    EXT.check16(code, q, k, v, go, got, span_vis(cu, S, 1, 31, 0), softcap, sink, f"S {S} D{D} cap {softcap} sink {with_sink}")
    EXT.check_labels(labels - {"attn_span_table"}, ("doc", cu, True), D, softcap, sink)


# ---- every output is written in full, whatever it held ----
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64), (H.F32, 64)])
def test_outputs_are_written_in_full(code, D):
    S = 257 if code != H.F32 else 70
    rng = np.random.default_rng(D + code)
    q, k, v, go = F.inputs(rng, code, 2, 2, 1, S, S, D)
    cu = cu_of([[S // 3, S - S // 3], [S // 4, S // 4]])     # the second row: a tail of half the row in no document
    pre = np.array([[9, 40], [0, 33]], np.int64)
    want = run(code, q, k, v, go, cu, 1, 20, -1, pre, fill=0x00)
    for fill in (0xFF, 0x7F):
        got = run(code, q, k, v, go, cu, 1, 20, -1, pre, fill=fill)
        W.no_nan(code, got[:5], f"fill {fill:#x}")
        W.assert_same(got[:5], want[:5], f"outputs or workspace pre-filled with {fill:#x} changed the result")


# ---- K and V rows at n >= len_b are never read ----
@pytest.mark.parametrize("poison_value", [np.nan, np.inf])
@pytest.mark.parametrize("code,D,mask", [(H.BF16, 128, (1, 31, 0, False)), (H.F16, 64, (0, 5, 7, False)), (H.BF16, 80, (1, -1, -1, True))])
def test_padding_never_reaches_an_output(poison_value, code, D, mask):
    S = 200
    rows = [[200], [], [1], [30, 34], [65], [100, 50]]
    lens = [sum(r) for r in rows]
    cu = cu_of(rows)
    causal, wl, wr, with_prefix = mask
    pre = np.array([[77, 0], [0, 0], [1, 0], [11, 17], [33, 0], [45, 49]], np.int64) if with_prefix else None
    rng = np.random.default_rng(64 + code)
    q, k, v, go = F.inputs(rng, code, len(rows), 2, 2, S, S, D)
    kz, vz = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    kp, vp = kz.copy(), vz.copy()
    for b, ln in enumerate(lens):
        kz[b, :, ln:] = 0
        vz[b, :, ln:] = 0
        kp[b, :, ln:] = poison_value
        vp[b, :, ln:] = -poison_value
    clean = run(code, q, O.from_float(kz, code), O.from_float(vz, code), go, cu, causal, wl, wr, pre)
    W.check16(code, q, k, v, go, clean[:5], span_vis(cu, S, causal, wl, wr, pre), "zero padding")
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, cu, causal, wl, wr, pre)
    W.assert_same(dirty[:5], clean[:5], f"padding of {poison_value} changed the result")


# ---- grouped K/V heads ----
@pytest.mark.parametrize("Hq,Hkv", [(2, 1), (4, 2)])
@pytest.mark.parametrize("code,D,mask", [(H.BF16, 128, (1, 31, 0, False)), (H.F16, 64, (0, 5, 7, False)), (H.BF16, 64, (1, 40, -1, True))])
def test_gqa(code, D, mask, Hq, Hkv):
    S = 200
    cu = cu_of([[77, 123], [40, 33, 57], [200]])
    causal, wl, wr, with_prefix = mask
    pre = np.array([[30, 61, 0], [7, 33, 1], [99, 0, 0]], np.int64) if with_prefix else None
    rng = np.random.default_rng(Hkv + D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, Hkv, S, S, D)
    got = run(code, q, k, v, go, cu, causal, wl, wr, pre)
    W.check16(code, q, k, v, go, got[:5], span_vis(cu, S, causal, wl, wr, pre), f"gqa {Hq}/{Hkv}")


# ---- strided: the packed projection read in place ----
@pytest.mark.parametrize("code,D,S,mask", [(H.BF16, 128, 200, (1, 31, 0, False)), (H.F16, 64, 129, (1, 20, -1, True))])
def test_packed_layout_equals_contiguous(code, D, S, mask):
    B, Hq, Hkv = 2, 4, 2
    Wd, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = Wd + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = F.rnd(rng, code, (B * S, Wd)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    cu = cu_of([[S // 3, S - S // 3], [41, S - 70 - 41]])
    causal, wl, wr, with_prefix = mask
    pre = np.array([[13, 50], [40, 9]], np.int64) if with_prefix else None
    ref = run(code, q, k, v, go, cu, causal, wl, wr, pre)
    packed, flat, gpack = (S * Wd, D, Wd), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout)
    t = Tables(cu, S, causal, wl, wr, pre)
    t.launch()
    ob, o = F.guarded(B * S * d * es)
    lb, lse = F.guarded(4 * B * Hq * S)
    gb, g = F.guarded(B * S * PADW * es)
    scale = F.scale_of(D)
    H.attn_span_fwd(code, B, Hq, Hkv, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, layouts=(packed, packed, packed, flat),
                    **t.fwd_kw())
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    poison.fill(w.ptr, need, 0xFF)
    H.attn_span_bwd(code, B, Hq, Hkv, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                    g + (d + dkv) * es, w.ptr, need, layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack), **t.bwd_kw())
    H.device_sync()
    assert F.same(heads(F.read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert F.same(F.read(lse, (B, Hq, S), np.float32), ref[1])
    gq = F.read(g, (B * S, PADW), qkv.dtype)
    assert F.same(heads(gq[:, :d], Hq), ref[2]) and F.same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and F.same(heads(gq[:, d + dkv:Wd], Hkv), ref[4])
    assert (gq[:, Wd:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, nb in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es)):
        assert F.guards_ok(buf, nb)


# ---- generic path ----
@pytest.mark.parametrize("mask", [(1, 31, 0, False), (0, 5, 7, False), (1, 20, -1, True)])
@pytest.mark.parametrize("S", [33, 96, 300])
@pytest.mark.parametrize("code,D", [(H.F32, 64), (H.BF16, 80)])
def test_generic(code, D, S, mask):
    causal, wl, wr, with_prefix = mask
    cu, pre = case_mask(S, causal, wl, wr, with_prefix)
    rng = np.random.default_rng(D + S + code)
    q, k, v, go = F.inputs(rng, code, 4, 4, 2, S, S, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, cu, causal, wl, wr, pre))
    got = got[:5]
    vis = span_vis(cu, S, causal, wl, wr, pre)
    W.no_nan(code, got)
    if code == H.F32:
        W.check_generic(code, q, k, v, go, got, vis)
        W.zeros_where_nothing_is_seen(got, vis)
    else:
        W.check16(code, q, k, v, go, got, vis, f"generic D{D}")
    labels = labels - {"attn_span_table"}
    assert DOC.GENERIC_LABELS <= labels and not any("mfma" in n for n in labels), sorted(labels)
    assert all(n.startswith("attn_doc_") or n == "attn_full_bwd_delta_generic" for n in labels), sorted(labels)


# ---- determinism, graph capture (the table launch included) ----
def test_reproducible_and_capturable():
    rng = np.random.default_rng(513)
    for code, D, Hq, Hkv, S, rows, mask, mods in ((H.BF16, 128, 2, 2, 513, [[100, 257, 156], [300, 100]], (1, 64, 0, None), {}),
                                                  (H.F16, 64, 4, 1, 200, [[64, 64, 72], [33]], (1, 20, -1, [[31, 9, 50], [12, 0, 0]]), dict(softcap=0.25, sink=sinks_for(4)))):
        cu = cu_of(rows)
        causal, wl, wr, pre = mask
        pre = None if pre is None else np.array(pre, np.int64)
        q, k, v, go = F.inputs(rng, code, 2, Hq, Hkv, S, S, D)
        a, b, g = (run(code, q, k, v, go, cu, causal, wl, wr, pre, graph=gr, **mods) for gr in (False, False, True))
        W.assert_same(a[:5], b[:5], "two runs differ")
        W.assert_same(a[:5], g[:5], "the captured run differs from the eager one")
        if mods:
            assert F.same(a[5], b[5]) and F.same(a[5], g[5]), "dsink"
