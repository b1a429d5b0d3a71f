"""-m gpu: kfunca.doc_mask(cu_doclens, S, window=, prefix_lens=, causal=) and kfunca.attention / kfunca.attention_qkv with such a mask:
a sliding window, a causal rule and per-document prefixes inside packed documents.

The results are held to tests/attn_full_ref.py's float64 attention under tests/attn_span_ref.py's span_vis and to torch's
scaled_dot_product_attention on the CPU in f32, both through tests/test_gpu_attn_window.py's check_operator (its bounds, unchanged), with
gradients. With soft-capping and sinks the operator must give the bits of the C entries it calls (tests/test_gpu_attn_span.py holds those
to the float64 reference). A plain doc_mask(cu_doclens, S) must keep making the calls it made before: kf_attn_doc_*'s labels and bits."""
import numpy as np
import pytest

import kfunca_amd as kfunca
import tests.test_gpu_attn_doc as DOC
import tests.test_gpu_attn_full as F
import tests.test_gpu_attn_span as SPAN
import tests.test_gpu_attn_window as W
from kfunca_amd import hip_abi as H
from tests.attn_doc_ref import cu_of, doc_table
from tests.attn_ext_ref import sinks_for
from tests.attn_span_ref import span_table, span_vis

pytestmark = pytest.mark.gpu

dev_long = DOC.dev_long
OP_ROWS = DOC.OP_ROWS       # every row keeps at least 3/4 of its tokens inside documents
PREFIXES = {90: [[13, 50], [9, 0, 17]], 129: [[30, 33], [25, 1, 40]]}       # one beyond its document (50 of 50: all of it), one empty
# (window, with prefixes, causal); (0, 0) is not among them: with one key per query dq is zero in exact arithmetic
OP_MASKS = [((5, 0), False, False), ((5, None), False, True), ((7, 7), False, False), ((None, 3), False, False), (None, False, True), (None, True, True),
            ((9, None), True, True), ((9, 0), True, True)]


def abi_mask(window, with_prefix, causal, S):
    """the arguments of kf_attn_span_table that doc_mask(window=, prefix_lens=, causal=) stands for: causal closes the right side, prefixes
    leave it to the causal rule"""
    wl, wr = (-1, -1) if window is None else (-1 if window[0] is None else window[0], -1 if window[1] is None else window[1])
    if causal:
        wr = -1 if with_prefix else 0
    pre = None
    if with_prefix:
        rows = PREFIXES[S]
        n = max(len(r) for r in rows)
        pre = np.array([r + [0] * (n - len(r)) for r in rows], np.int64)
    return int(causal), wl, wr, pre


def build(cu, S, window, with_prefix, causal):
    c, wl, wr, pre = abi_mask(window, with_prefix, causal, S)
    mask = kfunca.doc_mask(dev_long(cu), S, window=window, prefix_lens=None if pre is None else dev_long(pre), causal=causal)
    return mask, (c, wl, wr, pre)


@pytest.mark.parametrize("window,with_prefix,causal", OP_MASKS)
def test_doc_mask_object(window, with_prefix, causal):
    S = 90
    cu = cu_of(OP_ROWS[S])
    mask, (c, wl, wr, pre) = build(cu, S, window, with_prefix, causal)
    kv, klo, khi, qlo, qhi = span_table(cu, S, c, wl, wr, pre)
    assert mask.B == 2 and mask.S == S and mask.span and mask.causal == causal
    assert np.array_equal(mask.kv_len.numpy(), kv)
    for name, want in (("doc_start", klo), ("doc_end", khi), ("key_lo", klo), ("key_hi", khi), ("query_lo", qlo), ("query_hi", qhi)):
        got = getattr(mask, name).numpy()
        assert got.dtype == np.int32 and np.array_equal(got, want), name
    left, right = (None, None) if window is None else window
    right = 0 if causal else right                     # causal closes the right side; the mask keeps its window as attention would read it
    assert mask.window == (None if left is None and right is None else (left, right))


def test_a_plain_doc_mask_is_what_it_was():
    S = 90
    cu = cu_of(OP_ROWS[S])
    for kw in (dict(), dict(window=None, prefix_lens=None, causal=False)):
        mask, labels = F.profiled(lambda: kfunca.doc_mask(dev_long(cu), S, **kw))
        assert {n for n in labels if n.startswith("attn_")} == {"attn_doc_table"}, sorted(labels)
        kv, s, e = doc_table(cu, S)
        assert np.array_equal(mask.kv_len.numpy(), kv) and np.array_equal(mask.doc_start.numpy(), s) and np.array_equal(mask.doc_end.numpy(), e)
        assert not mask.span and mask.query_lo is None and mask.query_hi is None and mask.window is None and mask.causal is False


@pytest.mark.parametrize("causal", [False, True])
def test_a_plain_doc_mask_makes_the_previous_calls(causal):
    """the operator with a plain mask launches what it launched before masks could hold a window: kf_attn_doc_*'s labels and bits"""
    code, D, S = H.BF16, 64, 129
    rng = np.random.default_rng(7)
    cu = cu_of(OP_ROWS[S])
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, S, S, D)
    want = DOC.run(code, q, k, v, go, cu, causal)
    mask = kfunca.doc_mask(dev_long(cu), S)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)

    def call():
        out = kfunca.attention(tq, tk, tv, causal=causal, doc_mask=mask)
        out.backward(F.value(go, code))
        return out

    out, labels = F.profiled(call)
    mine = {n for n in labels if n.startswith("attn_")}
    assert mine == {"attn_doc_fwd_mfma_d64", "attn_full_bwd_delta", "attn_doc_bwd_dq_mfma_d64", "attn_doc_bwd_dkv_mfma_d64"}, sorted(labels)
    for name, t, w in zip(("o", "dq", "dk", "dv"), (out, tq.grad(), tk.grad(), tv.grad()), (want[0], want[2], want[3], want[4])):
        assert F.same(F.as_np(t, code), w), name


@pytest.mark.parametrize("window,with_prefix,causal", OP_MASKS)
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention(code, D, window, with_prefix, causal):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv, S = 2, 4, 2, 90
    cu = cu_of(OP_ROWS[S])
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, S, S, D)
    mask, (c, wl, wr, pre) = build(cu, S, window, with_prefix, causal)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, causal=causal, doc_mask=mask))
    out.backward(F.value(go, code))
    got = [F.as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
    assert got[0].shape == q.shape and got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    W.check_operator(code, q, k, v, go, span_vis(cu, S, c, wl, wr, pre), got, f"attention D{D} window {window} prefixes {with_prefix} causal {causal}")
    if code == H.BF16:   # head size 40 is zero-padded to 64: the matrix-core kernels
        assert "attn_doc_fwd_mfma_d64" in labels, sorted(labels)
    else:
        assert "attn_doc_fwd_generic" in labels, sorted(labels)
    assert not any(n.startswith(("attn_full_fwd", "attn_prefix_", "attn_window_")) for n in labels), sorted(labels)


@pytest.mark.parametrize("window,with_prefix,causal", OP_MASKS)
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention_qkv(code, D, window, with_prefix, causal):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq, Hkv = 2, 129, 4, 2
    Wd, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    cu = cu_of(OP_ROWS[S])
    qkv, gout = F.rnd(rng, code, (B * S, Wd)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    mask, (c, wl, wr, pre) = build(cu, S, window, with_prefix, causal)
    tx = F.leaf(qkv, code)
    out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=Hkv, causal=causal, doc_mask=mask)
    out.backward(F.value(gout, code))
    o2, g2 = F.as_np(out, code), F.as_np(tx.grad(), code)
    assert o2.shape == (B * S, d) and g2.shape == qkv.shape
    got = [heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv)]
    W.check_operator(code, q, k, v, go, span_vis(cu, S, c, wl, wr, pre), got, f"attention_qkv D{D} window {window} prefixes {with_prefix} causal {causal}")


@pytest.mark.parametrize("softcap,with_sink", [(0.25, False), (None, True), (0.25, True)])
def test_modifiers_have_the_bits_of_the_entries(softcap, with_sink):
    code, D, S, Hq, Hkv = H.BF16, 64, 129, 4, 2
    rng = np.random.default_rng(11)
    cu = cu_of(OP_ROWS[S])
    q, k, v, go = F.inputs(rng, code, 2, Hq, Hkv, S, S, D)
    mask, (c, wl, wr, pre) = build(cu, S, (9, None), True, True)
    sink = sinks_for(Hq) if with_sink else None
    want = SPAN.run(code, q, k, v, go, cu, c, wl, wr, pre, softcap=softcap or 0.0, sink=sink)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    ts = None
    if with_sink:
        ts = kfunca.from_numpy(sink, 0)
        ts.set_requires_grad(True)
    out = kfunca.attention(tq, tk, tv, causal=True, doc_mask=mask, softcap=softcap, sinks=ts)
    out.backward(F.value(go, code))
    for name, t, w in zip(("o", "dq", "dk", "dv"), (out, tq.grad(), tk.grad(), tv.grad()), (want[0], want[2], want[3], want[4])):
        assert F.same(F.as_np(t, code), w), name
    if with_sink:
        assert F.same(ts.grad().numpy(), want[5]), "dsink"


def test_refusals():
    rng = np.random.default_rng(1)
    q, k, v, _ = F.inputs(rng, H.BF16, 2, 2, 2, 8, 8, 64)
    tq, tk, tv = (F.value(x, H.BF16) for x in (q, k, v))
    packed = F.value(F.rnd(rng, H.BF16, (16, 6 * 64)), H.BF16)
    cu = dev_long([[0, 3, 8], [0, 8, 8]])
    lens = dev_long([1, 2])
    calls = (("attention", lambda mask, **kw: kfunca.attention(tq, tk, tv, doc_mask=mask, **kw)),
             ("attention_qkv", lambda mask, **kw: kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, doc_mask=mask, **kw)))
    # the call's causal must repeat the mask's: the text names both values
    windowed, causal_mask = kfunca.doc_mask(cu, 8, window=(2, 2)), kfunca.doc_mask(cu, 8, window=(2, None), causal=True)
    for op, call in calls:
        with pytest.raises(Exception, match=f"{op}: causal = true but doc_mask was built with causal = false"):
            call(windowed, causal=True)
        with pytest.raises(Exception, match=f"{op}: causal = false but doc_mask was built with causal = true"):
            call(causal_mask)
        call(windowed)
        call(causal_mask, causal=True)
        # window, prefix_len and kv_len beside a mask stay refused, whichever form the mask has; the text points to doc_mask's arguments
        for mask, causal in ((windowed, False), (causal_mask, True), (kfunca.doc_mask(cu, 8), False)):
            for kw in (dict(kv_len=lens), dict(prefix_len=lens), dict(window=(4, 0)), dict(kv_len=lens, window=(4, None))):
                with pytest.raises(Exception, match=rf"{op}: doc_mask cannot be combined with kv_len, prefix_len or window .*doc_mask\(cu_doclens, S, window="):
                    call(mask, causal=causal, **kw)
    # a mask of another B or S, windowed or not
    for other in (kfunca.doc_mask(dev_long([[0, 8]]), 8, window=(1, 1)), kfunca.doc_mask(dev_long([[0, 3, 9], [0, 9, 9]]), 9, causal=True)):
        with pytest.raises(Exception, match="attention: doc_mask was built for B = "):
            kfunca.attention(tq, tk, tv, doc_mask=other, causal=other.causal)
    # doc_mask's own
    pre = dev_long([[1, 2], [3, 0]])
    with pytest.raises(Exception, match="doc_mask: prefix_lens needs causal = true"):
        kfunca.doc_mask(cu, 8, prefix_lens=pre)
    with pytest.raises(Exception, match="doc_mask: causal = true means window right = 0, got right = 3"):
        kfunca.doc_mask(cu, 8, window=(2, 3), causal=True)
    for bad in ((-1, 0), (2, -4), (1, 2, 3), 5, (1.5, 0)):
        with pytest.raises(Exception, match="doc_mask: window is a pair"):
            kfunca.doc_mask(cu, 8, window=bad)
    for bad in (dev_long([[1, 2, 3], [3, 0, 0]]), dev_long([1, 2]), dev_long([[1, 2]]), kfunca.from_numpy(np.zeros((2, 2), np.float32), 0)):
        with pytest.raises(Exception, match="doc_mask: prefix_lens must be of type Long and shape"):
            kfunca.doc_mask(cu, 8, prefix_lens=bad, causal=True)
    with pytest.raises(Exception, match="doc_mask expects cu_doclens"):
        kfunca.doc_mask(dev_long([0, 8]), 8, window=(1, 1))
