"""-m gpu: kfunca.attention(..., softcap=, sinks=) and kfunca.attention_qkv(..., softcap=, sinks=) through Tensor.backward.

The reference is torch on the CPU in f32, where softcap is a tanh on the scores and the sink a logit column that is concatenated before
the softmax and dropped after it; the comparison is tests/test_gpu_attn_window.py's: max |got - ref| <= TOL max |ref| with TOL = 2^-5
(bf16) and 1e-4 (f32), over the rows that see a key for o and dq (the others must be zeros), and for sinks.grad over its Hq entries.
sinks is a fourth differentiable input: its gradient is a Float [Hq]. The refusals carry the operator's name."""
import numpy as np
import pytest

import kfunca_amd as kfunca
import tests.test_gpu_attn_full as F
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.attn_doc_ref import cu_of, doc_vis
from tests.attn_ext_ref import CAPS, sinks_for
from tests.attn_full_ref import key_len_vis
from tests.attn_window_ref import window_vis
from tests.test_attn_ext_ref import prefix_vis

pytestmark = pytest.mark.gpu


def torch_ref(q, k, v, go, vis, softcap, sink):
    """o, dq, dk, dv, dsink in f32 on the CPU. A row without a key is given zero weights by hand (torch has no answer for it)."""
    import torch
    G = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float32, requires_grad=True) for x in (q, k, v))
    ts = None if sink is None else torch.tensor(np.asarray(sink, np.float32), requires_grad=True)
    x = tq @ tk.repeat_interleave(G, dim=1).transpose(-1, -2) / float(np.sqrt(q.shape[-1]))
    if softcap:
        x = softcap * torch.tanh(x / softcap)
    x = x.masked_fill(~torch.tensor(vis)[:, None], -np.inf)
    if ts is not None:
        x = torch.cat([x, ts[None, :, None, None].expand(x.shape[0], -1, x.shape[2], 1)], dim=-1)
    live = torch.isfinite(x).any(dim=-1, keepdim=True)
    p = torch.where(live, torch.softmax(torch.where(live, x, torch.zeros_like(x)), dim=-1), torch.zeros_like(x))
    o = p[..., :vis.shape[2]] @ tv.repeat_interleave(G, dim=1)
    o.backward(torch.tensor(go, dtype=torch.float32))
    out = [o, tq.grad, tk.grad, tv.grad] + ([ts.grad] if ts is not None else [])
    return [t.detach().numpy().astype(np.float64) for t in out]


def compare(code, got, want, vis, shape3, what):
    tol = 2.0 ** -5 if code == H.BF16 else 1e-4
    live = np.broadcast_to(vis.any(axis=2)[:, None, :], shape3)
    for name, a, r in zip(("o", "dq", "dk", "dv", "dsink"), got, want):
        a = np.asarray(a, np.float64)
        assert a.shape == r.shape, (what, name, a.shape, r.shape)
        assert np.isfinite(a).all(), (what, name)
        if name in ("o", "dq"):
            assert (a[~live] == 0).all(), (what, name)
            a, r = a[live], r[live]
        err = np.abs(a - r).max()
        print(f"{what} {name}: max error {err:.3e}, bound {tol * np.abs(r).max():.3e}")
        assert err <= tol * np.abs(r).max(), (what, name, err, tol * np.abs(r).max())


def dev_long(x):
    return None if x is None else kfunca.from_numpy(np.asarray(x, np.int64), 0)


def sink_leaf(sink):
    t = kfunca.from_numpy(np.asarray(sink, np.float32), 0)
    t.set_requires_grad(True)
    return t


# (mask keywords, visibility): the four kinds, the window one with queries that see no key
def mask_cases(B, Sq, Skv):
    lens = [Skv, 33]
    out = [("full", dict(kv_len=lens), key_len_vis(lens, Sq, Skv, B)),
           ("prefix", dict(kv_len=lens, causal=True, prefix_len=[20, 5]), prefix_vis(lens, [20, 5], Sq, Skv)),
           ("window", dict(kv_len=lens, window=(5, 0)), window_vis(lens, 5, 0, Sq, Skv, B))]
    if Sq == Skv:
        cu = cu_of([[40, Sq - 50], [33, 20, 17]], 3)
        out.append(("doc", dict(doc=cu, causal=True), doc_vis(cu, Sq, True)))
    return out


def keywords(kw, S):
    kw = dict(kw)
    for n in ("kv_len", "prefix_len"):
        if n in kw:
            kw[n] = dev_long(kw[n])
    if "doc" in kw:
        kw["doc_mask"] = kfunca.doc_mask(dev_long(kw.pop("doc")), S)
    return kw


MODS = [(CAPS[0], False), (None, True), (CAPS[1], True)]


@pytest.mark.parametrize("softcap,with_sink", MODS)
@pytest.mark.parametrize("code,D,Sq,Skv", [(H.BF16, 64, 90, 70), (H.BF16, 40, 90, 90), (H.F32, 48, 70, 70)])
def test_operator_attention(code, D, Sq, Skv, softcap, with_sink):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv = 2, 4, 2
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, Sq, Skv, D)
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    sink = sinks_for(Hq, D) if with_sink else None
    for name, kw, vis in mask_cases(B, Sq, Skv):
        tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
        ts = sink_leaf(sink) if with_sink else None
        out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, softcap=softcap, sinks=ts, **keywords(kw, Sq)))
        out.backward(F.value(go, code))
        got = [f(F.as_np(t, code)) for t in (out, tq.grad(), tk.grad(), tv.grad())]
        if with_sink:
            g = ts.grad()
            assert g.sizes() == [Hq] and g.dtype() == kfunca.float, (g.sizes(), g.dtype())
            got.append(g.numpy())
        compare(code, got, torch_ref(f(q), f(k), f(v), f(go), vis, softcap, sink), vis, q.shape[:3], f"attention {name} D{D} cap {softcap} sink {with_sink}")
        mid = "_cap" if softcap else ""
        want = f"attn_{name}{mid}_fwd_mfma_d64" if code == H.BF16 else f"attn_{name}{mid}_fwd_generic"    # head size 40 is zero-padded to 64
        assert want in labels, sorted(labels)


@pytest.mark.parametrize("softcap,with_sink", MODS)
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention_qkv(code, D, softcap, with_sink):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq, Hkv = 2, 129, 4, 2
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    sink = sinks_for(Hq, D) if with_sink else None
    for name, kw, vis in mask_cases(B, S, S):
        tx = F.leaf(qkv, code)
        ts = sink_leaf(sink) if with_sink else None
        out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=Hkv, softcap=softcap, sinks=ts, **keywords(kw, S))
        out.backward(F.value(gout, code))
        o2, g2 = F.as_np(out, code), F.as_np(tx.grad(), code)
        assert o2.shape == (B * S, d) and g2.shape == qkv.shape
        got = [f(x) for x in (heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv))]
        if with_sink:
            assert ts.grad().sizes() == [Hq]
            got.append(ts.grad().numpy())
        compare(code, got, torch_ref(f(q), f(k), f(v), f(go), vis, softcap, sink), vis, q.shape[:3], f"attention_qkv {name} D{D} cap {softcap} sink {with_sink}")


def test_sinks_alone_can_require_grad():
    """q, k, v without grad, sinks with: the output still has a backward and only sinks receives a gradient"""
    code = H.BF16
    rng = np.random.default_rng(3)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, 33, 33, 64)
    ts = sink_leaf(sinks_for(4))
    out = kfunca.attention(F.value(q, code), F.value(k, code), F.value(v, code), sinks=ts)
    out.backward(F.value(go, code))
    assert np.isfinite(ts.grad().numpy()).all() and np.abs(ts.grad().numpy()).max() > 0


def test_none_keywords_make_the_previous_calls():
    code = H.BF16
    rng = np.random.default_rng(4)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, 70, 90, 64)
    tq, tk, tv = (F.value(x, code) for x in (q, k, v))
    a, la = F.profiled(lambda: kfunca.attention(tq, tk, tv, window=(5, 0)))
    b, lb = F.profiled(lambda: kfunca.attention(tq, tk, tv, window=(5, 0), softcap=None, sinks=None))
    assert F.same(F.as_np(a, code), F.as_np(b, code)) and la == lb and "attn_window_fwd_mfma_d64" in lb


def test_refusals():
    rng = np.random.default_rng(1)
    q, k, v, _ = F.inputs(rng, H.BF16, 2, 4, 2, 8, 8, 64)
    tq, tk, tv = (F.value(x, H.BF16) for x in (q, k, v))
    packed = F.value(F.rnd(rng, H.BF16, (16, 8 * 64)), H.BF16)
    good = kfunca.from_numpy(np.zeros(4, np.float32), 0)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 0):
        with pytest.raises(Exception, match="attention: softcap must be positive and finite"):
            kfunca.attention(tq, tk, tv, softcap=bad)
        with pytest.raises(Exception, match="attention_qkv: softcap must be positive and finite"):
            kfunca.attention_qkv(packed, 2, 8, 4, kv_heads=2, softcap=bad, sinks=good)
    with pytest.raises(Exception, match="softcap is a positive float"):
        kfunca.attention(tq, tk, tv, softcap="50")
    with pytest.raises(Exception, match="attention: sinks must be of type Float"):
        kfunca.attention(tq, tk, tv, sinks=good.bfloat16())
    for shape in ((3,), (8,), (4, 1), (1, 4)):
        with pytest.raises(Exception, match="attention: sinks must be a dense tensor of shape \\[Hq\\]"):
            kfunca.attention(tq, tk, tv, sinks=kfunca.from_numpy(np.zeros(shape, np.float32), 0))
        with pytest.raises(Exception, match="attention_qkv: sinks must be a dense tensor of shape \\[Hq\\]"):
            kfunca.attention_qkv(packed, 2, 8, 4, kv_heads=2, sinks=kfunca.from_numpy(np.zeros(shape, np.float32), 0))
    if kfunca.device_count() > 1:
        with pytest.raises(Exception, match="attention: sinks must be on the operands' device"):
            kfunca.attention(tq, tk, tv, sinks=kfunca.from_numpy(np.zeros(4, np.float32), 1))
