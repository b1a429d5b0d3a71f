"""-m gpu: full (non-causal) attention with per-batch key lengths and grouped K/V heads (kf_attn_full_fwd / kf_attn_full_bwd,
kfunca.attention, kfunca.attention_qkv).

The reference is tests/attn_full_ref.py (float64, pinned to the oracle by tests/test_attn_full_ref.py); the 16-bit outputs are held to
the project's scale-aware bounds (oracle.checks.check_one: element, row and head), lse to 2e-6 (1 + |lse|) and to -inf exactly where a
row has no visible key; the generic path to the tolerances smoke() uses for f32 attention (rtol 1e-4 / atol 1e-4 forward, rtol 1e-3 /
atol 1e-4 backward). Inputs are U(-1, 1) rounded to the dtype. The matrix-core kernels use 128-row query blocks and 64-key tiles
(forward, dQ) and 128-key blocks with 64-query tiles (dK/dV): the shapes sit one below, at and one above those sizes.
Operator tests also compare with torch's scaled_dot_product_attention on the CPU in f32 under a boolean mask built from kv_len:
max |got - ref| <= TOL max |ref| per tensor, TOL = 2^-5 (bf16: 8 significant bits, outputs and gradients rounded once and P, dS rounded
inside) and 1e-4 (f32), the figures tests/test_gpu_attention_gqa.py states for the causal operators."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O
from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis, key_len_vis

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024


def rnd(rng, code, shape):
    return O.from_float(rng.uniform(-1, 1, shape).astype(np.float32), code)


def scale_of(D):
    return float(np.float32(1.0) / np.sqrt(np.float32(D)))


def bits(x):
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def inputs(rng, code, B, Hq, Hkv, Sq, Skv, D):
    q, go = rnd(rng, code, (B, Hq, Sq, D)), rnd(rng, code, (B, Hq, Sq, D))
    k, v = rnd(rng, code, (B, Hkv, Skv, D)), rnd(rng, code, (B, Hkv, Skv, D))
    return q, k, v, go


def run(code, q, k, v, go, kv_len=None, stream=None, graph=False):
    """kf_attn_full_fwd + kf_attn_full_bwd on contiguous tensors: o, lse, dq, dk, dv (graph: captured with kf_graph_* and launched once)."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    scale = scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bl = None if kv_len is None else H.DevBuf.from_numpy(np.asarray(kv_len, np.int64))
    lp = None if bl is None else bl.ptr
    bo, blse = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * Sq)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    w = H.DevBuf(need)
    fill = np.full(max(need, 1), 0xFF, np.uint8)   # the workspace needs no initialisation: NaN patterns
    H.check(H.lib().kf_memcpy_h2d(w.ptr, fill.ctypes.data, need, None))
    dq, dk, dv = H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(v.nbytes)
    H.device_sync()

    def calls(st):
        H.attn_full_fwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, kv_len=lp, stream=st)
        H.attn_full_bwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need,
                        kv_len=lp, stream=st)

    if graph:
        s = H.Stream()
        with H.Graph.capture(s) as g:
            calls(s.handle)
        g.launch()
        s.sync()
    else:
        calls(None)
    H.device_sync()
    return (bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, Sq), np.float32), dq.to_numpy(q.shape, q.dtype), dk.to_numpy(k.shape, k.dtype),
            dv.to_numpy(v.shape, v.dtype))


def check16(code, q, k, v, go, got, kv_len=None, what=""):
    B, _, Sq, _ = q.shape
    vis = key_len_vis(kv_len, Sq, k.shape[2], B)
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    fl = format_floor_vis(q, k, v, go, vis, code)
    for name, g in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4])):
        K.check_one(name, g, ref, code, what, floor=fl.get(name))
    check_lse(got[1], ref, what)
    return ref


def profiled(f):
    H.profile_reset()
    H.profile_enable(True)
    try:
        out = f()
    finally:
        H.profile_enable(False)
    return out, set(H.profile_results())


MFMA_LABELS = ("attn_full_fwd_mfma", "attn_full_bwd_dq_mfma", "attn_full_bwd_dkv_mfma")
SHAPES = [(1, 1), (1, 300), (300, 1), (64, 64), (128, 128), (257, 65), (65, 257), (256, 512), (200, 333), (513, 130)]


# ---- matrix-core forward and backward ----
@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
def test_matrix_core_fwd_bwd(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq * 7919 + Skv * 31 + D + code)
    q, k, v, go = inputs(rng, code, 2, 2, 2, Sq, Skv, D)
    got, labels = profiled(lambda: run(code, q, k, v, go))
    check16(code, q, k, v, go, got, what=f"{Sq}x{Skv} D{D}")
    for label in MFMA_LABELS:
        assert f"{label}_d{D}" in labels, (label, sorted(labels))
    assert "attn_full_bwd_delta" in labels and not any("generic" in n for n in labels), sorted(labels)


# ---- key lengths ----
LENS = [333, 0, 1, 64, 65, 200]


@pytest.fixture(scope="module")
def len_case():
    code, D, Sq, Skv = H.BF16, 128, 130, 333
    rng = np.random.default_rng(333)
    q, k, v, go = inputs(rng, code, len(LENS), 2, 2, Sq, Skv, D)
    got = run(code, q, k, v, go, LENS)
    return dict(code=code, q=q, k=k, v=v, go=go, got=got)


def test_key_lengths_against_the_reference(len_case):
    c = len_case
    got = c["got"]
    check16(c["code"], c["q"], c["k"], c["v"], c["go"], got, LENS, "kv_len")
    for b, ln in enumerate(LENS):   # dk, dv rows at n >= len_b are exactly zero
        assert not bits(got[3][b, :, ln:]).any() and not bits(got[4][b, :, ln:]).any(), b
    assert not bits(got[0][1]).any() and not bits(got[2][1]).any() and np.isneginf(got[1][1]).all()   # batch 1 sees no key


@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_padding_never_reaches_an_output(len_case, poison, code, D):
    if code == H.BF16 and D == 128:
        c = len_case
        q, k, v, go, clean = c["q"], c["k"], c["v"], c["go"], c["got"]
    else:
        rng = np.random.default_rng(64 + code)
        q, k, v, go = inputs(rng, code, len(LENS), 2, 2, 130, 333, D)
        clean = run(code, q, k, v, go, LENS)
    kp, vp = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    for b, ln in enumerate(LENS):
        kp[b, :, ln:] = poison
        vp[b, :, ln:] = -poison
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, LENS)
    for name, a, b in zip(("o", "lse", "dq", "dk", "dv"), dirty, clean):
        assert same(a, b), f"{name}: padding of {poison} changed the result"


def test_key_lengths_are_clamped_and_null_is_every_key():
    code, D, Sq, Skv = H.BF16, 64, 130, 333
    rng = np.random.default_rng(5)
    q, k, v, go = inputs(rng, code, 2, 2, 2, Sq, Skv, D)
    wild, tame = run(code, q, k, v, go, [-5, 10 ** 9]), run(code, q, k, v, go, [0, Skv])
    assert all(same(a, b) for a, b in zip(wild, tame))
    null, full = run(code, q, k, v, go, None), run(code, q, k, v, go, [Skv, Skv])
    assert all(same(a, b) for a, b in zip(null, full))


# ---- grouped K/V heads ----
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_gqa(code, D, Hkv):
    Hq, Sq, Skv = 4, 200, 333
    G = Hq // Hkv
    rng = np.random.default_rng(Hkv + D)
    q, k, v, go = inputs(rng, code, 2, Hq, Hkv, Sq, Skv, D)
    lens = [333, 130]
    got = run(code, q, k, v, go, lens)
    rep = run(code, q, np.repeat(k, G, axis=1), np.repeat(v, G, axis=1), go, lens)
    for name, a, b in zip(("o", "lse", "dq"), got[:3], rep[:3]):
        assert same(a, b), f"{name} differs from the Hkv = Hq call on repeated K/V"
    check16(code, q, k, v, go, got, lens, f"gqa {Hq}/{Hkv}")   # dk, dv: the helper's sums (and scales) over each group
    assert all(same(a, b) for a, b in zip(got, run(code, q, k, v, go, lens))), "not reproducible"


# ---- strided: the packed projection read in place ----
def guarded(nbytes):
    buf = H.DevBuf(nbytes + 2 * GUARD)
    fill = np.full(nbytes + 2 * GUARD, 0xAB, dtype=np.uint8)
    H.check(H.lib().kf_memcpy_h2d(buf.ptr, fill.ctypes.data, fill.nbytes, None))
    return buf, buf.ptr + GUARD


def guards_ok(buf, nbytes):
    whole = np.empty(nbytes + 2 * GUARD, dtype=np.uint8)
    H.check(H.lib().kf_memcpy_d2h(whole.ctypes.data, buf.ptr, whole.nbytes, None))
    return bool((whole[:GUARD] == 0xAB).all() and (whole[GUARD + nbytes:] == 0xAB).all())


def read(base, shape, dtype):
    out = np.empty(shape, dtype=dtype)
    H.check(H.lib().kf_memcpy_d2h(out.ctypes.data, base, out.nbytes, None))
    return out


@pytest.mark.parametrize("code,D,S", [(H.BF16, 128, 200), (H.F16, 64, 129)])
def test_packed_layout_equals_contiguous(code, D, S):
    B, Hq, Hkv = 2, 4, 2
    W, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = W + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = rnd(rng, code, (B * S, W)), rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    lens = [S, S - 70]
    ref = run(code, q, k, v, go, lens)
    packed, flat, gpack = (S * W, D, W), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo, bl = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout), H.DevBuf.from_numpy(np.asarray(lens, np.int64))
    ob, o = guarded(B * S * d * es)
    lb, lse = guarded(4 * B * Hq * S)
    gb, g = guarded(B * S * PADW * es)
    scale = scale_of(D)
    H.attn_full_fwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, kv_len=bl.ptr,
                    layouts=(packed, packed, packed, flat))
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    H.attn_full_bwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                    g + (d + dkv) * es, w.ptr, need, kv_len=bl.ptr, layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack))
    H.device_sync()
    assert same(heads(read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert same(read(lse, (B, Hq, S), np.float32), ref[1])
    gq = read(g, (B * S, PADW), qkv.dtype)
    assert same(heads(gq[:, :d], Hq), ref[2]) and same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and same(heads(gq[:, d + dkv:W], Hkv), ref[4])
    assert (gq[:, W:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, n in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es)):
        assert guards_ok(buf, n)


# ---- generic path ----
def check_generic(code, q, k, v, go, got, kv_len, labels):
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    ref = attn_ref64_vis(q, k, v, go, key_len_vis(kv_len, q.shape[2], k.shape[2], q.shape[0]), code)
    dead = np.isneginf(ref["lse"])
    assert np.allclose(f(got[0]), ref["o"], rtol=1e-4, atol=1e-4)
    assert np.isneginf(got[1][dead]).all() and np.allclose(got[1][~dead], ref["lse"][~dead], rtol=1e-4, atol=1e-4)
    for name, g in zip(("dq", "dk", "dv"), got[2:]):
        assert np.allclose(f(g), ref[name], rtol=1e-3, atol=1e-4), name
    assert {"attn_full_fwd_generic", "attn_full_bwd_dq_generic", "attn_full_bwd_dkv_generic"} <= labels and not any("mfma" in n for n in labels), sorted(labels)


@pytest.mark.parametrize("kv_len", [None, [17, 0, 40]])
@pytest.mark.parametrize("Sq,Skv", [(33, 70), (96, 17)])
@pytest.mark.parametrize("D", [64, 80])
def test_generic_f32(D, Sq, Skv, kv_len):
    rng = np.random.default_rng(D + Sq)
    q, k, v, go = inputs(rng, H.F32, 3, 4, 2, Sq, Skv, D)
    got, labels = profiled(lambda: run(H.F32, q, k, v, go, kv_len))
    check_generic(H.F32, q, k, v, go, got, kv_len, labels)


@pytest.mark.parametrize("kv_len", [None, [300, 5]])
def test_generic_bf16_head_80(kv_len):
    """bf16 outputs round once on top of the f32 arithmetic: held to the scale-aware 16-bit bounds, which are tighter than allclose"""
    rng = np.random.default_rng(80)
    q, k, v, go = inputs(rng, H.BF16, 2, 2, 1, 70, 300, 80)
    got, labels = profiled(lambda: run(H.BF16, q, k, v, go, kv_len))
    check16(H.BF16, q, k, v, go, got, kv_len, "bf16 D80")
    assert "attn_full_fwd_generic" in labels and "attn_full_bwd_dkv_generic" in labels and not any("mfma" in n for n in labels)


@pytest.mark.parametrize("kv_len", [None, [70, 5]])
def test_generic_f16_head_40(kv_len):
    """f16 at a head size the matrix-core kernels do not take: the generic kernels' third element type, held to the same 16-bit bounds"""
    rng = np.random.default_rng(40)
    q, k, v, go = inputs(rng, H.F16, 2, 2, 1, 33, 70, 40)
    got, labels = profiled(lambda: run(H.F16, q, k, v, go, kv_len))
    check16(H.F16, q, k, v, go, got, kv_len, "f16 D40")
    assert {"attn_full_fwd_generic", "attn_full_bwd_dq_generic", "attn_full_bwd_dkv_generic"} <= labels and not any("mfma" in n for n in labels)


# ---- determinism, graph capture ----
def test_reproducible_and_capturable():
    rng = np.random.default_rng(513)
    for code, D, Hq, Hkv, Sq, Skv, lens in ((H.BF16, 128, 2, 2, 513, 130, None), (H.F16, 64, 4, 1, 200, 333, [333, 77])):
        q, k, v, go = inputs(rng, code, 2, Hq, Hkv, Sq, Skv, D)
        a, b, g = run(code, q, k, v, go, lens), run(code, q, k, v, go, lens), run(code, q, k, v, go, lens, graph=True)
        assert all(same(x, y) for x, y in zip(a, b)), "two runs differ"
        assert all(same(x, y) for x, y in zip(a, g)), "the captured run differs from the eager one"


# ---- operator API ----
def value(x, code):
    t = kfunca.from_numpy(O.to_float(x, code).astype(np.float32), 0)
    return t.bfloat16() if code == H.BF16 else t


def leaf(x, code):
    t = value(x, code)
    t.set_requires_grad(True)
    return t


def as_np(t, code):
    return O.from_float(t.float().numpy(), code)


def torch_ref(q, k, v, go, kv_len):
    """torch's scaled_dot_product_attention on the CPU in f32 under a boolean mask built from kv_len (K/V repeated over each group)"""
    import torch
    G = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float32, requires_grad=True) for x in (q, k, v))
    mask = None
    if kv_len is not None:
        mask = (torch.arange(k.shape[2])[None, :] < torch.tensor(kv_len)[:, None])[:, None, None, :]
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1), attn_mask=mask)
    o.backward(torch.tensor(go, dtype=torch.float32))
    return [x.detach().numpy().astype(np.float64) for x in (o, tq.grad, tk.grad, tv.grad)]


def check_operator(code, q, k, v, go, kv_len, got, what):
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    vis = key_len_vis(kv_len, q.shape[2], k.shape[2], q.shape[0])
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    if code == H.F32:
        assert np.allclose(f(got[0]), ref["o"], rtol=1e-4, atol=1e-4)
        for name, g in zip(("dq", "dk", "dv"), got[1:]):
            assert np.allclose(f(g), ref[name], rtol=1e-3, atol=1e-4), name
    else:
        fl = format_floor_vis(q, k, v, go, vis, code)
        for name, g in zip(("o", "dq", "dk", "dv"), got):
            K.check_one(name, g, ref, code, what, floor=fl.get(name))
    tol = 2.0 ** -5 if code == H.BF16 else 1e-4
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, torch_ref(f(q), f(k), f(v), f(go), kv_len)):
        assert np.abs(f(a) - r).max() <= tol * np.abs(r).max(), (what, name)


@pytest.mark.parametrize("kv_len", [None, [90, 33]])
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention(code, D, kv_len):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv, Sq, Skv = 2, 4, 2, 70, 90
    q, k, v, go = inputs(rng, code, B, Hq, Hkv, Sq, Skv, D)
    tq, tk, tv = leaf(q, code), leaf(k, code), leaf(v, code)
    tl = None if kv_len is None else kfunca.from_numpy(np.asarray(kv_len, np.int64), 0)
    out, labels = profiled(lambda: kfunca.attention(tq, tk, tv, kv_len=tl))
    out.backward(value(go, code))
    got = [as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
    assert got[0].shape == q.shape and got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    check_operator(code, q, k, v, go, kv_len, got, f"attention D{D}")
    if code == H.BF16:   # head size 40 is zero-padded to 64: the matrix-core kernels
        assert "attn_full_fwd_mfma_d64" in labels, sorted(labels)


@pytest.mark.parametrize("kv_len", [None, [129, 50]])
@pytest.mark.parametrize("code,D,kv_heads", [(H.BF16, 64, 2), (H.BF16, 64, None), (H.BF16, 40, 2), (H.F32, 32, 2)])
def test_operator_attention_qkv(code, D, kv_heads, kv_len):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq = 2, 129, 4
    Hkv = Hq if kv_heads is None else kv_heads
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    qkv, gout = rnd(rng, code, (B * S, W)), rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    tx = leaf(qkv, code)
    tl = None if kv_len is None else kfunca.from_numpy(np.asarray(kv_len, np.int64), 0)
    out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=kv_heads, kv_len=tl)
    out.backward(value(gout, code))
    o2, g2 = as_np(out, code), as_np(tx.grad(), code)
    assert o2.shape == (B * S, d) and g2.shape == qkv.shape
    got = [heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv)]
    check_operator(code, q, k, v, go, kv_len, got, f"attention_qkv D{D}")
