"""-m gpu: prefix-LM and padded-causal attention (kf_attn_prefix_fwd / kf_attn_prefix_bwd, kfunca.attention(..., causal=True,
prefix_len=...), kfunca.attention_qkv): query m sees key n iff n < len_b and (n < pre_b or n <= m).

The reference is tests/attn_full_ref.py's float64 attention under the visibility of tests/attn_prefix_ref.py. The 16-bit outputs are
held to the project's scale-aware bounds (oracle.checks.check_one with the floors of format_floor_vis), lse to 2e-6 (1 + |lse|) and to
-inf exactly where a row sees no key. The f32 generic path is held to the rule tests/test_gpu_attn_full.py's check_generic applies
(rtol 1e-4 / atol 1e-4 forward and lse, rtol 1e-3 / atol 1e-4 backward), restated here for a visibility; the 16-bit generic cases
(D 80, D 40) round their outputs once to 8 / 11 significant bits, which rtol 1e-4 cannot hold by the formats' precision, so they are held
to the scale-aware 16-bit bounds like their siblings in that file. The operator tests add that file's comparison with torch's
scaled_dot_product_attention on the CPU in f32: max |got - ref| <= TOL max |ref|, TOL = 2^-5 (bf16) and 1e-4 (f32).

Shapes sit at the kernels' seams: 32 queries or keys per wave, 64 per tile, 128 per workgroup. The helpers that do not name an entry
(random inputs, bit comparison, guard bytes, the profiler scope) are tests/test_gpu_attn_full.py's own, through a module import."""
import numpy as np
import pytest

import kfunca_amd as kfunca
import tests.test_gpu_attn_full as F
from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O
from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis
from tests.attn_prefix_ref import prefix_vis

pytestmark = pytest.mark.gpu

NAMES = ("o", "lse", "dq", "dk", "dv")


def dev_i64(x):
    return None if x is None else H.DevBuf.from_numpy(np.asarray(x, np.int64))


def run(code, q, k, v, go, kv_len=None, prefix_len=None, graph=False, full=False):
    """kf_attn_prefix_fwd + kf_attn_prefix_bwd (full: kf_attn_full_*, which takes no prefix) on contiguous tensors: o, lse, dq, dk, dv.
    The workspace is pre-filled with 0xFF; graph: captured with kf_graph_* and launched once."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    scale = F.scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bl, bp = dev_i64(kv_len), dev_i64(prefix_len)
    lens = dict(kv_len=None if bl is None else bl.ptr)
    if not full:
        lens["prefix_len"] = None if bp is None else bp.ptr
    fwd, bwd = (H.attn_full_fwd, H.attn_full_bwd) if full else (H.attn_prefix_fwd, H.attn_prefix_bwd)
    bo, blse = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * Sq)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    w = H.DevBuf(need)
    fill = np.full(max(need, 1), 0xFF, np.uint8)
    H.check(H.lib().kf_memcpy_h2d(w.ptr, fill.ctypes.data, need, None))
    dq, dk, dv = H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(v.nbytes)
    H.device_sync()

    def calls(st):
        fwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, stream=st, **lens)
        bwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need, stream=st, **lens)

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


def check16(code, q, k, v, go, got, vis, what=""):
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    fl = format_floor_vis(q, k, v, go, vis, code)
    for name, g in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4])):
        K.check_one(name, g, ref, code, what, floor=fl.get(name))
    check_lse(got[1], ref, what)


def vis_of(q, k, kv_len, prefix_len):
    return prefix_vis(kv_len, prefix_len, q.shape[2], k.shape[2], q.shape[0])


def assert_same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert F.same(x, y), f"{name}: {what}"


def zero_bits(x):
    return not F.bits(np.ascontiguousarray(x)).any()


MFMA_LABELS = ("attn_prefix_fwd_mfma", "attn_prefix_bwd_dq_mfma", "attn_prefix_bwd_dkv_mfma")
SHAPES = [(1, 1), (33, 33), (64, 64), (128, 128), (200, 200), (65, 257), (257, 65), (130, 333), (513, 130)]


def six_batches(Skv):
    """(kv_len, prefix_len) of the six batches one call carries: causal, a one-key prefix, a prefix across a wave, a length that cuts
    the prefix's tile, no key at all, a prefix beyond the length (full attention of 100 keys)"""
    pairs = [(Skv, 0), (Skv, 1), (Skv, 33), (min(Skv, 65), 64), (0, 5), (min(Skv, 100), Skv + 7)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


# ---- matrix-core forward and backward ----
@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
def test_matrix_core_fwd_bwd(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq * 7919 + Skv * 31 + D + code)
    lens, pres = six_batches(Skv)
    q, k, v, go = F.inputs(rng, code, 6, 2, 2, Sq, Skv, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, lens, pres))
    check16(code, q, k, v, go, got, vis_of(q, k, lens, pres), f"{Sq}x{Skv} D{D}")
    for label in MFMA_LABELS:
        assert f"{label}_d{D}" in labels, (label, sorted(labels))
    assert "attn_full_bwd_delta" in labels and not any("generic" in n for n in labels), sorted(labels)
    assert not any(n.startswith("attn_full_") and n != "attn_full_bwd_delta" for n in labels), sorted(labels)


# ---- every prefix at which a skip or a body choice of one of the three kernels changes ----
def test_seam_sweep():
    code, D, S = H.BF16, 128, 200
    pres = [0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]
    rng = np.random.default_rng(200)
    q, k, v, go = F.inputs(rng, code, len(pres), 2, 2, S, S, D)
    got = run(code, q, k, v, go, None, pres)
    check16(code, q, k, v, go, got, vis_of(q, k, None, pres), "seam sweep")


# ---- exact zeros ----
def test_exact_zeros():
    code, D, Sq, Skv = H.BF16, 128, 65, 257
    lens, pres = six_batches(Skv)
    rng = np.random.default_rng(65257)
    q, k, v, go = F.inputs(rng, code, 6, 2, 2, Sq, Skv, D)
    o, lse, dq, dk, dv = run(code, q, k, v, go, lens, pres)
    vis = vis_of(q, k, lens, pres)
    for b, ln in enumerate(np.clip(lens, 0, Skv)):
        assert zero_bits(dk[b, :, ln:]) and zero_bits(dv[b, :, ln:]), f"batch {b}: rows at n >= len are not zeros"
        unseen = ~vis[b].any(axis=0)               # keys inside the length that no query sees: n >= pre and n >= Sq
        assert zero_bits(dk[b][:, unseen]) and zero_bits(dv[b][:, unseen]), f"batch {b}: an unseen key row is not zero"
    assert lens[0] == Skv and pres[0] == 0         # causal: the key blocks from 128 on have no query tile
    assert zero_bits(dk[0, :, Sq:]) and zero_bits(dv[0, :, Sq:]) and not zero_bits(dk[0, :, :Sq])
    assert lens[4] == 0
    assert zero_bits(o[4]) and zero_bits(dq[4]) and np.isneginf(lse[4]).all()


# ---- with the prefix at or beyond the length: the bits of full attention ----
@pytest.mark.parametrize("Sq,Skv", [(130, 333), (257, 65)])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_same_bits_as_full_attention(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq + D)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, Sq, Skv, D)
    assert_same(run(code, q, k, v, go, None, [Skv] * 4), run(code, q, k, v, go, None, full=True), "kv_len NULL, prefix_len = Skv")
    lens = [Skv, 64, 0, 33]
    want = run(code, q, k, v, go, lens, full=True)
    assert_same(run(code, q, k, v, go, lens, lens), want, "prefix_len = kv_len")
    assert_same(run(code, q, k, v, go, lens, [Skv + 9, 65, 3, 10 ** 9]), want, "prefix_len > kv_len")


# ---- K and V rows at n >= len_b are never read ----
@pytest.mark.parametrize("poison", [np.nan, np.inf])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_padding_never_reaches_an_output(poison, code, D):
    Sq, Skv = 130, 200
    lens, pres = [200, 0, 1, 64, 65, 150], [0, 5, 0, 40, 65, 33]
    rng = np.random.default_rng(64 + code)
    q, k, v, go = F.inputs(rng, code, len(lens), 2, 2, Sq, Skv, D)
    clean = run(code, q, k, v, go, lens, pres)
    check16(code, q, k, v, go, clean, vis_of(q, k, lens, pres), "clean padding")
    kp, vp = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    for b, ln in enumerate(lens):
        kp[b, :, ln:] = poison
        vp[b, :, ln:] = -poison
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, lens, pres)
    assert_same(dirty, clean, f"padding of {poison} changed the result")


# ---- grouped K/V heads ----
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_gqa(code, D, Hkv):
    Hq, Sq, Skv = 4, 130, 200
    lens, pres = [200, 130, 200], [0, 70, 129]
    rng = np.random.default_rng(Hkv + D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, Hkv, Sq, Skv, D)
    got = run(code, q, k, v, go, lens, pres)
    check16(code, q, k, v, go, got, vis_of(q, k, lens, pres), f"gqa {Hq}/{Hkv}")


# ---- strided: the packed projection read in place ----
@pytest.mark.parametrize("code,D,S", [(H.BF16, 128, 200), (H.F16, 64, 129)])
def test_packed_layout_equals_contiguous(code, D, S):
    B, Hq, Hkv = 2, 4, 2
    W, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = W + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    lens, pres = [S, S - 70], [40, 0]
    ref = run(code, q, k, v, go, lens, pres)
    packed, flat, gpack = (S * W, D, W), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo, bl, bp = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout), dev_i64(lens), dev_i64(pres)
    ob, o = F.guarded(B * S * d * es)
    lb, lse = F.guarded(4 * B * Hq * S)
    gb, g = F.guarded(B * S * PADW * es)
    scale = F.scale_of(D)
    H.attn_prefix_fwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, kv_len=bl.ptr,
                      prefix_len=bp.ptr, layouts=(packed, packed, packed, flat))
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    H.attn_prefix_bwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                      g + (d + dkv) * es, w.ptr, need, kv_len=bl.ptr, prefix_len=bp.ptr,
                      layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack))
    H.device_sync()
    assert F.same(heads(F.read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert F.same(F.read(lse, (B, Hq, S), np.float32), ref[1])
    gq = F.read(g, (B * S, PADW), qkv.dtype)
    assert F.same(heads(gq[:, :d], Hq), ref[2]) and F.same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and F.same(heads(gq[:, d + dkv:W], Hkv), ref[4])
    assert (gq[:, W:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, n in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es)):
        assert F.guards_ok(buf, n)


# ---- generic path ----
GENERIC_LABELS = {"attn_prefix_fwd_generic", "attn_prefix_bwd_dq_generic", "attn_prefix_bwd_dkv_generic"}


def check_generic(code, q, k, v, go, got, vis):
    """tests/test_gpu_attn_full.py's check_generic, for a visibility"""
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    dead = np.isneginf(ref["lse"])
    assert np.allclose(f(got[0]), ref["o"], rtol=1e-4, atol=1e-4)
    assert np.isneginf(got[1][dead]).all() and np.allclose(got[1][~dead], ref["lse"][~dead], rtol=1e-4, atol=1e-4)
    for name, g in zip(("dq", "dk", "dv"), got[2:]):
        assert np.allclose(f(g), ref[name], rtol=1e-3, atol=1e-4), name


def generic_lens(Skv):
    return [Skv, 17, 0, Skv + 3], [0, 5, 9, 20]


@pytest.mark.parametrize("Sq,Skv", [(33, 70), (96, 17)])
@pytest.mark.parametrize("code,D", [(H.F32, 64), (H.F32, 80), (H.BF16, 80), (H.F16, 40)])
def test_generic(code, D, Sq, Skv):
    lens, pres = generic_lens(Skv)
    rng = np.random.default_rng(D + Sq + code)
    q, k, v, go = F.inputs(rng, code, 4, 4, 2, Sq, Skv, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, lens, pres))
    vis = vis_of(q, k, lens, pres)
    if code == H.F32:
        check_generic(code, q, k, v, go, got, vis)
    else:
        check16(code, q, k, v, go, got, vis, f"generic D{D}")
    assert GENERIC_LABELS <= labels and not any("mfma" in n for n in labels), sorted(labels)
    for b, ln in enumerate(np.clip(lens, 0, Skv)):
        unseen = ~vis[b].any(axis=0)
        unseen[ln:] = True
        assert zero_bits(got[3][b][:, unseen]) and zero_bits(got[4][b][:, unseen]), b


# ---- determinism, graph capture ----
def test_reproducible_and_capturable():
    rng = np.random.default_rng(513)
    for code, D, Hq, Hkv, Sq, Skv, lens, pres in ((H.BF16, 128, 2, 2, 513, 130, None, [0, 70]), (H.F16, 64, 4, 1, 200, 333, [333, 77], [129, 0])):
        q, k, v, go = F.inputs(rng, code, 2, Hq, Hkv, Sq, Skv, D)
        a, b, g = run(code, q, k, v, go, lens, pres), run(code, q, k, v, go, lens, pres), run(code, q, k, v, go, lens, pres, graph=True)
        assert_same(a, b, "two runs differ")
        assert_same(a, g, "the captured run differs from the eager one")


# ---- operator API ----
def torch_ref(q, k, v, go, vis):
    """torch's scaled_dot_product_attention on the CPU in f32 under the boolean mask (K/V repeated over each group)"""
    import torch
    G = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float32, requires_grad=True) for x in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1),
                                                         attn_mask=torch.tensor(vis)[:, None])
    o.backward(torch.tensor(go, dtype=torch.float32))
    return [x.detach().numpy().astype(np.float64) for x in (o, tq.grad, tk.grad, tv.grad)]


def check_operator(code, q, k, v, go, vis, got, what):
    """tests/test_gpu_attn_full.py's check_operator, for a visibility in which every query sees a key"""
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
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
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, torch_ref(f(q), f(k), f(v), f(go), vis)):
        assert np.abs(f(a) - r).max() <= tol * np.abs(r).max(), (what, name)


def dev_long(x):
    return None if x is None else kfunca.from_numpy(np.asarray(x, np.int64), 0)


@pytest.mark.parametrize("kv_len,prefix_len", [(None, None), ([90, 33], [20, 70]), (None, [65, 0])])
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention(code, D, kv_len, prefix_len):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv, Sq, Skv = 2, 4, 2, 70, 90
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, Sq, Skv, D)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, kv_len=dev_long(kv_len), causal=True, prefix_len=dev_long(prefix_len)))
    out.backward(F.value(go, code))
    got = [F.as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
    assert got[0].shape == q.shape and got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    check_operator(code, q, k, v, go, vis_of(q, k, kv_len, prefix_len), got, f"attention D{D}")
    if code == H.BF16:   # head size 40 is zero-padded to 64: the matrix-core kernels
        assert "attn_prefix_fwd_mfma_d64" in labels, sorted(labels)
    else:
        assert "attn_prefix_fwd_generic" in labels, sorted(labels)


@pytest.mark.parametrize("kv_len,prefix_len", [(None, None), ([129, 50], [64, 10])])
@pytest.mark.parametrize("code,D,kv_heads", [(H.BF16, 64, 2), (H.BF16, 40, 2), (H.F32, 48, 2)])
def test_operator_attention_qkv(code, D, kv_heads, kv_len, prefix_len):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq, Hkv = 2, 129, 4, kv_heads
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    tx = F.leaf(qkv, code)
    out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=kv_heads, kv_len=dev_long(kv_len), causal=True, prefix_len=dev_long(prefix_len))
    out.backward(F.value(gout, code))
    o2, g2 = F.as_np(out, code), F.as_np(tx.grad(), code)
    assert o2.shape == (B * S, d) and g2.shape == qkv.shape
    got = [heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv)]
    check_operator(code, q, k, v, go, vis_of(q, k, kv_len, prefix_len), got, f"attention_qkv D{D}")


def test_prefix_len_without_causal_is_refused():
    rng = np.random.default_rng(1)
    q, k, v, _ = F.inputs(rng, H.BF16, 2, 2, 2, 8, 8, 64)
    tq, tk, tv = (F.value(x, H.BF16) for x in (q, k, v))
    with pytest.raises(Exception, match="attention: prefix_len"):
        kfunca.attention(tq, tk, tv, prefix_len=dev_long([1, 2]))
    with pytest.raises(Exception, match="attention_qkv: prefix_len"):
        kfunca.attention_qkv(F.value(F.rnd(rng, H.BF16, (16, 6 * 64)), H.BF16), 2, 8, 2, kv_heads=2, prefix_len=dev_long([1, 2]))
    with pytest.raises(Exception, match="prefix_len must hold B"):
        kfunca.attention(tq, tk, tv, causal=True, prefix_len=dev_long([1, 2, 3]))


@pytest.mark.parametrize("kv_len", [None, [90, 33]])
def test_causal_false_is_the_full_call(kv_len):
    """the operator without the mask has the bits of kf_attn_full_* on the same tensors (the path it took before the mask existed)"""
    code, D = H.BF16, 64
    rng = np.random.default_rng(7)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, 70, 90, D)
    want = run(code, q, k, v, go, kv_len, full=True)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, kv_len=dev_long(kv_len), causal=False))
    out.backward(F.value(go, code))
    assert "attn_full_fwd_mfma_d64" in labels and not any("prefix" in n for n in labels), sorted(labels)
    for name, t, w in zip(("o", "dq", "dk", "dv"), (out, tq.grad(), tk.grad(), tv.grad()), (want[0], want[2], want[3], want[4])):
        assert F.same(F.as_np(t, code), w), name
