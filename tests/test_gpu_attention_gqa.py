"""-m gpu: grouped-query attention (kf_attn_fwd_gqa / kf_attn_bwd_gqa, kfunca.causal_attention_gqa, causal_attention_qkv(kv_heads=)).

"MHA-on-repeat" below is the existing multi-head entry points (kf_attn_*_scaled, same scale) fed K and V repeated G = Hq / Hkv times along
the head dim (np.repeat(k, G, axis=1)). The GQA forward and dQ read the same values at the same addresses' worth of arithmetic, so o,
lse and dq must equal MHA-on-repeat BIT FOR BIT. dk and dv must equal the header's contract bit for bit: the dtype rounding of the f32 sum,
in ascending g from the g = 0 term, of MHA-on-repeat's per-head dk (dv) of heads j G + g.

Tolerance (stated) of the operator test against the torch-CPU float64 reference (repeat_interleave + autograd on the same rounded inputs):
max |got - ref| <= TOL * max |ref| per tensor, TOL = 2^-5 for bf16 and 1e-4 for f32.
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024


def rnd(rng, code, shape):
    return O.from_float(rng.uniform(-1, 1, shape).astype(np.float32), code)


def scale_of(D):
    return float(np.float32(1.0) / np.sqrt(np.float32(D)))


def mha(code, q, k, v, go, scale, ws="rec"):
    """MHA-on-repeat through kf_attn_fwd_scaled / kf_attn_bwd_scaled (k, v already repeated): o, lse, dq, dk, dv."""
    B, Hh, Sq, D = q.shape
    Skv = k.shape[2]
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bo, blse = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hh * Sq)
    H.check(H.lib().kf_attn_fwd_scaled(code, B, Hh, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, None))
    need = H.attn_bwd_workspace_bytes(code, B, Hh, Sq, Skv, D)
    if ws == "min":
        need = (B * Hh * Sq * 4 + 255) // 256 * 256 + 2 * ((B * Hh * ((Sq + 31) // 32 * 32) * 4 + 255) // 256 * 256)
    w = H.DevBuf(need)
    dq, dk, dv = H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(v.nbytes)
    H.check(H.lib().kf_attn_bwd_scaled(code, B, Hh, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr,
                                       w.ptr, need, None))
    H.device_sync()
    return (bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hh, Sq), np.float32), dq.to_numpy(q.shape, q.dtype), dk.to_numpy(k.shape, k.dtype),
            dv.to_numpy(v.shape, v.dtype))


def gqa(code, q, k, v, go, scale, ws="rec"):
    """kf_attn_fwd_gqa / kf_attn_bwd_gqa on contiguous tensors: o, lse, dq, dk, dv."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bo, blse = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * Sq)
    H.attn_fwd_gqa(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr)
    rec, mn = H.attn_bwd_gqa_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    need = rec if ws == "rec" else mn
    w = H.DevBuf(need)
    dq, dk, dv = H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(v.nbytes)
    H.attn_bwd_gqa(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need)
    H.device_sync()
    return (bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, Sq), np.float32), dq.to_numpy(q.shape, q.dtype), dk.to_numpy(k.shape, k.dtype),
            dv.to_numpy(v.shape, v.dtype))


def group_sum(x, G, code):
    """The contract: dtype(((f32 t_0 + t_1) + ...) + t_{G-1}) over the G query heads of each K/V head, in f32 adds."""
    B, Hq, S, D = x.shape
    t = O.to_float(x, code).astype(np.float32).reshape(B, Hq // G, G, S, D)
    acc = t[:, :, 0].copy()
    for g in range(1, G):
        acc = acc + t[:, :, g]
    return O.from_float(acc, code)


def bits(x):
    return x.view(np.uint16) if x.dtype.itemsize == 2 else x.view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_against_repeat(code, q, k, v, go, ws, what):
    G = q.shape[1] // k.shape[1]
    scale = scale_of(q.shape[3])
    want = mha(code, q, np.repeat(k, G, axis=1), np.repeat(v, G, axis=1), go, scale, ws)
    got = gqa(code, q, k, v, go, scale, ws)
    for name, a, b in zip(("o", "lse", "dq"), got[:3], want[:3]):
        assert same(a, b), f"{what}: {name} differs from MHA-on-repeat"
    assert same(got[3], group_sum(want[3], G, code)), f"{what}: dk is not the ascending-g group sum"
    assert same(got[4], group_sum(want[4], G, code)), f"{what}: dv is not the ascending-g group sum"
    return got


HEADS = [(8, 8), (8, 4), (8, 2), (8, 1), (6, 3)]
LENS16 = [(257, 257), (1000, 1000), (320, 1000), (384, 128), (65, 33)]


# 1 + 2 + 3: forward and backward bit for bit, on every tier, with the labels of the generated streams and of the group sum
@pytest.mark.parametrize("code", [H.BF16, H.F16])
@pytest.mark.parametrize("D", [64, 128, 96])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_16bit_equals_mha_on_repeat(code, D, Hq, Hkv):
    rng = np.random.default_rng(1000 * Hq + 10 * Hkv + D + code)
    for i, (Sq, Skv) in enumerate(LENS16):
        B = 1 + (i + Hkv) % 2
        q, go = rnd(rng, code, (B, Hq, Sq, D)), rnd(rng, code, (B, Hq, Sq, D))
        k, v = rnd(rng, code, (B, Hkv, Skv, D)), rnd(rng, code, (B, Hkv, Skv, D))
        H.profile_reset()
        H.profile_enable(True)
        check_against_repeat(code, q, k, v, go, "rec", f"{Hq}/{Hkv} D{D} {Sq}x{Skv} B{B}")
        H.profile_enable(False)
        labels = set(H.profile_results())
        assert ("attn_bwd_dkv_group_sum" in labels) == (Hkv < Hq), labels
        if D in (64, 128) and Skv >= Sq:
            sfx = "_d64" if D == 64 else ""
            for label in ("attn_fwd_mfma", "attn_bwd_dkv_mfma", "attn_bwd_dq_mfma"):
                assert label + sfx in labels, (label + sfx, sorted(labels))


@pytest.mark.parametrize("code", [H.BF16, H.F16])
@pytest.mark.parametrize("D", [64, 128])
def test_stored_ds_and_recomputing_forms(code, D):
    """recommended workspace: the stored-dS dQ kernel; minimum: the recomputing one (tiled shapes) - both bit for bit, multi-query included"""
    rng = np.random.default_rng(77 + D + code)
    for Hq, Hkv, Sq, Skv in ((8, 2, 512, 512), (4, 1, 256, 384), (6, 3, 384, 128)):
        q, go = rnd(rng, code, (2, Hq, Sq, D)), rnd(rng, code, (2, Hq, Sq, D))
        k, v = rnd(rng, code, (2, Hkv, Skv, D)), rnd(rng, code, (2, Hkv, Skv, D))
        for ws, label in (("rec", "attn_bwd_dq_mfma"), ("min", "attn_bwd_dq_mfma_split")):
            H.profile_reset()
            H.profile_enable(True)
            check_against_repeat(code, q, k, v, go, ws, f"{ws} {Hq}/{Hkv} {Sq}x{Skv} D{D}")
            H.profile_enable(False)
            labels = set(H.profile_results())
            assert label + ("_d64" if D == 64 else "") in labels, (ws, sorted(labels))


@pytest.mark.parametrize("D,Sq,Skv", [(64, 256, 256), (128, 320, 96), (128, 65, 33), (40, 64, 64)])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_f32_equals_mha_on_repeat(D, Sq, Skv, Hq, Hkv):
    rng = np.random.default_rng(5 * D + Sq + Hq * Hkv)
    B = 1 + Hkv % 2
    q, go = rnd(rng, H.F32, (B, Hq, Sq, D)), rnd(rng, H.F32, (B, Hq, Sq, D))
    k, v = rnd(rng, H.F32, (B, Hkv, Skv, D)), rnd(rng, H.F32, (B, Hkv, Skv, D))
    H.profile_reset()
    H.profile_enable(True)
    check_against_repeat(H.F32, q, k, v, go, "rec", f"f32 {Hq}/{Hkv} D{D} {Sq}x{Skv}")
    H.profile_enable(False)
    labels = set(H.profile_results())
    if D in (64, 128) and Sq % 32 == 0 and Skv % 32 == 0:
        assert {"attn_fwd_f32_mfma", "attn_bwd_dkv_f32_mfma", "attn_bwd_dq_f32_mfma"} <= labels, sorted(labels)
    assert ("attn_bwd_dkv_group_sum" in labels) == (Hkv < Hq)


@pytest.mark.parametrize("code,D", [(H.BF16, 33), (H.F16, 20), (H.F32, 39), (H.F32, 6)])
def test_head_sizes_off_16_bytes_take_the_scalar_group_sum(code, D):
    """a row of D elements that is not a whole number of 16-byte pieces: the group sum's element-wise path, same contract"""
    rng = np.random.default_rng(D + code)
    for Hq, Hkv, Sq, Skv in ((8, 2, 70, 70), (6, 3, 33, 65), (4, 1, 40, 17)):
        q, go = rnd(rng, code, (2, Hq, Sq, D)), rnd(rng, code, (2, Hq, Sq, D))
        k, v = rnd(rng, code, (2, Hkv, Skv, D)), rnd(rng, code, (2, Hkv, Skv, D))
        H.profile_reset()
        H.profile_enable(True)
        check_against_repeat(code, q, k, v, go, "rec", f"D{D} {Hq}/{Hkv} {Sq}x{Skv}")
        H.profile_enable(False)
        assert "attn_bwd_dkv_group_sum" in H.profile_results()


def guarded(nbytes):
    """(buffer, base): nbytes with GUARD bytes of 0xAB in front and behind"""
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


# 4: the packed projection [B*S, (Hq + 2 Hkv) D] read in place, o as [B*S, Hq D], one packed dqkv
@pytest.mark.parametrize("S", [512, 500])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
@pytest.mark.parametrize("D", [128, 64])
def test_packed_layout_equals_contiguous(code, D, S):
    B, Hq, Hkv = 2, 8, 2
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    rng = np.random.default_rng(S + D + code)
    qkv, gout = rnd(rng, code, (B * S, W)), rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    scale = scale_of(D)
    ref = gqa(code, q, k, v, go, scale)
    es = 2
    packed, flat = (S * W, D, W), (S * d, D, d)
    bqkv, bgo = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout)
    ob, o = guarded(B * S * d * es)
    lb, lse = guarded(4 * B * Hq * S)
    gb, g = guarded(B * S * W * es)
    H.attn_fwd_gqa(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse,
                   layouts=(packed, packed, packed, flat))
    rec, _ = H.attn_bwd_gqa_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(rec)
    H.attn_bwd_gqa(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                   g + (d + dkv) * es, w.ptr, rec, layouts=(packed, packed, packed, flat, flat, packed, packed, packed))
    H.device_sync()
    assert same(heads(read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert same(read(lse, (B, Hq, S), np.float32), ref[1])
    gq = read(g, (B * S, W), qkv.dtype)
    assert same(heads(gq[:, :d], Hq), ref[2]) and same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and same(heads(gq[:, d + dkv:], Hkv), ref[4])
    for buf, n in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * W * es)):
        assert guards_ok(buf, n)


# 5: Hkv == Hq is the multi-head path: same bits, same labels, no group sum
@pytest.mark.parametrize("code,D,S", [(H.BF16, 128, 256), (H.F16, 64, 1000), (H.BF16, 96, 65), (H.F32, 128, 64)])
def test_equal_heads_is_the_multi_head_path(code, D, S):
    rng = np.random.default_rng(9 + D + S)
    B, Hh = 2, 4
    q, k, v, go = (rnd(rng, code, (B, Hh, S, D)) for _ in range(4))
    scale = scale_of(D)
    runs = []
    for f in (mha, gqa):
        H.profile_reset()
        H.profile_enable(True)
        res = f(code, q, k, v, go, scale)
        H.profile_enable(False)
        runs.append((res, {n: c for n, (_, c) in H.profile_results().items()}))
    assert all(same(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert runs[0][1] == runs[1][1] and "attn_bwd_dkv_group_sum" not in runs[1][1]
    if code != H.F32 and D in (64, 128):  # and the strided entries, through the same code path
        d = Hh * D
        packed, flat = (S * 3 * d, D, 3 * d), (S * d, D, d)
        qkv = rnd(rng, code, (B * S, 3 * d))
        bqkv = H.DevBuf.from_numpy(qkv)
        outs = []
        for gq in (False, True):
            bo, bl = H.DevBuf(B * S * d * 2), H.DevBuf(4 * B * Hh * S)
            args = (bqkv.ptr, bqkv.ptr + 2 * d, bqkv.ptr + 4 * d, bo.ptr, bl.ptr)
            if gq:
                H.attn_fwd_gqa(code, B, Hh, Hh, S, S, D, scale, *args, layouts=(packed, packed, packed, flat))
            else:
                H.attn_fwd_strided(code, B, Hh, S, S, D, scale, args[0], packed, args[1], packed, args[2], packed, args[3], flat, args[4])
            H.device_sync()
            outs.append((bo.to_numpy((B * S, d), qkv.dtype), bl.to_numpy((B, Hh, S), np.float32)))
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])


def torch_ref(q, k, v, go):
    """float64 torch-CPU causal GQA: repeat_interleave of K/V + autograd (the inputs are the device's rounded values)"""
    import torch
    G = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, k, v))
    kk, vv = tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1)
    s = tq @ kk.transpose(-1, -2) / np.sqrt(q.shape[3])
    Sq, Skv = q.shape[2], k.shape[2]
    mask = torch.arange(Skv)[None, :] > torch.arange(Sq)[:, None]
    p = torch.softmax(s.masked_fill(mask, float("-inf")), dim=-1)
    o = p @ vv
    o.backward(torch.tensor(go, dtype=torch.float64))
    return o.detach().numpy(), tq.grad.numpy(), tk.grad.numpy(), tv.grad.numpy()


def value(x, code):
    t = kfunca.from_numpy(O.to_float(x, code).astype(np.float32), 0)
    return t.bfloat16() if code == H.BF16 else t


def leaf(x, code):
    t = value(x, code)
    t.set_requires_grad(True)
    return t


def as_np(t, code):
    return O.from_float(t.float().numpy(), code)


# 6: the operator API
@pytest.mark.parametrize("code,D,Sq,Skv", [(H.BF16, 128, 256, 256), (H.BF16, 80, 100, 100), (H.F32, 64, 96, 96), (H.F32, 48, 50, 70)])
def test_operator_matches_repeat_and_float64(code, D, Sq, Skv):
    rng = np.random.default_rng(D + Sq + code)
    B, Hq, Hkv = 2, 6, 2
    G = Hq // Hkv
    q, go = rnd(rng, code, (B, Hq, Sq, D)), rnd(rng, code, (B, Hq, Sq, D))
    k, v = rnd(rng, code, (B, Hkv, Skv, D)), rnd(rng, code, (B, Hkv, Skv, D))
    tq, tk, tv = leaf(q, code), leaf(k, code), leaf(v, code)
    out = kfunca.causal_attention_gqa(tq, tk, tv)
    out.backward(value(go, code))
    got = [as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
    assert got[0].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    rq, rk, rv = leaf(q, code), leaf(np.repeat(k, G, axis=1), code), leaf(np.repeat(v, G, axis=1), code)
    rout = kfunca.causal_attention(rq, rk, rv)
    rout.backward(value(go, code))
    want = [as_np(t, code) for t in (rout, rq.grad(), rk.grad(), rv.grad())]
    assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(got[2], group_sum(want[2], G, code)) and same(got[3], group_sum(want[3], G, code))
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    ref = torch_ref(f(q), f(k), f(v), f(go))
    tol = 2.0 ** -5 if code == H.BF16 else 1e-4
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, ref):
        assert np.abs(f(a) - r).max() <= tol * np.abs(r).max(), name


@pytest.mark.parametrize("S,D", [(128, 128), (100, 64), (64, 96)])
def test_rope_then_packed_attention_matches_split_heads(S, D):
    rng = np.random.default_rng(S + D)
    B, Hq, Hkv = 2, 8, 2
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    R = D
    i = np.arange(R // 2, dtype=np.float64)
    th = np.arange(S, dtype=np.float64)[:, None] * 10000.0 ** (-2 * i / R)[None, :]
    c, s = np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    x, g = rnd(rng, H.BF16, (B * S, W)), rnd(rng, H.BF16, (B * S, d))
    # packed: qkv -> rope_qkv(kv_heads) -> causal_attention_qkv(kv_heads) -> backward to qkv
    tx = leaf(x, H.BF16)
    rot = kfunca.rope_qkv(tx, tc, ts, B, S, Hq, kv_heads=Hkv)
    out = kfunca.causal_attention_qkv(rot, B, S, Hq, kv_heads=Hkv)
    out.backward(value(g, H.BF16))
    dx = as_np(tx.grad(), H.BF16)
    # split heads: the rotated projection's bits -> causal_attention_gqa -> packed d(rot) -> rope's inverse (its backward) on the device
    r = as_np(rot, H.BF16)
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    flat = lambda x4: x4.transpose(0, 2, 1, 3).reshape(B * S, -1)  # noqa: E731
    tq, tk, tv = leaf(heads(r[:, :d], Hq), H.BF16), leaf(heads(r[:, d:d + dkv], Hkv), H.BF16), leaf(heads(r[:, d + dkv:], Hkv), H.BF16)
    sout = kfunca.causal_attention_gqa(tq, tk, tv)
    sout.backward(value(heads(g, Hq), H.BF16))
    assert same(as_np(out, H.BF16), np.ascontiguousarray(flat(as_np(sout, H.BF16))))
    drot = np.ascontiguousarray(np.concatenate([flat(as_np(t.grad(), H.BF16)) for t in (tq, tk, tv)], axis=1))
    bd, bc, bs = H.DevBuf.from_numpy(drot), H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    by = H.DevBuf(drot.nbytes)
    lay = (S * W, D, W)
    H.rope(H.BF16, B, Hq + 2 * Hkv, S, D, bd.ptr, lay, y=by.ptr, ly=lay, cos=bc.ptr, sin=bs.ptr, table_rows=S, rotary_dim=R, h_rot=Hq + Hkv,
           inverse=True)
    H.device_sync()
    assert same(dx, by.to_numpy(drot.shape, np.uint16))


# 7: the flagship shape - Llama-style 32 / 8 heads at S 4096
def test_full_size_gqa_and_reproducibility():
    code, B, Hq, Hkv, S, D = H.BF16, 8, 32, 8, 4096, 128
    G = Hq // Hkv
    rng = np.random.default_rng(4096)
    q, go = rnd(rng, code, (B, Hq, S, D)), rnd(rng, code, (B, Hq, S, D))
    k, v = rnd(rng, code, (B, Hkv, S, D)), rnd(rng, code, (B, Hkv, S, D))
    got = check_against_repeat(code, q, k, v, go, "rec", "B8 32/8 S4096")
    for b, h in ((0, 0), (5, 27)):  # sampled heads: o, lse, dq against the f64 oracle on this head's own K/V head
        j = h // G
        sl = lambda x, hh: x[b:b + 1, hh:hh + 1]  # noqa: E731
        K.attn_check(sl(q, h), sl(k, j), sl(v, j), code, o=sl(got[0], h), lse=sl(got[1], h), d_o=sl(go, h), dq=sl(got[2], h),
                     what=f"b{b} h{h}")
    again = gqa(code, q, k, v, go, scale_of(D))
    assert all(same(a, b) for a, b in zip(got, again)), "two backward calls differ"
