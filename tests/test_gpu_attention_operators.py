"""-m gpu: what the six attention operators of the host core hand to the device library (causal_attention, causal_attention_gqa,
causal_attention_qkv with and without kv_heads, attention, attention_qkv).

Each case runs the operator (forward + backward) and, next to it, the C-ABI entry that case must reach, called directly through
hip_abi with the operands the host builds: the zero-padded copies where the host pads (head size to 64 / 128, f32 rows to multiples
of 32), the softmax scale of the REAL head size, the layouts of the packed projection, the recommended workspace of that entry's own
query. out and every gradient must be equal BIT FOR BIT, and the kernels whose labels start with "attn" must be the same ones, launched
the same number of times. A packed operator off its fast shape must equal the contiguous operator of its family on the split heads.
The refusals are held to their exact texts (the part of the message after "but got false. ").
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests.test_gpu_attention_gqa import as_np, leaf, rnd, same, scale_of, value

pytestmark = pytest.mark.gpu

B, HQ = 2, 2
MHA, GQA, FULL = "causal multi-head", "causal grouped", "full"


def pad(x, rows, cols=None):
    """zero-padded copy: [B, H, S, D] -> [B, H, rows, cols], or [B, H, S] -> [B, H, rows]"""
    out = np.zeros(x.shape[:2] + ((rows,) if x.ndim == 3 else (rows, cols)), x.dtype)
    out[(slice(None), slice(None)) + tuple(slice(0, n) for n in x.shape[2:])] = x
    return out


class Profiled:
    """with Profiled() as p: ...; p.attn = {label: launches} of the kernels whose label starts with "attn"; p.all = every label"""

    def __enter__(self):
        H.profile_reset()
        H.profile_enable(True)
        return self

    def __exit__(self, *exc):
        H.profile_enable(False)
        self.all = {n: c for n, (_, c) in H.profile_results().items()}
        self.attn = {n: c for n, c in self.all.items() if n.startswith("attn")}
        return False


def len_tensor(kv_len):
    return None if kv_len is None else kfunca.from_numpy(np.asarray(kv_len, np.int64), 0)


def operator(family, code, q, k, v, go, kv_len=None):
    """the contiguous operator of the family, forward + backward: out, dq, dk, dv"""
    tq, tk, tv = leaf(q, code), leaf(k, code), leaf(v, code)
    if family == MHA:
        out = kfunca.causal_attention(tq, tk, tv)
    elif family == GQA:
        out = kfunca.causal_attention_gqa(tq, tk, tv)
    else:
        out = kfunca.attention(tq, tk, tv, kv_len=len_tensor(kv_len))
    out.backward(value(go, code))
    return [as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]


def direct(family, code, q, k, v, go, padded=None, kv_len=None):
    """The family's C-ABI entries on the operands the host builds. padded = (Sqp, Skp, Dp): zero-padded copies go down, the scale stays
    that of the real head size, and the backward reads the forward's un-padded out and lse zero-padded again: out, dq, dk, dv."""
    Bq, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    Sqp, Skp, Dp = padded or (Sq, Skv, D)
    scale = scale_of(D)
    bq, bk, bv, bg = (H.DevBuf.from_numpy(x) for x in (pad(q, Sqp, Dp), pad(k, Skp, Dp), pad(v, Skp, Dp), pad(go, Sqp, Dp)))
    bn = None if kv_len is None else H.DevBuf.from_numpy(np.asarray(kv_len, np.int64))
    lens = None if bn is None else bn.ptr
    pshape = (Bq, Hq, Sqp, Dp)
    bo, bl = H.DevBuf(bq.nbytes), H.DevBuf(4 * Bq * Hq * Sqp)
    if family == MHA and padded:
        H.check(H.lib().kf_attn_fwd_scaled(code, Bq, Hq, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, None))
    elif family == MHA:
        H.attn_fwd(code, Bq, Hq, Sq, Skv, D, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr)
    elif family == GQA:
        H.attn_fwd_gqa(code, Bq, Hq, Hkv, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr)
    else:
        H.attn_full_fwd(code, Bq, Hq, Hkv, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, kv_len=lens)
    H.device_sync()
    o = bo.to_numpy(pshape, q.dtype)[:, :, :Sq, :D]
    lse = bl.to_numpy(pshape[:3], np.float32)[:, :, :Sq]
    bo, bl = H.DevBuf.from_numpy(pad(o, Sqp, Dp)), H.DevBuf.from_numpy(pad(lse, Sqp))
    if family == MHA:
        need = H.attn_bwd_workspace_bytes(code, Bq, Hq, Sqp, Skp, Dp)
    elif family == GQA:
        need, _ = H.attn_bwd_gqa_workspace_bytes(code, Bq, Hq, Hkv, Sqp, Skp, Dp)
    else:
        need = H.attn_full_bwd_workspace_bytes(code, Bq, Hq, Hkv, Sqp, Skp, Dp)
    w = H.DevBuf(max(need, 1))
    dq, dk, dv = H.DevBuf(bq.nbytes), H.DevBuf(bk.nbytes), H.DevBuf(bv.nbytes)
    if family == MHA and padded:
        H.check(H.lib().kf_attn_bwd_scaled(code, Bq, Hq, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, bg.ptr, dq.ptr, dk.ptr, dv.ptr,
                                           w.ptr, need, None))
    elif family == MHA:
        H.attn_bwd(code, Bq, Hq, Sq, Skv, D, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, bg.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need)
    elif family == GQA:
        H.attn_bwd_gqa(code, Bq, Hq, Hkv, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, bg.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need)
    else:
        H.attn_full_bwd(code, Bq, Hq, Hkv, Sqp, Skp, Dp, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, bl.ptr, bg.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need,
                        kv_len=lens)
    H.device_sync()
    kshape = (Bq, Hkv, Skp, Dp)
    return [np.ascontiguousarray(o), np.ascontiguousarray(dq.to_numpy(pshape, q.dtype)[:, :, :Sq, :D]),
            np.ascontiguousarray(dk.to_numpy(kshape, q.dtype)[:, :, :Skv, :D]), np.ascontiguousarray(dv.to_numpy(kshape, q.dtype)[:, :, :Skv, :D])]


def check_contiguous(family, code, Hkv, D, Sq, Skv, padded, kv_len=None):
    rng = np.random.default_rng(1000 * D + 10 * Sq + Skv + code)
    q, go = rnd(rng, code, (B, HQ, Sq, D)), rnd(rng, code, (B, HQ, Sq, D))
    k, v = rnd(rng, code, (B, Hkv, Skv, D)), rnd(rng, code, (B, Hkv, Skv, D))
    with Profiled() as op:
        got = operator(family, code, q, k, v, go, kv_len)
    with Profiled() as abi:
        want = direct(family, code, q, k, v, go, padded, kv_len)
    for name, a, b in zip(("out", "dq", "dk", "dv"), got, want):
        assert same(a, b), f"{family} D{D} {Sq}x{Skv}: {name} differs from the direct call"
    assert op.attn == abi.attn and op.attn, (op.attn, abi.attn)
    return op.attn


# (dtype, D, Sq, Skv, the padded sizes the host hands down or None): the four paths of the causal pad plan
CAUSAL = [(H.BF16, 128, 128, 128, None),        # matrix-core kernels, nothing padded
          (H.BF16, 96, 65, 65, (65, 65, 128)),  # the head is padded, 16-bit rows never are
          (H.F32, 64, 50, 70, (64, 96, 64)),    # f32 rows are padded to multiples of 32
          (H.F32, 48, 65, 33, None)]            # Skv < Sq: nothing is padded, the generic kernels run


@pytest.mark.parametrize("code,D,Sq,Skv,padded", CAUSAL)
def test_causal_attention(code, D, Sq, Skv, padded):
    labels = check_contiguous(MHA, code, HQ, D, Sq, Skv, padded)
    if code == H.BF16:
        assert {"attn_fwd_mfma", "attn_bwd_dkv_mfma", "attn_bwd_dq_mfma"} <= set(labels), labels
    elif padded:
        assert {"attn_fwd_f32_mfma", "attn_bwd_dkv_f32_mfma", "attn_bwd_dq_f32_mfma"} <= set(labels), labels
    else:
        assert not any("mfma" in n for n in labels), labels


@pytest.mark.parametrize("code,D,Sq,Skv,padded", CAUSAL)
def test_causal_attention_gqa(code, D, Sq, Skv, padded):
    labels = check_contiguous(GQA, code, 1, D, Sq, Skv, padded)
    assert "attn_bwd_dkv_group_sum" in labels, labels


def test_causal_attention_gqa_without_queries_launches_nothing():
    q = kfunca.from_numpy(np.zeros((B, HQ, 0, 64), np.float32), 0)
    k, v = (kfunca.from_numpy(np.ones((B, 1, 33, 64), np.float32), 0) for _ in range(2))
    with Profiled() as op:
        out = kfunca.causal_attention_gqa(q, k, v)
    assert out.sizes() == [B, HQ, 0, 64] and op.all == {}, (out.sizes(), op.all)


@pytest.mark.parametrize("code,D,Sq,Skv,padded,kv_len", [
    (H.BF16, 128, 128, 192, None, [192, 70]),
    (H.BF16, 80, 33, 65, (33, 65, 128), None),   # the head is padded to 128, rows never are
    (H.BF16, 80, 33, 65, (33, 65, 128), [65, 20]),
    (H.F32, 80, 33, 65, None, None)])            # f32 is never padded
def test_attention(code, D, Sq, Skv, padded, kv_len):
    labels = check_contiguous(FULL, code, 1, D, Sq, Skv, padded, kv_len)
    assert all(n.startswith("attn_full") for n in labels), labels
    assert any("mfma" in n for n in labels) == (code == H.BF16), labels


# ---- the packed projection ----
def packed_operator(family, code, qkv, gout, S, kv_heads, kv_len=None):
    """the packed operator of the family, forward + backward: out [B*S, Hq D], dqkv"""
    tx = leaf(qkv, code)
    if family == FULL:
        out = kfunca.attention_qkv(tx, B, S, HQ, kv_heads=kv_heads, kv_len=len_tensor(kv_len))
    elif kv_heads is None:
        out = kfunca.causal_attention_qkv(tx, B, S, HQ)
    else:
        out = kfunca.causal_attention_qkv(tx, B, S, HQ, kv_heads=kv_heads)
    out.backward(value(gout, code))
    return [as_np(out, code), as_np(tx.grad(), code)]


def packed_direct(entry, code, qkv, gout, S, Hkv, kv_len=None):
    """kf_attn_{fwd,bwd}_strided (entry MHA), _gqa with every layout given (GQA) or kf_attn_full_* with layouts (FULL) on the packed
    projection in place: q at column 0, k at Hq D, v at (Hq + Hkv) D; out and its gradient as [B*S, Hq D]: out, dqkv"""
    W = qkv.shape[1]
    D = W // (HQ + 2 * Hkv)
    d, dkv, es = HQ * D, Hkv * D, 2
    packed, flat = (S * W, D, W), (S * d, D, d)
    scale = scale_of(D)
    bx, bg = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout)
    bn = None if kv_len is None else H.DevBuf.from_numpy(np.asarray(kv_len, np.int64))
    lens = None if bn is None else bn.ptr
    bo, bl, bd = H.DevBuf(B * S * d * es), H.DevBuf(4 * B * HQ * S), H.DevBuf(qkv.nbytes)
    x = (bx.ptr, bx.ptr + d * es, bx.ptr + (d + dkv) * es)
    g = (bd.ptr, bd.ptr + d * es, bd.ptr + (d + dkv) * es)
    fwd_lay, bwd_lay = (packed, packed, packed, flat), (packed, packed, packed, flat, flat, packed, packed, packed)
    if entry == MHA:
        assert Hkv == HQ
        H.attn_fwd_strided(code, B, HQ, S, S, D, scale, x[0], packed, x[1], packed, x[2], packed, bo.ptr, flat, bl.ptr)
        need = H.attn_bwd_workspace_bytes(code, B, HQ, S, S, D)
        w = H.DevBuf(max(need, 1))
        H.attn_bwd_strided(code, B, HQ, S, S, D, scale, x[0], packed, x[1], packed, x[2], packed, bo.ptr, flat, bl.ptr, bg.ptr, flat, g[0], packed,
                           g[1], packed, g[2], packed, w.ptr, need)
    elif entry == GQA:
        H.attn_fwd_gqa(code, B, HQ, Hkv, S, S, D, scale, *x, bo.ptr, bl.ptr, layouts=fwd_lay)
        need, _ = H.attn_bwd_gqa_workspace_bytes(code, B, HQ, Hkv, S, S, D)
        w = H.DevBuf(max(need, 1))
        H.attn_bwd_gqa(code, B, HQ, Hkv, S, S, D, scale, *x, bo.ptr, bl.ptr, bg.ptr, *g, w.ptr, need, layouts=bwd_lay)
    else:
        H.attn_full_fwd(code, B, HQ, Hkv, S, S, D, scale, *x, bo.ptr, bl.ptr, kv_len=lens, layouts=fwd_lay)
        need = H.attn_full_bwd_workspace_bytes(code, B, HQ, Hkv, S, S, D)
        w = H.DevBuf(max(need, 1))
        H.attn_full_bwd(code, B, HQ, Hkv, S, S, D, scale, *x, bo.ptr, bl.ptr, bg.ptr, *g, w.ptr, need, kv_len=lens, layouts=bwd_lay)
    H.device_sync()
    return [bo.to_numpy((B * S, d), qkv.dtype), bd.to_numpy(qkv.shape, qkv.dtype)]


def packed_inputs(code, D, S, Hkv):
    rng = np.random.default_rng(100 * D + S + Hkv + code)
    return rnd(rng, code, (B * S, (HQ + 2 * Hkv) * D)), rnd(rng, code, (B * S, HQ * D))


# (operator family, kv_heads as the caller passes it, K/V heads, the C-ABI entry of the fast shape)
PACKED = [(MHA, None, HQ, MHA),    # causal_attention_qkv(qkv, B, S, H): the strided entries
          (GQA, HQ, HQ, MHA),      # kv_heads equal to H: the strided entries too
          (GQA, 1, 1, GQA),        # kv_heads != H: the grouped entries with every layout given
          (FULL, 1, 1, FULL),
          (FULL, None, HQ, FULL)]  # the full entries also when Hkv = H


@pytest.mark.parametrize("family,kv_heads,Hkv,entry", PACKED)
def test_packed_fast_shape(family, kv_heads, Hkv, entry):
    code, D, S = H.BF16, 64, 100
    kv_len = [100, 37] if family == FULL and Hkv == 1 else None
    qkv, gout = packed_inputs(code, D, S, Hkv)
    with Profiled() as op:
        got = packed_operator(family, code, qkv, gout, S, kv_heads, kv_len)
    with Profiled() as abi:
        want = packed_direct(entry, code, qkv, gout, S, Hkv, kv_len)
    assert same(got[0], want[0]), "out differs from the direct call"
    assert same(got[1], want[1]), "dqkv differs from the direct call"
    assert op.attn == abi.attn and op.attn, (op.attn, abi.attn)
    assert ("attn_bwd_dkv_group_sum" in op.attn) == (entry == GQA), op.attn


@pytest.mark.parametrize("code,D,S", [(H.F32, 64, 64), (H.BF16, 96, 65)])
@pytest.mark.parametrize("family,kv_heads,Hkv", [(MHA, None, HQ), (GQA, 1, 1), (FULL, 1, 1)])
def test_packed_fallback_is_the_contiguous_operator(family, kv_heads, Hkv, code, D, S):
    kv_len = [S, 20] if family == FULL else None
    qkv, gout = packed_inputs(code, D, S, Hkv)
    d, dkv = HQ * D, Hkv * D
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    flat = lambda x4: x4.transpose(0, 2, 1, 3).reshape(B * S, -1)  # noqa: E731
    with Profiled() as op:
        got = packed_operator(family, code, qkv, gout, S, kv_heads, kv_len)
    with Profiled() as split:
        want = operator(family, code, heads(qkv[:, :d], HQ), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, HQ), kv_len)
    assert same(got[0], np.ascontiguousarray(flat(want[0]))), "out differs from the contiguous operator on the split heads"
    assert same(got[1], np.ascontiguousarray(np.concatenate([flat(x) for x in want[1:]], axis=1))), "dqkv differs"
    assert op.attn == split.attn and op.attn, (op.attn, split.attn)


# ---- refusals: the exact texts ----
def text_of(call):
    with pytest.raises(RuntimeError) as e:
        call()
    head, sep, text = str(e.value).partition("but got false. ")
    assert sep, str(e.value)
    return text.rstrip("\n")


def f32(*shape):
    return kfunca.from_numpy(np.zeros(shape, np.float32), 0)


def i64(*shape):
    return kfunca.from_numpy(np.zeros(shape, np.int64), 0)


def test_causal_attention_refusal():
    assert text_of(lambda: kfunca.causal_attention(i64(2, 2, 8, 64), i64(2, 2, 8, 64), i64(2, 2, 8, 64))) == "Unsupported ScalarType Long"


@pytest.mark.parametrize("name,dtype_text", [("causal_attention_gqa", "Unsupported ScalarType Long"),
                                             ("attention", "attention supports float, half and bfloat16")])
def test_contiguous_refusals(name, dtype_text):
    fn = getattr(kfunca, name)
    q, k = f32(2, 4, 8, 64), f32(2, 2, 8, 64)
    assert text_of(lambda: fn(f32(2, 4, 64), k, k)) == f"{name} expects q [B, Hq, Sq, D] and k, v [B, Hkv, Skv, D]"
    assert text_of(lambda: fn(q, f32(2, 2, 8, 32), f32(2, 2, 8, 32))) == f"{name}: shapes of q, k, v do not match"
    assert text_of(lambda: fn(q, k, f32(2, 2, 9, 64))) == f"{name}: shapes of q, k, v do not match"
    assert text_of(lambda: fn(q, f32(2, 3, 8, 64), f32(2, 3, 8, 64))) == f"{name}: the K/V head count 3 must divide the query head count 4"
    assert text_of(lambda: fn(q, f32(2, 8, 8, 64), f32(2, 8, 8, 64))) == f"{name}: the K/V head count 8 must divide the query head count 4"
    assert text_of(lambda: fn(q, k.bfloat16(), k.bfloat16())) == f"{name}: q, k, v must share a dtype"
    assert text_of(lambda: fn(i64(2, 4, 8, 64), i64(2, 2, 8, 64), i64(2, 2, 8, 64))) == dtype_text
    assert text_of(lambda: fn(f32(2, 8, 4, 64).permute(0, 2, 1, 3), k, k)) == f"{name} expects dense tensors"
    assert text_of(lambda: fn(q, f32(2, 2, 0, 64), f32(2, 2, 0, 64))) == f"{name}: keys are empty"


def test_attention_refusals_of_its_own():
    q, k = f32(2, 4, 8, 64), f32(2, 2, 8, 64)
    assert text_of(lambda: kfunca.attention(f32(2, 4, 8, 257), f32(2, 2, 8, 257), f32(2, 2, 8, 257))) == "attention: head size 257 outside [1, 256]"
    assert text_of(lambda: kfunca.attention(q, k, k, kv_len=f32(2))) == "attention: kv_len must be of type Long"
    assert text_of(lambda: kfunca.attention(q, k, k, kv_len=i64(3))) == "attention: kv_len must hold B = 2 elements on the operands' device"


def bf16(*shape):
    return f32(*shape).bfloat16()


def test_causal_attention_qkv_refusals():
    fn = kfunca.causal_attention_qkv
    assert text_of(lambda: fn(bf16(2, 8, 3 * 2 * 64), 2, 8, 2)) == "causal_attention_qkv expects a contiguous [B*S, 3*H*D] tensor"
    assert text_of(lambda: fn(bf16(16, 3 * 2 * 64), 2, 9, 2)) == "causal_attention_qkv: shape does not match B, S, H"
    assert text_of(lambda: fn(bf16(16, 3 * 2 * 64 + 1), 2, 8, 2)) == "causal_attention_qkv: shape does not match B, S, H"
    wide = "causal_attention_qkv expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor"
    assert text_of(lambda: fn(bf16(2, 8, 6 * 64), 2, 8, 4, kv_heads=1)) == wide
    assert text_of(lambda: fn(bf16(16, 10 * 64), 2, 8, 4, kv_heads=3)) == "causal_attention_qkv: kv_heads 3 must divide H 4"
    assert text_of(lambda: fn(bf16(16, 6 * 64), 2, 9, 4, kv_heads=1)) == "causal_attention_qkv: shape does not match B, S, H, kv_heads"
    assert text_of(lambda: fn(bf16(16, 6 * 64 + 1), 2, 8, 4, kv_heads=1)) == "causal_attention_qkv: shape does not match B, S, H, kv_heads"


def test_attention_qkv_refusals():
    fn = kfunca.attention_qkv
    assert text_of(lambda: fn(bf16(2, 8, 6 * 64), 2, 8, 4, kv_heads=1)) == "attention_qkv expects a contiguous [B*S, (H + 2*kv_heads)*D] tensor"
    assert text_of(lambda: fn(bf16(16, 10 * 64), 2, 8, 4, kv_heads=3)) == "attention_qkv: kv_heads 3 must divide H 4"
    assert text_of(lambda: fn(bf16(16, 6 * 64), 2, 9, 4, kv_heads=1)) == "attention_qkv: shape does not match B, S, H, kv_heads"
    assert text_of(lambda: fn(bf16(16, 6 * 64 + 1), 2, 8, 4, kv_heads=1)) == "attention_qkv: shape does not match B, S, H, kv_heads"
    # kv_len, on the fast shape (checked by the packed operator itself) and off it (checked by the contiguous operator it falls back to)
    for x in (bf16(16, 6 * 64), f32(16, 6 * 64)):
        assert text_of(lambda: fn(x, 2, 8, 4, kv_heads=1, kv_len=f32(2))) == "attention: kv_len must be of type Long"
        assert text_of(lambda: fn(x, 2, 8, 4, kv_heads=1, kv_len=i64(3))) == "attention: kv_len must hold B = 2 elements on the operands' device"
