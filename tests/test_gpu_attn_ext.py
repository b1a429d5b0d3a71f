"""-m gpu: the masked attention family with score modifiers (kf_attn_ext_fwd / kf_attn_ext_bwd): logit soft-capping,
s = cap tanh(scale q.k / cap), and attention sinks, one logit per query head that joins the softmax denominator and owns no value row,
under each of the four masks (full, prefix, window, document).

The reference is tests/attn_ext_ref.py's float64 attention (tests/test_attn_ext_ref.py holds it to torch's float64 autograd and shows
that every cap and sink vector used here moves each output beyond its bound, so a kernel that ignored a modifier fails here). 16-bit
o, dq, dk, dv: oracle.checks.check_one with the floors of format_floor_vis, unchanged. lse: 2e-6 (1 + |lse|) + softcap 2^-20
(attn_ext_ref.check_lse_ext, where the second term is derived from the kernels' tanh); a row without a key is -inf exactly without a
sink and the f32 sink itself with one. dsink: the bound the reference returns per head. The f32 generic path: the rule
tests/test_gpu_attn_window.py restates (rtol 1e-4 / atol 1e-4 forward and lse - plus softcap 2^-20 for lse -, rtol 1e-3 / atol 1e-4
backward).

Every output (o, lse, dq, dk, dv, dsink) and the workspace are pre-filled with 0xFF (tests/poison.py). Shapes sit at the kernels' seams:
32 queries or keys per wave, 64 per tile, 128 per workgroup."""
import numpy as np
import pytest

import tests.test_gpu_attn_doc as DOC
import tests.test_gpu_attn_full as F
import tests.test_gpu_attn_prefix as P
import tests.test_gpu_attn_window as WIN
from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O
from tests import poison
from tests.attn_doc_ref import cu_of, doc_vis
from tests.attn_ext_ref import BIG_CAP, CAPS, attn_ref64_ext, check_lse_ext, sinks_for
from tests.attn_full_ref import format_floor_vis, key_len_vis
from tests.attn_window_ref import abi, window_vis

pytestmark = pytest.mark.gpu

NAMES = ("o", "lse", "dq", "dk", "dv")


# ---- a mask as the tests name it: (kind, kv_len or cu, prefix_len | window | causal) ----
def vis_of(mask, q, k):
    kind, lens, arg = mask
    B, Sq, Skv = q.shape[0], q.shape[2], k.shape[2]
    if kind == "full":
        return key_len_vis(lens, Sq, Skv, B)
    if kind == "prefix":
        return P.vis_of(q, k, lens, arg)
    if kind == "window":
        return window_vis(lens, arg[0], arg[1], Sq, Skv, B)
    return doc_vis(np.asarray(lens, np.int64), Sq, arg)


def dev_mask(mask, S):
    """(AttnMask, the device buffers it points into, what must run first on the stream)"""
    kind, lens, arg = mask
    if kind == "doc":
        bcu, (bkv, bs, be), n = DOC.build_table(np.asarray(lens, np.int64), S)
        B = np.asarray(lens).shape[0]
        first = lambda st: H.attn_doc_table(B, S, n, bcu.ptr, bkv.ptr, bs.ptr, be.ptr, stream=st)  # noqa: E731
        return H.attn_mask(H.ATTN_MASK_DOC, kv_len=bkv.ptr, doc_start=bs.ptr, doc_end=be.ptr, causal=arg), (bcu, bkv, bs, be), first
    bl = WIN.dev_i64(lens)
    lp = None if bl is None else bl.ptr
    if kind == "full":
        return H.attn_mask(H.ATTN_MASK_FULL, kv_len=lp), (bl,), None
    if kind == "prefix":
        bp = WIN.dev_i64(arg)
        return H.attn_mask(H.ATTN_MASK_PREFIX, kv_len=lp, prefix_len=None if bp is None else bp.ptr), (bl, bp), None
    return H.attn_mask(H.ATTN_MASK_WINDOW, kv_len=lp, window_left=abi(arg[0]), window_right=abi(arg[1])), (bl,), None


def run(code, q, k, v, go, mask, softcap=0.0, sink=None, graph=False, fill=0xFF):
    """kf_attn_ext_fwd + kf_attn_ext_bwd on contiguous tensors: (o, lse, dq, dk, dv, dsink or None). Outputs and workspace pre-filled."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    scale = F.scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    m, keep, first = dev_mask(mask, Sq)
    bsink = None if sink is None else H.DevBuf.from_numpy(np.asarray(sink, np.float32))
    need = H.attn_ext_bwd_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    sizes = (q.nbytes, 4 * B * Hq * Sq, q.nbytes, k.nbytes, v.nbytes, need, 4 * Hq)
    bo, blse, dq, dk, dv, w, bds = (H.DevBuf(max(n, 1)) for n in sizes)
    for buf, n in zip((bo, blse, dq, dk, dv, w, bds), sizes):
        poison.fill(buf.ptr, n, fill)
    H.device_sync()
    kw = dict(mask=m, softcap=softcap, sink=None if bsink is None else bsink.ptr)

    def calls(st):
        if first:
            first(st)
        H.attn_ext_fwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, stream=st, **kw)
        H.attn_ext_bwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need,
                       dsink=None if bsink is None else bds.ptr, stream=st, **kw)

    if graph:
        s = H.Stream()
        with H.Graph.capture(s) as g:
            calls(s.handle)
        g.launch()
        s.sync()
    else:
        calls(None)
    H.device_sync()
    del keep
    return (bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, Sq), np.float32), dq.to_numpy(q.shape, q.dtype), dk.to_numpy(k.shape, k.dtype),
            dv.to_numpy(v.shape, v.dtype), None if bsink is None else bds.to_numpy((Hq,), np.float32))


def no_nan(code, got, what=""):
    for name, g in zip(NAMES + ("dsink",), got):
        if g is not None:
            x = g if name in ("lse", "dsink") else O.to_float(g, code)
            assert not np.isnan(x).any(), f"{what} {name}: NaN"


def check_dead_rows(got, vis, sink, what=""):
    """zero BITS in o and dq of a query that sees no key, in dk and dv of a key no query sees; the dead row's lse is the f32 sink itself"""
    WIN.zeros_where_nothing_is_seen(got[:5], vis, what)
    if sink is not None:
        dead = ~vis.any(axis=2)
        for b in range(vis.shape[0]):
            for h in range(got[1].shape[1]):
                assert F.same(got[1][b, h][dead[b]], np.full(int(dead[b].sum()), sink[h], np.float32)), f"{what} batch {b} head {h}: a dead row's lse is not the sink"


def check_dsink(got, ref, what=""):
    d = np.abs(got[5].astype(np.float64) - ref["dsink"])
    print(f"{what} dsink: error / bound {np.max(d / np.maximum(ref['dsink_bound'], np.finfo(np.float64).tiny)):.3f}")
    assert np.isfinite(got[5]).all() and (d <= ref["dsink_bound"]).all(), f"{what} dsink: {got[5]} vs {ref['dsink']} (bound {ref['dsink_bound']})"


def check16(code, q, k, v, go, got, vis, softcap, sink, what="", dsink=True):
    no_nan(code, got, what)
    ref = attn_ref64_ext(q, k, v, go, vis, code, softcap=softcap, sink=sink)
    fl = format_floor_vis(q, k, v, go, vis, code)
    for name, g in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4])):
        K.check_one(name, g, ref, code, what, floor=fl.get(name))
    check_lse_ext(got[1], ref, softcap, sink, what)
    check_dead_rows(got, vis, sink, what)
    if sink is not None and dsink:
        check_dsink(got, ref, what)
    return ref


def label_kind(mask):
    if mask[0] == "window":      # the two windows an older family already is
        l, r = mask[2]
        return "full" if l is None and r is None else ("prefix" if l is None and r == 0 else "window")
    return mask[0]


def check_labels(labels, mask, D, softcap, sink, generic=False):
    kind, mine = label_kind(mask), {n for n in labels if n.startswith("attn_") and n != "attn_doc_table"}
    mid = "_cap" if softcap else ""
    if generic:
        want = {f"attn_{kind}{mid}_fwd_generic", f"attn_{kind}{mid}_bwd_dq_generic", f"attn_{kind}{mid}_bwd_dkv_generic", "attn_full_bwd_delta_generic"}
    else:
        want = {f"attn_{kind}{mid}_fwd_mfma_d{D}", f"attn_{kind}{mid}_bwd_dq_mfma_d{D}", f"attn_{kind}{mid}_bwd_dkv_mfma_d{D}", "attn_full_bwd_delta"}
    if sink is not None:
        want.add("attn_sink_grad")
    assert mine == want, (sorted(mine), sorted(want))


def mixed_lens(Skv):
    return WIN.mixed_lens(Skv)


def masks_for(Sq, Skv):
    """each kind over four batches with mixed lengths (one of them 0); the document mask where Sq = Skv"""
    lens = mixed_lens(Skv)
    out = [("full", lens, None), ("prefix", lens, [Skv // 3, 0, 5, 200]), ("window", lens, (40, 3))]
    if Sq == Skv:
        S = Sq
        out.append(("doc", cu_of([[S], [], [S // 3, S - S // 3 - min(S - S // 3, 5)], [1] * min(S, 3)], 3), True))
    return out


# ---- matrix-core forward and backward: every mask, cap only / sink only / both ----
SHAPES = [(1, 1), (33, 33), (200, 200), (65, 257), (257, 65), (130, 333)]


@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
def test_matrix_core_fwd_bwd(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq * 7919 + Skv * 31 + D + code)
    Hq, Hkv = (2, 1) if D == 64 else (4, 2)
    q, k, v, go = F.inputs(rng, code, 4, Hq, Hkv, Sq, Skv, D)
    sink = sinks_for(Hq, D)
    for mask in masks_for(Sq, Skv):
        vis = vis_of(mask, q, k)
        for softcap, sk in ((CAPS[0], None), (0.0, sink), (CAPS[1], sink)):
            what = f"{Sq}x{Skv} D{D} {mask[0]} cap {softcap} sink {sk is not None}"
            got, labels = F.profiled(lambda: run(code, q, k, v, go, mask, softcap, sk))
            check16(code, q, k, v, go, got, vis, softcap, sk, what)
            check_labels(labels, mask, D, softcap, sk)


def test_a_large_cap_agrees_with_the_uncapped_call():
    code, D, S = H.BF16, 128, 200
    rng = np.random.default_rng(5)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    mask = ("window", [S, 150], (70, 0))
    got = run(code, q, k, v, go, mask, BIG_CAP)
    vis, what = vis_of(mask, q, k), "a cap that bends nothing, against the uncapped reference"
    no_nan(code, got, what)
    ref = attn_ref64_ext(q, k, v, go, vis, code)
    fl = format_floor_vis(q, k, v, go, vis, code)
    for name, g in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4])):
        K.check_one(name, g, ref, code, what, floor=fl.get(name))
    # lse is f32: the kernel's tanh error scales with the cap it ran with, so lse is held to that cap's own reference and tolerance
    check_lse_ext(got[1], attn_ref64_ext(q, k, v, None, vis, code, softcap=BIG_CAP), BIG_CAP, None, what)


# ---- rows that see no key ----
@pytest.mark.parametrize("softcap", [0.0, CAPS[1]])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_dead_rows(code, D, softcap):
    Sq, Skv, Hq = 257, 200, 4
    rng = np.random.default_rng(D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, 2, Sq, Skv, D)
    mask = ("window", [40, 0, 130], (31, 0))       # queries m >= len_b + 31 see no key
    vis, sink = vis_of(mask, q, k), sinks_for(Hq, 7)
    assert (~vis.any(axis=2)).sum() > 3 * 100
    for sk in (None, sink):
        o, lse, dq, dk, dv, ds = got = run(code, q, k, v, go, mask, softcap, sk)
        if softcap or sk is not None:
            check16(code, q, k, v, go, got, vis, softcap, sk, f"dead rows, sink {sk is not None}")
        for b, first_dead in ((0, 71), (1, 0), (2, 161)):
            assert WIN.zero_bits(o[b, :, first_dead:]) and WIN.zero_bits(dq[b, :, first_dead:]), b
            if sk is None:
                assert np.isneginf(lse[b, :, first_dead:]).all()
            else:
                assert (lse[b, :, first_dead:] == sink[None, :, None]).all() and np.isfinite(lse[b]).all()


# ---- sinks of any size ----
@pytest.mark.parametrize("code,D,softcap", [(H.BF16, 128, 0.0), (H.F16, 64, 0.0), (H.BF16, 64, CAPS[1]), (H.F32, 64, 0.0), (H.F32, 48, CAPS[0])])
def test_extreme_sinks(code, D, softcap):
    Sq, Skv = (130, 200) if code != H.F32 else (40, 70)
    rng = np.random.default_rng(D + 1)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, Sq, Skv, D)
    mask = ("prefix", [Skv, 77 if code != H.F32 else 30], [10, 0])
    sink = np.array([100.0, -100.0, -np.inf, 0.5], np.float32)
    got = run(code, q, k, v, go, mask, softcap, sink)
    plain = run(code, q, k, v, go, mask, softcap, None)
    for name, g in zip(NAMES + ("dsink",), got):
        x = g if name in ("lse", "dsink") else O.to_float(g, code)
        assert np.isfinite(x).all(), f"{name}: non-finite values"
    o = O.to_float(got[0], code)
    assert np.abs(o[:, 0]).max() <= 1e-30, "sink = +100 leaves o ~ 0"
    assert (np.abs(got[1][:, 0].astype(np.float64) - 100.0) <= 2e-6 * 101.0).all(), "sink = +100: lse ~ 100"
    for h, what in ((1, "-100"), (2, "-inf")):
        assert F.same(got[0][:, h], plain[0][:, h]) and F.same(got[1][:, h], plain[1][:, h]), f"sink = {what} does not have the bits of the call without a sink"
    assert got[5][2] == 0.0 and abs(got[5][1]) < 1e-30
    if code != H.F32:   # (dsink of the +-100 heads is a sum of weights near 1e-44, below anything f32 holds relative to it: not held to the bound here)
        check16(code, q, k, v, go, got, vis_of(mask, q, k), softcap, sink, "extreme sinks", dsink=False)


# ---- modifiers off: the four families' kernels, labels and bits ----
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64), (H.F32, 40)])
def test_modifiers_off_is_each_family_bit_for_bit(code, D):
    S = 130 if code != H.F32 else 40
    rng = np.random.default_rng(S + D)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, S, S, D)
    lens, pre, window = [S, 64, 0, 33], [20, 0, 5, 40], (17, 5)
    cu = cu_of([[S], [40, S - 50], [], [33]], 2)
    generic = code == H.F32
    for mask, want in ((("full", lens, None), lambda: F.run(code, q, k, v, go, lens)),
                       (("prefix", lens, pre), lambda: P.run(code, q, k, v, go, lens, pre)),
                       (("window", lens, window), lambda: WIN.run(code, q, k, v, go, lens, window)),
                       (("window", lens, (None, 0)), lambda: P.run(code, q, k, v, go, lens, None)),
                       (("doc", cu, True), lambda: DOC.run(code, q, k, v, go, cu, True))):
        got, labels = F.profiled(lambda: run(code, q, k, v, go, mask))
        assert got[5] is None
        WIN.assert_same(got[:5], want(), f"kf_attn_ext_* without modifiers is not the {mask[0]} family's call")
        check_labels(labels, mask, D, 0.0, None, generic)


# ---- dsink: reproducible to the bit, capturable ----
@pytest.mark.parametrize("code,D,softcap", [(H.BF16, 128, 0.0), (H.F16, 64, CAPS[0]), (H.F32, 80, CAPS[1])])
def test_dsink_is_reproducible_and_capturable(code, D, softcap):
    Sq, Skv, Hq = (513, 130, 4) if code != H.F32 else (70, 40, 4)
    rng = np.random.default_rng(513 + D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, 2, Sq, Skv, D)
    mask, sink = ("window", [Skv, 77 % Skv, 0], (70, 0)), sinks_for(Hq, 3)
    a, b, g = (run(code, q, k, v, go, mask, softcap, sink, graph=gr) for gr in (False, False, True))
    for name, x, y, z in zip(NAMES + ("dsink",), a, b, g):
        assert F.same(x, y), f"{name}: two runs differ"
        assert F.same(x, z), f"{name}: the captured run differs from the eager one"
    ref = attn_ref64_ext(q, k, v, go, vis_of(mask, q, k), code, softcap=softcap, sink=sink)
    check_dsink(a, ref, f"D{D}")
    for fill in (0x00, 0x7F):
        c = run(code, q, k, v, go, mask, softcap, sink, fill=fill)
        assert all(F.same(x, y) for x, y in zip(a, c)), f"outputs or workspace pre-filled with {fill:#x} changed the result"


# ---- K and V rows at n >= len_b are never read ----
@pytest.mark.parametrize("code,D,softcap", [(H.BF16, 128, CAPS[0]), (H.F16, 64, 0.0), (H.BF16, 80, CAPS[1])])
def test_padding_never_reaches_an_output(code, D, softcap):
    Sq, Skv, lens = 130, 200, [200, 0, 1, 64, 65, 150]
    rng = np.random.default_rng(64 + code)
    q, k, v, go = F.inputs(rng, code, len(lens), 2, 2, Sq, Skv, D)
    kz, vz = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    kp, vp = kz.copy(), vz.copy()
    for b, ln in enumerate(lens):
        kz[b, :, ln:] = 0
        vz[b, :, ln:] = 0
        kp[b, :, ln:] = np.nan
        vp[b, :, ln:] = np.inf
    mask, sink = ("window", lens, (40, 3)), sinks_for(2, 9)
    clean = run(code, q, O.from_float(kz, code), O.from_float(vz, code), go, mask, softcap, sink)
    check16(code, q, k, v, go, clean, vis_of(mask, q, k), softcap, sink, "zero padding")
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, mask, softcap, sink)
    for name, x, y in zip(NAMES + ("dsink",), dirty, clean):
        assert F.same(x, y), f"{name}: NaN / Inf padding changed the result"


# ---- strided: the packed projection read in place ----
@pytest.mark.parametrize("code,D,S,softcap", [(H.BF16, 128, 200, CAPS[0]), (H.F16, 64, 129, 0.0)])
def test_packed_layout_equals_contiguous(code, D, S, softcap):
    B, Hq, Hkv = 2, 4, 2
    W, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = W + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    lens, window, sink = [S, S - 70], (70, 0), sinks_for(Hq, 11)
    ref = run(code, q, k, v, go, ("window", lens, window), softcap, sink)
    packed, flat, gpack = (S * W, D, W), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo, bl, bsink = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout), WIN.dev_i64(lens), H.DevBuf.from_numpy(sink)
    ob, o = F.guarded(B * S * d * es)
    lb, lse = F.guarded(4 * B * Hq * S)
    gb, g = F.guarded(B * S * PADW * es)
    sb, ds = F.guarded(4 * Hq)
    scale = F.scale_of(D)
    kw = dict(mask=H.attn_mask(H.ATTN_MASK_WINDOW, kv_len=bl.ptr, window_left=window[0], window_right=window[1]), softcap=softcap, sink=bsink.ptr)
    H.attn_ext_fwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, layouts=(packed, packed, packed, flat), **kw)
    need = H.attn_ext_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    poison.fill(w.ptr, need, 0xFF)
    H.attn_ext_bwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                   g + (d + dkv) * es, w.ptr, need, dsink=ds, layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack), **kw)
    H.device_sync()
    assert F.same(heads(F.read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert F.same(F.read(lse, (B, Hq, S), np.float32), ref[1])
    gq = F.read(g, (B * S, PADW), qkv.dtype)
    assert F.same(heads(gq[:, :d], Hq), ref[2]) and F.same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and F.same(heads(gq[:, d + dkv:W], Hkv), ref[4])
    assert F.same(F.read(ds, (Hq,), np.float32), ref[5])
    assert (gq[:, W:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, n in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es), (sb, 4 * Hq)):
        assert F.guards_ok(buf, n)


# ---- generic path ----
def check_generic(code, q, k, v, go, got, vis, softcap, sink):
    """tests/test_gpu_attn_window.py's check_generic with the modifiers' reference; lse gets softcap 2^-20 beside its atol"""
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    ref = attn_ref64_ext(q, k, v, go, vis, code, softcap=softcap, sink=sink)
    dead = np.isneginf(ref["lse"])
    assert np.allclose(f(got[0]), ref["o"], rtol=1e-4, atol=1e-4)
    assert np.isneginf(got[1][dead]).all() and np.allclose(got[1][~dead], ref["lse"][~dead], rtol=1e-4, atol=1e-4 + (softcap or 0.0) * 2.0 ** -20)
    for name, g in zip(("dq", "dk", "dv"), got[2:5]):
        assert np.allclose(f(g), ref[name], rtol=1e-3, atol=1e-4), name
    if sink is not None:
        check_dsink(got, ref, "generic f32")


@pytest.mark.parametrize("softcap,with_sink", [(CAPS[0], False), (0.0, True), (CAPS[1], True)])
@pytest.mark.parametrize("Sq,Skv", [(33, 70), (300, 290), (70, 70)])
@pytest.mark.parametrize("code,D", [(H.F32, 64), (H.BF16, 80), (H.F16, 40)])
def test_generic(code, D, Sq, Skv, softcap, with_sink):
    rng = np.random.default_rng(D + Sq + code)
    Hq = 4
    q, k, v, go = F.inputs(rng, code, 4, Hq, 2, Sq, Skv, D)
    sink = sinks_for(Hq, D) if with_sink else None
    lens = [Skv, 17, 0, Skv + 3]
    masks = [("full", lens, None), ("prefix", lens, [5, 0, 3, 30]), ("window", lens, (5, 2))]
    if Sq == Skv:
        masks.append(("doc", cu_of([[Sq], [20, 30], [], [1, 2, 3]], 3), False))
    for mask in masks:
        got, labels = F.profiled(lambda: run(code, q, k, v, go, mask, softcap, sink))
        vis = vis_of(mask, q, k)
        no_nan(code, got)
        if code == H.F32:
            check_generic(code, q, k, v, go, got, vis, softcap, sink)
            check_dead_rows(got, vis, sink)
        else:
            check16(code, q, k, v, go, got, vis, softcap, sink, f"generic D{D} {mask[0]}")
        check_labels(labels, mask, D, softcap, sink, generic=True)
