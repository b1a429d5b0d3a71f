"""-m gpu: sliding-window attention (kf_attn_window_fwd / kf_attn_window_bwd, kfunca.attention(..., window=(left, right)),
kfunca.attention_qkv): query m sees key n iff n < len_b and (left unbounded or n >= m - left) and (right unbounded or n <= m + right).

The reference is tests/attn_full_ref.py's float64 attention under the visibility of tests/attn_window_ref.py. The 16-bit outputs are
held to the project's scale-aware bounds (oracle.checks.check_one with the floors of format_floor_vis), lse to 2e-6 (1 + |lse|) and to
-inf exactly where a row sees no key - which a window makes possible inside a live batch (m - left >= len_b). The f32 generic path is
held to the rule tests/test_gpu_attn_prefix.py's check_generic applies (rtol 1e-4 / atol 1e-4 forward and lse, rtol 1e-3 / atol 1e-4
backward), restated here; the 16-bit generic cases (D 80, D 40) to the scale-aware 16-bit bounds, as there. The operator tests add that
file's comparison with torch's scaled_dot_product_attention on the CPU in f32: max |got - ref| <= TOL max |ref|, TOL = 2^-5 (bf16) and
1e-4 (f32), over the rows that see a key; the others must be zeros.

Every call here finds its outputs (o, lse, dq, dk, dv) and its workspace pre-filled with 0xFF (tests/poison.py): whatever a kernel does
not write, or reads before writing, is a NaN in the result. Shapes sit at the kernels' seams: 32 queries or keys per wave, 64 per tile,
128 per workgroup. The helpers that do not name an entry are tests/test_gpu_attn_full.py's own, through a module import."""
import numpy as np
import pytest

import kfunca_amd as kfunca
import tests.test_gpu_attn_full as F
import tests.test_gpu_attn_prefix as P
from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O
from tests import poison
from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis
from tests.attn_window_ref import abi, window_vis

pytestmark = pytest.mark.gpu

NAMES = ("o", "lse", "dq", "dk", "dv")


def dev_i64(x):
    return None if x is None else H.DevBuf.from_numpy(np.asarray(x, np.int64))


def run(code, q, k, v, go, kv_len=None, window=(None, None), graph=False, fill=0xFF):
    """kf_attn_window_fwd + kf_attn_window_bwd on contiguous tensors: o, lse, dq, dk, dv. The outputs and the workspace are pre-filled
    with `fill`; graph: captured with kf_graph_* and launched once."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    scale = F.scale_of(D)
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    bl = dev_i64(kv_len)
    kw = dict(kv_len=None if bl is None else bl.ptr, window_left=abi(window[0]), window_right=abi(window[1]))
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    sizes = (q.nbytes, 4 * B * Hq * Sq, q.nbytes, k.nbytes, v.nbytes, need)
    bo, blse, dq, dk, dv, w = (H.DevBuf(n) for n in sizes)
    for buf, n in zip((bo, blse, dq, dk, dv, w), sizes):
        poison.fill(buf.ptr, n, fill)
    H.device_sync()

    def calls(st):
        H.attn_window_fwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, stream=st, **kw)
        H.attn_window_bwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, w.ptr, need,
                          stream=st, **kw)

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


def vis_of(q, k, kv_len, window):
    return window_vis(kv_len, window[0], window[1], q.shape[2], k.shape[2], q.shape[0])


def no_nan(code, got, what=""):
    for name, g in zip(NAMES, got):
        x = g if name == "lse" else O.to_float(g, code)
        assert not np.isnan(x).any(), f"{what} {name}: NaN"


def check16(code, q, k, v, go, got, vis, what=""):
    no_nan(code, got, what)
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    fl = format_floor_vis(q, k, v, go, vis, code)
    for name, g in zip(("o", "dq", "dk", "dv"), (got[0], got[2], got[3], got[4])):
        K.check_one(name, g, ref, code, what, floor=fl.get(name))
    check_lse(got[1], ref, what)
    zeros_where_nothing_is_seen(got, vis, what)


def zeros_where_nothing_is_seen(got, vis, what=""):
    """zero BITS: o and dq of a query that sees no key, dk and dv of a key no query sees (beyond the length or outside every window)"""
    o, _, dq, dk, dv = got
    for b in range(vis.shape[0]):
        dead_q, dead_k = ~vis[b].any(axis=1), ~vis[b].any(axis=0)
        assert zero_bits(o[b][:, dead_q]) and zero_bits(dq[b][:, dead_q]), f"{what} batch {b}: a query row that sees no key is not zero"
        assert zero_bits(dk[b][:, dead_k]) and zero_bits(dv[b][:, dead_k]), f"{what} batch {b}: a key row no query sees is not zero"


def assert_same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert F.same(x, y), f"{name}: {what}"


def zero_bits(x):
    return not F.bits(np.ascontiguousarray(x)).any()


MFMA_LABELS = ("attn_window_fwd_mfma", "attn_window_bwd_dq_mfma", "attn_window_bwd_dkv_mfma")
SHAPES = [(1, 1), (33, 33), (128, 128), (200, 200), (65, 257), (257, 65), (130, 333), (513, 130)]
WINDOWS = [(0, 0), (31, 0), (64, 0), (100, None), (17, 5), (70, 70)]


def mixed_lens(Skv):
    """the key lengths of the four batches one call carries: every key, none, a length that cuts a tile (and, at the shapes above, the
    window's tile of the last query blocks), a length one past a tile"""
    return [Skv, 0, max(1, Skv - 37), min(Skv, 65)]


def only_window_labels(labels, D):
    for label in MFMA_LABELS:
        assert f"{label}_d{D}" in labels, (label, sorted(labels))
    assert "attn_full_bwd_delta" in labels and not any("generic" in n for n in labels), sorted(labels)
    assert not any((n.startswith("attn_full_") and n != "attn_full_bwd_delta") or n.startswith("attn_prefix_") for n in labels), sorted(labels)


# ---- matrix-core forward and backward ----
@pytest.mark.parametrize("Sq,Skv", SHAPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("code", [H.BF16, H.F16])
def test_matrix_core_fwd_bwd(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq * 7919 + Skv * 31 + D + code)
    lens = mixed_lens(Skv)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, Sq, Skv, D)
    for window in WINDOWS:
        got, labels = F.profiled(lambda: run(code, q, k, v, go, lens, window))
        check16(code, q, k, v, go, got, vis_of(q, k, lens, window), f"{Sq}x{Skv} D{D} window {window}")
        only_window_labels(labels, D)


# ---- every window size at which a skip, a tile range or a body choice of one of the three kernels changes ----
SEAMS = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129, 199, 200, 300]


@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_seam_sweep(side):
    code, D, S = H.BF16, 128, 200
    rng = np.random.default_rng(200)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, S, S, D)
    lens = [S, 150]
    for w in SEAMS:
        window = {"left": (w, 0), "right": (0, w), "both": (w, w)}[side]
        got = run(code, q, k, v, go, lens, window)
        check16(code, q, k, v, go, got, vis_of(q, k, lens, window), f"seam sweep {window}")


# ---- exact zeros ----
def test_exact_zeros_queries_beyond_the_keys():
    code, D, Sq, Skv, window = H.BF16, 128, 257, 129, (10, 0)
    rng = np.random.default_rng(257129)
    q, k, v, go = F.inputs(rng, code, 2, 2, 2, Sq, Skv, D)
    lens = [Skv, 70]
    o, lse, dq, dk, dv = got = run(code, q, k, v, go, lens, window)
    no_nan(code, got)
    for b, first_dead in ((0, 139), (1, 80)):   # m - 10 >= len_b
        assert zero_bits(o[b, :, first_dead:]) and zero_bits(dq[b, :, first_dead:]) and np.isneginf(lse[b, :, first_dead:]).all(), b
        assert not zero_bits(o[b, :, first_dead - 1]) and np.isfinite(lse[b, :, :first_dead]).all(), b
    check16(code, q, k, v, go, got, vis_of(q, k, lens, window), "queries beyond the keys")


def test_exact_zeros_keys_no_query_sees():
    code, D, Sq, Skv, window = H.BF16, 128, 65, 257, (3, 2)
    rng = np.random.default_rng(65257)
    lens = [Skv, 40, 0, 66]
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, Sq, Skv, D)
    o, lse, dq, dk, dv = got = run(code, q, k, v, go, lens, window)
    no_nan(code, got)
    for b, ln in enumerate(lens):
        last = min(ln, 67)                  # the last query, 64, sees keys 61 .. 66
        assert zero_bits(dk[b, :, last:]) and zero_bits(dv[b, :, last:]), f"batch {b}: rows n > 66 or n >= len are not zeros"
        assert last == 0 or not zero_bits(dk[b, :, last - 1])
    assert zero_bits(o[2]) and zero_bits(dq[2]) and np.isneginf(lse[2]).all()
    check16(code, q, k, v, go, got, vis_of(q, k, lens, window), "keys no query sees")


# ---- every output is written in full, whatever it held ----
@pytest.mark.parametrize("code,D,window", [(H.BF16, 128, (10, 0)), (H.F16, 64, (3, 40)), (H.F32, 64, (10, 0))])
def test_outputs_are_written_in_full(code, D, window):
    Sq, Skv = (257, 129) if code != H.F32 else (70, 40)
    rng = np.random.default_rng(D + code)
    q, k, v, go = F.inputs(rng, code, 2, 2, 1, Sq, Skv, D)
    lens = [Skv, Skv // 2]
    want = run(code, q, k, v, go, lens, window, fill=0x00)
    for fill in (0xFF, 0x7F):
        got = run(code, q, k, v, go, lens, window, fill=fill)
        no_nan(code, got, f"fill {fill:#x}")
        assert_same(got, want, f"outputs or workspace pre-filled with {fill:#x} changed the result")


# ---- K and V rows at n >= len_b are never read ----
@pytest.mark.parametrize("poison_value", [np.nan, np.inf])
@pytest.mark.parametrize("code,D,window", [(H.BF16, 128, (40, 0)), (H.F16, 64, (20, 70)), (H.BF16, 80, (40, 3))])
def test_padding_never_reaches_an_output(poison_value, code, D, window):
    Sq, Skv = 130, 200
    lens = [200, 0, 1, 64, 65, 150]
    rng = np.random.default_rng(64 + code)
    q, k, v, go = F.inputs(rng, code, len(lens), 2, 2, Sq, Skv, D)
    kz, vz = O.to_float(k, code).copy(), O.to_float(v, code).copy()
    kp, vp = kz.copy(), vz.copy()
    for b, ln in enumerate(lens):
        kz[b, :, ln:] = 0
        vz[b, :, ln:] = 0
        kp[b, :, ln:] = poison_value
        vp[b, :, ln:] = -poison_value
    clean = run(code, q, O.from_float(kz, code), O.from_float(vz, code), go, lens, window)
    check16(code, q, k, v, go, clean, vis_of(q, k, lens, window), "zero padding")
    dirty = run(code, q, O.from_float(kp, code), O.from_float(vp, code), go, lens, window)
    assert_same(dirty, clean, f"padding of {poison_value} changed the result")


# ---- the two windows an older family already is: its bits ----
@pytest.mark.parametrize("Sq,Skv", [(130, 333), (257, 65)])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)])
def test_degenerate_windows_have_the_older_families_bits(code, D, Sq, Skv):
    rng = np.random.default_rng(Sq + D)
    q, k, v, go = F.inputs(rng, code, 4, 2, 2, Sq, Skv, D)
    for lens in (None, [Skv, 64, 0, 33]):
        assert_same(run(code, q, k, v, go, lens, (None, None)), P.run(code, q, k, v, go, lens, full=True), f"(-1, -1) is not kf_attn_full_*, kv_len {lens}")
        assert_same(run(code, q, k, v, go, lens, (None, 0)), P.run(code, q, k, v, go, lens, None), f"(-1, 0) is not kf_attn_prefix_*, kv_len {lens}")


# ---- grouped K/V heads ----
@pytest.mark.parametrize("Hkv", [2, 1])
@pytest.mark.parametrize("code,D,window", [(H.BF16, 128, (40, 0)), (H.F16, 64, (33, 65))])
def test_gqa(code, D, window, Hkv):
    Hq, Sq, Skv = 8, 130, 200
    lens = [200, 130, 77]
    rng = np.random.default_rng(Hkv + D)
    q, k, v, go = F.inputs(rng, code, 3, Hq, Hkv, Sq, Skv, D)
    got = run(code, q, k, v, go, lens, window)
    check16(code, q, k, v, go, got, vis_of(q, k, lens, window), f"gqa {Hq}/{Hkv}")


# ---- strided: the packed projection read in place ----
@pytest.mark.parametrize("code,D,S,window", [(H.BF16, 128, 200, (70, 0)), (H.F16, 64, 129, (5, 31))])
def test_packed_layout_equals_contiguous(code, D, S, window):
    B, Hq, Hkv = 2, 4, 2
    W, d, dkv, es = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D, 2
    PADW = W + 64   # the gradient lives in a wider buffer: the columns between its rows are guard bytes too
    rng = np.random.default_rng(S + D)
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    lens = [S, S - 70]
    ref = run(code, q, k, v, go, lens, window)
    packed, flat, gpack = (S * W, D, W), (S * d, D, d), (S * PADW, D, PADW)
    bqkv, bgo, bl = H.DevBuf.from_numpy(qkv), H.DevBuf.from_numpy(gout), dev_i64(lens)
    ob, o = F.guarded(B * S * d * es)
    lb, lse = F.guarded(4 * B * Hq * S)
    gb, g = F.guarded(B * S * PADW * es)
    scale = F.scale_of(D)
    kw = dict(kv_len=bl.ptr, window_left=abi(window[0]), window_right=abi(window[1]))
    H.attn_window_fwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse,
                      layouts=(packed, packed, packed, flat), **kw)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    w = H.DevBuf(need)
    H.attn_window_bwd(code, B, Hq, Hkv, S, S, D, scale, bqkv.ptr, bqkv.ptr + d * es, bqkv.ptr + (d + dkv) * es, o, lse, bgo.ptr, g, g + d * es,
                      g + (d + dkv) * es, w.ptr, need, layouts=(packed, packed, packed, flat, flat, gpack, gpack, gpack), **kw)
    H.device_sync()
    assert F.same(heads(F.read(o, (B * S, d), qkv.dtype), Hq), ref[0])
    assert F.same(F.read(lse, (B, Hq, S), np.float32), ref[1])
    gq = F.read(g, (B * S, PADW), qkv.dtype)
    assert F.same(heads(gq[:, :d], Hq), ref[2]) and F.same(heads(gq[:, d:d + dkv], Hkv), ref[3]) and F.same(heads(gq[:, d + dkv:W], Hkv), ref[4])
    assert (gq[:, W:].view(np.uint8) == 0xAB).all(), "the bytes between the gradient's rows were written"
    for buf, n in ((ob, B * S * d * es), (lb, 4 * B * Hq * S), (gb, B * S * PADW * es)):
        assert F.guards_ok(buf, n)


# ---- generic path ----
GENERIC_LABELS = {"attn_window_fwd_generic", "attn_window_bwd_dq_generic", "attn_window_bwd_dkv_generic"}


def check_generic(code, q, k, v, go, got, vis):
    """tests/test_gpu_attn_prefix.py's check_generic, for this visibility"""
    f = lambda x: O.to_float(x, code).astype(np.float64)  # noqa: E731
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    dead = np.isneginf(ref["lse"])
    assert np.allclose(f(got[0]), ref["o"], rtol=1e-4, atol=1e-4)
    assert np.isneginf(got[1][dead]).all() and np.allclose(got[1][~dead], ref["lse"][~dead], rtol=1e-4, atol=1e-4)
    for name, g in zip(("dq", "dk", "dv"), got[2:]):
        assert np.allclose(f(g), ref[name], rtol=1e-3, atol=1e-4), name


@pytest.mark.parametrize("window", [(0, 0), (5, 0), (3, 9), (None, 4), (20, None)])
@pytest.mark.parametrize("Sq,Skv", [(33, 70), (96, 17), (300, 290)])
@pytest.mark.parametrize("code,D", [(H.F32, 64), (H.BF16, 80), (H.F16, 40)])
def test_generic(code, D, Sq, Skv, window):
    lens = [Skv, 17, 0, Skv + 3]
    rng = np.random.default_rng(D + Sq + code)
    q, k, v, go = F.inputs(rng, code, 4, 4, 2, Sq, Skv, D)
    got, labels = F.profiled(lambda: run(code, q, k, v, go, lens, window))
    vis = vis_of(q, k, lens, window)
    no_nan(code, got)
    if code == H.F32:
        check_generic(code, q, k, v, go, got, vis)
        zeros_where_nothing_is_seen(got, vis)
    else:
        check16(code, q, k, v, go, got, vis, f"generic D{D}")
    assert GENERIC_LABELS <= labels and not any("mfma" in n for n in labels), sorted(labels)


# ---- determinism, graph capture ----
def test_reproducible_and_capturable():
    rng = np.random.default_rng(513)
    for code, D, Hq, Hkv, Sq, Skv, lens, window in ((H.BF16, 128, 2, 2, 513, 130, None, (70, 0)), (H.F16, 64, 4, 1, 200, 333, [333, 77], (33, 129))):
        q, k, v, go = F.inputs(rng, code, 2, Hq, Hkv, Sq, Skv, D)
        a, b, g = run(code, q, k, v, go, lens, window), run(code, q, k, v, go, lens, window), run(code, q, k, v, go, lens, window, graph=True)
        assert_same(a, b, "two runs differ")
        assert_same(a, g, "the captured run differs from the eager one")


# ---- operator API ----
def torch_ref(q, k, v, go, vis):
    """torch's scaled_dot_product_attention on the CPU in f32 under the boolean mask (K/V repeated over each group). torch has no answer
    for a row without a key: such a row is given key 0 and a zero gradient, so that it adds nothing to dk and dv, and is left out of the
    comparison of o and dq by the caller."""
    import torch
    G = q.shape[1] // k.shape[1]
    live = vis.any(axis=2)
    safe = vis.copy()
    safe[~live, 0] = True
    go = go * live[:, None, :, None]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float32, requires_grad=True) for x in (q, k, v))
    o = torch.nn.functional.scaled_dot_product_attention(tq, tk.repeat_interleave(G, dim=1), tv.repeat_interleave(G, dim=1),
                                                         attn_mask=torch.tensor(safe)[:, None])
    o.backward(torch.tensor(go, dtype=torch.float32))
    return [x.detach().numpy().astype(np.float64) for x in (o, tq.grad, tk.grad, tv.grad)]


def check_operator(code, q, k, v, go, vis, got, what):
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
    live = np.broadcast_to(vis.any(axis=2)[:, None, :], q.shape[:3])
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, torch_ref(f(q), f(k), f(v), f(go), vis)):
        a = f(a)
        if name in ("o", "dq"):     # only the rows that see a key are compared; the others must be zeros
            assert (a[~live] == 0).all(), (what, name)
            a, r = a[live], r[live]
        assert np.abs(a - r).max() <= tol * np.abs(r).max(), (what, name)


def dev_long(x):
    return None if x is None else kfunca.from_numpy(np.asarray(x, np.int64), 0)


# ((0, 0) is not among them: with one key per query dq is zero in exact arithmetic, and a bound relative to max |ref| says nothing)
OP_WINDOWS = [((5, 0), False), ((5, None), True), ((7, 7), False), ((None, 3), False), ((1, 0), True)]


@pytest.mark.parametrize("window,causal", OP_WINDOWS)
@pytest.mark.parametrize("kv_len", [None, [60, 33]])
@pytest.mark.parametrize("code,D", [(H.BF16, 64), (H.BF16, 40), (H.F32, 48)])
def test_operator_attention(code, D, kv_len, window, causal):
    rng = np.random.default_rng(D + code)
    B, Hq, Hkv, Sq, Skv = 2, 4, 2, 90, 70         # queries 75 .. 89 of (5, 0) see no key
    q, k, v, go = F.inputs(rng, code, B, Hq, Hkv, Sq, Skv, D)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)
    out, labels = F.profiled(lambda: kfunca.attention(tq, tk, tv, kv_len=dev_long(kv_len), causal=causal, window=window))
    out.backward(F.value(go, code))
    got = [F.as_np(t, code) for t in (out, tq.grad(), tk.grad(), tv.grad())]
    assert got[0].shape == q.shape and got[1].shape == q.shape and got[2].shape == k.shape and got[3].shape == v.shape
    seen = (window[0], 0) if causal else window    # causal = True closes the right side
    check_operator(code, q, k, v, go, vis_of(q, k, kv_len, seen), got, f"attention D{D} window {window}")
    if code == H.BF16:   # head size 40 is zero-padded to 64: the matrix-core kernels
        assert "attn_window_fwd_mfma_d64" in labels, sorted(labels)
    else:
        assert "attn_window_fwd_generic" in labels, sorted(labels)


@pytest.mark.parametrize("window,causal", OP_WINDOWS)
@pytest.mark.parametrize("kv_len", [None, [129, 50]])
@pytest.mark.parametrize("code,D,kv_heads", [(H.BF16, 64, 2), (H.BF16, 40, 2), (H.F32, 48, 2)])
def test_operator_attention_qkv(code, D, kv_heads, kv_len, window, causal):
    rng = np.random.default_rng(D + code + 1)
    B, S, Hq, Hkv = 2, 129, 4, kv_heads
    W, d, dkv = (Hq + 2 * Hkv) * D, Hq * D, Hkv * D
    qkv, gout = F.rnd(rng, code, (B * S, W)), F.rnd(rng, code, (B * S, d))
    heads = lambda x2, n: np.ascontiguousarray(x2.reshape(B, S, n, D).transpose(0, 2, 1, 3))  # noqa: E731
    q, k, v, go = heads(qkv[:, :d], Hq), heads(qkv[:, d:d + dkv], Hkv), heads(qkv[:, d + dkv:], Hkv), heads(gout, Hq)
    tx = F.leaf(qkv, code)
    out = kfunca.attention_qkv(tx, B, S, Hq, kv_heads=kv_heads, kv_len=dev_long(kv_len), causal=causal, window=window)
    out.backward(F.value(gout, code))
    o2, g2 = F.as_np(out, code), F.as_np(tx.grad(), code)
    assert o2.shape == (B * S, d) and g2.shape == qkv.shape
    got = [heads(o2, Hq), heads(g2[:, :d], Hq), heads(g2[:, d:d + dkv], Hkv), heads(g2[:, d + dkv:], Hkv)]
    seen = (window[0], 0) if causal else window
    check_operator(code, q, k, v, go, vis_of(q, k, kv_len, seen), got, f"attention_qkv D{D} window {window}")


def test_refusals():
    rng = np.random.default_rng(1)
    q, k, v, _ = F.inputs(rng, H.BF16, 2, 2, 2, 8, 8, 64)
    tq, tk, tv = (F.value(x, H.BF16) for x in (q, k, v))
    packed = F.value(F.rnd(rng, H.BF16, (16, 6 * 64)), H.BF16)
    with pytest.raises(Exception, match="attention: causal = true means window right = 0"):
        kfunca.attention(tq, tk, tv, causal=True, window=(4, 3))
    with pytest.raises(Exception, match="attention_qkv: causal = true means window right = 0"):
        kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, causal=True, window=(None, 1))
    with pytest.raises(Exception, match="attention: window and prefix_len"):
        kfunca.attention(tq, tk, tv, causal=True, prefix_len=dev_long([1, 2]), window=(4, 0))
    with pytest.raises(Exception, match="attention_qkv: window and prefix_len"):
        kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, causal=True, prefix_len=dev_long([1, 2]), window=(4, None))
    for bad in ((-1, 0), (3, -2), (-5, -5)):
        with pytest.raises(Exception, match="attention: window .*non-negative"):
            kfunca.attention(tq, tk, tv, window=bad)
        with pytest.raises(Exception, match="attention_qkv: window .*non-negative"):
            kfunca.attention_qkv(packed, 2, 8, 2, kv_heads=2, window=bad)
    with pytest.raises(Exception, match="window is a pair"):
        kfunca.attention(tq, tk, tv, window=(1, 2, 3))
    # causal = True with right = 0 or None is the same call
    a = kfunca.attention(tq, tk, tv, causal=True, window=(4, 0))
    b = kfunca.attention(tq, tk, tv, causal=True, window=(4, None))
    c = kfunca.attention(tq, tk, tv, window=(4, 0))
    assert F.same(F.as_np(a, H.BF16), F.as_np(b, H.BF16)) and F.same(F.as_np(a, H.BF16), F.as_np(c, H.BF16))


@pytest.mark.parametrize("causal,prefix_len", [(False, None), (True, None), (True, [20, 70])])
@pytest.mark.parametrize("kv_len", [None, [90, 33]])
def test_window_none_makes_the_previous_calls(kv_len, causal, prefix_len):
    """without a window the operator launches what it launched before windows existed: the same labels, and the bits of the entry it
    called then, on the same tensors"""
    code, D = H.BF16, 64
    rng = np.random.default_rng(7)
    q, k, v, go = F.inputs(rng, code, 2, 4, 2, 70, 90, D)
    want = P.run(code, q, k, v, go, kv_len, prefix_len, full=not causal)
    tq, tk, tv = F.leaf(q, code), F.leaf(k, code), F.leaf(v, code)

    def call():
        out = kfunca.attention(tq, tk, tv, kv_len=dev_long(kv_len), causal=causal, prefix_len=dev_long(prefix_len), window=None)
        out.backward(F.value(go, code))
        return out

    out, labels = F.profiled(call)
    family = "prefix" if causal else "full"
    mine = {n for n in labels if n.startswith("attn_")}
    assert mine == {f"attn_{family}_fwd_mfma_d64", "attn_full_bwd_delta", f"attn_{family}_bwd_dq_mfma_d64", f"attn_{family}_bwd_dkv_mfma_d64"}, sorted(labels)
    for name, t, w in zip(("o", "dq", "dk", "dv"), (out, tq.grad(), tk.grad(), tv.grad()), (want[0], want[2], want[3], want[4])):
        assert F.same(F.as_np(t, code), w), name
