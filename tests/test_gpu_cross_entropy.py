"""-m gpu: softmax cross-entropy (kf_cross_entropy_* and kfunca.cross_entropy) forward and backward, against an f64 numpy reference on
the same rounded inputs and against torch-CPU F.cross_entropy / autograd.

Tolerances (stated):
  loss per row      |got - ref| <= 1e-4 + 1e-5 |ref| (f32 accumulation over up to 128k classes; the loss is formed as (max - x_t) + log(sum),
                    which stays exact at large logits)
  dlogits           |got - ref| <= r |ref| + 1e-6 |g| / count with r one output rounding: 2^-8 bf16, 2^-11 f16, 2^-16 f32 (f32: the
                    exponential's and the stored f32 lse's own rounding, a few units in 2^-24 times |x - lse|)
  large logits      |lse| ~ 1e4 has an f32 ulp of 2^-10: the f32 gradient there is held to r = 2^-9
  sums / means      the f32 sum of the per-row losses in a fixed order: rtol 1e-5
Reproducibility is bitwise: the reductions have no atomics and the split regime merges its chunks in chunk order.
"""
import zlib

import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

OUT_R = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 2.0 ** -16}
NP = {H.BF16: np.uint16, H.F16: np.float16, H.F32: np.float32}


def ref(x, t, ignore=-100, eps=0.0):
    """f64: (lse[rows], loss[rows], dlogits/g [rows, V]) of the rounded logits x (float array)."""
    x = np.asarray(x, np.float64)
    rows, V = x.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(x - m)
        s = e.sum(1, keepdims=True)
        lse = (m + np.log(s))[:, 0]
        p = e / s
        ok = (t >= 0) & (t < V)
        tc = np.where(ok, t, 0)
        xt = x[np.arange(rows), tc]
        loss = (1 - eps) * (lse - xt) + (eps * (lse - x.mean(1)) if eps > 0 else 0.0)
        d = p - eps / V
        d[np.arange(rows)[ok], tc[ok]] -= 1 - eps
    loss = np.where(t == ignore, 0.0, np.where(ok, loss, np.nan))
    d[t == ignore] = 0.0
    d[(t != ignore) & ~ok] = np.nan
    return lse, loss, d


def run(code, x_store, t, V, ld=None, ignore=-100, eps=0.0, reduction=H.CE_NONE, g=None, backward=True):
    """Through the C ABI. x_store: [rows, ld] in the storage dtype. Returns (loss, lse, count, dlogits [rows, ld] or None)."""
    rows = x_store.shape[0]
    ld = V if ld is None else ld
    bx, bt = H.DevBuf.from_numpy(x_store), H.DevBuf.from_numpy(t.astype(np.int64))
    nloss = rows if reduction == H.CE_NONE else 1
    bl, blse, bc = H.DevBuf(4 * max(nloss, 1)), H.DevBuf(4 * max(rows, 1)), H.DevBuf(4)
    ws = H.ce_fwd(code, rows, V, bx.ptr, bt.ptr, bl.ptr, blse.ptr, bc.ptr, ignore, eps, reduction, ld=ld)
    H.device_sync()
    del ws
    loss, lse, count = bl.to_numpy((nloss,), np.float32), blse.to_numpy((rows,), np.float32), bc.to_numpy((1,), np.float32)[0]
    dx = None
    if backward:
        g = np.ones(nloss, np.float32) if g is None else np.asarray(g, np.float32).reshape(nloss)
        bg, bd = H.DevBuf.from_numpy(g), H.DevBuf(x_store.nbytes)
        bd.zero()
        H.ce_bwd(code, rows, V, bx.ptr, bt.ptr, blse.ptr, bc.ptr, bg.ptr, bd.ptr, ignore, eps, reduction, ld=ld)
        H.device_sync()
        dx = bd.to_numpy(x_store.shape, NP[code])
    return loss, lse, count, dx


def make(rng, code, rows, V, ld=None, scale=3.0):
    ld = V if ld is None else ld
    x32 = rng.uniform(-scale, scale, (rows, ld)).astype(np.float32)
    xs = O.from_float(x32, code)
    return xs, O.to_float(xs, code).astype(np.float64)[:, :V]


def check_dx(code, got, want, g_eff, what):
    got = O.to_float(got, code).astype(np.float64)
    r = OUT_R[code]
    assert_close(got, want * g_eff, rtol=r, atol=1e-6 * np.abs(g_eff).max() + 1e-30, what=what)


# (rows, V, ld): every regime - one wave per row (V <= 4096), one block per row (rows >= 1024), split rows (few long rows) - and odd strides
SHAPES = [(37, 1, None), (64, 7, None), (300, 1000, None), (5, 4096, None), (32768, 1000, None), (40, 1000, 1003),
          (1024, 32000, None), (3, 32000, None), (1100, 50257, None), (1, 50257, None), (16, 128256, None), (1024, 4097, None),
          (1000, 8192, None), (1200, 5000, 5001), (7, 20000, 20003), (2, 128256, 128263)]


@pytest.mark.parametrize("code", [H.F32, H.BF16, H.F16])
@pytest.mark.parametrize("rows,V,ld", SHAPES)
def test_dtypes_shapes_regimes(code, rows, V, ld):
    rng = np.random.default_rng(rows * 7 + V + code)
    xs, x = make(rng, code, rows, V, ld)
    t = rng.integers(0, V, rows)
    t[rng.random(rows) < 0.1] = -100
    g = rng.uniform(0.5, 2.0, rows).astype(np.float32)
    loss, lse, count, dx = run(code, xs, t, V, ld=ld, g=g)
    # seeded sampled rows at multi-hundred-MB shapes, the whole tensor otherwise
    pick = np.arange(rows) if rows * V <= 1 << 22 else np.unique(np.r_[0, rows - 1, rng.choice(rows, 48, replace=False)])
    rlse, rloss, rd = ref(x[pick], t[pick])
    keep = t[pick] != -100
    assert_close(loss[pick], rloss, rtol=1e-5, atol=1e-4, what="loss")
    assert_close(lse[pick][keep], rlse[keep], rtol=1e-5, atol=1e-4, what="lse")
    check_dx(code, dx[pick][:, :V], rd, g[pick][:, None].astype(np.float64), "dlogits")
    if ld is not None and ld > V:
        assert not dx[:, V:].any(), "the backward wrote beyond V"
    if rows * V <= 1 << 22:
        for red in (H.CE_SUM, H.CE_MEAN):
            l2, _, c2, _ = run(code, xs, t, V, ld=ld, reduction=red, backward=False)
            n = (t != -100).sum()
            assert c2 == n
            want = rloss.sum() / (n if red == H.CE_MEAN else 1)
            assert_close(l2, [want], rtol=1e-5, atol=1e-4, what=f"reduction {red}")


def torch_ce(x, t, **kw):
    import torch
    import torch.nn.functional as F
    tx = torch.tensor(x, dtype=torch.float32, requires_grad=True)
    loss = F.cross_entropy(tx, torch.tensor(t, dtype=torch.int64), **kw)
    return tx, loss


def kf_ce(x, t, g, **kw):
    tx = kfunca.from_numpy(np.ascontiguousarray(x, np.float32), 0)
    tx.set_requires_grad(True)
    loss = kfunca.cross_entropy(tx, kfunca.from_numpy(np.ascontiguousarray(t, np.int64), 0), **kw)
    loss.backward(kfunca.from_numpy(np.ascontiguousarray(g, np.float32).reshape(loss.sizes()), 0))
    return loss.numpy(), tx.grad().numpy()


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("case", ["plain", "ignore", "smooth", "neg_inf", "large", "ignore_smooth_3d"])
def test_semantics_vs_torch(reduction, case):
    import torch
    rng = np.random.default_rng(zlib.crc32(f"{reduction} {case}".encode()))
    shape, V = ((4, 9), 1000) if case == "ignore_smooth_3d" else ((50,), 1000)
    x = rng.uniform(-4, 4, shape + (V,)).astype(np.float32)
    t = rng.integers(0, V, shape)
    kw = dict(reduction=reduction)
    rtol = OUT_R[H.F32]
    if case in ("ignore", "ignore_smooth_3d"):
        t[rng.random(shape) < 0.3] = 7 if case == "ignore" else -100
        kw["ignore_index"] = 7 if case == "ignore" else -100
    if case in ("smooth", "ignore_smooth_3d"):
        kw["label_smoothing"] = 0.1
    if case == "neg_inf":
        x[..., V - 24:] = -np.inf  # a padded vocabulary; no target points there
        t = np.minimum(t, V - 25)
    if case == "large":
        x = (1e4 + rng.uniform(-3, 3, shape + (V,))).astype(np.float32)
        x[::2] -= 2e4
        rtol = 2.0 ** -9
    tx, tl = torch_ce(x.reshape(-1, V), t.reshape(-1), **kw)
    g = rng.uniform(0.5, 2, tl.shape).astype(np.float32)
    tl.backward(torch.tensor(g))
    loss, dx = kf_ce(x, t, g, **kw)
    want = tl.detach().numpy().reshape(loss.shape if reduction == "none" else (1,))
    assert loss.shape == (t.shape if reduction == "none" else (1,))
    assert np.isfinite(loss).all()
    assert_close(loss, want, rtol=1e-5, atol=1e-4, what=f"{case} {reduction} loss")
    tg = tx.grad.numpy().reshape(x.shape)
    count = max(1, int((t != kw.get("ignore_index", -100)).sum())) if reduction == "mean" else 1
    assert_close(dx, tg, rtol=rtol, atol=1e-6 * np.abs(g).max() / count + 1e-7, what=f"{case} {reduction} dlogits")
    if case == "neg_inf":
        assert not dx[..., V - 24:].any()


def test_all_rows_ignored():
    x = np.random.default_rng(1).uniform(-2, 2, (6, 33)).astype(np.float32)
    t = np.full(6, -100)
    for reduction in ("mean", "sum", "none"):
        g = np.ones(6 if reduction == "none" else 1, np.float32)
        loss, dx = kf_ce(x, t, g, reduction=reduction)
        if reduction == "mean":
            assert np.isnan(loss).all()
        else:
            assert (loss == 0).all()
        assert (dx == 0).all()


def test_out_of_range_target_is_a_nan_row_only():
    rng = np.random.default_rng(2)
    for rows, V in ((20, 100), (8, 50000), (1100, 5000)):  # the three regimes
        x = rng.uniform(-2, 2, (rows, V)).astype(np.float32)
        t = rng.integers(0, V, rows)
        t[3], t[5] = V + 5, -7
        loss, dx = kf_ce(x, t, np.ones(rows, np.float32), reduction="none")
        bad = np.zeros(rows, bool)
        bad[[3, 5]] = True
        assert np.isnan(loss[bad]).all() and np.isnan(dx[bad]).all()
        _, rloss, rd = ref(x[~bad], t[~bad])
        assert_close(loss[~bad], rloss, rtol=1e-5, atol=1e-4, what="other rows' loss")
        assert_close(dx[~bad], rd, rtol=2.0 ** -16, atol=1e-6, what="other rows' dlogits")
        m, _ = kf_ce(x, t, np.ones(1, np.float32), reduction="mean")
        assert np.isnan(m).all()


@pytest.mark.parametrize("rows,V", [(4096, 1000), (2048, 32000), (16, 128256), (3, 50257)])
def test_bitwise_reproducible(rows, V):
    rng = np.random.default_rng(rows + V)
    xs, _ = make(rng, H.BF16, rows, V)
    t = rng.integers(0, V, rows)
    t[::9] = -100
    outs = [run(H.BF16, xs, t, V, eps=0.1, reduction=H.CE_MEAN) for _ in range(2)]
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(np.atleast_1d(a).view(np.uint8), np.atleast_1d(b).view(np.uint8))


@pytest.mark.parametrize("rows,V,reduction", [(16, 128256, H.CE_MEAN), (300, 1000, H.CE_NONE), (1024, 8192, H.CE_SUM)])
def test_graph_capture_replays_bit_identical(rows, V, reduction):
    rng = np.random.default_rng(77 + rows)
    xs, _ = make(rng, H.BF16, rows, V)
    t = rng.integers(0, V, rows)
    t[::5] = -100
    nloss = rows if reduction == H.CE_NONE else 1
    g = rng.uniform(0.5, 2, nloss).astype(np.float32)
    bx, bt, bg = H.DevBuf.from_numpy(xs), H.DevBuf.from_numpy(t), H.DevBuf.from_numpy(g)
    bl, blse, bc, bd = H.DevBuf(4 * nloss), H.DevBuf(4 * rows), H.DevBuf(4), H.DevBuf(xs.nbytes)
    need = H.ce_workspace_bytes(H.BF16, rows, V, reduction)
    ws = H.DevBuf(max(need, 1))
    st = H.Stream()

    def step():
        H.check(H.lib().kf_cross_entropy_fwd(H.BF16, rows, V, V, bx.ptr, bt.ptr, -100, 0.05, reduction, bl.ptr, blse.ptr, bc.ptr, ws.ptr, need,
                                             st.handle))
        H.check(H.lib().kf_cross_entropy_bwd(H.BF16, rows, V, V, bx.ptr, bt.ptr, -100, 0.05, reduction, blse.ptr, bc.ptr, bg.ptr, bd.ptr, V,
                                             st.handle))

    def read():
        return bl.to_numpy((nloss,), np.float32).copy(), bd.to_numpy(xs.shape, np.uint16).copy()

    step()
    st.sync()
    want_l, want_d = read()
    bl.zero(st.handle)
    bd.zero(st.handle)
    st.sync()
    with H.Graph.capture(st) as graph:
        step()
    graph.launch()
    st.sync()
    got_l, got_d = read()
    assert np.array_equal(got_l.view(np.uint32), want_l.view(np.uint32)) and np.array_equal(got_d, want_d)


def test_tiny_lm_step_end_to_end():
    """embedding -> rms_norm -> gemm LM head -> cross_entropy(mean, some tokens ignored) -> backward: the embedding table's and the head
    weight's gradients against torch-CPU autograd in f32."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    vocab, d, n = 257, 64, 96
    table = rng.uniform(-1, 1, (vocab, d)).astype(np.float32)
    w_norm = rng.uniform(0.5, 1.5, d).astype(np.float32)
    head = rng.uniform(-0.3, 0.3, (d, vocab)).astype(np.float32)
    tokens = rng.integers(0, vocab, n)
    target = np.r_[tokens[1:], -100]
    target[rng.random(n) < 0.2] = -100

    tt, tw, th = (kfunca.from_numpy(a, 0) for a in (table, w_norm, head))
    for p in (tt, tw, th):
        p.set_requires_grad(True)
    h = kfunca.rms_norm(kfunca.embedding(tt, kfunca.from_numpy(tokens, 0)), tw, 1e-5)
    loss = kfunca.cross_entropy(kfunca.gemm(h, th, 1.0, 0.0), kfunca.from_numpy(target, 0))
    loss.backward(kfunca.from_numpy(np.ones(1, np.float32), 0))

    rt, rw, rh = (torch.tensor(a, requires_grad=True) for a in (table, w_norm, head))
    e = rt[torch.tensor(tokens)]
    hh = e * torch.rsqrt((e * e).mean(-1, keepdim=True) + 1e-5) * rw
    rl = F.cross_entropy(hh @ rh, torch.tensor(target))
    rl.backward()
    assert_close(loss.numpy(), [rl.item()], rtol=1e-5, atol=1e-5, what="loss")
    assert_close(tt.grad().numpy(), rt.grad.numpy(), rtol=1e-3, atol=1e-6, what="d table")
    assert_close(th.grad().numpy(), rh.grad.numpy(), rtol=1e-3, atol=1e-6, what="d head")
    assert_close(tw.grad().numpy(), rw.grad.numpy(), rtol=1e-3, atol=1e-6, what="d norm weight")


def test_bf16_and_f16_through_the_operator_api():
    rng = np.random.default_rng(9)
    x = O.bf16_to_f32(O.f32_to_bf16(rng.uniform(-3, 3, (2, 3, 5000)).astype(np.float32)))
    t = rng.integers(0, 5000, (2, 3))
    for conv in ("bfloat16", "half"):
        tx = getattr(kfunca.from_numpy(x, 0), conv)()
        tx.set_requires_grad(True)
        loss = kfunca.cross_entropy(tx, kfunca.from_numpy(t, 0), reduction="sum")
        assert loss.sizes() == [1] and loss.dtype() == kfunca.from_numpy(np.zeros(1, np.float32), 0).dtype()
        loss.backward(kfunca.from_numpy(np.ones(1, np.float32), 0))
        xr = getattr(kfunca.from_numpy(x, 0), conv)().float().numpy().reshape(6, 5000)
        _, rloss, rd = ref(xr, t.reshape(-1))
        assert_close(loss.numpy(), [rloss.sum()], rtol=1e-5, atol=1e-4, what=conv)
        assert_close(tx.grad().float().numpy().reshape(6, 5000), rd, rtol=2.0 ** -8, atol=1e-6, what=conv)


@pytest.mark.slow
def test_bf16_beyond_2_31_elements():
    """bf16 [16800, 128256] (2.15e9 elements, 4.3 GB): rows on both sides of element 2^31 checked. The logits are a 97-row random tile
    repeated down the rows (row r holds tile row r % 97), so the host builds 25 MB instead of 4.3 GB."""
    rows, V, R = 16800, 128256, 97
    assert rows * V > 1 << 31
    rng = np.random.default_rng(31)
    tile, tile64 = make(rng, H.BF16, R, V)
    t = rng.integers(0, V, rows)
    bx, bt = H.DevBuf(rows * V * 2), H.DevBuf.from_numpy(t)
    for r0 in range(0, rows, R):
        n = min(R, rows - r0)
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r0 * V * 2, tile.ctypes.data, n * V * 2, None))
    bl, blse, bc, bg, bd = H.DevBuf(4 * rows), H.DevBuf(4 * rows), H.DevBuf(4), H.DevBuf.from_numpy(np.ones(rows, np.float32)), H.DevBuf(rows * V * 2)
    ws = H.ce_fwd(H.BF16, rows, V, bx.ptr, bt.ptr, bl.ptr, blse.ptr, bc.ptr, reduction=H.CE_NONE)
    H.ce_bwd(H.BF16, rows, V, bx.ptr, bt.ptr, blse.ptr, bc.ptr, bg.ptr, bd.ptr, reduction=H.CE_NONE)
    H.device_sync()
    del ws
    loss = bl.to_numpy((rows,), np.float32)
    edge = (1 << 31) // V
    for r in (0, edge - 1, edge, edge + 1, rows - 1):
        _, rloss, rd = ref(tile64[r % R][None], t[r:r + 1])
        assert_close(loss[r:r + 1], rloss, rtol=1e-5, atol=1e-4, what=f"loss row {r}")
        row = np.empty(V, np.uint16)
        H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, bd.ptr + r * V * 2, V * 2, None))
        assert_close(O.bf16_to_f32(row)[None].astype(np.float64), rd, rtol=2.0 ** -8, atol=1e-6, what=f"dlogits row {r}")
