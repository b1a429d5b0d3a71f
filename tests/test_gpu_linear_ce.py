"""-m gpu: kfunca.linear_cross_entropy - the LM head and its loss in chunks of tokens, never holding the [T, V] logits - against the
f64 reference of tests/linear_ce_ref.py on the STORED (rounded) operands, and against torch-CPU autograd for a tied head.

Bounds:
  loss      |got - ref| <= 1e-4 + 1e-5 |ref|
  dX, dW    |err[i, j]| <= r (sum |dlogits| |operand| + |want[i, j]|) + 1e-7, the sum over the contraction in the f64 reference and r one
            rounding of the operands' dtype (2^-8 bf16, 2^-11 f16, 2^-16 f32): the gradient of the logits is rounded once to that dtype
            before the two products (half an ulp: r / 2 of the sum), and a 16-bit dX is rounded when it is stored and again when the
            upstream gradient and the mean's divisor are applied (r |want|); dW leaves f32 accumulators and is rounded once. 1e-7 is half
            an f16 subnormal step, which a mean's divisor can push a small dX into.
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from tests import linear_ce_ref as R
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

OUT_R = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -16}
MiB = 1 << 20

# (T, V, d, chunk_rows, x's shape): tile kernels with two chunks; everything ragged with a tail of 44 rows; a whole-tile part plus a
# ragged remainder in the last chunk; T below one chunk (the default chunk_rows); a 3-D x
SHAPES = [(256, 512, 64, 128, None), (300, 1000, 48, 128, None), (520, 512, 128, 256, None), (100, 384, 64, 0, None),
          (260, 384, 64, 128, (2, 130, 64))]
SHAPE_IDS = ["tiles-2chunks", "ragged-tail44", "whole+remainder", "below-a-chunk", "3d"]
# (name, ignored rows, label smoothing, z-loss)
VARIANTS = [("plain", False, 0.0, 0.0), ("ignore", True, 0.0, 0.0), ("smooth", False, 0.1, 0.0), ("zloss", False, 0.0, 1e-3),
            ("all", True, 0.1, 1e-3)]


def to_t(a, dtype, grad=False):
    t = kfunca.from_numpy(np.ascontiguousarray(a, np.float32), 0)
    t = t if dtype == "f32" else t.bfloat16() if dtype == "bf16" else t.half()
    if grad:
        t.set_requires_grad(True)
    return t


def stored(t):
    return t.float().numpy().astype(np.float64)


def ones():
    return kfunca.from_numpy(np.ones(1, np.float32), 0)


def draw(T, V, d, seed, ignored):
    rng = np.random.default_rng(seed)
    x, W = rng.uniform(-1, 1, (T, d)).astype(np.float32), rng.uniform(-0.5, 0.5, (V, d)).astype(np.float32)
    t = rng.integers(0, V, T)
    if ignored:
        t[rng.random(T) < 0.2] = -100
        t[T // 3] = -100
    return x, W, t


def check_grad(got, want, abs_sum, r, what):
    got = np.asarray(got, np.float64).reshape(want.shape)
    bound = r * (abs_sum + np.abs(want)) + 1e-7
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / bound, 0)), want.shape)
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} outside the bound; worst at {i}: got {got[i]} want {want[i]} bound {bound[i]}")


def run(x, W, t, dtype, shape=None, g=None, grad_x=True, grad_w=True, **kw):
    """One forward + backward. Returns (loss, dX or None, dW or None, stored x [T, d], stored W) - the gradients as f64."""
    tx, tw = to_t(x.reshape(shape) if shape else x, dtype, grad_x), to_t(W, dtype, grad_w)
    tt = kfunca.from_numpy(np.ascontiguousarray(t.reshape(shape[:-1]) if shape else t, np.int64), 0)
    loss = kfunca.linear_cross_entropy(tx, tw, tt, **kw)
    assert loss.sizes() == [1]
    if grad_x or grad_w:
        out = loss if g is None else loss * float(g)
        out.backward(ones())
    dx = stored(tx.grad()).reshape(x.shape) if grad_x else None
    dw = stored(tw.grad()) if grad_w else None
    return float(loss.numpy()[0]), dx, dw, stored(tx).reshape(x.shape), stored(tw)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("T,V,d,chunk,shape", SHAPES, ids=SHAPE_IDS)
def test_loss_and_gradients(T, V, d, chunk, shape, dtype, reduction):
    for name, ignored, eps, z in VARIANTS:
        x, W, t = draw(T, V, d, T + V + d, ignored)
        loss, dx, dw, xs, ws = run(x, W, t, dtype, shape, reduction=reduction, label_smoothing=eps, z_loss=z, chunk_rows=chunk)
        want = R.linear_ce(xs, ws, t, reduction=reduction, eps=eps, z=z)
        what = f"{name} {reduction} {dtype} ({T}, {V}, {d}, {chunk})"
        assert_close([loss], [want["loss"]], rtol=1e-5, atol=1e-4, what=f"{what}: loss")
        check_grad(dx, want["dX"], want["abs_dX"], OUT_R[dtype], f"{what}: dX")
        check_grad(dw, want["dW"], want["abs_dW"], OUT_R[dtype], f"{what}: dW")
        assert np.abs(want["dX"]).max() > 0 and np.abs(want["dW"]).max() > 0


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_chunks_in_the_split_row_regime(dtype):
    """V > 4096 with chunks of fewer than 1024 rows: kf_ce_fused_rows splits the rows through scratch the operator sizes for its largest
    chunk (128 rows, then a tail of 72), three launches per chunk, f32 in place across the launch boundaries."""
    T, V, d, chunk = 200, 4160, 64, 128
    x, W, t = draw(T, V, d, 41, True)
    loss, dx, dw, xs, ws = run(x, W, t, dtype, reduction="mean", label_smoothing=0.1, z_loss=1e-3, chunk_rows=chunk)
    want = R.linear_ce(xs, ws, t, reduction="mean", eps=0.1, z=1e-3)
    assert_close([loss], [want["loss"]], rtol=1e-5, atol=1e-4, what="loss")
    check_grad(dx, want["dX"], want["abs_dX"], OUT_R[dtype], f"{dtype} dX")
    check_grad(dw, want["dW"], want["abs_dW"], OUT_R[dtype], f"{dtype} dW")


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_gradient_for_one_input_or_neither(dtype):
    T, V, d, chunk = 300, 1000, 48, 128
    x, W, t = draw(T, V, d, 11, True)
    kw = dict(reduction="mean", label_smoothing=0.1, z_loss=1e-3, chunk_rows=chunk)
    loss, dx, dw, xs, ws = run(x, W, t, dtype, **kw)
    want = R.linear_ce(xs, ws, t, reduction="mean", eps=0.1, z=1e-3)
    lx, dx1, none_w, _, _ = run(x, W, t, dtype, grad_w=False, **kw)
    lw, none_x, dw1, _, _ = run(x, W, t, dtype, grad_x=False, **kw)
    assert none_w is None and none_x is None
    # the same products in the same order: the same bits, whichever gradients were asked for
    assert lx == loss and lw == loss and np.array_equal(dx1, dx) and np.array_equal(dw1, dw)
    check_grad(dx1, want["dX"], want["abs_dX"], OUT_R[dtype], "dX alone")
    check_grad(dw1, want["dW"], want["abs_dW"], OUT_R[dtype], "dW alone")
    # neither: the loss alone, and the pool grows by no more than one chunk's buffers (f32 logits; no gradient buffer, no dX, no dWacc)
    tx, tw, tt = to_t(x, dtype), to_t(W, dtype), kfunca.from_numpy(t.astype(np.int64), 0)
    kfunca.synchronize(0)
    kfunca.release_cached(0)
    before = kfunca.memstat_dict(0)
    l0 = kfunca.linear_cross_entropy(tx, tw, tt, **kw)
    kfunca.synchronize(0)
    after = kfunca.memstat_dict(0)
    assert float(l0.numpy()[0]) == loss and not l0.requires_grad()
    grown = after["active_bytes"] + after["cached_bytes"] - before["active_bytes"] - before["cached_bytes"]
    assert grown <= chunk * V * 4 + T * 4 + 4096, grown   # the chunk's logits, the row losses, the loss and allocation rounding


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_upstream_gradient(dtype):
    T, V, d, chunk = 256, 512, 64, 128
    x, W, t = draw(T, V, d, 3, True)
    for reduction in ("mean", "sum"):
        loss, dx, dw, xs, ws = run(x, W, t, dtype, g=3.0, reduction=reduction, chunk_rows=chunk)
        want = R.linear_ce(xs, ws, t, reduction=reduction, g=3.0)
        assert_close([loss], [want["loss"]], rtol=1e-5, atol=1e-4, what="loss")
        check_grad(dx, want["dX"], want["abs_dX"], OUT_R[dtype], f"dX, 3 x {reduction}")
        check_grad(dw, want["dW"], want["abs_dW"], OUT_R[dtype], f"dW, 3 x {reduction}")


def test_tied_weights_against_torch():
    """embedding(W, ids) -> rms_norm -> linear_cross_entropy(h, W): the table receives the head's gradient and the embedding's through the
    engine's accumulation. Against torch-CPU autograd in f32, at the tolerances of test_tiny_lm_step_end_to_end."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    vocab, d, n = 257, 64, 200
    table = rng.uniform(-1, 1, (vocab, d)).astype(np.float32)
    w_norm = rng.uniform(0.5, 1.5, d).astype(np.float32)
    tokens = rng.integers(0, vocab, n)
    target = np.r_[tokens[1:], -100]
    target[rng.random(n) < 0.2] = -100

    tt, tw = kfunca.from_numpy(table, 0), kfunca.from_numpy(w_norm, 0)
    tt.set_requires_grad(True)
    tw.set_requires_grad(True)
    h = kfunca.rms_norm(kfunca.embedding(tt, kfunca.from_numpy(tokens, 0)), tw, 1e-5)
    loss = kfunca.linear_cross_entropy(h, tt, kfunca.from_numpy(target, 0), chunk_rows=128)
    loss.backward(ones())

    rt, rw = torch.tensor(table, requires_grad=True), torch.tensor(w_norm, requires_grad=True)
    e = rt[torch.tensor(tokens)]
    hh = e * torch.rsqrt((e * e).mean(-1, keepdim=True) + 1e-5) * rw
    rl = F.cross_entropy(F.linear(hh, rt), torch.tensor(target))
    rl.backward()
    assert_close(loss.numpy(), [rl.item()], rtol=1e-5, atol=1e-5, what="loss")
    assert_close(tt.grad().numpy(), rt.grad.numpy(), rtol=1e-3, atol=1e-6, what="d table (head + embedding)")
    assert_close(tw.grad().numpy(), rw.grad.numpy(), rtol=1e-3, atol=1e-6, what="d norm weight")


def pool_bytes():
    s = kfunca.memstat_dict(0)
    return s["active_bytes"] + s["cached_bytes"]


def test_memory_stays_below_half_of_one_logits_tensor():
    T, V, d, chunk = 4096, 4096, 64, 256
    x, W, t = draw(T, V, d, 17, True)
    tx, tw, tt = to_t(x, "bf16", True), to_t(W, "bf16", True), kfunca.from_numpy(t.astype(np.int64), 0)
    twt = to_t(np.ascontiguousarray(W.T), "bf16", True)    # [d, V] for the composition's gemm
    kfunca.synchronize(0)
    kfunca.release_cached(0)
    before = pool_bytes()
    loss = kfunca.linear_cross_entropy(tx, tw, tt, chunk_rows=chunk)
    kfunca.synchronize(0)
    kfunca.release_cached(0)
    fused = pool_bytes() - before
    print(f"linear_cross_entropy forward (gradients formed): pool growth {fused / MiB:.2f} MiB")
    assert fused < 16 * MiB, fused     # half of ONE [T, V] bf16 tensor
    value = float(loss.numpy()[0])
    del loss
    kfunca.synchronize(0)
    kfunca.release_cached(0)
    before = pool_bytes()
    comp = kfunca.cross_entropy(kfunca.gemm(tx, twt, 1.0, 0.0), tt)
    kfunca.synchronize(0)
    kfunca.release_cached(0)
    composed = pool_bytes() - before
    print(f"gemm -> cross_entropy forward: pool growth {composed / MiB:.2f} MiB")
    assert composed > 32 * MiB, composed   # the measurement does see a [T, V] tensor where one is held
    # the two losses differ only by the rounding of the composition's bf16 logits
    assert abs(value - float(comp.numpy()[0])) <= 2.0 ** -8 * 4.0


def test_chunking_is_reproducible_and_does_not_change_the_result():
    T, V, d = 520, 512, 128
    x, W, t = draw(T, V, d, 23, True)
    for dtype in ("bf16", "f32"):
        kw = dict(reduction="mean", label_smoothing=0.1, z_loss=1e-3)
        a = run(x, W, t, dtype, chunk_rows=128, **kw)
        b = run(x, W, t, dtype, chunk_rows=128, **kw)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), f"{dtype}: the same chunk_rows twice differs"
        c = run(x, W, t, dtype, chunk_rows=384, **kw)
        want = R.linear_ce(a[3], a[4], t, reduction="mean", eps=0.1, z=1e-3)
        assert_close([c[0]], [a[0]], rtol=1e-5, atol=1e-4, what="loss, 128 vs 384")
        for k, name, s in ((1, "dX", "abs_dX"), (2, "dW", "abs_dW")):
            check_grad(c[k], want[name], want[s], OUT_R[dtype], f"{dtype} {name}, chunk_rows 384")
            check_grad(c[k], a[k], want[s], OUT_R[dtype], f"{dtype} {name}, chunk_rows 128 vs 384")


def test_graph_capture_replays_to_the_eager_bits():
    T, V, d, chunk = 256, 512, 64, 128
    x, W, t = draw(T, V, d, 29, True)
    kw = dict(reduction="mean", label_smoothing=0.1, z_loss=1e-3, chunk_rows=chunk)
    eager = None
    for _ in range(2):   # warms the allocator
        eager = run(x, W, t, "bf16", **kw)
    tx, tw, tt, g = to_t(x, "bf16", True), to_t(W, "bf16", True), kfunca.from_numpy(t.astype(np.int64), 0), ones()
    kfunca.synchronize(0)
    kfunca.graph_begin(0)
    loss = kfunca.linear_cross_entropy(tx, tw, tt, **kw)   # recorded, not run
    loss.backward(g)
    graph = kfunca.graph_end(0)
    try:
        for _ in range(2):
            kfunca.graph_launch(graph, 0)
            kfunca.synchronize(0)
            assert float(loss.numpy()[0]) == eager[0]
            assert np.array_equal(stored(tx.grad()), eager[1]) and np.array_equal(stored(tw.grad()), eager[2])
    finally:
        kfunca.graph_destroy(graph)


def test_refusals():
    x, W, t = draw(64, 128, 32, 1, False)
    tx, tw, tt = to_t(x, "f32"), to_t(W, "f32"), kfunca.from_numpy(t.astype(np.int64), 0)
    with pytest.raises(Exception, match="'none' is not supported"):
        kfunca.linear_cross_entropy(tx, tw, tt, reduction="none")
    with pytest.raises(Exception, match="not a valid value"):
        kfunca.linear_cross_entropy(tx, tw, tt, reduction="avg")
    with pytest.raises(Exception, match="share a dtype"):
        kfunca.linear_cross_entropy(tx, to_t(W, "bf16"), tt)
    with pytest.raises(Exception, match=r"weight must be \[V, d\]"):
        kfunca.linear_cross_entropy(tx, to_t(W[:, :16], "f32"), tt)
    with pytest.raises(Exception, match="shape of x without its last dim"):
        kfunca.linear_cross_entropy(tx, tw, kfunca.from_numpy(t[:63].astype(np.int64), 0))
    with pytest.raises(Exception, match="type Long"):
        kfunca.linear_cross_entropy(tx, tw, kfunca.from_numpy(t.astype(np.int32), 0))
    with pytest.raises(Exception, match="multiple of 128"):
        kfunca.linear_cross_entropy(tx, tw, tt, chunk_rows=100)
    with pytest.raises(Exception, match="label_smoothing"):
        kfunca.linear_cross_entropy(tx, tw, tt, label_smoothing=1.5)
    with pytest.raises(Exception, match="z_loss"):
        kfunca.linear_cross_entropy(tx, tw, tt, z_loss=-1.0)
