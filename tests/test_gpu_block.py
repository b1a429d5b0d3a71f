"""-m gpu: BASELINE config C5 as a parity case - one causal-attention transformer block, forward + backward, built ONLY from
operators the reference API has (gemm, view / permute / contiguous / split, causal_attention, add, mul: SURVEY.md §8d) and run
through Tensor.backward. The reference's autograd stops at add, so the expected values come from torch-CPU autograd on the
same expression in f32 (a floating-point path: tolerances stated below). The batch-sharded form is checked by summing the
weight gradients of two half-batches (what the RCCL all-reduce does across ranks)."""
import numpy as np
import pytest
import torch

import kfunca_amd as kfunca
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def block(x, w, B, S, H, D, api):
    """x [B*S, d]; w = (Wqkv [d, 3d], Wo [d, d], Wg [d, f], Wu [d, f], Wd [f, d])."""
    d = H * D
    qkv = api.gemm(x, w[0])                                  # [T, 3d]
    q, k, v = api.split(qkv, [d, d, d], 1)
    heads = [api.contiguous(api.permute(api.view(t_, [B, S, H, D]), [0, 2, 1, 3])) for t_ in (api.contiguous(q), api.contiguous(k), api.contiguous(v))]
    a = api.attention(*heads)                                # [B, H, S, D]
    a = api.view(api.contiguous(api.permute(a, [0, 2, 1, 3])), [B * S, d])
    h = api.add(x, api.gemm(a, w[1]))                        # residual
    gate, up = api.gemm(h, w[2]), api.gemm(h, w[3])
    return api.add(h, api.gemm(api.mul(gate, up), w[4]))     # gating is a plain product: the reference has no activation op


def block2(x, w, B, S, H, D, api):
    """The same block as a real pre-norm block, on the fused operators: rms_norm before each half,
    attention straight on the packed QKV projection, residual adds and the gating product fused into the GEMMs' stores.
    w = (Wqkv, Wo, Wg, Wu, Wd, g1 [d], g2 [d])."""
    n1 = api.rms_norm(x, w[5])
    a = api.attention_qkv(api.gemm(n1, w[0]), B, S, H)       # [T, d], no split / permute / contiguous
    h = api.gemm_fused(a, w[1], add=x)                       # x + a Wo
    n2 = api.rms_norm(h, w[6])
    up = api.gemm(n2, w[3])
    gu = api.gemm_fused(n2, w[2], mul=up)                    # (n2 Wg) o (n2 Wu)
    return api.gemm_fused(gu, w[4], add=h)                   # h + gu Wd


class KfApi:
    rms_norm = staticmethod(lambda x, g: kfunca.rms_norm(x, g, 1e-5))
    attention_qkv = staticmethod(kfunca.causal_attention_qkv)
    gemm_fused = staticmethod(lambda a, b, mul=None, add=None: kfunca.gemm_fused(a, b, 1.0, None, mul, add))
    gemm = staticmethod(lambda a, b: kfunca.gemm(a, b, 1.0, 0.0))
    split = staticmethod(lambda t, sizes, dim: t.split(sizes, dim))
    view = staticmethod(lambda t, s: t.view(*s))
    permute = staticmethod(lambda t, p: t.permute(*p))
    contiguous = staticmethod(lambda t: t.contiguous())
    attention = staticmethod(kfunca.causal_attention)
    add = staticmethod(lambda a, b: a + b)
    mul = staticmethod(lambda a, b: a * b)


def _torch_attention_qkv(qkv, B, S, H):
    d = qkv.shape[1] // 3
    q, k, v = (t.reshape(B, S, H, d // H).permute(0, 2, 1, 3) for t in torch.split(qkv, [d, d, d], 1))
    a = torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    return a.permute(0, 2, 1, 3).reshape(B * S, d)


class TorchApi:
    rms_norm = staticmethod(lambda x, g: torch.nn.functional.rms_norm(x, (x.shape[-1],), g, eps=1e-5))
    attention_qkv = staticmethod(_torch_attention_qkv)
    gemm_fused = staticmethod(lambda a, b, mul=None, add=None: ((a @ b) * (mul if mul is not None else 1.0)) + (add if add is not None else 0.0))
    gemm = staticmethod(lambda a, b: a @ b)
    split = staticmethod(lambda t, sizes, dim: torch.split(t, sizes, dim))
    view = staticmethod(lambda t, s: t.reshape(s))
    permute = staticmethod(lambda t, p: t.permute(*p))
    contiguous = staticmethod(lambda t: t.contiguous())
    attention = staticmethod(lambda q, k, v: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True))
    add = staticmethod(lambda a, b: a + b)
    mul = staticmethod(lambda a, b: a * b)


def make(rng, B, S, H, D, f):
    d = H * D
    x = rng.uniform(-1, 1, (B * S, d)).astype(np.float32)
    w = [(rng.uniform(-1, 1, shp) / np.sqrt(shp[0])).astype(np.float32) for shp in ((d, 3 * d), (d, d), (d, f), (d, f), (f, d))]
    g = rng.uniform(-1, 1, (B * S, d)).astype(np.float32)
    return x, w, g


def run_torch(x, w, g, B, S, H, D, fn=block):
    tx = torch.tensor(x, requires_grad=True)
    tw = [torch.tensor(a, requires_grad=True) for a in w]
    y = fn(tx, tw, B, S, H, D, TorchApi)
    y.backward(torch.tensor(g))
    return y.detach().numpy(), tx.grad.numpy(), [a.grad.numpy() for a in tw]


def run_kf(x, w, g, B, S, H, D, bf16=False, fn=block):
    def up(a):
        t = kfunca.from_numpy(a, 0)
        t = t.bfloat16() if bf16 else t
        t.set_requires_grad(True)
        return t
    tx, tw = up(x), [up(a) for a in w]
    y = fn(tx, tw, B, S, H, D, KfApi)
    tg = kfunca.from_numpy(g, 0)
    y.backward(tg.bfloat16() if bf16 else tg)
    out = lambda t: (t.float() if bf16 else t).numpy()  # noqa: E731
    return out(y), out(tx.grad()), [out(a.grad()) for a in tw]


def rel_err(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


@pytest.mark.parametrize("B,S,H,D,f", [(2, 64, 2, 64, 256), (1, 96, 3, 128, 128)])
def test_block_f32_forward_backward_vs_torch_autograd(B, S, H, D, f):
    rng = np.random.default_rng(900 + S)
    x, w, g = make(rng, B, S, H, D, f)
    y0, dx0, dw0 = run_torch(x, w, g, B, S, H, D)
    y1, dx1, dw1 = run_kf(x, w, g, B, S, H, D)
    # f32 end to end (exact-f32 MFMA GEMMs and attention): 1e-4 of the tensor's scale; the reference's own bar is 1e-3
    assert rel_err(y1, y0) < 1e-4 and rel_err(dx1, dx0) < 1e-4
    for a, b in zip(dw1, dw0):
        assert a.shape == b.shape and rel_err(a, b) < 1e-4


def test_block_bf16_and_batch_sharded_gradients():
    B, S, H, D, f = 2, 128, 2, 128, 512
    rng = np.random.default_rng(910)
    x, w, g = make(rng, B, S, H, D, f)
    xb, gb = (O.bf16_to_f32(O.f32_to_bf16(a)) for a in (x, g))
    wb = [O.bf16_to_f32(O.f32_to_bf16(a)) for a in w]
    y0, dx0, dw0 = run_torch(xb, wb, gb, B, S, H, D)
    y1, dx1, dw1 = run_kf(xb, wb, gb, B, S, H, D, bf16=True)
    # bf16 storage between every operator (8 mantissa bits, ~10 roundings deep): 3e-2 of the tensor's scale
    assert rel_err(y1, y0) < 3e-2 and rel_err(dx1, dx0) < 3e-2
    for a, b in zip(dw1, dw0):
        assert rel_err(a, b) < 3e-2
    # data-parallel form: rank r runs batch element r with the same weights; dW = sum over ranks (the all-reduce), f32 here
    T = S
    parts = [run_kf(xb[r * T:(r + 1) * T], wb, gb[r * T:(r + 1) * T], 1, S, H, D) for r in range(B)]
    _, dxf, dwf = run_kf(xb, wb, gb, B, S, H, D)
    assert rel_err(np.concatenate([p[1] for p in parts]), dxf) < 1e-5
    for i in range(len(wb)):
        assert rel_err(sum(p[2][i] for p in parts), dwf[i]) < 1e-4


def test_view_slice_mul_scalar_cat_gradients():
    rng = np.random.default_rng(920)
    a = rng.uniform(-1, 1, (6, 10)).astype(np.float32)
    b = rng.uniform(-1, 1, (6, 4)).astype(np.float32)
    g = rng.uniform(-1, 1, (4, 3, 5)).astype(np.float32)

    def expr(A, Bm, cat, is_torch):
        left = A[:, 2:8] * 0.5 - 1.0                         # slice view, scalar ops
        z = cat([left, Bm * Bm], 1)                          # [6, 10]
        z = z - A / 4.0
        z = (z.permute(1, 0) if not is_torch else z.permute(1, 0)).contiguous()
        z = z.view(2, 5, 6) if not is_torch else z.reshape(2, 5, 6)
        return z[:, 1:4, 1:6:1].permute(2, 1, 0)[:4]         # [4, 3, 2] ... select a window again

    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    yt = expr(ta, tb, torch.cat, True)
    gt = torch.tensor(g[:, :, :2].copy())
    yt.backward(gt)
    ka, kb = kfunca.from_numpy(a, 0), kfunca.from_numpy(b, 0)
    ka.set_requires_grad(True)
    kb.set_requires_grad(True)
    yk = expr(ka, kb, kfunca.cat, False)
    assert yk.sizes() == list(yt.shape)
    assert np.allclose(yk.contiguous().numpy(), yt.detach().numpy(), atol=1e-6)
    yk.backward(kfunca.from_numpy(g[:, :, :2].copy(), 0))
    assert np.allclose(ka.grad().numpy(), ta.grad.numpy(), atol=1e-6)
    assert np.allclose(kb.grad().numpy(), tb.grad.numpy(), atol=1e-6)


def _leaf(a, requires=True):
    t = kfunca.from_numpy(a, 0)
    t.set_requires_grad(requires)
    return t


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_broadcast_operand_gets_its_gradient_summed_to_its_own_shape():
    """x[M, N] (op) b[1, N], b[M, 1], b[1, 1] and a b[N] viewed as [1, N] (operands of different rank are refused, as on the host this one was
    modelled on) for + - * /: b's gradient is the sum over the stretched dims, in b's shape - not the [M, N] tensor the engine used to hand
    over (add) and not a graph cut without a word (sub, mul, div). Small integers and divisors that are powers of two: exact in any summation
    order, so torch's bits."""
    rng = np.random.default_rng(921)
    x = rng.integers(-3, 4, (4, 6)).astype(np.float32)
    g = rng.integers(-2, 3, (4, 6)).astype(np.float32)
    ops = {"add": lambda a, b: a + b, "sub": lambda a, b: a - b, "mul": lambda a, b: a * b, "div": lambda a, b: a / b, "rsub": lambda a, b: b - a,
           "rdiv": lambda a, b: b / a}
    for shape in ((6,), (1, 6), (4, 1), (1, 1)):
        for name, op in ops.items():
            f = op if len(shape) == 2 else (lambda a, b, op=op: op(a, b.view(1, 6)))   # noqa: E731  (torch's view and this host's agree)
            b = rng.choice([0.5, 1.0, 2.0, 4.0], size=shape).astype(np.float32) * rng.choice([-1.0, 1.0], size=shape).astype(np.float32)
            xs = rng.choice([1.0, 2.0, 4.0], size=x.shape).astype(np.float32) if name == "rdiv" else x   # a divisor: powers of two
            tx, tb = torch.tensor(xs, requires_grad=True), torch.tensor(b, requires_grad=True)
            f(tx, tb).backward(torch.tensor(g))
            kx, kb = _leaf(xs), _leaf(b)
            y = f(kx, kb)
            assert y.requires_grad(), (name, shape)
            y.backward(kfunca.from_numpy(g, 0))
            assert kb.grad().sizes() == list(shape), (name, shape, kb.grad().sizes())
            assert _same_bits(kb.grad().numpy(), tb.grad.numpy()) and _same_bits(kx.grad().numpy(), tx.grad.numpy()), (name, shape)


def test_broadcast_intermediate_feeds_the_next_backward_in_its_own_shape():
    """The broadcast operand is an INTERMEDIATE: its [1, N] gradient goes on into a GradFunction that assumes [1, N] (a scale, a view), and a leaf
    reached both ways accumulates tensors of one shape."""
    rng = np.random.default_rng(922)
    x, w = rng.integers(-3, 4, (5, 4)).astype(np.float32), rng.integers(-3, 4, (1, 4)).astype(np.float32)
    g = rng.integers(-2, 3, (5, 2)).astype(np.float32)

    def expr(X, W):
        s = W * 2.0                      # [1, 4], an intermediate
        return (X * s + s)[:, 1:3] - X[:, 1:3] * W[:, 1:3]

    tx, tw = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
    expr(tx, tw).backward(torch.tensor(g))
    kx, kw = _leaf(x), _leaf(w)
    expr(kx, kw).backward(kfunca.from_numpy(g, 0))
    assert _same_bits(kw.grad().numpy(), tw.grad.numpy()) and _same_bits(kx.grad().numpy(), tx.grad.numpy())


def test_gradient_dtype_behind_a_mixed_dtype_cat_and_a_promoting_add():
    """cat converts its inputs to the first one's dtype and f32 + f64 promotes: each leaf's gradient comes back in the LEAF's dtype."""
    rng = np.random.default_rng(923)
    a, b = rng.integers(-3, 4, (3, 4)).astype(np.float64), rng.integers(-3, 4, (3, 2)).astype(np.float32)
    g = rng.integers(-2, 3, (3, 10)).astype(np.float64)
    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    (torch.cat([ta, tb.double(), ta], 1) * 2.0).backward(torch.tensor(g))
    ka, kb = _leaf(a), _leaf(b)
    (kfunca.cat([ka, kb, ka], 1) * 2.0).backward(kfunca.from_numpy(g, 0))
    assert _same_bits(ka.grad().numpy(), ta.grad.numpy()) and _same_bits(kb.grad().numpy(), tb.grad.numpy())
    c = rng.integers(-3, 4, (3, 2)).astype(np.float64)
    tb2, tc = torch.tensor(b, requires_grad=True), torch.tensor(c, requires_grad=True)
    (tb2 + tc).backward(torch.tensor(g[:, :2].copy()))
    kb2, kc = _leaf(b), _leaf(c)
    (kb2 + kc).backward(kfunca.from_numpy(g[:, :2].copy(), 0))
    assert _same_bits(kb2.grad().numpy(), tb2.grad.numpy()) and _same_bits(kc.grad().numpy(), tc.grad.numpy())


def test_block_step_replays_from_a_hip_graph():
    """A whole forward + backward step of the block recorded from the operator API (kfunca.graph_begin / graph_end) and replayed
    with one submission: the replay's output and gradients are bit-identical to the eager step's."""
    B, S, H, D, f = 1, 128, 2, 128, 256
    rng = np.random.default_rng(930)
    x, w, g = make(rng, B, S, H, D, f)

    def up(a):
        t = kfunca.from_numpy(a, 0).bfloat16()
        t.set_requires_grad(True)
        return t

    tx, tw, tg = up(x), [up(a) for a in w], kfunca.from_numpy(g, 0).bfloat16()
    bits = lambda t: t.float().numpy().view(np.uint32).copy()  # noqa: E731

    def step():
        y = block(tx, tw, B, S, H, D, KfApi)
        y.backward(tg)
        return y

    y = step()  # warms the allocator; leaf gradients now hold 1 x the step's gradient
    y = step()  # ... 2 x
    kfunca.synchronize(0)
    want_y = bits(y)
    g2 = [bits(t.grad()) for t in [tx] + tw]
    kfunca.graph_begin(0)
    yg = step()  # recorded, not run: gradients still 2 x
    graph = kfunca.graph_end(0)
    kfunca.graph_launch(graph, 0)  # 3 x
    kfunca.synchronize(0)
    assert np.array_equal(bits(yg), want_y)
    g3 = [bits(t.grad()) for t in [tx] + tw]
    y = step()  # eager: 4 x
    kfunca.synchronize(0)
    g4 = [bits(t.grad()) for t in [tx] + tw]
    kfunca.graph_launch(graph, 0)  # 5 x
    kfunca.synchronize(0)
    g5 = [bits(t.grad()) for t in [tx] + tw]
    f32 = lambda a: a.view(np.float32)  # noqa: E731
    for a2, a3, a4, a5 in zip(g2, g3, g4, g5):
        # the replay added exactly what an eager step adds (bf16 accumulation: compare the increments through the eager path)
        assert not np.array_equal(a3, a2) and not np.array_equal(a5, a4)
        assert np.allclose(f32(a3) - f32(a2), f32(a4) - f32(a3), rtol=0.1, atol=0.05 * np.abs(f32(a2)).max())
    kfunca.graph_destroy(graph)


def test_graph_scratch_never_reenters_the_shared_cache():
    """Allocator capture mode: temporaries the recorded step allocated and freed stay in a pool private to the graph, so a tensor
    allocated between two replays can never be handed memory the graph still writes on replay (before: the temporary's block
    went back to the shared cache at capture time and the next same-size allocation was clobbered by every replay)."""
    n = 1 << 16
    rng = np.random.default_rng(931)
    a, b, c = (rng.uniform(-1, 1, (n,)).astype(np.float32) for _ in range(3))
    ta, tb, tc = (kfunca.from_numpy(x, 0) for x in (a, b, c))
    warm = (ta + tb) * tc  # same sizes once eagerly: the cache now holds a block of the temporary's size
    del warm
    kfunca.synchronize(0)
    before = kfunca.memstat_dict(0)
    kfunca.graph_begin(0)
    out = (ta + tb) * tc  # the sum is a temporary: freed during the capture
    graph = kfunca.graph_end(0)
    held = kfunca.memstat_dict(0)
    assert held["graph_blocks"] >= 1 and held["graph_bytes"] >= 4 * n, held
    assert held["cached_blocks"] <= before["cached_blocks"], (before, held)
    # new tensors of the temporary's size: none may alias the graph's scratch
    fresh = [kfunca.empty([n], kfunca.dtype.float, 0).fill_(7.0) for _ in range(8)]
    for _ in range(3):
        kfunca.graph_launch(graph, 0)
    kfunca.synchronize(0)
    assert np.array_equal(out.numpy(), (a + b) * c)
    for t in fresh:
        assert (t.numpy() == 7.0).all()
    del out
    kfunca.graph_destroy(graph)
    after = kfunca.memstat_dict(0)
    # the graph's pool is back in the shared cache: no block is lost, none is still held for the graph
    assert after["graph_blocks"] == 0, after
    assert (after["cached_blocks"] + after["active_blocks"] ==
            held["cached_blocks"] + held["active_blocks"] + held["graph_blocks"] + after["driver_allocs"] - held["driver_allocs"]), (held, after)


def _with_gains(rng, w, d):
    return w + [rng.uniform(0.5, 1.5, (d,)).astype(np.float32) for _ in range(2)]


@pytest.mark.parametrize("B,S,H,D,f", [(2, 64, 2, 64, 256), (1, 128, 2, 128, 128)])
def test_fused_block_f32_vs_torch_autograd(B, S, H, D, f):
    """block2 in f32 (attention takes the operator's fall-back composition here: the strided kernels are 16-bit): y, dx and all
    seven parameter gradients within 1e-4 of torch-CPU autograd."""
    rng = np.random.default_rng(940 + S)
    x, w, g = make(rng, B, S, H, D, f)
    w = _with_gains(rng, w, H * D)
    y0, dx0, dw0 = run_torch(x, w, g, B, S, H, D, fn=block2)
    y1, dx1, dw1 = run_kf(x, w, g, B, S, H, D, fn=block2)
    assert rel_err(y1, y0) < 1e-4 and rel_err(dx1, dx0) < 1e-4
    for a, b in zip(dw1, dw0):
        assert a.shape == b.shape and rel_err(a, b) < 1e-4


def test_fused_block_bf16_runs_the_fused_kernels():
    """block2 in bf16 at D = 128, S % 128 == 0: the strided attention kernels and the GEMM tails run (asserted by kernel label:
    no copy kernel between the QKV projection and the output projection), results within the bf16 bar of torch autograd."""
    from kfunca_amd import hip_abi as HA
    B, S, H, D, f = 2, 128, 2, 128, 512
    rng = np.random.default_rng(950)
    x, w, g = make(rng, B, S, H, D, f)
    w = _with_gains(rng, w, H * D)
    xb, gb = (O.bf16_to_f32(O.f32_to_bf16(a)) for a in (x, g))
    wb = [O.bf16_to_f32(O.f32_to_bf16(a)) for a in w]
    y0, dx0, dw0 = run_torch(xb, wb, gb, B, S, H, D, fn=block2)
    def leaf(a):
        t = kfunca.from_numpy(a, 0).bfloat16()
        t.set_requires_grad(True)
        return t
    tx, tw, tg = leaf(xb), [leaf(a) for a in wb], kfunca.from_numpy(gb, 0).bfloat16()
    HA.profile_reset()
    HA.profile_enable(True)
    y = block2(tx, tw, B, S, H, D, KfApi)
    y.backward(tg)
    kfunca.synchronize(0)
    HA.profile_enable(False)
    ran = HA.profile_results()
    y1, dx1, dw1 = y.float().numpy(), tx.grad().float().numpy(), [t.grad().float().numpy() for t in tw]
    assert "attn_fwd_mfma" in ran and "attn_bwd_dkv_mfma" in ran and "norm_fwd" in ran and "norm_bwd" in ran, ran
    ew = {k: n for k, (ms, n) in ran.items() if k.startswith("ew_")}
    # what is left between the GEMMs / attention / norms: the two products of the gate's backward (dy o mul, dy o raw) and the
    # sums where a tensor feeds two consumers (x, h, n2); no copy, no layout change, no first-gradient copy of the eight leaves
    assert sum(ew.values()) <= 8 and not any("copy" in k or "transpose" in k for k in ew), ran
    assert rel_err(y1, y0) < 3e-2 and rel_err(dx1, dx0) < 3e-2
    for a, b in zip(dw1, dw0):
        assert rel_err(a, b) < 3e-2


def test_gradient_bucket_collects_the_same_bits_and_fires_chunks_in_arrival_order():
    """kfunca.GradBucket (csrc/core/comm.cpp) on a small block, one process, no communicator: the bucketed weights' gradients are the
    SAME BITS as plain autograd gives (GEMM backward writes dW straight into the bucket's flat buffer, fan-in and norm gains are
    copied in), p.grad() are views into flat(), chunks leave in the order the backward completes them (the last parameters first),
    zero_grad + a second step reproduce the first, and detach restores ordinary gradients."""
    B, S, H, D, f = 1, 128, 2, 64, 256
    d = H * D
    rng = np.random.default_rng(930)
    x, w, g = make(rng, B, S, H, D, f)
    gains = [np.ones(d, np.float32) + 0.1 * rng.uniform(-1, 1, d).astype(np.float32) for _ in range(2)]

    def up(a):
        t = kfunca.from_numpy(a, 0).bfloat16()
        t.set_requires_grad(True)
        return t
    tx, tw, tg = up(x), [up(a) for a in w + gains], kfunca.from_numpy(g, 0).bfloat16()

    def step():
        for t in [tx] + tw:
            t.zero_grad()
        y = block2(tx, tw, B, S, H, D, KfApi)
        y.backward(tg)
        return y
    step()
    plain = [t.grad().numpy().copy() for t in tw]
    order_used = [5, 0, 1, 6, 2, 3, 4]  # the bucket takes the parameters in the order the forward uses them: g1 Wqkv Wo g2 Wgate Wup Wdown
    cap_mb = (2 * d * f) * 2 / 1048576 + 1e-3  # room for [up, down] in the first chunk
    bucket = kfunca.GradBucket([tw[i] for i in order_used], cap_mb)
    chunks = bucket.chunks()
    assert chunks[0][:2] == (5, 6) and chunks[-1][0] == 0 and sum(c[3] for c in chunks) == bucket.flat().numel()
    bucket.attach()
    for rep in range(2):
        step()
        bucket.wait()
        flat_ptr, flat_bytes = bucket.flat().data_ptr(), bucket.reduced_bytes()
        for i, t in enumerate(tw):
            got = t.grad().numpy()
            assert np.array_equal(got, plain[i]), (rep, i)
            assert flat_ptr <= t.grad().data_ptr() < flat_ptr + flat_bytes  # the gradient IS its slot of the flat buffer
        order = bucket.fired_order()
        assert sorted(order) == list(range(len(chunks))) and order[0] == 0 and order[-1] == len(chunks) - 1, order  # [up, down] first, g1 / Wqkv last
    bucket.detach()
    step()
    assert all(np.array_equal(t.grad().numpy(), p) for t, p in zip(tw, plain))
    assert not (flat_ptr <= tw[0].grad().data_ptr() < flat_ptr + flat_bytes)


def test_collectives_on_one_rank_through_the_operator_api():
    """all_reduce_(tensor | list) and the bucket's chunked all-reduce with a REAL RCCL communicator of one rank (the sum over one
    rank is the identity: bit-identical results, every stream / event hand-off of the N > 1 path exercised). Runs in a child
    process: a process owns one communicator."""
    import subprocess
    import sys
    code = r'''
import numpy as np, kfunca_amd as kfunca
kfunca.comm_init(kfunca.comm_unique_id(), 0, 1, 0)
assert kfunca.comm_initialized() and kfunca.comm_world_size() == 1 and kfunca.comm_rank() == 0
rng = np.random.default_rng(1)
a, b = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((257, 33), (1000,)))
ta, tb = kfunca.from_numpy(a, 0), kfunca.from_numpy(b, 0).bfloat16()
kfunca.all_reduce_(ta)
assert np.array_equal(ta.numpy(), a)
tc = kfunca.from_numpy(a * 2, 0)
kfunca.all_reduce_([ta, tc])
assert np.array_equal(ta.numpy(), a) and np.array_equal(tc.numpy(), a * 2)
try:
    kfunca.all_reduce_(ta.permute(1, 0))
    raise SystemExit("a strided tensor was accepted")
except RuntimeError:
    pass
w = [kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16() for _ in range(3)]
for t in w:
    t.set_requires_grad(True)
x = kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16()
g = kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16()
def step():
    for t in w:
        t.zero_grad()
    kfunca.gemm(kfunca.gemm(kfunca.gemm(x, w[0], 1.0, 0.0), w[1], 1.0, 0.0), w[2], 1.0, 0.0).backward(g)
step()
plain = [t.grad().numpy().copy() for t in w]
bucket = kfunca.GradBucket(w, 256 * 256 * 2 / 1048576)  # one weight per chunk: three collectives per step
bucket.attach()
for _ in range(3):
    step()
    bucket.wait()
    assert bucket.fired_order() == [0, 1, 2]
    assert all(np.array_equal(t.grad().numpy(), p) for t, p in zip(w, plain))
bucket.detach()
kfunca.comm_destroy()
assert not kfunca.comm_initialized()
print("ok")
'''
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_c5_full_size_shard_and_the_multi_rank_runner_on_one_gpu():
    """Config C5 at its full per-GPU size (B 1, S 4096, d 4096, 32 x 128 heads, MLP 16384) through tools/block_bench.py --check with a
    one-rank RCCL communicator: the whole multi-rank program (gloo rendezvous, C++ communicator, gradient bucket reduced in four
    chunks on the communication stream, bucket.wait) and its two verdicts - the reduced bucket equals the rank's own gradients bit for
    bit, and the shard's y, dx and all five dW agree with oracle/block_ref.py within 1.5e-2 of each tensor's norm (whole tensor and 64
    sampled rows), on the matrix-core kernels (labels asserted)."""
    import json
    import os
    import subprocess
    import sys
    from pathlib import Path
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    res = subprocess.run([sys.executable, str(Path(__file__).resolve().parent.parent / "tools" / "block_bench.py"), "--gpus", "1", "--force-comm", "--check",
                          "--steps", "2", "--warmup", "1"], capture_output=True, text=True, env=env, timeout=1500)
    assert res.returncode == 0, (res.stdout[-3000:], res.stderr[-3000:])
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.strip()][-1])
    c = line["checks"]
    assert c["allreduce_vs_gloo_sum"] is True and c["shard_vs_oracle"] is True and c["shard_kernels_are_the_matrix_core_ones"] is True, c
    assert line["bucket"]["collective"] == "RCCL" and [ch[:2] for ch in line["bucket"]["chunks_first_last_offset_numel"]] == [[4, 4], [3, 3], [2, 2], [0, 1]]
    assert sorted(line["bucket"]["fired_order_last_step"]) == [0, 1, 2, 3] and line["bucket"]["fired_order_last_step"][-1] == 3
    assert set(c["shard_figures"]) == {"y", "dx", "dWqkv", "dWo", "dWgate", "dWup", "dWdown"}


def test_bucketed_weight_used_by_two_products_gets_the_sum():
    """one bucketed W feeding TWO matmuls of a graph (weight tying). Both backward products used to write their
    dW with beta = 0 straight into the same bucket slot - the gradient came out as 2 dW_last. The sink now hands the slot to the first
    product of a pass only (GradSink::take_slot); the second allocates, the engine sums. Checked against plain autograd (no bucket)
    bit for bit and against numpy, for the pair-launch shape (256 multiples, both inputs need gradients) and for the two-call shape."""
    rng = np.random.default_rng(77)
    for n, fused in ((256, False), (256, True), (192, False)):
        x1, x2, w, g = (rng.uniform(-1, 1, (n, n)).astype(np.float32) for _ in range(4))

        def up(a, grad=True):
            t = kfunca.from_numpy(a, 0).bfloat16()
            t.set_requires_grad(grad)
            return t
        t1, t2, tw, tg = up(x1), up(x2), up(w), kfunca.from_numpy(g, 0).bfloat16()

        def step():
            for t in (t1, t2, tw):
                t.zero_grad()
            if fused:
                y = kfunca.gemm_fused(t1, tw, 1.0, None, None, None) + kfunca.gemm_fused(t2, tw, 1.0, None, None, None)
            else:
                y = kfunca.gemm(t1, tw, 1.0, 0.0) + kfunca.gemm(t2, tw, 1.0, 0.0)
            y.backward(tg)
        step()
        plain = tw.grad().numpy().copy()
        f = lambda t: t.float().numpy().astype(np.float64)
        want = f(t1).T @ f(tg) + f(t2).T @ f(tg)
        got = (plain.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        assert np.abs(got - want).max() <= 2.0 ** -6 * np.abs(want).max(), "plain autograd itself"
        bucket = kfunca.GradBucket([tw], 64.0)
        bucket.attach()
        for rep in range(2):
            step()
            bucket.wait()
            assert np.array_equal(tw.grad().numpy(), plain), (n, fused, rep)  # dW_1 + dW_2, not 2 dW_2
        assert tw.grad().data_ptr() == bucket.flat().data_ptr()
        bucket.detach()


def test_dropping_a_bucket_frees_it_without_detach():
    """attach() used to store the bucket in every parameter's TensorImpl (bucket -> params -> impl -> bucket): a
    dropped bucket was never freed. Parameters now hold it weakly: after `del bucket` the flat buffer returns to the allocator's
    cache and the parameters get ordinary gradients again."""
    import gc
    rng = np.random.default_rng(5)
    w = kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16()
    w.set_requires_grad(True)
    x = kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16()
    g = kfunca.from_numpy(rng.uniform(-1, 1, (256, 256)).astype(np.float32), 0).bfloat16()
    gc.collect()  # cyclic garbage of earlier tests must not be freed between the two counts (the collect below would take it along)
    before = kfunca.memstat_dict(0)["active_blocks"]
    bucket = kfunca.GradBucket([w], 64.0)
    bucket.attach()
    assert kfunca.memstat_dict(0)["active_blocks"] == before + 1  # the flat buffer
    del bucket
    gc.collect()
    assert kfunca.memstat_dict(0)["active_blocks"] == before
    kfunca.gemm(x, w, 1.0, 0.0).backward(g)
    want = kfunca.gemm_ex(x, True, g, False, 1.0) if hasattr(kfunca, "gemm_ex") else None
    assert w.grad().defined()
    if want is not None:
        assert np.array_equal(w.grad().numpy(), want.numpy())


def test_float_gradient_bucket_keeps_the_accumulators_unrounded():
    """VERDICT round 3 #7 / ADVICE: GradBucket(..., accum_f32=True) - the flat buffer and every .grad view of it are float, the dW GEMMs
    of the bf16 layers write their f32 accumulators straight into the slots (kf_gemm_epilogue.c_f32), fan-in and norm gains are added in
    float. Checked: (1) rounding the float gradients once gives exactly the bf16 gradients plain autograd produces (same accumulators,
    one rounding either way) for every weight used once; (2) against f64 numpy on the weight of a lone matmul: f32 accumulation noise;
    (3) a weight used TWICE sums in float; (4) the all-reduce of the float bucket on a one-rank communicator is the identity."""
    B, S, H, D, f = 1, 128, 2, 64, 256
    d = H * D
    rng = np.random.default_rng(931)
    x, w, g = make(rng, B, S, H, D, f)

    def up(a):
        t = kfunca.from_numpy(a, 0).bfloat16()
        t.set_requires_grad(True)
        return t
    tx, tw, tg = up(x), [up(a) for a in w], kfunca.from_numpy(g, 0).bfloat16()

    def step():
        for t in [tx] + tw:
            t.zero_grad()
        block(tx, tw, B, S, H, D, KfApi).backward(tg)
    step()
    plain = [t.grad().numpy().copy() for t in tw]          # bf16 bits
    bucket = kfunca.GradBucket(tw, 64.0, True)
    bucket.attach()
    step()
    bucket.wait()
    assert bucket.flat().dtype() == kfunca.float and bucket.reduced_bytes() == bucket.flat().numel() * 4
    for i, t in enumerate(tw):
        got = t.grad().numpy()
        assert got.dtype == np.float32
        assert np.array_equal(O.f32_to_bf16(got), plain[i]), i   # one rounding of the same accumulators
    bucket.detach()
    # (2) + (3): a lone product and a tied weight, against f64
    n = 256
    a1, a2, ww, gg = (rng.uniform(-1, 1, (n, n)).astype(np.float32) for _ in range(4))
    t1, t2, t_w, t_g = up(a1), up(a2), up(ww), kfunca.from_numpy(gg, 0).bfloat16()
    b2 = kfunca.GradBucket([t_w], 64.0, True)
    b2.attach()
    f = lambda t: t.float().numpy().astype(np.float64)
    for t in (t1, t2, t_w):
        t.zero_grad()
    (kfunca.gemm(t1, t_w, 1.0, 0.0) + kfunca.gemm(t2, t_w, 1.0, 0.0)).backward(t_g)
    b2.wait()
    want = f(t1).T @ f(t_g) + f(t2).T @ f(t_g)
    mag = np.abs(f(t1)).T @ np.abs(f(t_g)) + np.abs(f(t2)).T @ np.abs(f(t_g))
    got = t_w.grad().numpy().astype(np.float64)
    assert (np.abs(got - want) <= 4e-6 * mag + 1e-6).all()   # nothing of the 16-bit format's 2^-8 in it
    b2.detach()
