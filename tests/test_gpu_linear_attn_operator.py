"""-m gpu: kfunca.linear_attention and Tensor.backward through it against the float64 reference of tests/linear_attn_ref.py, random tier
(bound and rounding count c = 2 as in tests/test_gpu_linear_attn.py); q is a transposed view of a [B, S, H, D] buffer and scale is
left to its default D ** -0.5. Then forward and backward captured into a graph and replayed twice, and the raised errors."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from tests import gemm_views as V
from tests.linear_attn_ref import check_random, reference

pytestmark = pytest.mark.gpu
B, Hh = 1, 2


def to_t(a, dt, grad=True):
    t = kfunca.from_numpy(np.ascontiguousarray(a, np.float32), 0)
    t = t if dt == "f32" else t.bfloat16() if dt == "bf16" else t.half()
    t.set_requires_grad(grad)
    return t


def draw(S, D, dt):
    rng = np.random.default_rng(S + D)
    q, k, v, do = (V.decode(V.encode(rng.uniform(-1, 1, (B, Hh, S, D)), dt), dt) for _ in range(4))
    g = -rng.uniform(0, 0.05, (B, Hh, S)).astype(np.float32).astype(np.float64)
    return q, k, v, g, do


def tensors(q, k, v, g, do, dt):
    qb = to_t(q.transpose(0, 2, 1, 3), dt)   # [B, S, H, D]: the operator sees a transposed view of it
    return qb, to_t(k, dt), to_t(v, dt), to_t(g, "f32"), to_t(do, dt, grad=False)


def results(out, qb, tk, tv, tg):
    f = lambda t: t.contiguous().float().numpy().astype(np.float64)
    return dict(o=f(out), dq=f(qb.grad()).transpose(0, 2, 1, 3), dk=f(tk.grad()), dv=f(tv.grad()), dg=f(tg.grad()))


@pytest.mark.parametrize("S,D,dt", [(130, 64, "bf16"), (256, 128, "f16")])
def test_forward_and_backward(S, D, dt):
    q, k, v, g, do = draw(S, D, dt)
    qb, tk, tv, tg, tdo = tensors(q, k, v, g, do, dt)
    out = kfunca.linear_attention(qb.permute(0, 2, 1, 3), tk, tv, tg)
    out.backward(tdo)
    got = results(out, qb, tk, tv, tg)
    flat = lambda x: x.reshape((B * Hh,) + x.shape[2:])
    ref, absref = reference(*(flat(x) for x in (q, k, v, g, do)), float(np.float32(D ** -0.5)))
    check_random({n: flat(x) for n, x in got.items()}, ref, absref, S, 2)


def test_captured_forward_and_backward_replay_to_the_eager_bits():
    q, k, v, g, do = draw(130, 64, "bf16")
    for _ in range(2):   # warms the allocator
        qb, tk, tv, tg, tdo = tensors(q, k, v, g, do, "bf16")
        out = kfunca.linear_attention(qb.permute(0, 2, 1, 3), tk, tv, tg)
        out.backward(tdo)
        eager = results(out, qb, tk, tv, tg)
    qb, tk, tv, tg, tdo = tensors(q, k, v, g, do, "bf16")
    kfunca.synchronize(0)
    kfunca.graph_begin(0)
    out = kfunca.linear_attention(qb.permute(0, 2, 1, 3), tk, tv, tg)   # recorded, not run
    out.backward(tdo)
    graph = kfunca.graph_end(0)
    try:
        for _ in range(2):
            kfunca.graph_launch(graph, 0)
            kfunca.synchronize(0)
            got = results(out, qb, tk, tv, tg)   # (16-bit and f32 values widened exactly: equal values are equal bits)
            assert all(np.array_equal(got[n], eager[n]) for n in eager)
    finally:
        kfunca.graph_destroy(graph)


def test_refusals():
    q, k, v, g, do = draw(16, 64, "bf16")
    _, tk, tv, tg, _ = tensors(q, k, v, g, do, "bf16")
    with pytest.raises(Exception, match="linear_attention supports half and bfloat16"):
        kfunca.linear_attention(to_t(q, "f32"), to_t(k, "f32"), to_t(v, "f32"), tg)
    with pytest.raises(Exception, match=r"linear_attention: Dk 64 != Dv 32"):
        kfunca.linear_attention(to_t(q, "bf16"), tk, to_t(v[..., :32], "bf16"), tg)
