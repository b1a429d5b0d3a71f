"""-m gpu: kfunca.causal_conv1d and kfunca.causal_conv1d_step through the module API, against tests/causal_conv1d_ref.py with the bounds
of tests/test_gpu_causal_conv1d.py (n = K + 1 for y, K + 2 for dx and d initial_state, R + 3 + W + K + 2 for dw and dbias). Through the
engine y and the returned state each have a node and their gradients are added in the operands' dtype: the state node's dx is d_hT in the
last K - 1 rows and zero elsewhere, its dw and dbias are zero, so the sums take one more rounding of dx and d initial_state, u (|ref| + absref)."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from tests.causal_conv1d_ref import ROWS as R, U, bound, reference, stored

pytestmark = pytest.mark.gpu
B, S, C, K = 2, R + 5, 72, 4


def to_t(a, dt, grad=False):
    t = kfunca.from_numpy(np.ascontiguousarray(a, np.float32), 0)
    t = t if dt == "f32" else t.bfloat16() if dt == "bf16" else t.half()
    t.set_requires_grad(grad)
    return t


f64 = lambda t: t.contiguous().float().numpy().astype(np.float64)
bits = lambda t: t.contiguous().float().numpy().view(np.uint32).copy()


def draw(dt, seed=0):
    rng = np.random.default_rng(seed)
    u = lambda *shape: stored(rng.uniform(-2, 2, shape), dt)
    return dict(x=u(B, S, C), w=u(K, C), bias=u(C), h0=u(B, K - 1, C), dy=u(B, S, C), d_hT=u(B, K - 1, C))


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_a_column_slice_is_read_in_place(dt):
    a = draw(dt)
    wide = np.concatenate([np.full((B, S, 16), 9.0), a["x"], np.full((B, S, 8), -9.0)], 2)   # z | x | dt of an in-projection row
    y, state = kfunca.causal_conv1d(to_t(wide, dt)[:, :, 16:16 + C], to_t(a["w"], dt), to_t(a["bias"], dt), "silu", to_t(a["h0"], dt), True)
    ref, absref = reference(a["x"], a["w"], a["bias"], a["h0"], True)
    assert (np.abs(f64(y) - ref["y"]) <= bound(ref["y"], absref["y"], dt, K + 1, True)).all() and np.array_equal(f64(state), ref["hT"])


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_backward_through_y_and_the_returned_state(dt):
    a = draw(dt, 1)
    t = {n: to_t(a[n], dt, True) for n in ("x", "w", "bias", "h0")}
    y, state = kfunca.causal_conv1d(t["x"], t["w"], t["bias"], "silu", t["h0"], True)
    kfunca.cat([y, state], 1).backward(to_t(np.concatenate([a["dy"], a["d_hT"]], 1), dt))
    ref, absref = reference(a["x"], a["w"], a["bias"], a["h0"], True, a["dy"], a["d_hT"])
    for n, key, count, sums in (("x", "dx", K + 2, 1), ("h0", "dh0", K + 2, 1), ("w", "dw", R + 3 + B + K + 2, 0), ("bias", "dbias", R + 3 + B + K + 2, 0)):
        lim = bound(ref[key], absref[key], dt, count, True) + sums * U[dt] * (np.abs(ref[key]) + absref[key])
        assert (np.abs(f64(t[n].grad()) - ref[key]) <= lim).all(), n


def test_prefill_then_steps_give_the_bits_of_one_call():
    """the same K fused multiply-adds in the same order on both routes: token by token (T = 1) and one call of T = 5"""
    dt, P = "bf16", S - 5
    a = draw(dt, 2)
    op = lambda x, **kw: kfunca.causal_conv1d(to_t(x, dt), to_t(a["w"], dt), to_t(a["bias"], dt), "silu", to_t(a["h0"], dt), **kw)
    want = bits(op(a["x"]))
    for T in (1, 5):
        y, state = op(a["x"][:, :P], return_state=True)
        assert np.array_equal(bits(y), want[:, :P])
        for lo in range(P, S, T):
            y = kfunca.causal_conv1d_step(to_t(a["x"][:, lo:lo + T], dt), to_t(a["w"], dt), state, to_t(a["bias"], dt), "silu")
            assert np.array_equal(bits(y), want[:, lo:lo + T]), (T, lo)
        assert np.array_equal(f64(state), a["x"][:, S - (K - 1):])


def test_forward_and_backward_replay_from_a_graph():
    a = draw("f32", 3)
    t = {n: to_t(a[n], "f32", True) for n in ("x", "w", "bias", "h0")}
    dy = to_t(a["dy"], "f32")

    def step():
        y = kfunca.causal_conv1d(t["x"], t["w"], t["bias"], "silu", t["h0"])
        y.backward(dy)
        return y

    want = bits(step())
    once = [t[n].grad().numpy().copy() for n in t]
    step()                                   # warms the allocator; the leaves now hold twice the gradient
    kfunca.synchronize(0)
    kfunca.graph_begin(0)
    y = step()                               # recorded, not run
    graph = kfunca.graph_end(0)
    acc = [g + g for g in once]
    for _ in range(3):
        kfunca.graph_launch(graph, 0)
        kfunca.synchronize(0)
        acc = [s + g for s, g in zip(acc, once)]   # the engine's f32 accumulation of the same increment
        assert np.array_equal(bits(y), want) and all(np.array_equal(t[n].grad().numpy(), s) for n, s in zip(t, acc))
    kfunca.graph_destroy(graph)
