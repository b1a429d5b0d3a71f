"""-m gpu: one mixture-of-experts layer through the operator API with no host round trip between x and y,

    gemm -> softmax -> topk -> moe_plan -> moe_gate(normalize=True) -> moe_dispatch -> expert_linear -> swiglu -> expert_linear -> moe_combine

against an f64 numpy restatement that rounds to bf16 wherever an operator stores (as oracle/block_ref.py does; the expert ids are taken
from the device run), relative Frobenius error of y, dx, dw1, dw2 and dwr <= 1.5e-2. Then the forward is captured in a graph, the router
weight is overwritten in place so that other experts win, and the replay must equal an eager run on the new weights bit for bit: nothing
was read back while capturing."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle.block_ref import r16, rel_fro
from tests import gemm_views as V
from tests import moe_ref as M

pytestmark = pytest.mark.gpu

T, D, E, K, F = 96, 128, 8, 2, 128


def to_t(vals, requires_grad=False):
    t = kfunca.from_numpy_bf16(np.ascontiguousarray(V.encode(vals, "bf16")), 0)
    t.set_requires_grad(requires_grad)
    return t


def from_t(t):
    return V.decode(np.ascontiguousarray(t.numpy()).view(np.uint16), "bf16")


def bits(t):
    return np.ascontiguousarray(t.numpy()).view(np.uint16).copy()


def r(x):
    return r16(np.asarray(x, dtype=np.float32)).astype(np.float64)


def silu(g):
    return g / (1.0 + np.exp(-g))


def dsilu(g):
    s = 1.0 / (1.0 + np.exp(-g))
    return s + g * s * (1.0 - s)


def layer(tx, twr, tw1, tw2):
    p = kfunca.softmax(kfunca.gemm(tx, twr, 1.0, 0.0))                     # [T, E]
    ids = p.topk(K, -1, True)[1]                                           # [T, k] Long, on the device
    plan = kfunca.moe_plan(ids, E)
    gate = kfunca.moe_gate(p, plan, True)                                  # [T, k]
    xs = kfunca.moe_dispatch(tx, plan)                                     # [T k, d]
    a = kfunca.swiglu(kfunca.expert_linear(xs, tw1, plan.offsets))         # [T k, F]
    ys = kfunca.expert_linear(a, tw2, plan.offsets)                        # [T k, d]
    return kfunca.moe_combine(ys, plan, gate), plan


def draw():
    rng = np.random.default_rng(17)
    x, wr = r(rng.uniform(-1, 1, (T, D))), r(rng.uniform(-1, 1, (D, E)) * 0.3)
    w1, w2 = r(rng.uniform(-1, 1, (E, D, 2 * F)) * 0.15), r(rng.uniform(-1, 1, (E, F, D)) * 0.15)
    dy = r(rng.uniform(-1, 1, (T, D)))
    wr_new = r(rng.uniform(-1, 1, (D, E)) * 0.3)
    return x, wr, w1, w2, dy, wr_new


def test_layer_against_the_rounded_f64_restatement():
    x, wr, w1, w2, dy, _ = draw()
    tx, twr, tw1, tw2 = (to_t(v, True) for v in (x, wr, w1, w2))
    y, plan = layer(tx, twr, tw1, tw2)
    y.backward(to_t(dy))
    ids = plan.ids.numpy().astype(np.int64)
    assert ids.shape == (T, K) and ((ids >= 0) & (ids < E)).all()

    # the plan of the device's ids
    offsets, row_pair, pair_row = M.plan(ids, E)
    assert np.array_equal(plan.offsets.numpy(), offsets) and np.array_equal(plan.row_pair.numpy(), row_pair)
    assert np.array_equal(plan.pair_row.numpy().reshape(-1), pair_row)
    pr, token = pair_row.reshape(T, K).astype(np.int64), row_pair.astype(np.int64) // K
    seg = [slice(int(offsets[e]), int(offsets[e + 1])) for e in range(E)]

    # forward
    logits = r(x @ wr)
    ex = np.exp(logits - logits.max(1, keepdims=True))
    rp = r(ex / ex.sum(1, keepdims=True))
    s = np.take_along_axis(rp, ids, 1)
    S = s.sum(1, keepdims=True)
    rgate = r(s / S)
    rxs = x[token]
    rh = np.zeros((T * K, 2 * F))
    for e in range(E):
        rh[seg[e]] = rxs[seg[e]] @ w1[e]
    rh = r(rh)
    hg, hu = rh[:, :F], rh[:, F:]
    ra = r(silu(hg) * hu)
    rys = np.zeros((T * K, D))
    for e in range(E):
        rys[seg[e]] = ra[seg[e]] @ w2[e]
    rys = r(rys)
    ry = r(sum(rgate[:, j, None] * rys[pr[:, j]] for j in range(K)))       # one rounding
    # backward
    dys, dgate = np.zeros((T * K, D)), np.zeros((T, K))
    for j in range(K):
        dys[pr[:, j]] = rgate[:, j, None] * dy
        dgate[:, j] = (dy * rys[pr[:, j]]).sum(1)
    dys, dgate = r(dys), r(dgate)
    da, dw2 = np.zeros((T * K, F)), np.zeros_like(w2)
    for e in range(E):
        da[seg[e]] = dys[seg[e]] @ w2[e].T
        dw2[e] = ra[seg[e]].T @ dys[seg[e]]
    da, dw2 = r(da), r(dw2)
    dh = r(np.concatenate([da * hu * dsilu(hg), da * silu(hg)], 1))
    dxs, dw1 = np.zeros((T * K, D)), np.zeros_like(w1)
    for e in range(E):
        dxs[seg[e]] = dh[seg[e]] @ w1[e].T
        dw1[e] = rxs[seg[e]].T @ dh[seg[e]]
    dxs, dw1 = r(dxs), r(dw1)
    dx_experts = r(sum(dxs[pr[:, j]] for j in range(K)))
    ds = (dgate - (dgate * rgate).sum(1, keepdims=True)) / S
    dp = np.zeros((T, E))
    for j in range(K):
        np.add.at(dp, (np.arange(T), ids[:, j]), ds[:, j])
    dp = r(dp)
    dlogits = r(rp * (dp - (dp * rp).sum(1, keepdims=True)))
    dwr = r(x.T @ dlogits)
    dx = r(dx_experts + r(dlogits @ wr.T))

    for name, got, want in (("y", y, ry), ("dx", tx.grad(), dx), ("dw1", tw1.grad(), dw1), ("dw2", tw2.grad(), dw2), ("dwr", twr.grad(), dwr)):
        assert np.linalg.norm(want) > 0, name   # (a gradient that is identically zero would meet any relative bound)
        err = rel_fro(from_t(got), want)
        print(f"moe layer {name}: relative Frobenius error {err:.3e}")
        assert err <= 1.5e-2, (name, err)
    for e in range(E):
        if offsets[e] == offsets[e + 1]:
            assert not from_t(tw1.grad())[e].any()


def test_the_captured_forward_follows_the_router_on_replay():
    x, wr, w1, w2, _, wr_new = draw()
    tx, twr, tw1, tw2 = (to_t(v) for v in (x, wr, w1, w2))
    for _ in range(2):                                   # warms the allocator
        y, plan = layer(tx, twr, tw1, tw2)
    kfunca.synchronize(0)
    ids_old, y_old = plan.ids.numpy().copy(), bits(y)
    kfunca.graph_begin(0)
    yg, plan_g = layer(tx, twr, tw1, tw2)                # recorded, not run
    graph = kfunca.graph_end(0)
    kfunca.graph_launch(graph, 0)
    kfunca.synchronize(0)
    assert np.array_equal(bits(yg), y_old)
    # new router weights in the same storage: other experts win
    new_bits = np.ascontiguousarray(V.encode(wr_new, "bf16"))
    H.check(H.lib().kf_memcpy_h2d(twr.data_ptr(), new_bits.ctypes.data, new_bits.nbytes, None))
    H.device_sync()
    kfunca.graph_launch(graph, 0)
    kfunca.synchronize(0)
    replay, ids_replay = bits(yg), plan_g.ids.numpy().copy()
    y_new, plan_new = layer(tx, twr, tw1, tw2)           # eager, on the new weights
    kfunca.synchronize(0)
    assert not np.array_equal(plan_new.ids.numpy(), ids_old), "the new router picks the same experts: the test shows nothing"
    assert np.array_equal(ids_replay, plan_new.ids.numpy())
    assert np.array_equal(replay, bits(y_new)) and not np.array_equal(replay, y_old)
    kfunca.graph_destroy(graph)
