"""-m gpu: the mixture-of-experts layer of tests/test_gpu_moe_layer.py with the fused router in front and the auxiliary loss beside it,

    gemm -> moe_route -> moe_plan -> moe_dispatch -> expert_linear -> swiglu -> expert_linear -> moe_combine -> cross_entropy
         \\-> moe_aux_loss(logits, plan)                                                       total = cross_entropy + aux

against an f64 numpy restatement that rounds to bf16 wherever an operator stores (the expert ids are taken from the device run, as that
test does), relative Frobenius error of y, dx, dw1, dw2 and dwr <= 1.5e-2: that test's own tolerance. logits feeds two consumers, so
its two gradients meet in the engine's ordinary fan-in sum. Then the router and the aux forward are captured in a graph, logits is
overwritten in place so that other experts win, and the replay must equal an eager run on the new logits bit for bit."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle.block_ref import r16, rel_fro
from tests import gemm_views as V
from tests import moe_ref as M
from tests import moe_router_ref as R

pytestmark = pytest.mark.gpu

T, D, E, K, F = 96, 128, 8, 2, 128
BALANCE_COEF, Z_COEF = 0.1, 0.01       # ten times the usual: the aux gradient is a third of the router's, so dwr shows it


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


def route(logits):
    ids, gate = kfunca.moe_route(logits, K)                                # softmax, normalised over the chosen k
    plan = kfunca.moe_plan(ids, E)
    aux = kfunca.moe_aux_loss(logits, plan, balance_coef=BALANCE_COEF, z_coef=Z_COEF)
    return gate, plan, aux


def layer(tx, twr, tw1, tw2):
    logits = kfunca.gemm(tx, twr, 1.0, 0.0)                                # [T, E]
    gate, plan, aux = route(logits)
    xs = kfunca.moe_dispatch(tx, plan)                                     # [T k, d]
    a = kfunca.swiglu(kfunca.expert_linear(xs, tw1, plan.offsets))         # [T k, F]
    ys = kfunca.expert_linear(a, tw2, plan.offsets)                        # [T k, d]
    return kfunca.moe_combine(ys, plan, gate), plan, aux


def draw():
    rng = np.random.default_rng(23)
    x, wr = r(rng.uniform(-1, 1, (T, D))), r(rng.uniform(-1, 1, (D, E)) * 0.3)
    w1, w2 = r(rng.uniform(-1, 1, (E, D, 2 * F)) * 0.15), r(rng.uniform(-1, 1, (E, F, D)) * 0.15)
    target = rng.integers(0, D, T).astype(np.int64)
    return x, wr, w1, w2, target


def test_layer_with_the_fused_router_and_the_aux_loss_against_the_rounded_f64_restatement():
    x, wr, w1, w2, target = draw()
    tx, twr, tw1, tw2 = (to_t(v, True) for v in (x, wr, w1, w2))
    y, plan, aux = layer(tx, twr, tw1, tw2)
    ce = kfunca.cross_entropy(y, kfunca.from_numpy(target, 0))
    total = ce + aux
    total.backward(kfunca.from_numpy(np.ones(1, np.float32), 0))
    ids = plan.ids.numpy().astype(np.int64)
    assert ids.shape == (T, K) and ((ids >= 0) & (ids < E)).all()

    offsets, row_pair, pair_row = M.plan(ids, E)
    assert np.array_equal(plan.offsets.numpy(), offsets) and np.array_equal(plan.row_pair.numpy(), row_pair)
    pr, token = pair_row.reshape(T, K).astype(np.int64), row_pair.astype(np.int64) // K
    seg = [slice(int(offsets[e]), int(offsets[e + 1])) for e in range(E)]
    counts = np.diff(offsets)

    # forward
    logits = r(x @ wr)
    rgate = r(R.gate(logits, ids, R.SOFTMAX, True))
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
    ry = r(sum(rgate[:, j, None] * rys[pr[:, j]] for j in range(K)))
    # the two losses
    ey = np.exp(ry - ry.max(1, keepdims=True))
    py = ey / ey.sum(1, keepdims=True)
    ce_ref = float(-np.log(py[np.arange(T), target]).mean())
    aux_ref = R.aux_forward(logits, counts, K, BALANCE_COEF, Z_COEF)[0]
    assert abs(float(ce.numpy()[0]) - ce_ref) <= 1e-3 * abs(ce_ref)
    assert abs(float(aux.numpy()[0]) - aux_ref) <= R.loss_bound(aux_ref)
    assert abs(float(total.numpy()[0]) - (ce_ref + aux_ref)) <= 1e-3 * abs(ce_ref + aux_ref)
    # backward
    onehot = np.zeros((T, D))
    onehot[np.arange(T), target] = 1.0
    dy = r((py - onehot) / T)
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
    dl_router = r(R.router_backward(logits, ids, dgate, R.SOFTMAX, True))
    dl_aux = r(R.aux_backward(logits, counts, K, BALANCE_COEF, Z_COEF, 1.0))
    assert np.linalg.norm(dl_aux) > 1e-3 * np.linalg.norm(dl_router), "the aux gradient is too small to show in dwr"
    dlogits = r(dl_router + dl_aux)                                        # the engine's fan-in sum, stored in bf16
    dwr = r(x.T @ dlogits)
    dx = r(dx_experts + r(dlogits @ wr.T))

    for name, got, want in (("y", y, ry), ("dx", tx.grad(), dx), ("dw1", tw1.grad(), dw1), ("dw2", tw2.grad(), dw2), ("dwr", twr.grad(), dwr)):
        assert np.linalg.norm(want) > 0, name
        err = rel_fro(from_t(got), want)
        print(f"moe router layer {name}: relative Frobenius error {err:.3e}")
        assert err <= 1.5e-2, (name, err)
    # without the aux term dwr is another matrix: the bound above does see it
    assert rel_fro(r(x.T @ dl_router), dwr) > 1.5e-2


def test_the_captured_router_and_aux_forward_follow_the_logits_on_replay():
    x, wr, _, _, _ = draw()
    rng = np.random.default_rng(5)
    logits_new = r(rng.uniform(-1, 1, (T, E)))
    tl = to_t(r(x @ wr))
    for _ in range(2):                                   # warms the allocator
        gate, plan, aux = route(tl)
    kfunca.synchronize(0)
    old = (bits(gate), plan.ids.numpy().copy(), aux.numpy().copy())
    kfunca.graph_begin(0)
    gate_g, plan_g, aux_g = route(tl)                    # recorded, not run
    graph = kfunca.graph_end(0)
    kfunca.graph_launch(graph, 0)
    kfunca.synchronize(0)
    assert np.array_equal(bits(gate_g), old[0]) and np.array_equal(plan_g.ids.numpy(), old[1]) and aux_g.numpy().tobytes() == old[2].tobytes()
    new_bits = np.ascontiguousarray(V.encode(logits_new, "bf16"))
    H.check(H.lib().kf_memcpy_h2d(tl.data_ptr(), new_bits.ctypes.data, new_bits.nbytes, None))
    H.device_sync()
    kfunca.graph_launch(graph, 0)
    kfunca.synchronize(0)
    replay = (bits(gate_g), plan_g.ids.numpy().copy(), plan_g.offsets.numpy().copy(), aux_g.numpy().copy())
    gate_n, plan_n, aux_n = route(tl)                    # eager, on the new logits
    kfunca.synchronize(0)
    assert not np.array_equal(plan_n.ids.numpy(), old[1]), "the new logits pick the same experts: the test shows nothing"
    assert np.array_equal(replay[1], plan_n.ids.numpy()) and np.array_equal(replay[2], plan_n.offsets.numpy())
    assert np.array_equal(replay[0], bits(gate_n)) and replay[3].tobytes() == aux_n.numpy().tobytes()
    assert replay[3].tobytes() != old[2].tobytes()
    kfunca.graph_destroy(graph)
