"""-m gpu: kfunca.expert_linear - output, dx and dw against the f64 reference of the rounded inputs within the bounds of
tests/test_gpu_gemm_seg.py (|got - ref| <= 2^-8 |ref| + K 2^-23 sum_k |a_k b_k| for bf16, 2^-23 |ref| as the first term for f32; K the
contraction length, the segment's length for dw), and one mixture-of-experts layer end to end through the operator API against an f64
numpy restatement that rounds to bf16 at the operator boundaries (as oracle/block_ref.py does), relative Frobenius error <= 1.5e-2."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from oracle.block_ref import r16, rel_fro
from tests import gemm_seg_ref as R
from tests import gemm_views as V

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "empty expert": (300, [0, 1, 129, 129, 300]),
    "uncovered tail": (400, [37, 165, 165, 390]),
}


def to_t(vals, dt, requires_grad=False):
    """f64 values (already representable in dt) -> a device tensor of dt."""
    if dt == "bf16":
        t = kfunca.from_numpy_bf16(np.ascontiguousarray(V.encode(vals, "bf16")), 0)
    else:
        t = kfunca.from_numpy(np.ascontiguousarray(vals, dtype=np.float32), 0)
    t.set_requires_grad(requires_grad)
    return t


def from_t(t, dt):
    a = np.ascontiguousarray(t.numpy())
    return V.decode(a.view(np.uint16), "bf16") if dt == "bf16" else a.astype(np.float64)


def rounded(rng, shape, dt):
    return V.decode(V.encode(rng.uniform(-1, 1, shape), dt), dt)


def within(got, ref, absref, K, dt, what):
    lim = (2.0 ** -23 if dt == "f32" else 2.0 ** -8) * np.abs(ref) + K * 2.0 ** -23 * absref
    print(f"{what}: max excess over the bound {(np.abs(got - ref) - lim).max():.3e}")
    assert (np.abs(got - ref) <= lim).all(), what


@pytest.mark.parametrize("dt,Din,Dout", [("bf16", 128, 256), ("f32", 128, 256), ("bf16", 40, 72)])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_output_and_gradients(layout, dt, Din, Dout):
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    rng = np.random.default_rng(T + Din + len(dt))
    x, w, dy = rounded(rng, (T, Din), dt), rounded(rng, (E, Din, Dout), dt), rounded(rng, (T, Dout), dt)
    tx, tw = to_t(x, dt, True), to_t(w, dt, True)
    toff = kfunca.from_numpy(np.asarray(offsets, dtype=np.int64), 0)
    y = kfunca.expert_linear(tx, tw, toff)
    assert y.sizes() == [T, Dout]
    y.backward(to_t(dy, dt))
    owner = R.row_expert(offsets, T)
    got_y, got_dx, got_dw = from_t(y, dt), from_t(tx.grad(), dt), from_t(tw.grad(), dt)
    within(got_y, R.forward(x, w, offsets), R.abs_forward(x, w, offsets), Din, dt, "y")
    wt = np.swapaxes(w, 1, 2)
    within(got_dx, R.forward(dy, wt, offsets), R.abs_forward(dy, wt, offsets), Dout, dt, "dx")
    lens = np.diff(R.sanitize(offsets, T)).astype(np.float64)[:, None, None]
    within(got_dw, R.wgrad(x, dy, offsets), R.abs_wgrad(x, dy, offsets), lens, dt, "dw")
    # a row no expert covers: a zero output and a zero gradient; an empty expert: a zero weight gradient
    assert not got_y[owner < 0].any() and not got_dx[owner < 0].any()
    for e in range(E):
        if not (owner == e).any():
            assert not got_dw[e].any()
    assert not toff.requires_grad()


def test_a_row_pitched_input_is_read_in_place():
    T, offsets = LAYOUTS["empty expert"]
    rng = np.random.default_rng(5)
    wide, w = rounded(rng, (T, 256), "bf16"), rounded(rng, (4, 128, 256), "bf16")
    toff = kfunca.from_numpy(np.asarray(offsets, dtype=np.int64), 0)
    a = kfunca.expert_linear(to_t(wide, "bf16")[:, 128:], to_t(w, "bf16"), toff)
    b = kfunca.expert_linear(to_t(np.ascontiguousarray(wide[:, 128:]), "bf16"), to_t(w, "bf16"), toff)
    assert np.array_equal(a.numpy(), b.numpy())


@pytest.mark.parametrize("accum_f32", [False, True])
def test_a_bucketed_weight_takes_its_gradient_in_the_bucket(accum_f32):
    """A weight in a GradBucket: the first pass writes dw into its slot (a bf16 bucket: straight from the kernel; an f32 bucket: the
    rounded gradient converted), a second pass without zero_grad adds to it - the values of the unbucketed run, then twice them."""
    T, offsets = LAYOUTS["empty expert"]
    rng = np.random.default_rng(23)
    x, w, dy = rounded(rng, (T, 128), "bf16"), rounded(rng, (4, 128, 256), "bf16"), rounded(rng, (T, 256), "bf16")
    toff = kfunca.from_numpy(np.asarray(offsets, dtype=np.int64), 0)
    plain = to_t(w, "bf16", True)
    kfunca.expert_linear(to_t(x, "bf16"), plain, toff).backward(to_t(dy, "bf16"))
    want = from_t(plain.grad(), "bf16")
    assert want.any()
    tw = to_t(w, "bf16", True)
    bucket = kfunca.GradBucket([tw], 1.0, accum_f32)
    bucket.attach()
    for times in (1.0, 2.0):
        kfunca.expert_linear(to_t(x, "bf16"), tw, toff).backward(to_t(dy, "bf16"))
        bucket.wait()
        got = from_t(tw.grad(), "f32" if accum_f32 else "bf16")
        assert np.array_equal(got, times * want), f"pass {int(times)}"
    bucket.detach()


def test_refuses():
    x = kfunca.from_numpy(np.zeros((8, 4), np.float32), 0)
    w = kfunca.from_numpy(np.zeros((2, 4, 6), np.float32), 0)
    off = kfunca.from_numpy(np.array([0, 4, 8], np.int64), 0)
    assert kfunca.expert_linear(x, w, off).sizes() == [8, 6]
    for bad in ((x, w, kfunca.from_numpy(np.array([0, 8], np.int64), 0)), (x, w, kfunca.from_numpy(np.array([0, 4, 8], np.int32), 0)),
                (x, kfunca.from_numpy(np.zeros((2, 5, 6), np.float32), 0), off), (x, w.bfloat16(), off),
                (kfunca.from_numpy(np.zeros((8, 4), np.float64), 0), kfunca.from_numpy(np.zeros((2, 4, 6), np.float64), 0), off)):
        with pytest.raises(RuntimeError):
            kfunca.expert_linear(*bad)


# ---- one MoE layer end to end ----------------------------------------------------------------------------------------------------------
def silu(g):
    return g / (1.0 + np.exp(-g))


def dsilu(g):
    s = 1.0 / (1.0 + np.exp(-g))
    return s + g * s * (1.0 - s)


def r(x):
    return r16(np.asarray(x, dtype=np.float32)).astype(np.float64)


def test_moe_layer_end_to_end():
    T, d, E, k, F = 96, 128, 8, 2, 128
    rng = np.random.default_rng(17)
    x, wr = r(rng.uniform(-1, 1, (T, d))), r(rng.uniform(-1, 1, (d, E)) * 0.3)
    w1, w2 = r(rng.uniform(-1, 1, (E, d, 2 * F)) * 0.15), r(rng.uniform(-1, 1, (E, F, d)) * 0.15)
    dy = r(rng.uniform(-1, 1, (T, d)))
    tx, twr, tw1, tw2 = (to_t(v, "bf16", True) for v in (x, wr, w1, w2))

    # the layer, from operators: router, top-k, the permutation (built on the host), gather, two expert products, weighted combine
    p = kfunca.softmax(kfunca.gemm(tx, twr, 1.0, 0.0))                     # [T, E]
    ids = p.topk(k, -1, True)[1].numpy().astype(np.int64)                  # [T, k]
    flat = ids.reshape(-1)
    order = np.argsort(flat, kind="stable")                                # sorted row s holds pair order[s] = t * k + j
    keys, token = flat[order], order // k
    inv = np.empty(T * k, dtype=np.int64)
    inv[order] = np.arange(T * k)
    dev = lambda a: kfunca.from_numpy(np.ascontiguousarray(a, dtype=np.int64), 0)  # noqa: E731
    offsets = kfunca.segment_offsets(dev(keys), E)
    assert np.array_equal(offsets.numpy(), R.segment_offsets(keys, E))
    gate = kfunca.embedding(p.view(T * E, 1), dev(token * E + keys))       # [T k, 1], differentiable in p
    xs = kfunca.embedding(tx, dev(token))                                  # [T k, d]
    a = kfunca.swiglu(kfunca.expert_linear(xs, tw1, offsets))              # [T k, F]
    ys = kfunca.expert_linear(a, tw2, offsets)                             # [T k, d]
    yg = ys * gate
    y = kfunca.embedding(yg, dev(inv.reshape(T, k)[:, 0])) + kfunca.embedding(yg, dev(inv.reshape(T, k)[:, 1]))
    y.backward(to_t(dy, "bf16"))

    # the same in f64 numpy, rounded to bf16 wherever an operator stores
    so = R.segment_offsets(keys, E)
    seg = [slice(int(so[e]), int(so[e + 1])) for e in range(E)]
    logits = r(x @ wr)
    ex = np.exp(logits - logits.max(1, keepdims=True))
    rp = r(ex / ex.sum(1, keepdims=True))
    rgate = rp[token, keys][:, None]
    rxs = x[token]
    rh = np.zeros((T * k, 2 * F))
    for e in range(E):
        rh[seg[e]] = rxs[seg[e]] @ w1[e]
    rh = r(rh)
    hg, hu = rh[:, :F], rh[:, F:]
    ra = r(silu(hg) * hu)
    rys = np.zeros((T * k, d))
    for e in range(E):
        rys[seg[e]] = ra[seg[e]] @ w2[e]
    rys = r(rys)
    ryg = r(rys * rgate)
    ry = r(ryg[inv.reshape(T, k)[:, 0]] + ryg[inv.reshape(T, k)[:, 1]])
    # backward
    dyg = dy[token]                                                        # every sorted row is gathered exactly once
    dys = r(dyg * rgate)
    dgate = r(r(dyg * rys).sum(1, keepdims=True))
    da, dw2 = np.zeros((T * k, F)), np.zeros_like(w2)
    for e in range(E):
        da[seg[e]] = dys[seg[e]] @ w2[e].T
        dw2[e] = ra[seg[e]].T @ dys[seg[e]]
    da, dw2 = r(da), r(dw2)
    dh = r(np.concatenate([da * hu * dsilu(hg), da * silu(hg)], 1))
    dxs, dw1 = np.zeros((T * k, d)), np.zeros_like(w1)
    for e in range(E):
        dxs[seg[e]] = dh[seg[e]] @ w1[e].T
        dw1[e] = rxs[seg[e]].T @ dh[seg[e]]
    dxs, dw1 = r(dxs), r(dw1)
    dx_experts = np.zeros((T, d))
    np.add.at(dx_experts, token, dxs)
    dx_experts = r(dx_experts)
    dp = np.zeros((T, E))
    dp[token, keys] = dgate[:, 0]
    dlogits = r(rp * (dp - (dp * rp).sum(1, keepdims=True)))
    dwr = r(x.T @ dlogits)
    dx = r(dx_experts + r(dlogits @ wr.T))

    for name, got, want in (("y", y, ry), ("dx", tx.grad(), dx), ("dw1", tw1.grad(), dw1), ("dw2", tw2.grad(), dw2), ("dwr", twr.grad(), dwr)):
        assert np.linalg.norm(want) > 0, name   # (a gradient that is identically zero would meet any relative bound)
        err = rel_fro(from_t(got, "bf16"), want)
        print(f"moe layer {name}: relative Frobenius error {err:.3e}")
        assert err <= 1.5e-2, (name, err)
    empty = [e for e in range(E) if so[e] == so[e + 1]]
    for e in empty:
        assert not from_t(tw1.grad(), "bf16")[e].any()
