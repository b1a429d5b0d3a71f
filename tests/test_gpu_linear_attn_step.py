"""-m gpu: kf_linear_attn_step against the float64 recurrence of tests/linear_attn_state_ref.py on the inputs as stored, o and the state
between 64 untouched guard elements, o filled with 0xA5.
Bounds, from the operations the kernel issues, all in f32 (2^-23 bounds a rounding twice over): a state element takes per step exp(g_t)
(one ulp), the product with it and one fused multiply-add of k v - under the 4 T 2^-23 of absref the issue sets; o adds Dk / 16 fused
multiply-adds in the lane, 15 additions over the row groups and the product with scale, fewer than Dk, then its one rounding to 16 bits:
  state: |got - ref| <= 4 T 2^-23 absref,   o: |got - ref| <= u |ref| + (Dk + 4 T) 2^-23 absref,   u = 2^-8."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests.linear_attn_state_ref import U, bound, reference, step_reference

pytestmark = pytest.mark.gpu
CODE, GUARD = {"bf16": H.BF16, "f16": H.F16}, 64


def draw(dt, N, T, D):
    rng = np.random.default_rng(N + T + D)
    x = {n: V.decode(V.encode(rng.uniform(-1, 1, (N, T, D)), dt), dt) for n in ("q", "k", "v")}
    x["g"] = -rng.uniform(0, 0.05, (N, T)).astype(np.float32).astype(np.float64)
    return x, rng.uniform(-1, 1, (N, D, D)).astype(np.float32).astype(np.float64), float(np.float32(D ** -0.5))


def step(dt, B, Hh, x, scale, state):
    N, T, D = x["q"].shape
    dev = [H.DevBuf.from_numpy(V.encode(x[n], dt)) for n in ("q", "k", "v")] + [H.DevBuf.from_numpy(x["g"].astype(np.float32))]
    st = np.full(N * D * D + 2 * GUARD, np.float32(-7.0))
    st[GUARD:-GUARD] = state.ravel()
    bst, bo = H.DevBuf.from_numpy(st.astype(np.float32)), H.DevBuf.from_numpy(np.full((N * T * D + 2 * GUARD) * 2, 0xA5, np.uint8))
    H.linear_attn_step(CODE[dt], B, Hh, T, D, D, scale, *(b.ptr for b in dev), bst.ptr + GUARD * 4, bo.ptr + GUARD * 2)
    st, o = bst.to_numpy(st.shape, np.float32), bo.to_numpy((N * T * D + 2 * GUARD,), np.uint16)
    assert (st[:GUARD] == -7).all() and (st[-GUARD:] == -7).all() and (o[:GUARD] == 0xA5A5).all() and (o[-GUARD:] == 0xA5A5).all(), "guard written"
    return V.decode(o[GUARD:-GUARD].copy(), dt).reshape(N, T, D), st[GUARD:-GUARD].astype(np.float64).reshape(N, D, D)


# T: one token / a handful / more than four batches of 16 steps with a tail; B H: fewer workgroups than compute units and more
@pytest.mark.parametrize("B,Hh", [(1, 2), (20, 15)])
@pytest.mark.parametrize("T", [1, 3, 70])
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)])
def test_step(dt, D, T, B, Hh):
    x, state, scale = draw(dt, B * Hh, T, D)
    o, s = step(dt, B, Hh, x, scale, state)
    (ro, rs), (ao, as_) = step_reference(x["q"], x["k"], x["v"], x["g"], scale, state)
    eo, es = np.abs(o - ro) - (U * np.abs(ro) + (D + 4 * T) * 2.0 ** -23 * ao), np.abs(s - rs) - 4 * T * 2.0 ** -23 * as_
    print("worst excess over the bound (<= 0 passes): o", eo.max(), "state", es.max())
    assert eo.max() <= 0 and es.max() <= 0
    if B * Hh == 2:   # the same bits from a second call
        o2, s2 = step(dt, B, Hh, x, scale, state)
        assert np.array_equal(o, o2) and np.array_equal(s, s2)


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("f16", 64)])
def test_prefill_hands_over_to_decode(dt, D):
    """70 steps from a random state, token by token and through the chunk kernels, agree within the sum of the two routes' bounds"""
    T = 70
    x, state, scale = draw(dt, 2, T, D)
    o, s = step(dt, 1, 2, x, scale, state)
    dev = [H.DevBuf.from_numpy(V.encode(x[n], dt)) for n in ("q", "k", "v")] + [H.DevBuf.from_numpy(a.astype(np.float32)) for a in (x["g"], state)]
    bo, bhT = H.DevBuf(2 * T * D * 2), H.DevBuf(2 * D * D * 4)
    H.linear_attn_state_fwd(CODE[dt], 1, 2, T, D, D, scale, *(b.ptr for b in dev), bo.ptr, bhT.ptr)
    co, chT = V.decode(bo.to_numpy((2 * T * D,), np.uint16), dt).reshape(2, T, D), bhT.to_numpy((2, D, D), np.float32).astype(np.float64)
    ref, absref = reference(x["q"], x["k"], x["v"], x["g"], np.zeros_like(x["q"]), scale, state)
    assert (np.abs(o - co) <= bound(ref["o"], absref["o"], T, 2) + U * np.abs(ref["o"]) + (D + 4 * T) * 2.0 ** -23 * absref["o"]).all()
    assert (np.abs(s - chT) <= bound(ref["hT"], absref["hT"], T, 2) + 4 * T * 2.0 ** -23 * absref["hT"]).all()
