"""-m gpu: kfunca.linear_attention with initial_state / return_state and kfunca.linear_attention_step through the module API. A sequence
is run as two segments chained through the state; one root (the two outputs and the last state, concatenated) takes the gradient, so the
first segment's o node and state node both report and the engine sums them. Everything is compared with the float64 reference of the
WHOLE sequence (tests/linear_attn_state_ref.py) within the random tier's bound, c = 2, with the bounds of the segments that feed a
value summed: the second segment's outputs and gradients see one segment, the first segment's gradients and d initial_state see both."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests.linear_attn_state_ref import bound, reference

pytestmark = pytest.mark.gpu
B, Hh = 1, 2


def to_t(a, dt, grad=True):
    t = kfunca.from_numpy(np.ascontiguousarray(a, np.float32), 0)
    t = t if dt == "f32" else t.bfloat16() if dt == "bf16" else t.half()
    t.set_requires_grad(grad)
    return t


f64 = lambda t: t.contiguous().float().numpy().astype(np.float64)
flat = lambda x: x.reshape((B * Hh,) + x.shape[2:])


def draw(S, D, dt):
    rng = np.random.default_rng(S + D)
    q, k, v, do = (V.decode(V.encode(rng.uniform(-1, 1, (B, Hh, S, D)), dt), dt) for _ in range(4))
    g = -rng.uniform(0, 0.05, (B, Hh, S)).astype(np.float32).astype(np.float64)
    h0, dhT = (V.decode(V.encode(rng.uniform(-1, 1, (B, Hh, D, D)), dt), dt) for _ in range(2))   # (d_hT passes through a 16-bit root)
    return q, k, v, g, do, h0, dhT


@pytest.mark.parametrize("S,c,D,dt", [(130, 70, 64, "bf16"), (150, 64, 128, "f16")])
def test_two_segments_have_the_gradients_of_the_whole(S, c, D, dt):
    q, k, v, g, do, h0, dhT = draw(S, D, dt)
    seg = [[to_t(x[:, :, lo:hi], dt if x is not g else "f32") for x in (q, k, v, g)] for lo, hi in ((0, c), (c, S))]
    th0 = to_t(h0, "f32")
    o1, s1 = kfunca.linear_attention(*seg[0], initial_state=th0, return_state=True)
    o2, s2 = kfunca.linear_attention(*seg[1], initial_state=s1, return_state=True)
    root = kfunca.cat([o1, o2, s2.bfloat16() if dt == "bf16" else s2.half()], 2)
    root.backward(to_t(np.concatenate([do, dhT], 2), dt, grad=False))
    ref, absref = reference(*(flat(x) for x in (q, k, v, g, do)), float(np.float32(D ** -0.5)), flat(h0), flat(dhT))
    lim = {n: bound(ref[n], absref[n], S, 2) for n in ref if n not in ("a", "b")}

    def within(name, got, n, lo, hi, segments):
        sl = (slice(None), slice(lo, hi)) if n not in ("hT", "dh0") else ()
        err = np.abs(flat(got) - ref[n][sl]) - segments * lim[n][sl]
        assert err.max() <= 0, (name, np.unravel_index(err.argmax(), err.shape), err.max())

    within("o1", f64(o1), "o", 0, c, 1), within("o2", f64(o2), "o", c, S, 2), within("hT", f64(s2), "hT", 0, S, 2)
    for i, (lo, hi) in enumerate(((0, c), (c, S))):
        for t, n in zip(seg[i], ("dq", "dk", "dv", "dg")):
            within(f"{n} of segment {i}", f64(t.grad()), n, lo, hi, 2 - i)
    within("d initial_state", f64(th0.grad()), "dh0", 0, S, 2)


def test_step_after_prefill_gives_the_next_token():
    S, D, dt = 100, 128, "bf16"
    q, k, v, g, _, h0, _ = draw(S + 1, D, dt)
    ts = [to_t(x, dt if x is not g else "f32", grad=False) for x in (q, k, v, g)]
    whole = f64(kfunca.linear_attention(*ts, initial_state=to_t(h0, "f32", grad=False)))
    _, state = kfunca.linear_attention(*(to_t(x[:, :, :S], dt if x is not g else "f32", grad=False) for x in (q, k, v, g)),
                                       initial_state=to_t(h0, "f32", grad=False), return_state=True)
    o = f64(kfunca.linear_attention_step(*(to_t(x[:, :, S:], dt if x is not g else "f32", grad=False) for x in (q, k, v, g)), state))
    ref, absref = reference(*(flat(x) for x in (q, k, v, g, np.zeros_like(q))), float(np.float32(D ** -0.5)), flat(h0))
    lim = bound(ref["o"], absref["o"], S + 1, 2)[:, S:]   # the prefill's bound covers the step's (D + 4) 2^-23
    assert (np.abs(flat(o) - ref["o"][:, S:]) <= lim).all() and (np.abs(flat(o) - flat(whole)[:, S:]) <= 2 * lim).all()
    assert (np.abs(flat(f64(state)) - ref["hT"]) <= bound(ref["hT"], absref["hT"], S + 1, 2)).all()   # updated in place


def test_without_a_state_the_call_is_the_stateless_path():
    q, k, v, g, do, _, _ = draw(130, 64, "bf16")
    out = []
    for kw in ({}, dict(initial_state=None, return_state=False)):
        ts = [to_t(x, "bf16" if x is not g else "f32") for x in (q, k, v, g)]
        o = kfunca.linear_attention(*ts, **kw)
        o.backward(to_t(do, "bf16", grad=False))
        out.append([f64(o)] + [f64(t.grad()) for t in ts])
    dev = {n: H.DevBuf.from_numpy(V.encode(x, "bf16")) for n, x in dict(q=q, k=k, v=v).items()}
    dev["g"], bo = H.DevBuf.from_numpy(g.astype(np.float32)), H.DevBuf(q.size * 2)
    H.linear_attn_fwd(H.BF16, B, Hh, 130, 64, 64, float(np.float32(0.125)), *(dev[n].ptr for n in "qkvg"), bo.ptr)
    assert np.array_equal(V.decode(bo.to_numpy((q.size,), np.uint16), "bf16").reshape(q.shape), out[0][0])   # kf_linear_attn_fwd's bits
    assert all(np.array_equal(a, b) for a, b in zip(*out))
