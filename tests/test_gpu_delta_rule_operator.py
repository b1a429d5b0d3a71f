"""-m gpu: kfunca.gated_delta_rule and kfunca.gated_delta_rule_step through the module API against the float64 recurrence of
tests/delta_rule_ref.py, within the random tier's bound (C = 5, per head): a prefill with initial_state and return_state, then the next
tokens on the returned state, updated in place; g=None; the default scale; results without a gradient node."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from tests.delta_rule_ref import C, U, cut, random_case, reference, worst

pytestmark = pytest.mark.gpu
B, Hh = 1, 2


def to_t(a, dt):
    t = kfunca.from_numpy(np.ascontiguousarray(a.reshape((B, Hh) + a.shape[1:]), np.float32), 0)
    return t if dt == "f32" else t.bfloat16() if dt == "bf16" else t.half()


f64 = lambda t: t.contiguous().float().numpy().astype(np.float64).reshape((B * Hh,) + tuple(t.sizes())[2:])
tensors = lambda x, dt: [None if x[n] is None else to_t(x[n], "f32" if n in ("g", "beta") else dt) for n in ("q", "k", "v", "g", "beta")]


@pytest.mark.parametrize("dt,D,gate", [("bf16", 128, True), ("f16", 64, False)])
def test_prefill_then_decode(dt, D, gate):
    x, h0, scale, _ = random_case(dt, 2, 192, D)
    x = cut(x, 0, 130) if gate else {**cut(x, 0, 130), "g": None}
    ro, rs = reference(**x, scale=scale, h0=h0)
    first = tensors(cut(x, 0, 100), dt)
    for t in first:
        if t is not None:
            t.set_requires_grad(True)   # the backward is not implemented: nothing may claim a gradient
    o1, state = kfunca.gated_delta_rule(*first, initial_state=to_t(h0, "f32"), return_state=True)
    assert not o1.requires_grad() and not state.requires_grad()
    o2 = kfunca.gated_delta_rule_step(*tensors(cut(x, 100, 130), dt), state)   # the default scale is D ** -0.5
    assert worst(np.concatenate([f64(o1), f64(o2)], 1), ro) <= C * U and worst(f64(state), rs) <= C * U   # updated in place
    whole = kfunca.gated_delta_rule(*tensors(x, dt), scale=scale, initial_state=to_t(h0, "f32"))
    assert worst(f64(whole), ro) <= C * U
