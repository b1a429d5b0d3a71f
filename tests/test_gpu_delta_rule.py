"""-m gpu: kf_delta_rule_fwd through the C ABI against the float64 recurrence of tests/delta_rule_ref.py on the inputs as stored, always on
outputs and a workspace filled with 0xA5 between 64 untouched guard elements.
Exact tier: one-hot keys that repeat inside and across chunks, beta in {0, 1}, q, v, h0 in {-1, 0, 1}, g = 0 (absent without a state,
zeros with one), scale 1/8 - every intermediate is a small integer, so |o - ref| <= 2^-8 |ref| (the one rounding of o) and hT == ref.
Random tier and chaining, per head: max|got - ref| <= C 2^-8 max|ref| for o and hT, C = 5 roundings to 16 bits between an operand's load
and an accumulator on the longest path: T (with its column scaling), W or Ubar, U, the decayed U fragment, the state's 16-bit copy."""
import numpy as np
import pytest

from tests.delta_rule_ref import C, CASES, U, cut, exact_case, fwd, random_case, worst

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 128, 200])
@pytest.mark.parametrize("dt,D", CASES)
def test_exact(dt, D, S, state):
    x, h0, plain, carried = exact_case(3, S, D)
    if state:
        x = {**x, "g": np.zeros(x["beta"].shape)}
    (ro, rs), (o, hT) = carried if state else plain, fwd(dt, 1, 3, x, 0.125, h0 if state else None, want_hT=state)
    assert (np.abs(o - ro) <= U * np.abs(ro)).all()
    assert not state or np.array_equal(hT, rs)


# three whole chunks / sixteen chunks with a tail of 40 steps / more workgroups than compute units
@pytest.mark.parametrize("dt,D,B,Hh,S", [(dt, D, 1, 2, S) for dt, D in CASES for S in (192, 1000)] + [("bf16", 128, 20, 15, 64)])
def test_random(dt, D, B, Hh, S):
    x, h0, scale, (ro, rs) = random_case(dt, B * Hh, S, D)
    o, hT = fwd(dt, B, Hh, x, scale, h0)
    print("error over 2^-8 max|ref|: o", worst(o, ro) / U, "hT", worst(hT, rs) / U, "bound", C)
    assert worst(o, ro) <= C * U and worst(hT, rs) <= C * U
    if S == 192:   # the same bits from a second call
        o2, hT2 = fwd(dt, B, Hh, x, scale, h0)
        assert np.array_equal(o, o2) and np.array_equal(hT, hT2)


@pytest.mark.parametrize("S1", [1, 64, 100])
@pytest.mark.parametrize("dt,D", [("bf16", 128), ("f16", 64)])
def test_chained_segments(dt, D, S1):
    """a prefill of S1 steps, then the rest from its hT: within the bound of the whole sequence's reference, as test_random holds the one call"""
    x, h0, scale, (ro, rs) = random_case(dt, 2, 192, D)
    o1, h1 = fwd(dt, 1, 2, cut(x, 0, S1), scale, h0)
    o2, h2 = fwd(dt, 1, 2, cut(x, S1, 192), scale, h1)
    assert worst(np.concatenate([o1, o2], 1), ro) <= C * U and worst(h2, rs) <= C * U
