"""-m gpu: kf_delta_rule_step against the float64 recurrence of tests/delta_rule_ref.py from a random state, the state updated in place, o
and the state between 64 untouched guard elements.
The bound is in f32 terms (2^-23 bounds a rounding twice over), per head and normwise. A step does to a state element: exp(g_t) and
the product with it (3 roundings); k S', Dk / 16 fused multiply-adds in the lane and 15 additions over the row groups, each on terms
whose magnitudes sum to at most |k|_1 max|S| <= sqrt(Dk) max|S| for a unit k; v - k S' and the product with beta (4 on that scale); one
fused multiply-add of k u. That is n = (sqrt(Dk) (Dk / 16 + 15) + 8) / 2 roundings of 2^-23 a step - 80 at Dk 64, 134 at Dk 128 - and
the recurrence does not amplify what it carries (it is contractive for beta |k|^2 <= 1):
  state: max|got - ref| <= n T 2^-23 max|ref|,   o: max|got - ref| <= 2^-8 max|ref o| + (n T + Dk) 2^-23 max|ref state|
(o's own sums are fewer than Dk, and scale |q|_1 <= 1 for a unit q and the default scale; then o's one rounding to 16 bits)."""
import numpy as np
import pytest

from tests.delta_rule_ref import C, CASES, U, cut, fwd, random_case, reference, step, worst

pytestmark = pytest.mark.gpu
N_ROUND = {64: 80, 128: 134}


def check(o, s, ro, rs, T, D):
    ax = (1, 2)
    eo = np.abs(o - ro).max(ax) - (U * np.abs(ro).max(ax) + (N_ROUND[D] * T + D) * 2.0 ** -23 * np.abs(rs).max(ax))
    print("state error over n T 2^-23 max|ref|:", worst(s, rs) / (N_ROUND[D] * T * 2.0 ** -23), "worst excess of o (<= 0 passes):", eo.max())
    assert worst(s, rs) <= N_ROUND[D] * T * 2.0 ** -23 and eo.max() <= 0


# T: one token / a handful / a full batch of 16 steps / one more / two batches and a tail
@pytest.mark.parametrize("T", [1, 5, 16, 17, 40])
@pytest.mark.parametrize("dt,D", CASES)
def test_step(dt, D, T):
    x, h0, scale, _ = random_case(dt, 2, 192, D)
    x, state = cut(x, 0, T), 8 * h0   # a state of the operands' size
    if T == 5:
        x["g"] = None
    o, s = step(dt, 1, 2, x, scale, state)
    check(o, s, *reference(**x, scale=scale, h0=state), T, D)
    o2, s2 = step(dt, 1, 2, x, scale, state)   # the same bits from a second call
    assert np.array_equal(o, o2) and np.array_equal(s, s2)


def test_more_workgroups_than_compute_units():
    x, h0, scale, _ = random_case("bf16", 300, 64, 128)
    x = cut(x, 0, 3)
    o, s = step("bf16", 20, 15, x, scale, h0)
    check(o, s, *reference(**x, scale=scale, h0=h0), 3, 128)


@pytest.mark.parametrize("dt,D", [("bf16", 128), ("f16", 64)])
def test_prefill_hands_over_to_decode(dt, D):
    """100 steps through the chunk kernels, then 92 token by token from their hT: within the random tier's bound of the whole's reference"""
    x, h0, scale, (ro, rs) = random_case(dt, 2, 192, D)
    o1, hT = fwd(dt, 1, 2, cut(x, 0, 100), scale, h0)
    o2, s = step(dt, 1, 2, cut(x, 100, 192), scale, hT)
    assert worst(np.concatenate([o1, o2], 1), ro) <= C * U and worst(s, rs) <= C * U
