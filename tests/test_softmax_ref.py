"""CPU-only: the f64 reference of tests/softmax_ref.py equals torch-CPU f64 softmax / log_softmax and their autograd, its special values
are torch's, and the bounds of the GPU tests reject wrong formulas on the GPU tests' own input draws."""
import numpy as np
import pytest
import torch

from tests import softmax_ref as R

TORCH = {R.SOFTMAX: torch.softmax, R.LOG_SOFTMAX: torch.log_softmax}


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("logits", R.LOGITS)
def test_reference_equals_torch_f64(kind, scale, logits):
    rng = np.random.default_rng(5)
    x = R.floats(R.draw_logits(rng, logits, R.F32, 6, 257), R.F32)
    dy = R.floats(R.draw_dy(rng, "huge", R.F32, 6, 257), R.F32)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ty = TORCH[kind](t * scale, dim=-1)
    ty.backward(torch.tensor(dy, dtype=torch.float64))
    y, lse = R.forward(kind, x, scale)
    assert np.abs(y - ty.detach().numpy()).max() <= 1e-12
    assert np.abs(lse[:, 0] - torch.logsumexp(t.detach() * scale, dim=-1).numpy()).max() <= 1e-12 * np.abs(lse).max()
    dx = R.backward(kind, y, dy, scale)
    want = t.grad.numpy()
    assert np.abs(dx - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def special_rows():
    """Rows: clean, some -inf, all -inf, a NaN, a +inf, clean."""
    x = np.random.default_rng(2).normal(0, 1, (6, 9))
    x[1, [0, 4]] = -np.inf
    x[2, :] = -np.inf
    x[3, 5] = np.nan
    x[4, 2] = np.inf
    return x


@pytest.mark.parametrize("kind", R.KINDS)
def test_special_values_are_torchs(kind):
    x = special_rows()
    dy = np.random.default_rng(3).normal(0, 1, x.shape)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ty = TORCH[kind](t, dim=-1)
    ty.backward(torch.tensor(dy))
    y, _ = R.forward(kind, x, 1.0)
    assert np.array_equal(np.isnan(y), np.isnan(ty.detach().numpy())) and np.array_equal(np.isinf(y), np.isinf(ty.detach().numpy()))
    fin = np.isfinite(y)
    assert np.abs(y[fin] - ty.detach().numpy()[fin]).max() <= 1e-12
    # the rules, said out loud
    assert np.isnan(y[[2, 3, 4]]).all() and np.isfinite(y[[0, 5]]).all()
    assert (y[1, [0, 4]] == (0.0 if kind == R.SOFTMAX else -np.inf)).all() and np.isfinite(np.delete(y[1], [0, 4])).all()
    dx = R.backward(kind, y, dy, 1.0)
    want = t.grad.numpy()
    assert np.array_equal(np.isnan(dx), np.isnan(want))
    assert np.abs(dx[np.isfinite(want)] - want[np.isfinite(want)]).max() <= 1e-12
    if kind == R.SOFTMAX:
        assert (dx[1, [0, 4]] == 0.0).all()   # no gradient reaches a -inf logit through softmax


# ---- the bounds reject wrong formulas ----------------------------------------------------------------------------------------------
def leaves(err, tol):
    return bool((~(err <= tol)).any())   # a NaN leaves the bound too


@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_bounds_reject_wrong_formulas_on_the_gpu_tests_draws(code, kind):
    for rows, V in R.value_shapes():
        for logits, scale, dyk in R.value_cases():
            rng = np.random.default_rng(V + 7 * code)
            x = R.floats(R.draw_logits(rng, logits, code, rows, V), code)
            dy = R.floats(R.draw_dy(rng, dyk, code, rows, V), code)
            what = (rows, V, logits, scale, dyk)
            y, lse = R.forward(kind, x, scale)
            assert np.isfinite(y).all(), what
            sc = float(np.float32(scale))
            if logits == "large":
                # the forward without the max subtraction, in f32 as a kernel would: exp overflows
                with np.errstate(over="ignore", invalid="ignore"):
                    s = (x * sc).astype(np.float32)
                    e = np.exp(s)
                    naive = e / e.sum(axis=-1, keepdims=True) if kind == R.SOFTMAX else s - np.log(e.sum(axis=-1, keepdims=True))
                assert leaves(np.abs(naive.astype(np.float64) - y), R.forward_bound(kind, code, y, lse)), ("no max subtraction", what)
            ys = R.floats(R.bits(y, code), code)   # the stored result the backward reads
            ref = R.backward(kind, ys, dy, scale)
            tol = R.backward_bound(kind, code, ys, dy, scale, ref)
            assert not leaves(np.abs(ref - ref), tol)
            rowsum = (dy * ys).sum(-1, keepdims=True) if kind == R.SOFTMAX else dy.sum(-1, keepdims=True)
            no_sum = sc * ys * dy if kind == R.SOFTMAX else sc * dy
            assert leaves(np.abs(no_sum - ref), tol), ("row sum dropped", what)
            if scale != 1.0:
                assert leaves(np.abs(ref / sc - ref), tol), ("scale forgotten", what)
            if kind == R.LOG_SOFTMAX:
                assert leaves(np.abs(sc * (dy - ys * rowsum) - ref), tol), ("y in place of exp(y)", what)
