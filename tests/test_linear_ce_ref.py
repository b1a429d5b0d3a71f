"""CPU: the f64 reference of the chunked linear + cross-entropy loss (tests/linear_ce_ref.py) against torch-CPU autograd on
F.cross_entropy(F.linear(x, W)) + z * mean-or-sum(lse^2) in float64, to 1e-10; chunking the reference changes nothing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import linear_ce_ref as R

CASES = [dict(), dict(ignore=True), dict(eps=0.1), dict(z=1e-3), dict(ignore=True, eps=0.1, z=1e-3), dict(ignore=True, eps=1.0, z=0.5)]


def problem(seed, T=37, V=53, d=11, ignore=False):
    rng = np.random.default_rng(seed)
    x, W = rng.normal(0, 1.0, (T, d)), rng.normal(0, 0.7, (V, d))
    t = rng.integers(0, V, T)
    if ignore:
        t[rng.random(T) < 0.25] = -100
        t[0] = -100
    return x, W, t


def torch_side(x, W, t, reduction, eps, z, g):
    tx, tw = torch.tensor(x, requires_grad=True), torch.tensor(W, requires_grad=True)
    logits = F.linear(tx, tw)
    tt = torch.tensor(t)
    loss = F.cross_entropy(logits, tt, ignore_index=-100, reduction=reduction, label_smoothing=eps)
    keep = tt != -100
    lse2 = (torch.logsumexp(logits, 1) ** 2)[keep]
    loss = loss + z * (lse2.mean() if reduction == "mean" else lse2.sum())
    (loss * g).backward()
    return loss.item(), tx.grad.numpy(), tw.grad.numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_matches_torch_autograd(reduction, case):
    kw = dict(CASES[case])
    x, W, t = problem(100 + case, ignore=kw.pop("ignore", False))
    eps, z, g = kw.get("eps", 0.0), kw.get("z", 0.0), 1.7
    want_loss, want_dx, want_dw = torch_side(x, W, t, reduction, eps, z, g)
    got = R.linear_ce(x, W, t, reduction=reduction, eps=eps, z=z, g=g)
    assert got["count"] == (t != -100).sum()
    assert abs(got["loss"] - want_loss) <= 1e-10 * max(1.0, abs(want_loss))
    np.testing.assert_allclose(got["dX"], want_dx, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(got["dW"], want_dw, rtol=1e-10, atol=1e-10)
    # the bounds' sums dominate the gradients they bound
    assert (got["abs_dX"] >= np.abs(got["dX"]) - 1e-12).all() and (got["abs_dW"] >= np.abs(got["dW"]) - 1e-12).all()


@pytest.mark.parametrize("chunk", [1, 7, 16, 36, 37, 64])
def test_chunking_the_reference_changes_nothing(chunk):
    x, W, t = problem(7, ignore=True)
    whole = R.linear_ce(x, W, t, reduction="mean", eps=0.1, z=1e-3, g=0.5)
    parts = R.linear_ce(x, W, t, reduction="mean", eps=0.1, z=1e-3, g=0.5, chunk_rows=chunk)
    assert abs(whole["loss"] - parts["loss"]) <= 1e-13 * abs(whole["loss"])
    for k in ("dX", "dW", "abs_dX", "abs_dW"):
        np.testing.assert_allclose(parts[k], whole[k], rtol=1e-12, atol=1e-14)


def test_rows_semantics():
    rng = np.random.default_rng(3)
    x = rng.normal(0, 2.0, (6, 9))
    x[:, 7:] = -np.inf                      # a padded vocabulary
    t = np.array([0, 3, -100, 9, 6, -1])    # ignored, out of range (9, -1)
    lse, loss, d = R.ce_rows(x, t, z=1e-3)
    assert np.isfinite(lse).all() and loss[2] == 0.0 and not d[2].any()
    assert np.isnan(loss[[3, 5]]).all() and np.isnan(d[[3, 5]]).all() and np.isfinite(loss[[0, 1, 4]]).all()
    assert (d[[0, 1, 4]][:, 7:] == 0).all()
    # without z-loss and smoothing every kept row of the gradient sums to zero
    _, _, d0 = R.ce_rows(x, t)
    np.testing.assert_allclose(d0[[0, 1, 4]].sum(1), 0.0, atol=1e-14)
    # all rows ignored: the mean is NaN (0 / 0), the sum 0
    r = R.linear_ce(rng.normal(size=(4, 3)), rng.normal(size=(5, 3)), np.full(4, -100), reduction="mean")
    assert np.isnan(r["loss"]) and R.linear_ce(rng.normal(size=(4, 3)), rng.normal(size=(5, 3)), np.full(4, -100), reduction="sum")["loss"] == 0.0
