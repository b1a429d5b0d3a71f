"""CPU-only: the f64 numpy reference of the fused QK-norm + rotary embedding (tests/qk_norm_ref.py) against torch-CPU f64 - a manual RMS
norm per head followed by HF's rotate_half or GPT-J's rotate_every_two - forward, and backward against torch.autograd on that composition,
to 1e-12 relative."""
import numpy as np
import pytest
import torch

from tests import qk_norm_ref as R

B, S, HQ, HK, HV, D, P = 2, 5, 3, 2, 2, 16, 11
T, W = B * S, (HQ + HK + HV) * D


def rotate_half(x):
    x1, x2 = x[..., : x.shape[-1] // 2], x[..., x.shape[-1] // 2:]
    return torch.cat([-x2, x1], -1)


def rotate_every_two(x):
    x1, x2 = x[..., ::2], x[..., 1::2]
    return torch.stack([-x2, x1], -1).flatten(-2)


def torch_forward(x, wq, wk, cos, sin, pos, rot, interleaved, eps):
    """x [T, W] f64 (requires grad) -> y [T, W] by torch operators alone."""
    h = x.reshape(T, HQ + HK + HV, D)
    qk, v = h[:, :HQ + HK], h[:, HQ + HK:]
    n = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + eps)
    w = torch.cat([(torch.ones(D, dtype=torch.float64) if wq is None else wq).expand(HQ, D),
                   (torch.ones(D, dtype=torch.float64) if wk is None else wk).expand(HK, D)], 0)
    n = n * w
    if rot:
        p = torch.arange(T) % S if pos is None else pos
        c, s = cos[p][:, None, :], sin[p][:, None, :]
        if interleaved:
            c, s = c.repeat_interleave(2, -1), s.repeat_interleave(2, -1)
            r = n[..., :rot] * c + rotate_every_two(n[..., :rot]) * s
        else:
            c, s = torch.cat([c, c], -1), torch.cat([s, s], -1)
            r = n[..., :rot] * c + rotate_half(n[..., :rot]) * s
        n = torch.cat([r, n[..., rot:]], -1)
    return torch.cat([n, v], 1).reshape(T, W)


@pytest.mark.parametrize("rot", [D, D // 2, 0])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("use_pos", [False, True])
@pytest.mark.parametrize("use_w", [False, True])
def test_reference_matches_torch_f64(rot, interleaved, use_pos, use_w):
    g = torch.Generator().manual_seed(rot * 8 + interleaved * 4 + use_pos * 2 + use_w)
    x = torch.randn(T, W, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(T, W, dtype=torch.float64, generator=g)
    wq = (1 + 0.3 * torch.randn(D, dtype=torch.float64, generator=g)).requires_grad_() if use_w else None
    wk = (1 + 0.3 * torch.randn(D, dtype=torch.float64, generator=g)).requires_grad_() if use_w else None
    ang = torch.rand(P, max(rot // 2, 1), dtype=torch.float64, generator=g) * 6.0
    cos, sin = (ang.cos(), ang.sin()) if rot else (None, None)
    pos = torch.randint(0, P, (T,), generator=g) if use_pos else None
    eps = 1e-6
    y = torch_forward(x, wq, wk, cos, sin, pos, rot, interleaved, eps)
    y.backward(dy)
    num = lambda t: None if t is None else t.detach().numpy()  # noqa: E731
    args = (num(wq), num(wk), num(cos), num(sin), num(pos), B, S, HQ, HK, HV, D, rot, interleaved, eps)
    ry, tol = R.forward(num(x), *args)
    np.testing.assert_allclose(ry, num(y), rtol=1e-12, atol=1e-13)
    assert tol.shape == ry.shape and (tol[:, (HQ + HK) * D:] == 0).all() and (tol[:, : (HQ + HK) * D] > 0).all()
    np.testing.assert_array_equal(ry[:, (HQ + HK) * D:], num(x)[:, (HQ + HK) * D:])
    rb = R.backward(num(x), num(dy), *args)
    np.testing.assert_allclose(rb["dx"], num(x.grad), rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(rb["dx"][:, (HQ + HK) * D:], num(dy)[:, (HQ + HK) * D:])
    if use_w:
        np.testing.assert_allclose(rb["dwq"], num(wq.grad), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(rb["dwk"], num(wk.grad), rtol=1e-12, atol=1e-13)
    assert (rb["dwq_tol"] > 0).all() and (rb["dx_tol"][:, : (HQ + HK) * D] > 0).all()


def test_bad_position_is_nan_in_that_token_only():
    rng = np.random.default_rng(3)
    x, dy = rng.standard_normal((T, W)), rng.standard_normal((T, W))
    ang = rng.uniform(0, 6, (P, D // 4))
    pos = np.arange(T) % P
    pos[3], pos[7] = P, -1
    args = (None, None, np.cos(ang), np.sin(ang), pos, B, S, HQ, HK, HV, D, D // 2, False, 1e-6)
    y, _ = R.forward(x, *args)
    bad = np.zeros((T, HQ + HK + HV, D), bool)
    bad[[3, 7], : HQ + HK, : D // 2] = True
    np.testing.assert_array_equal(np.isnan(y), bad.reshape(T, W))
    rb = R.backward(x, dy, *args)
    bad[[3, 7], : HQ + HK, :] = True   # m is NaN: the whole head
    np.testing.assert_array_equal(np.isnan(rb["dx"]), bad.reshape(T, W))
    assert np.isnan(rb["dwq"][: D // 2]).all() and not np.isnan(rb["dwq"][D // 2:]).any()


def test_within():
    ref, tol = np.array([1.0, 2.0, np.nan, 0.0]), np.array([0.1, 0.0, 0.0, 0.0])
    assert R.within(np.array([1.05, 2.0, np.nan, 0.0]), ref, tol, 0.0) == (True, pytest.approx(0.5))
    assert not R.within(np.array([1.0, 2.0, 0.0, 0.0]), ref, tol, 0.0)[0]        # a NaN went missing
    assert not R.within(np.array([1.0, 2.001, np.nan, 0.0]), ref, tol, 0.0)[0]   # exact where the bound is 0
    assert R.within(np.array([1.0, 2.001, np.nan, 0.0]), ref, tol, 2.0 ** -8)[0]
