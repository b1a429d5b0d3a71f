"""f64 numpy reference of the chunked linear + cross-entropy loss (kfunca.linear_cross_entropy, kf_ce_fused_rows): the loss, the UNSCALED
gradient of the logits, dX and dW, with ignored rows, label smoothing, z-loss and both reductions. tests/test_linear_ce_ref.py holds it to
torch-CPU autograd; the GPU tests hold the kernels to it.

    lse_r      = log(sum_v exp(x_rv))
    rowloss_r  = (1 - eps) (lse_r - x_r,t) + eps (lse_r - mean_v x_rv) + z lse_r^2        0 for an ignored row
    dlogits_rv = p_rv (1 + 2 z lse_r) - (1 - eps) [v == t] - eps / V                      0 for an ignored row
    loss       = sum_r rowloss_r        (mean: / the number of rows not ignored)
"""
import numpy as np


def ce_rows(logits, target, ignore=-100, eps=0.0, z=0.0):
    """(lse [rows], rowloss [rows], dlogits [rows, V] unscaled) in f64. A target outside [0, V) that is not `ignore`: NaN loss, NaN row."""
    x = np.asarray(logits, np.float64)
    t = np.asarray(target, np.int64)
    rows, V = x.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(x - m)
        s = e.sum(1, keepdims=True)
        lse = (m + np.log(s))[:, 0]
        p = e / s
        ok = (t >= 0) & (t < V)
        tc = np.where(ok, t, 0)
        xt = x[np.arange(rows), tc]
        loss = (1 - eps) * (lse - xt) + (eps * (lse - x.mean(1)) if eps > 0 else 0.0) + z * lse * lse
        d = p * (1 + 2 * z * lse)[:, None] - eps / V
        d[np.arange(rows)[ok], tc[ok]] -= 1 - eps
    loss = np.where(t == ignore, 0.0, np.where(ok, loss, np.nan))
    d[t == ignore] = 0.0
    d[(t != ignore) & ~ok] = np.nan
    return lse, loss, d


def linear_ce(x, W, target, ignore=-100, reduction="mean", eps=0.0, z=0.0, g=1.0, chunk_rows=None):
    """The operator in f64. x [T, d], W [V, d], target [T]; g the upstream gradient of the scalar loss. Returns a dict:
    loss, count, dX [T, d], dW [V, d], and for the scale-aware bounds abs_dX = |dlogits| |W| and abs_dW = |dlogits|^T |x| (the sums of the
    contractions' absolute terms). chunk_rows walks the tokens in chunks the way the operator does: the result must not depend on it."""
    x = np.asarray(x, np.float64)
    W = np.asarray(W, np.float64)
    t = np.asarray(target, np.int64).reshape(-1)
    T, d = x.shape
    V = W.shape[0]
    assert reduction in ("sum", "mean") and W.shape[1] == d and t.shape == (T,)
    C = T if not chunk_rows else int(chunk_rows)
    count = int((t != ignore).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.float64(g) / np.float64(count) if reduction == "mean" else np.float64(g)
    total = 0.0
    dX, abs_dX = np.zeros((T, d)), np.zeros((T, d))
    dW, abs_dW = np.zeros((V, d)), np.zeros((V, d))
    for r0 in range(0, T, max(C, 1)):
        sl = slice(r0, min(T, r0 + C))
        _, rl, dl = ce_rows(x[sl] @ W.T, t[sl], ignore, eps, z)
        total += rl.sum()
        dX[sl] = dl @ W
        abs_dX[sl] = np.abs(dl) @ np.abs(W)
        dW += dl.T @ x[sl]
        abs_dW += np.abs(dl).T @ np.abs(x[sl])
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(total) / np.float64(count) if reduction == "mean" else np.float64(total)
        return dict(loss=loss, count=count, dX=dX * scale, dW=dW * scale, abs_dX=abs_dX * abs(scale), abs_dW=abs_dW * abs(scale))
