"""The f64 numpy reference of the fused per-head QK-norm + rotary embedding (kf_qk_norm_rope_fwd / _bwd), and the bounds the GPU tests hold
the kernels to. It takes the FLOAT VALUES of the stored inputs (x, dy, weights as the device holds them, tables as f32), so the only
differences left are the kernel's f32 arithmetic and its one rounding at the store.

Layout: x, dy [T, W], T = B*S, W = (Hq + Hk + Hv) D, heads of a token in the order q | k | v. wq, wk: [D] or None (1). cos, sin: [P, R/2]
or None with R = 0. positions: [T] int or None (p = t % S). Pairs as kf_rope: rotate-half (i, i + R/2), interleaved (2i, 2i + 1).

    forward    rstd = 1 / sqrt(mean_d x_d^2 + eps)   n_d = x_d rstd w_d   y_a = n_a c - n_b s, y_b = n_b c + n_a s  (d >= R: y = n)
    backward   g = the inverse rotation of dy (s -> -s), xhat = x rstd, gw = g w, m = mean_d(gw_d xhat_d)
               dx_d = rstd (gw_d - xhat_d m)          dwq_d = sum over tokens and q heads of g_d xhat_d, dwk likewise
    v heads: y = x, dx = dy.
A position outside [0, P) makes that token's rotated elements NaN (forward), hence g, m and the whole of dx of its q and k heads.

Bounds (r = the rounding of the output type: 2^-8 bf16, 2^-11 f16, 0 f32; below the type's normal range one rounding is half the
subnormal spacing instead - 2^-25 in f16, where |y| < 2^-14 is met all the time: the correctly rounded result itself is that far off):
    forward   |got - ref| <= r |ref| + 2^-20 (|n_a| + |n_b|)     a <= 256-term f32 tree sum, one division, sqrt and reciprocal, two products and
                                                                  the rotation's product and FMA stay under 16 f32 ulps of the pair's magnitude
                                                                  (a dim beyond R is its own pair: 2^-20 |n_d|); v heads are exact
    dx        r |ref| + 2^-20 rstd (|gw_d| + |xhat_d| mean_d |gw_d xhat_d|)     on the terms, not on their difference
    dw        r |ref| + (N + 8) 2^-24 sum |g_d xhat_d| over the N (token, head) rows summed: valid for any summation order
"""
import numpy as np

ROUNDING = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}
SUBNORMAL_ROUNDING = {"bf16": 2.0 ** -134, "f16": 2.0 ** -25, "f32": 0.0}   # half the spacing below the smallest normal number
FWD_ULPS = 2.0 ** -20
DW_ULP = 2.0 ** -24


def pair_index(D, R, interleaved):
    """(a, b): index arrays of the R/2 pairs' first and second dims."""
    i = np.arange(R // 2)
    return (2 * i, 2 * i + 1) if interleaved else (i, i + R // 2)


def token_tables(cos, sin, positions, T, S, R):
    """cos, sin [T, R/2] f64 of each token (NaN rows for positions outside the table)."""
    if R == 0:
        return np.zeros((T, 0)), np.zeros((T, 0))
    cos, sin = np.asarray(cos, np.float64), np.asarray(sin, np.float64)
    p = np.arange(T) % S if positions is None else np.asarray(positions, np.int64)
    ok = (p >= 0) & (p < cos.shape[0])
    c, s = cos[np.where(ok, p, 0)], sin[np.where(ok, p, 0)]
    c[~ok] = np.nan
    s[~ok] = np.nan
    return c, s


def rotate(n, c, s, R, interleaved, inverse=False):
    """n [T, H, D] -> (rotated, |term| + |term| per element: the magnitude the rotation's rounding is relative to)."""
    out, mag = n.copy(), np.abs(n)
    if R:
        D = n.shape[-1]
        a, b = pair_index(D, R, interleaved)
        cc, ss = c[:, None, :], (-s if inverse else s)[:, None, :]
        na, nb = n[..., a], n[..., b]
        out[..., a] = na * cc - nb * ss
        out[..., b] = nb * cc + na * ss
        mag[..., a] = mag[..., b] = np.abs(na) + np.abs(nb)
    return out, mag


def _split(x, T, Hq, Hk, Hv, D):
    x = np.asarray(x, np.float64).reshape(T, Hq + Hk + Hv, D)
    return x[:, :Hq + Hk], x[:, Hq + Hk:]


def _weights(wq, wk, Hq, Hk, D):
    """[Hq + Hk, D] f64: the weight of every normalised head."""
    one = np.ones(D)
    q = one if wq is None else np.asarray(wq, np.float64)
    k = one if wk is None else np.asarray(wk, np.float64)
    return np.concatenate([np.tile(q, (Hq, 1)), np.tile(k, (Hk, 1))], 0).reshape(Hq + Hk, D)


def forward(x, wq, wk, cos, sin, positions, B, S, Hq, Hk, Hv, D, R, interleaved=False, eps=1e-6):
    """-> (y [T, W] f64, tol [T, W]): |got - y| <= r |y| + tol."""
    T = B * S
    qk, v = _split(x, T, Hq, Hk, Hv, D)
    w = _weights(wq, wk, Hq, Hk, D)
    rstd = 1.0 / np.sqrt((qk * qk).mean(-1, keepdims=True) + eps)
    n = qk * rstd * w[None]
    c, s = token_tables(cos, sin, positions, T, S, R)
    y, mag = rotate(n, c, s, R, interleaved)
    tol = FWD_ULPS * mag
    tol[..., R:] = FWD_ULPS * np.abs(n[..., R:])
    return (np.concatenate([y, v], 1).reshape(T, -1), np.concatenate([tol, np.zeros_like(v)], 1).reshape(T, -1))


def backward(x, dy, wq, wk, cos, sin, positions, B, S, Hq, Hk, Hv, D, R, interleaved=False, eps=1e-6):
    """-> dict: dx [T, W], dx_tol [T, W], dwq, dwk [D], dwq_tol, dwk_tol [D] (the absolute parts of the bounds; the caller adds r |ref|)."""
    T = B * S
    qk, _ = _split(x, T, Hq, Hk, Hv, D)
    gy, gv = _split(dy, T, Hq, Hk, Hv, D)
    w = _weights(wq, wk, Hq, Hk, D)
    rstd = 1.0 / np.sqrt((qk * qk).mean(-1, keepdims=True) + eps)
    xhat = qk * rstd
    c, s = token_tables(cos, sin, positions, T, S, R)
    g, _ = rotate(gy, c, s, R, interleaved, inverse=True)
    gw = g * w[None]
    m = (gw * xhat).mean(-1, keepdims=True)
    dx = rstd * (gw - xhat * m)
    dx_tol = FWD_ULPS * rstd * (np.abs(gw) + np.abs(xhat) * np.abs(gw * xhat).mean(-1, keepdims=True))
    t = g * xhat
    out = {"dx": np.concatenate([dx, gv], 1).reshape(T, -1), "dx_tol": np.concatenate([dx_tol, np.zeros_like(gv)], 1).reshape(T, -1)}
    for name, sl in (("dwq", slice(0, Hq)), ("dwk", slice(Hq, Hq + Hk))):
        rows = T * (sl.stop - sl.start)
        out[name] = t[:, sl].sum((0, 1))
        out[name + "_tol"] = (rows + 8) * DW_ULP * np.abs(t[:, sl]).sum((0, 1))
    return out


def within(got, ref, tol, r, floor=0.0):
    """(ok, worst fraction of the bound max(r |ref|, floor) + tol): NaN must meet NaN; where the bound is 0 the values must be equal.
    floor: SUBNORMAL_ROUNDING of the output type."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    bound = np.maximum(r * np.abs(ref), floor) + tol
    err = np.abs(got - ref)
    err[nan] = 0.0
    bound = np.where(nan, 1.0, bound)
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return bool((err <= bound).all()), float(frac.max()) if frac.size else 0.0
