"""The float64 reference of linear attention with a scalar decay, shared by tests/test_gpu_linear_attn*.py: the direct O(S^2) expression
O = scale ((Q K^T) . A) V with A[t, s] = exp(G_t - G_s) for s <= t, its closed-form gradients, and the same expressions over absolute
values (the `absref` of the tests' bounds). Arrays are [N, S, D] (N = B H), g is [N, S]."""
import numpy as np

U = 2.0 ** -8


def reference(q, k, v, g, do, scale):
    """-> (ref, absref), dicts over o, dq, dk, dv, dg; ref also holds a = q . dq and b = k . dk per step."""
    G = np.cumsum(g, axis=1)
    A = np.tril(np.exp(np.minimum(G[:, :, None] - G[:, None, :], 0.0)))
    T, rcumsum = lambda x: np.swapaxes(x, 1, 2), lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1]
    out = []
    for f in (lambda x: x, np.abs):
        P, dP = scale * (f(q) @ T(f(k))) * A, f(do) @ T(f(v))
        r = dict(o=P @ f(v), dq=scale * (dP * A) @ f(k), dk=scale * T(dP * A) @ f(q), dv=T(P) @ f(do))
        r["a"], r["b"] = (P * dP).sum(2), (P * dP).sum(1)   # = q . dq and k . dk per step
        r["dg"] = rcumsum(r["a"] - r["b"]) if not out else rcumsum(r["a"] + r["b"])
        out.append(r)
    return out


def check_random(got, ref, absref, S, c):
    """|got - ref| <= u |ref| + (c u + S 2^-23) absref for every output."""
    for n in ("o", "dq", "dk", "dv", "dg"):
        if n in got:
            err = np.abs(got[n] - ref[n]) - (U * np.abs(ref[n]) + (c * U + S * 2.0 ** -23) * absref[n])
            assert err.max() <= 0, (n, np.unravel_index(err.argmax(), err.shape), err.max())
