"""The float64 reference of linear attention with a carried state, shared by tests/test_gpu_linear_attn_state*.py and
tests/test_gpu_linear_attn_step.py: tests/linear_attn_ref.py's O(S^2) expressions with the terms of an initial state h0 and of a gradient
d_hT through the final state, and the same expressions over absolute values with + for every - (`absref`). Arrays are [N, S, D]
(N = B H), g is [N, S], states are [N, D, D]; a missing state is zero."""
import numpy as np

U = 2.0 ** -8


def reference(q, k, v, g, do, scale, h0=None, dhT=None):
    """-> (ref, absref), dicts over o, hT, dq, dk, dv, dg, dh0; ref also holds a = q . dq and b = k . dk per step."""
    N, S, D = q.shape
    h0, dhT = (np.zeros((N, D, D)) if x is None else x for x in (h0, dhT))
    G = np.cumsum(g, axis=1)
    A = np.tril(np.exp(np.minimum(G[:, :, None] - G[:, None, :], 0.0)))
    Dt, kd, DT = np.exp(G)[:, :, None], np.exp(G[:, -1:] - G)[:, :, None], np.exp(G[:, -1])[:, None, None]
    T, rcumsum = lambda x: np.swapaxes(x, 1, 2), lambda x: np.cumsum(x[:, ::-1], axis=1)[:, ::-1]
    out = []
    for f in (lambda x: x, np.abs):
        P, dP = scale * (f(q) @ T(f(k))) * A, f(do) @ T(f(v))
        r = dict(o=P @ f(v) + scale * Dt * (f(q) @ f(h0)), hT=DT * f(h0) + T(kd * f(k)) @ f(v),
                 dq=scale * (dP * A) @ f(k) + scale * Dt * (f(do) @ T(f(h0))), dk=scale * T(dP * A) @ f(q) + kd * (f(v) @ T(f(dhT))),
                 dv=T(P) @ f(do) + kd * (f(k) @ f(dhT)), dh0=scale * T(Dt * f(q)) @ f(do) + DT * f(dhT))
        r["a"], r["b"] = (f(q) * r["dq"]).sum(2), (f(k) * r["dk"]).sum(2)
        through = (f(dhT) * r["hT"]).sum((1, 2))[:, None]   # <d_hT, hT>: what every dg_r gains from a gradient through the final state
        r["dg"] = rcumsum(r["a"] - r["b"]) + through if not out else rcumsum(r["a"] + r["b"]) + through
        out.append(r)
    return out


def step_reference(q, k, v, g, scale, state):
    """The recurrence itself, token by token: -> (o [N, T, D], final state), (the same over absolute values)."""
    out = []
    for f in (lambda x: x, np.abs):
        s, o, fq, fk, fv = f(state).copy(), np.empty(q.shape), f(q), f(k), f(v)
        for t in range(q.shape[1]):
            s *= np.exp(g[:, t])[:, None, None]
            s += fk[:, t, :, None] * fv[:, t, None, :]
            o[:, t] = scale * (fq[:, t, None, :] @ s)[:, 0]
        out.append((o, s))
    return out


def bound(ref, absref, S, c):
    """u |ref| + (c u + S 2^-23) absref, the random tier's bound"""
    return U * np.abs(ref) + (c * U + S * 2.0 ** -23) * absref


def check_random(got, ref, absref, S, c):
    for n in got:
        err = np.abs(got[n] - ref[n]) - bound(ref[n], absref[n], S, c)
        assert err.max() <= 0, (n, np.unravel_index(err.argmax(), err.shape), err.max())
