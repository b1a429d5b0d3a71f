"""The float64 reference of the gated delta rule and what tests/test_gpu_delta_rule*.py share: the recurrence itself, token by token, on
the inputs as stored; the two tiers' inputs; and the runners of kf_delta_rule_fwd / kf_delta_rule_step through the C ABI, always on
outputs and a workspace filled with 0xA5 with 64 untouched guard elements around every output. Arrays are [N, S, D] (N = B H), g and
beta [N, S], states [N, D, D].

Random-tier bound, per head: max|got - ref| <= C 2^-8 max|ref| with C = 5, the 16-bit roundings between an operand's load and an
accumulator on the longest path of the kernels as built: T (with its column scaling), W or Ubar, U, the decayed U
fragment on its way into the state, and the state's 16-bit copy on its way into the next chunk's products. No bound is built from the
recurrence over absolute values: it grows like prod (1 + beta_t) and would pass anything; the true recurrence is contractive for
beta |k|^2 <= 1, so the bound is normwise."""
import functools

import numpy as np

from kfunca_amd import hip_abi as H
from tests import gemm_views as V

U, C, GUARD = 2.0 ** -8, 5, 64
CODE = {"bf16": H.BF16, "f16": H.F16}
CASES = [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)]


def reference(q, k, v, g, beta, scale, h0=None):
    """-> o [N, S, D], the final state [N, D, D]"""
    N, S, D = q.shape
    s, o = np.zeros((N, D, D)) if h0 is None else h0.copy(), np.empty(q.shape)
    for t in range(S):
        if g is not None:
            s *= np.exp(g[:, t])[:, None, None]
        u = beta[:, t, None] * (v[:, t] - (k[:, t, None, :] @ s)[:, 0])
        s += k[:, t, :, None] * u[:, None, :]
        o[:, t] = scale * (q[:, t, None, :] @ s)[:, 0]
    return o, s


def rounded(a, dt):
    return V.decode(V.encode(a, dt), dt)


@functools.lru_cache(maxsize=None)
def exact_case(N, S, D):
    """One-hot keys from 8 indices (they repeat inside and across chunks), beta in {0, 1}, q, v, h0 in {-1, 0, 1}, g = 0, scale 1/8: L, T,
    W, Ubar, U and the state are small integers, exact in both formats. -> inputs, h0, (o, hT) from zero, (o, hT) from h0"""
    rng = np.random.default_rng(S * 3 + D)
    x = dict(q=rng.integers(-1, 2, (N, S, D)).astype(np.float64), v=rng.integers(-1, 2, (N, S, D)).astype(np.float64),
             k=np.eye(D)[rng.integers(0, 8, (N, S)) * (D // 8) + 3], beta=rng.integers(0, 2, (N, S)).astype(np.float64), g=None)
    h0 = rng.integers(-1, 2, (N, D, D)).astype(np.float64)
    return x, h0, reference(**x, scale=0.125), reference(**x, scale=0.125, h0=h0)


@functools.lru_cache(maxsize=None)
def random_case(dt, N, S, D):
    """k and q unit-norm per step before the rounding to dt, v in U(-1, 1), beta in U(0, 1), g in -U(0, 0.05), h0 in U(-1/8, 1/8)
    -> inputs, h0, scale, (o, hT)"""
    rng = np.random.default_rng(N + S + D)
    unit = lambda a: a / np.linalg.norm(a, axis=-1, keepdims=True)
    x = dict(q=rounded(unit(rng.normal(size=(N, S, D))), dt), k=rounded(unit(rng.normal(size=(N, S, D))), dt), v=rounded(rng.uniform(-1, 1, (N, S, D)), dt),
             g=-rng.uniform(0, 0.05, (N, S)).astype(np.float32).astype(np.float64), beta=rng.uniform(0, 1, (N, S)).astype(np.float32).astype(np.float64))
    h0, scale = rng.uniform(-0.125, 0.125, (N, D, D)).astype(np.float32).astype(np.float64), float(np.float32(D ** -0.5))
    return x, h0, scale, reference(**x, scale=scale, h0=h0)


def cut(x, lo, hi):
    return {n: None if a is None else a[:, lo:hi] for n, a in x.items()}


def worst(got, ref):
    """max over heads of max|got - ref| / max|ref|"""
    ax = tuple(range(1, ref.ndim))
    return (np.abs(got - ref).max(ax) / np.abs(ref).max(ax)).max()


def guarded(count, es, init=None):
    b = np.full((count + 2 * GUARD) * es, 0xA5, np.uint8)
    if init is not None:
        b[GUARD * es:-GUARD * es] = init.astype(np.float32).ravel().view(np.uint8)
    return H.DevBuf.from_numpy(b)


def body(buf, count, es, what):
    b = buf.to_numpy(((count + 2 * GUARD) * es,), np.uint8)
    assert (b[:GUARD * es] == 0xA5).all() and (b[-GUARD * es:] == 0xA5).all(), f"guard of {what} written"
    return b[GUARD * es:-GUARD * es].copy()


def operands(x, dt):
    dev = {n: H.DevBuf.from_numpy(V.encode(x[n], dt)) for n in ("q", "k", "v")}
    dev.update({n: None if x[n] is None else H.DevBuf.from_numpy(x[n].astype(np.float32)) for n in ("g", "beta")})
    return dev, [None if dev[n] is None else dev[n].ptr for n in ("q", "k", "v", "g", "beta")]


def fwd(dt, B, Hh, x, scale, h0=None, want_hT=True):
    """kf_delta_rule_fwd -> o [N, S, D] f64, hT [N, D, D] f64 or None"""
    N, S, D = x["q"].shape
    dev, ins = operands(x, dt)
    bo, bh0, bhT = guarded(N * S * D, 2), None if h0 is None else guarded(N * D * D, 4, h0), guarded(N * D * D, 4) if want_hT else None
    wsb = H.delta_rule_fwd_workspace_bytes(CODE[dt], B, Hh, S, D, D)
    ws = guarded(wsb, 1)
    H.delta_rule_fwd(CODE[dt], B, Hh, S, D, D, scale, *ins, None if bh0 is None else bh0.ptr + GUARD * 4, bo.ptr + GUARD * 2,
                     None if bhT is None else bhT.ptr + GUARD * 4, workspace=ws.ptr + GUARD, workspace_bytes=wsb)
    body(ws, wsb, 1, "the workspace")
    o = V.decode(body(bo, N * S * D, 2, "o").view(np.uint16), dt).reshape(N, S, D)
    return o, body(bhT, N * D * D, 4, "hT").view(np.float32).astype(np.float64).reshape(N, D, D) if want_hT else None


def step(dt, B, Hh, x, scale, state):
    """kf_delta_rule_step -> o [N, T, D] f64, the state after the call"""
    N, T, D = x["q"].shape
    dev, ins = operands(x, dt)
    bo, bst = guarded(N * T * D, 2), guarded(N * D * D, 4, state)
    H.delta_rule_step(CODE[dt], B, Hh, T, D, D, scale, *ins, bst.ptr + GUARD * 4, bo.ptr + GUARD * 2)
    return (V.decode(body(bo, N * T * D, 2, "o").view(np.uint16), dt).reshape(N, T, D),
            body(bst, N * D * D, 4, "the state").view(np.float32).astype(np.float64).reshape(N, D, D))
