"""-m gpu: kf_linear_attn_state_fwd / kf_linear_attn_state_bwd through the C ABI against the float64 expressions of
tests/linear_attn_state_ref.py on the inputs as stored, always on outputs and a workspace filled with 0xA5 with 64 untouched guard
elements around every output, hT and d_h0 included.
Exact tier (tests/test_gpu_linear_attn.py's: q, k, v, dO in {-1, 0, 1}, g = 0, scale 1/8, every intermediate exact): a sequence run in
one call and run as two segments chained through hT -> h0 and d_h0 -> d_hT must agree to the bit.
Random tier: |got - ref| <= u |ref| + (c u + S 2^-23) absref with u = 2^-8 and c = 2 as in the stateless test - the state variants add no
16-bit rounding to a path: h0 (d_hT) enters the first chunk's products through the same 16-bit copy a carried state (dS) takes, hT and
d_h0 leave as the f32 accumulators, and <d_hT, hT> is an f32 sum over f32 values."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests.linear_attn_state_ref import check_random, reference

pytestmark = pytest.mark.gpu
CODE, GUARD = {"bf16": H.BF16, "f16": H.F16}, 64
CASES = [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)]
same = lambda a, b: np.array_equal(a.view(np.int64), b.view(np.int64))   # values widened exactly: equal bits, the sign of zero included


def run(dt, B, Hh, x, scale, h0=None, dhT=None, want=("hT", "dh0"), alias=False, stateless=False):
    """x: q, k, v, do [B Hh, S, D] f64 representable in dt and g [B Hh, S]; states [B Hh, D, D] -> dict of f64 outputs, guards asserted.
    alias: hT is written over h0 and d_h0 over d_hT (the backward runs first: it needs the h0 the forward then overwrites)."""
    N, S, D = x["q"].shape
    sizes = dict(o=(N * S * D, 2), dq=(N * S * D, 2), dk=(N * S * D, 2), dv=(N * S * D, 2), dg=(N * S, 4), hT=(N * D * D, 4), dh0=(N * D * D, 4))

    def guarded(n, init=None):
        cnt, es = sizes[n]
        b = np.full((cnt + 2 * GUARD) * es, 0xA5, np.uint8)
        if init is not None:
            b[GUARD * es:-GUARD * es] = init.astype(np.float32).ravel().view(np.uint8)
        return H.DevBuf.from_numpy(b)

    dev = {n: H.DevBuf.from_numpy(V.encode(x[n], dt)) for n in ("q", "k", "v", "do")}
    dev["g"] = H.DevBuf.from_numpy(x["g"].astype(np.float32))
    out = {n: guarded(n) for n in sizes if n not in ("hT", "dh0") or (n in want and not alias)}
    bh0, bdhT = (None if s is None else guarded("hT", s) for s in (h0, dhT))
    if alias:
        out["hT"], out["dh0"] = bh0, bdhT
    at = lambda b, n: None if b is None else b.ptr + GUARD * sizes[n][1]
    p = {n: at(out.get(n), n) for n in sizes}
    head, ins = (CODE[dt], B, Hh, S, D, D, scale), [dev[n].ptr for n in ("q", "k", "v", "g")]
    if stateless:
        wsb = H.linear_attn_bwd_workspace_bytes(*head[:-1])
        ws = H.DevBuf.from_numpy(np.full(wsb, 0xA5, np.uint8))
        H.linear_attn_bwd(*head, *ins, dev["do"].ptr, p["dq"], p["dk"], p["dv"], p["dg"], workspace=ws.ptr, workspace_bytes=wsb)
        H.linear_attn_fwd(*head, *ins, p["o"])
    else:
        wsb = H.linear_attn_state_bwd_workspace_bytes(*head[:-1])
        ws = H.DevBuf.from_numpy(np.full(wsb, 0xA5, np.uint8))
        H.linear_attn_state_bwd(*head, *ins, at(bh0, "hT"), dev["do"].ptr, at(bdhT, "hT"), p["dq"], p["dk"], p["dv"], p["dg"], p["dh0"],
                                workspace=ws.ptr, workspace_bytes=wsb)
        H.linear_attn_state_fwd(*head, *ins, at(bh0, "hT"), p["o"], p["hT"])
    got = {}
    for n, buf in out.items():
        cnt, es = sizes[n]
        b = buf.to_numpy(((cnt + 2 * GUARD) * es,), np.uint8)
        assert (b[:GUARD * es] == 0xA5).all() and (b[-GUARD * es:] == 0xA5).all(), f"guard of {n} written"
        body = b[GUARD * es:-GUARD * es].copy()
        got[n] = (V.decode(body.view(np.uint16), dt) if es == 2 else body.view(np.float32).astype(np.float64)).reshape(
            (N, S, D) if es == 2 else (N, S) if n == "dg" else (N, D, D))
    return got


def cut(x, lo, hi):
    return {n: a[:, lo:hi] for n, a in x.items()}


@pytest.mark.parametrize("c", [1, 63, 64, 65, 100])
@pytest.mark.parametrize("dt,D", CASES)
def test_split_is_exact(dt, D, c):
    B, Hh, S = 2, 3, 200
    rng = np.random.default_rng(S * 7 + D + c)
    x = {n: rng.integers(-1, 2, (B * Hh, S, D)).astype(np.float64) for n in ("q", "k", "v", "do")}
    x["g"] = np.zeros((B * Hh, S))
    whole = run(dt, B, Hh, x, 0.125, want=("hT",))
    first = run(dt, B, Hh, cut(x, 0, c), 0.125, want=("hT",))
    second = run(dt, B, Hh, cut(x, c, S), 0.125, h0=first["hT"])
    first = run(dt, B, Hh, cut(x, 0, c), 0.125, dhT=second["dh0"], want=("hT",))   # the backward of the first segment wants the second's d_h0
    ref, _ = reference(x["q"], x["k"], x["v"], x["g"], x["do"], 0.125)
    assert np.array_equal(second["hT"], ref["hT"]) and np.array_equal(whole["hT"], ref["hT"])   # integers
    for n in ("o", "dq", "dk", "dv"):
        assert same(np.concatenate([first[n], second[n]], 1), whole[n]), n
    dg = np.concatenate([first["dg"], second["dg"]], 1)
    assert (np.abs(dg - ref["dg"]) <= 2.0 ** -20 * (np.abs(ref["a"]) + np.abs(ref["b"])).sum(1, keepdims=True)).all()


def draw(dt, N, S, D, seed):
    rng = np.random.default_rng(seed)
    x = {n: V.decode(V.encode(rng.uniform(-1, 1, (N, S, D)), dt), dt) for n in ("q", "k", "v", "do")}
    x["g"] = -rng.uniform(0, 0.05, (N, S)).astype(np.float32).astype(np.float64)
    h0, dhT = (rng.uniform(-1, 1, (N, D, D)).astype(np.float32).astype(np.float64) for _ in range(2))
    return x, h0, dhT, float(np.float32(D ** -0.5))


# one step / a carried state and a one-step tail / three whole chunks. dg is checked with d_hT != 0: without <d_hT, hT> it is off by
# that constant. With states of random signs the constant is a small share of absref, which sums magnitudes: at these inputs it lies
# outside this bound at D = 128, S = 1 (1.7 times the bound) and inside it elsewhere; test_split_is_exact's dg bound is 2^-20 of the
# sums and fails without the term at every split.
@pytest.mark.parametrize("S", [1, 65, 192])
@pytest.mark.parametrize("dt,D", CASES)
def test_random(dt, D, S):
    x, h0, dhT, scale = draw(dt, 2, S, D, S + D)
    got = run(dt, 1, 2, x, scale, h0=h0, dhT=dhT)
    check_random(got, *reference(x["q"], x["k"], x["v"], x["g"], x["do"], scale, h0, dhT), S, 2)   # c = 2: the docstring


@pytest.mark.parametrize("use_h0,use_dhT,want", [(True, False, ()), (False, False, ("hT",)), (False, True, ()), (False, False, ())])
@pytest.mark.parametrize("dt,D", [("bf16", 128), ("f16", 64)])
def test_null_combinations(dt, D, use_h0, use_dhT, want):
    x, h0, dhT, scale = draw(dt, 2, 65, D, D)
    h0, dhT = h0 if use_h0 else None, dhT if use_dhT else None
    got = run(dt, 1, 2, x, scale, h0=h0, dhT=dhT, want=want)
    assert set(got) == {"o", "dq", "dk", "dv", "dg", *want}
    check_random(got, *reference(x["q"], x["k"], x["v"], x["g"], x["do"], scale, h0, dhT), 65, 2)
    if not (use_h0 or use_dhT or want):   # all null: the stateless entries, bit for bit
        plain = run(dt, 1, 2, x, scale, want=(), stateless=True)
        assert all(same(got[n], plain[n]) for n in plain)


def test_more_workgroups_than_compute_units_and_aliased_states():
    x, h0, dhT, scale = draw("bf16", 300, 64, 128, 300)
    got = run("bf16", 20, 15, x, scale, h0=h0, dhT=dhT, alias=True)
    check_random(got, *reference(x["q"], x["k"], x["v"], x["g"], x["do"], scale, h0, dhT), 64, 2)
