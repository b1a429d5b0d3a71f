"""-m gpu: kf_linear_attn_fwd / kf_linear_attn_bwd through the C ABI against the float64 O(S^2) expression on the inputs as stored
(tests/linear_attn_ref.py), always on outputs and a workspace filled with 0xA5 with 64 untouched guard elements around each output.
Exact tier: q, k, v, dO in {-1, 0, 1}, scale 1/8, g = 0 but -40 at reset steps: every intermediate is a multiple of 1/8 below 256, exact
in both formats; only the last rounding of each output is allowed, and what the residue of a reset does to an f32 sum (RESIDUE below).
Random tier: |got - ref| <= u |ref| + (c u + S 2^-23) absref with u = 2^-8 and c = 2, the 16-bit roundings between an operand's load and
the accumulator on the longest path of the kernels as built: (1) V, or dO, times its in-chunk decay as it enters the state product, (2) the
16-bit copy of the f32 state that the next chunk's products read. (The other path has one: P, or dP, rounded into LDS.) The state itself
stays in f32, so the roundings do not grow with the number of chunks."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests.linear_attn_ref import U, check_random, reference

pytestmark = pytest.mark.gpu
CODE, GUARD = {"bf16": H.BF16, "f16": H.F16}, 64
# A reset leaves e^-40 of the steps before it: at most 256 e^-40 in any output, terms that cancel among themselves and that f16 flushes
# (RESIDUE). Beside an integer such a term also costs an f32 ulp: the matrix instruction aligns its addends to the largest exponent and
# appears to drop the bits shifted out instead of rounding them: integer - tiny comes out as the float below the integer (2^-23 measured where
# the exact value is 0). The 16-bit state copy rounds that away, so only an output's own chains see it: the 4 + D / 16 <= 12 matrix
# steps into its accumulator, each at most one ulp of a partial sum that absref bounds. Without a reset the issue's bound stands alone.
RESIDUE = 256 * np.exp(-40.0)


def run(dt, B, Hh, S, D, q, k, v, g, do, scale, twice=False):
    """arrays [B Hh, S, D] f64 already representable in dt -> dict of f64 outputs; guards and (twice) bit-reproducibility asserted."""
    N = B * Hh
    dev = {n: H.DevBuf.from_numpy(V.encode(x, dt)) for n, x in dict(q=q, k=k, v=v, do=do).items()}
    dev["g"] = H.DevBuf.from_numpy(g.astype(np.float32))
    sizes = dict(o=(N * S * D, 2), dq=(N * S * D, 2), dk=(N * S * D, 2), dv=(N * S * D, 2), dg=(N * S, 4))
    wsb = H.linear_attn_bwd_workspace_bytes(CODE[dt], B, Hh, S, D, D)
    runs = []
    for _ in range(2 if twice else 1):
        out = {n: H.DevBuf.from_numpy(np.full((cnt + 2 * GUARD) * es, 0xA5, np.uint8)) for n, (cnt, es) in sizes.items()}
        ws = H.DevBuf.from_numpy(np.full(wsb, 0xA5, np.uint8))
        p = {n: out[n].ptr + GUARD * es for n, (cnt, es) in sizes.items()}
        H.linear_attn_fwd(CODE[dt], B, Hh, S, D, D, scale, dev["q"].ptr, dev["k"].ptr, dev["v"].ptr, dev["g"].ptr, p["o"])
        H.linear_attn_bwd(CODE[dt], B, Hh, S, D, D, scale, dev["q"].ptr, dev["k"].ptr, dev["v"].ptr, dev["g"].ptr, dev["do"].ptr, p["dq"], p["dk"],
                          p["dv"], p["dg"], workspace=ws.ptr, workspace_bytes=wsb)
        raw = {}
        for n, (cnt, es) in sizes.items():
            b = out[n].to_numpy(((cnt + 2 * GUARD) * es,), np.uint8)
            assert (b[:GUARD * es] == 0xA5).all() and (b[-GUARD * es:] == 0xA5).all(), f"guard of {n} written"
            raw[n] = b[GUARD * es:-GUARD * es].copy()
        runs.append(raw)
    if twice:
        assert all(np.array_equal(runs[0][n], runs[1][n]) for n in sizes), "two calls differ"
    got = {n: V.decode(runs[0][n].view(np.uint16), dt).reshape(N, S, D) for n in ("o", "dq", "dk", "dv")}
    got["dg"] = runs[0]["dg"].view(np.float32).astype(np.float64).reshape(N, S)
    return got


def exact_case(dt, S, D, reset, twice=False):
    B, Hh = 2, 3
    rng = np.random.default_rng(S * 7 + D + (reset or 0))
    q, k, v, do = (rng.integers(-1, 2, (B * Hh, S, D)).astype(np.float64) for _ in range(4))
    g = np.zeros((B * Hh, S))
    if reset is not None:
        g[:, reset] = -40.0
    got = run(dt, B, Hh, S, D, q, k, v, g, do, 0.125, twice)
    ref, absref = reference(q, k, v, g, do, 0.125)
    for n in ("o", "dq", "dk", "dv"):
        err = np.abs(got[n] - ref[n]) - U * np.abs(ref[n]) - (0.0 if reset is None else RESIDUE + 12 * 2.0 ** -23 * absref[n])
        assert err.max() <= 0, (n, np.unravel_index(err.argmax(), err.shape), err.max())
    assert (np.abs(got["dg"] - ref["dg"]) <= 2.0 ** -20 * (np.abs(ref["a"]) + np.abs(ref["b"])).sum(1, keepdims=True)).all()


# one partial chunk / one whole / the first carried state / two carries / a ragged tail after carries; resets: none, step 0, the first and
# the last step of a chunk, inside a chunk
@pytest.mark.parametrize("S,reset", [(S, r) for S in (1, 63, 64, 65, 128, 200, 256) for r in (None, 0, 64, 63, 100) if r is None or r < S])
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)])
def test_exact(dt, D, S, reset):
    exact_case(dt, S, D, reset)


@pytest.mark.parametrize("dt,D", [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)])
def test_tail_stores_dropped_and_bits_repeat(dt, D):
    exact_case(dt, 65, D, 63, twice=True)


def random_case(dt, B, Hh, S, D):
    rng = np.random.default_rng(S + D + B)
    q, k, v, do = (V.decode(V.encode(rng.uniform(-1, 1, (B * Hh, S, D)), dt), dt) for _ in range(4))
    g = -rng.uniform(0, 0.05, (B * Hh, S)).astype(np.float32).astype(np.float64)
    scale = float(np.float32(D ** -0.5))
    got = run(dt, B, Hh, S, D, q, k, v, g, do, scale)
    ref, absref = reference(q, k, v, g, do, scale)
    check_random(got, ref, absref, S, 2)   # c = 2: the docstring


@pytest.mark.parametrize("S", [192, 1000])   # 1000: 15 whole chunks and a tail, the double buffer wraps many times
@pytest.mark.parametrize("dt,D", [("bf16", 64), ("bf16", 128), ("f16", 64), ("f16", 128)])
def test_random(dt, D, S):
    random_case(dt, 1, 2, S, D)


@pytest.mark.parametrize("D", [64, 128])
def test_more_workgroups_than_compute_units(D):
    random_case("bf16", 20, 15, 64, D)
