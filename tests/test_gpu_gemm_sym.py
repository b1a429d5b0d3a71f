"""-m gpu: kf_gemm_sym through the C ABI - C = alpha X X^T + beta D + gamma I against the f64 value of the whole expression on the rounded
inputs, within |got - ref| <= r |ref| + K 2^-23 absref (r = 2^-8 for 16 bits, 2^-23 for f32; absref = |alpha| |X| |X|^T + |beta D| +
|gamma I|: the output rounding plus f32 accumulation, the bound of tests/test_gpu_gemm_seg.py). Every case also asserts that C is
symmetric bit for bit, that the 0xA5 bytes of C's buffer outside [M, M] are untouched, and which kernel ran (per-launch profile labels)."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V

pytestmark = pytest.mark.gpu

CODE = {"f32": H.F32, "bf16": H.BF16, "f16": H.F16}
NP = {"f32": np.float32, "bf16": np.uint16, "f16": np.uint16}
GUARD = 64  # elements in front of and behind C: 16-byte alignment is kept
PLAIN, NEWTON = (1.0, 0.0, 0.0), (2.0315, -4.775, 3.4445)


def stored(vals, dt):
    return np.ascontiguousarray(V.encode(vals, dt)).view(NP[dt])


def run(dt, M, K, coef, with_d, pad, off=0, label=None):
    alpha, beta, gamma = coef
    rng = np.random.default_rng(M * 1000 + K + pad)
    es, ldx, ldd, ldc = np.dtype(NP[dt]).itemsize, K + pad, M + pad, M + pad
    X = V.decode(V.encode(rng.uniform(-1, 1, (M, K)), dt), dt)
    D = rng.uniform(-1, 1, (M, M))
    D = V.decode(V.encode(np.tril(D) + np.tril(D, -1).T, dt), dt)
    xh = np.full((M, ldx), np.nan)
    xh[:, :K] = X
    dh = np.full((M, ldd), np.nan)
    dh[:, :M] = D
    xb = H.DevBuf.from_numpy(np.concatenate([stored(np.zeros(off), dt), stored(xh, dt).ravel()]))
    db = H.DevBuf.from_numpy(stored(dh, dt)) if with_d else None
    before = np.full((2 * GUARD + off + M * ldc) * es, 0xA5, np.uint8)
    cb = H.DevBuf.from_numpy(before)
    H.profile_enable(True)
    H.profile_reset()
    try:
        H.gemm_sym(CODE[dt], M, K, alpha, xb.ptr + off * es, ldx, cb.ptr + (GUARD + off) * es, ldc, beta=beta, D=db.ptr if with_d else None, ldd=ldd,
                   gamma=gamma)
        ran = H.profile_results()
    finally:
        H.profile_enable(False)
    assert {k: v[1] for k, v in ran.items()} == {label: 1}
    after = cb.to_numpy(before.shape, np.uint8)
    win = after.view(NP[dt])[GUARD + off: GUARD + off + M * ldc].reshape(M, ldc)
    got = win[:, :M].copy()
    bits = got.view(np.uint32 if dt == "f32" else np.uint16)
    assert np.array_equal(bits, bits.T), "C is not bitwise symmetric"
    win[:, :M] = before.view(NP[dt])[0]
    assert np.array_equal(after, before), "bytes outside [M, M] were written"
    ref = alpha * X @ X.T + (beta * D if with_d else 0.0) + gamma * np.eye(M)
    absref = abs(alpha) * np.abs(X) @ np.abs(X).T + (np.abs(beta * D) if with_d else 0.0) + abs(gamma) * np.eye(M)
    r = 2.0 ** -23 if dt == "f32" else 2.0 ** -8
    err = np.abs(V.decode(got, dt) - ref) - (r * np.abs(ref) + K * 2.0 ** -23 * absref)
    assert err.max() <= 0, (np.unravel_index(err.argmax(), err.shape), err.max())


# one diagonal tile / the first mirrored tile / the first grid whose decode is not trivial; one K tile (shorter than the ring) / five (it wraps)
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("coef", [PLAIN, NEWTON])
@pytest.mark.parametrize("with_d", [False, True])
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("M", [128, 256, 384])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fast_path(dt, M, K, with_d, coef, pad):
    run(dt, M, K, coef, with_d, pad, label=f"gemm_sym_{dt}_mfma")


# 528 workgroups: more than the CUs, the decode at large ids; 66: tile rows 8 .. 10 are a group that is not whole
@pytest.mark.parametrize("M", [4096, 1408])
def test_fast_path_many_tiles(M):
    run("bf16", M, 64, NEWTON, True, 0, label="gemm_sym_bf16_mfma")


@pytest.mark.parametrize("dt,M,K,off", [("bf16", 200, 72, 0), ("f32", 130, 33, 0), ("bf16", 128, 64, 1)])
def test_plain_path(dt, M, K, off):
    run(dt, M, K, NEWTON, True, 0 if off else 3, off=off, label="gemm_sym_generic")


@pytest.mark.parametrize("what", ["overlap", "ldc", "null"])
def test_refusals_come_before_any_launch(what):
    M = K = 128
    x, c = H.DevBuf(M * K * 2), H.DevBuf(M * M * 2)
    args = dict(X=x.ptr, D=None, ldc=M)
    args.update({"overlap": dict(D=c.ptr + 2 * M), "ldc": dict(ldc=M - 1), "null": dict(X=None)}[what])
    H.profile_enable(True)
    H.profile_reset()
    try:
        rc = H.lib().kf_gemm_sym(H.BF16, M, K, 1.0, args["X"], K, 1.0, args["D"], M, 0.0, c.ptr, args["ldc"], None)
        assert rc == H.KF_ERR_INVALID and "kf_gemm_sym" in H.lib().kf_last_error().decode()
        assert H.profile_results() == {}
    finally:
        H.profile_enable(False)
