"""-m gpu: kf_gemm_fp8 against tests/fp8_ref.py.

Exact tier: integer operands both formats hold exactly (-16..16 for e4m3; 0, +-1..+-8, +-10, +-12, +-14, +-16 for e5m2), power-of-two
scale_inv values, every partial sum below 2^24 - the f32 output must EQUAL the integer product. An asymmetric B throughout, an A = identity
case, and a one-hot-in-k case for every k of the instruction's 128 byte positions; all four format pairs; lda, ldb and ldc wider than the
matrices; 0xFF (NaN) bytes in the operand allocations outside the [rows, K] regions, rows behind the last one included.
Rounded tier: random codes, outputs in f32, bf16 and f16, |got - c| <= eps_out |c| + ACC_TERM mag + half a subnormal ulp against the f64
product of the decoded operands (tests/fp8_ref.gemm_bound; ACC_TERM = 3.8e-4, twice the worst measured: the 1e-6 of oracle/checks.gemm_ok
does not hold for this instruction's 128-term block sum, which cuts each product no more than 16 bits below the block's largest - see
tests/fp8_ref.py). Every byte of the C allocation outside [M, N] keeps its poison; M = 0 and
N = 0 write nothing; two runs give the same bits."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import fp8_ref as R
from tests import poison as P

pytestmark = pytest.mark.gpu

OUT = {"f32": (H.F32, np.float32), "bf16": (H.BF16, np.uint16), "f16": (H.F16, np.float16)}
FILL = 0xA5
EXTRA_ROWS = 8       # NaN rows behind the last row of each operand
SHAPES = [(1, 1, 16), (16, 16, 128), (64, 64, 112), (128, 128, 144), (130, 70, 272), (257, 129, 128), (256, 384, 1024)]
PAIRS = [(R.E4M3, R.E4M3), (R.E4M3, R.E5M2), (R.E5M2, R.E4M3), (R.E5M2, R.E5M2)]
INTS = {R.E4M3: np.arange(-16, 17, dtype=np.float64),
        R.E5M2: np.array([0] + [s * v for v in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16) for s in (1, -1)], dtype=np.float64)}


def operand(codes, ld):
    rows, K = codes.shape
    host = np.full((rows + EXTRA_ROWS, ld), 0xFF, dtype=np.uint8)
    host[:rows, :K] = codes
    return H.DevBuf.from_numpy(host)


def scale(v):
    return H.DevBuf.from_numpy(np.array([v], dtype=np.float32))


def launch(ba, lda, bb, ldb, bsa, bsb, fa, fb, out, M, N, K, ldc):
    """One kf_gemm_fp8 on operands that are on the device already. Returns the stored [M, N] window and asserts that the rest of the C
    allocation (pitch gaps and guard band) kept its poison."""
    code, store = OUT[out]
    nbytes = M * ldc * np.dtype(store).itemsize
    bc = H.DevBuf(nbytes + P.GUARD)
    P.fill(bc.ptr, nbytes + P.GUARD, FILL)
    H.gemm_fp8(fa, fb, code, M, N, K, ba.ptr, lda, bb.ptr, ldb, bsa.ptr, bsb.ptr, bc.ptr, ldc)
    H.device_sync()
    raw = bc.to_numpy(nbytes + P.GUARD, np.uint8)
    img = raw[:nbytes].view(store).reshape(M, ldc)
    assert (img[:, N:].view(np.uint8) == FILL).all() and (raw[nbytes:] == FILL).all(), "bytes outside C[M, N] were written"
    return np.ascontiguousarray(img[:, :N])


def default_ldc(N):
    return N + 8 if N % 2 == 0 else N + 5    # rows of C that keep and that lose 16-byte alignment


def run(a, fa, b, fb, out, sa=1.0, sb=1.0, lda=None, ldb=None, ldc=None, repeat=1):
    """a [M, K], b [N, K] codes. Returns the decoded [M, N] window as f64 and asserts that the rest of the C allocation kept its poison."""
    (M, K), N = a.shape, b.shape[0]
    lda, ldb, ldc = lda or K + 16, ldb or K + 32, ldc or default_ldc(N)
    ba, bb, bsa, bsb = operand(a, lda), operand(b, ldb), scale(sa), scale(sb)
    results = [launch(ba, lda, bb, ldb, bsa, bsb, fa, fb, out, M, N, K, ldc) for _ in range(repeat)]
    for r in results[1:]:
        assert np.array_equal(r.view(np.uint8), results[0].view(np.uint8)), "two runs differ"
    return R.to_f32(results[0], out).astype(np.float64)


def int_codes(rng, shape, fmt):
    vals = rng.choice(INTS[fmt], size=shape)
    codes = R.encode(vals, fmt)
    assert np.array_equal(R.decode(codes, fmt), vals)
    return codes, vals


@pytest.mark.parametrize("fa,fb", PAIRS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact_integer_products(M, N, K, fa, fb):
    rng = np.random.default_rng(M * 7 + N * 3 + K + fa * 2 + fb)
    (a, av), (b, bv) = int_codes(rng, (M, K), fa), int_codes(rng, (N, K), fb)
    sa, sb = 2.0 ** -3, 2.0 ** 2
    want = (av @ bv.T) * sa * sb
    assert (np.abs(av) @ np.abs(bv).T).max() < 2 ** 24        # every partial sum is an integer f32 holds
    got = run(a, fa, b, fb, "f32", sa, sb, repeat=2)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {M * N} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_identity_a_returns_the_asymmetric_b(fa, fb):
    rng = np.random.default_rng(17 + fa * 2 + fb)
    K = 128
    a = R.encode(np.eye(K), fa)
    b, bv = int_codes(rng, (70, K), fb)
    assert not np.array_equal(bv[:70, :70], bv[:70, :70].T)
    got = run(a, fa, b, fb, "f32")
    assert np.array_equal(got, bv.T)


@pytest.mark.parametrize("fa,fb", [PAIRS[0], PAIRS[3]])
def test_one_hot_in_k_hits_every_byte_position(fa, fb):
    rng = np.random.default_rng(23 + fa)
    K, M, N = 128, 16, 16
    b, bv = int_codes(rng, (N, K), fb)
    col = rng.choice(INTS[fa][INTS[fa] != 0], size=M)
    for k in range(K):
        av = np.zeros((M, K))
        av[:, k] = col
        got = run(R.encode(av, fa), fa, b, fb, "f32")
        assert np.array_equal(got, np.outer(col, bv[:, k])), f"k = {k}"


def random_codes(rng, shape, fmt):
    c = rng.integers(0, 256, shape).astype(np.uint8)
    if fmt == R.E4M3:
        c[(c & 0x7f) == 0x7f] = 0x35          # no NaN
    else:
        c &= 0xbf                             # magnitudes below 2: no infinity, no NaN
    return c


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("M,N,K", SHAPES + [(512, 512, 4096)])
def test_rounded_products_within_the_bound(M, N, K, out):
    fa, fb = PAIRS[(M + K + len(out)) % 4]
    rng = np.random.default_rng(M + N + K)
    a, b = random_codes(rng, (M, K), fa), random_codes(rng, (N, K), fb)
    sa = 2.0 ** -9 if fa == R.E4M3 else 1.0    # e4m3 codes reach 448: bring the operands below 1, so that f16 holds the sum over K
    sb = 2.0 ** -9 if fb == R.E4M3 else 1.0
    c, mag = R.product(a, fa, b, fb, sa, sb)
    got = run(a, fa, b, fb, out, sa, sb)
    frac = R.gemm_frac(got, c, mag, out)
    print(f"gemm_fp8 {M}x{N}x{K} {out} formats ({fa}, {fb}): worst fraction of the bound {frac:.3f}")
    assert frac <= 1.0


def test_empty_products_write_nothing():
    a, b = np.zeros((4, 16), np.uint8), np.zeros((4, 16), np.uint8)
    ba, bb, s = operand(a, 16), operand(b, 16), scale(1.0)
    bc = H.DevBuf(256)
    P.fill(bc.ptr, 256, FILL)
    H.gemm_fp8(R.E4M3, R.E4M3, H.F32, 0, 4, 16, ba.ptr, 16, bb.ptr, 16, s.ptr, s.ptr, bc.ptr, 4)
    H.gemm_fp8(R.E4M3, R.E4M3, H.F32, 4, 0, 16, ba.ptr, 16, bb.ptr, 16, s.ptr, s.ptr, bc.ptr, 4)
    H.device_sync()
    assert (bc.to_numpy(256, np.uint8) == FILL).all()
