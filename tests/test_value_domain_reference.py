"""CPU only: the expectations of tests/test_gpu_ew_values.py are sound, and its vectors are sharp.

Soundness: the oracle and the numpy restatement (tests/value_domain.py) agree on every vector the GPU test feeds - bit for bit outside
NaN payloads, bf16 NaNs exactly 0x7FC0 - so a GPU mismatch is about the kernels (or the GPU's arithmetic mode), never about the
expectation. Sharpness: three wrong narrowing conversions, restated in numpy, each differ from the reference on the boundary vectors -
the GPU test fails for a kernel that rounds that way."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import value_domain as V


def test_vector_sizes_and_contents():
    a, b = V.f32_boundaries_f16(), V.f32_boundaries_bf16()
    extras = V.f32_extras().size
    assert a.size == 4 * 2 * 0x7C00 + extras == 253952 + extras and b.size == 4 * 2 * 0x7F80 + extras == 261120 + extras
    for v in (a, b):
        u = V.bits(v)
        for want in (0x477FE000, 0x477FF000, 0x47800000, 0x33800000, 0x33000000, 0x33000001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0, 0x80000000, 1,
                     0x7FC00001, 0xFFC12345):   # 65504, 65520, 65536, 2^-24, 2^-25 and its successor, FLT_MAX, +-inf, +-0, the smallest subnormal, NaNs
            assert (u == want).any(), hex(want)
    assert (V.bits(b) == 0x7F7F8000).any()   # a finite f32 that becomes bf16 inf
    for code in (V.F16, V.BF16):
        assert np.unique(V.bits(V.all_patterns16(code))).size == 65536
    for code in (V.F32, V.F64):
        s = V.float_specials(code)
        assert np.isnan(s).sum() == 1 and np.isinf(s).sum() == 2 and (V.bits(s) == 0).sum() == 1 and np.signbit(s[s == 0]).sum() == 1
    for code in (V.U8, V.I8):
        assert np.unique(V.int_domain(code)).size == 256


@pytest.mark.parametrize("code", [V.F16, V.BF16, V.F32, V.F64, V.U8, V.I8, V.I16, V.I32, V.I64])
def test_references_agree_same_dtype_arithmetic(code):
    avals, bvals = V.operand_vectors(code)
    a, b = V.with_pad(avals, code), V.with_pad(bvals, code)
    for op in V.OPS:
        for swap in (False, True):
            w, defined = V.expected_binary(op, a, code, b, code, swap)   # asserts the agreement
            assert w.shape == (b.size, a.size)
            if op == "div" and code in V.INTS:
                x, y = (b[:, None], a[None, :]) if swap else (a[None, :], b[:, None])
                undefined = (y == 0) | ((x == np.iinfo(x.dtype).min) & (y.astype(np.int64) == -1)) if code != V.U8 else (y == 0) | (x != x)
                assert np.array_equal(~defined, np.broadcast_to(undefined, defined.shape))   # exactly the two excluded classes, by the inputs
            else:
                assert defined.all()


def test_references_agree_mixed_dtype_arithmetic():
    for ca, avals, cb, bvals in V.mixed_pairs():
        for op in ("add", "sub", "mul"):
            for swap in (False, True):
                V.expected_binary(op, V.with_pad(avals, ca), ca, V.with_pad(bvals, cb), cb, swap)


def test_references_agree_convert_and_fill():
    for src, vals, dsts in V.convert_cases():
        for dst in dsts:
            V.expected_convert(V.with_pad(vals, src), src, dst)
    for code in V.FLOATS:
        for s in V.fill_scalars():
            V.expected_fill(s, code)
    # the scalar handed to a *_SCALAR operator is the vector's value again after fill's rounding
    for code in V.SAME_DTYPE_KERNEL:
        _, bvals = V.operand_vectors(code)
        for k in range(bvals.size):
            s = V.scalar_of(bvals, code, k)
            if s is not None and not V.is_nan(bvals[k:k + 1], code)[0]:
                got = O.fill(np.empty(1, dtype=V.NP[code]), s, dst_code=code)
                assert np.array_equal(V.bits(got), V.bits(bvals[k:k + 1])), (V.NAME[code], k)


def test_integer_wrap_and_wide_quotients_are_in_the_vectors():
    for code in (V.I32, V.I64):
        v = V.int_specials(code)
        w = 8 * v.dtype.itemsize
        exact = [[int(x) + int(y) for x in v] for y in v]
        assert any(not -(1 << (w - 1)) <= s < (1 << (w - 1)) for row in exact for s in row)            # a sum that wraps
        assert any(abs(int(x) * int(y)) >= 1 << (w - 1) for x in v for y in v)                         # a product that wraps
    v = V.int_specials(V.I64)
    assert any(abs(int(x)) > 1 << 32 and abs(int(y)) > 1 << 32 and abs(int(x)) // abs(int(y)) > 1 for x in v for y in v)  # both operands above 2^32, quotient > 1


# ---- sharpness: wrong converters, restated --------------------------------------------------------------------------
def _bf16_truncate(f):
    return (V.bits(f) >> np.uint32(16)).astype(np.uint16)


def _bf16_half_up(f):
    u = V.bits(f).astype(np.uint64)
    r = ((u + 0x8000) >> 16).astype(np.uint16)
    r[np.isnan(f)] = 0x7FC0
    return r


def _bf16_nan_keeps_payload(f):
    """round-to-nearest-even, a NaN keeps the top of its payload (quietened): what the hardware's packed converter does."""
    u = V.bits(f).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f)
    r[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def _f16_parts(f):
    """(|f| in float64, which are finite, the spacing of the f16 grid at |f|): x / ulp is exact in float64."""
    with np.errstate(invalid="ignore"):   # (a signalling NaN is quietened by the widening)
        x = np.abs(f.astype(np.float64))
    finite = np.isfinite(x)
    e = np.floor(np.log2(np.where(finite & (x > 0), x, 1.0)))
    ulp = 2.0 ** (np.maximum(e, -14) - 10)
    return x, finite, ulp


def _f16_from_rounded(f, mag):
    """magnitude (float64, already on the f16 grid or beyond its range) -> f16 bits with f's sign; beyond 65504 -> inf."""
    with np.errstate(all="ignore"):
        h = V.bits(np.where(mag > 65504, np.inf, mag).astype(np.float16))
    return (h | np.where(np.signbit(f), 0x8000, 0).astype(np.uint16)).astype(np.uint16)


def _f16_truncate(f):
    x, finite, ulp = _f16_parts(f)
    mag = np.where(finite, np.floor(x / ulp) * ulp, x)
    out = _f16_from_rounded(f, np.where(finite, np.minimum(mag, 65504), mag))
    out[np.isnan(f)] = 0x7E00
    return out


def _f16_half_up(f):
    x, finite, ulp = _f16_parts(f)
    mag = np.where(finite, np.floor(x / ulp + 0.5) * ulp, x)
    out = _f16_from_rounded(f, mag)
    out[np.isnan(f)] = 0x7E00
    return out


def _f16_nan_keeps_payload(f):
    with np.errstate(all="ignore"):
        out = V.bits(f.astype(np.float16)).copy()
    nan = np.isnan(f)
    out[nan] = ((V.bits(f)[nan] >> np.uint32(16)) & 0x8000 | 0x7C00 | 0x200 | ((V.bits(f)[nan] >> np.uint32(13)) & 0x3FF)).astype(np.uint16)
    return out


def test_wrong_converters_are_caught_by_the_boundary_vectors():
    f = V.f32_boundaries_bf16()
    want = V.expected_convert(f, V.F32, V.BF16)
    sane = V.np_f32_to_bf16(f)
    assert not V.mismatches(sane, want, V.BF16)[0].any()
    caught = {}
    for name, wrong in (("truncate", _bf16_truncate), ("half_up", _bf16_half_up), ("nan_payload", _bf16_nan_keeps_payload)):
        bad, _ = V.mismatches(wrong(f), want, V.BF16)
        caught["bf16 " + name] = int(bad.sum())
    # on non-NaN inputs the three stay what they claim to be: truncate <= RNE, half-up == RNE except on the ties to an even pattern
    ok = ~np.isnan(f)
    assert (_bf16_nan_keeps_payload(f)[ok] == sane[ok]).all()
    ties_to_even = ((V.bits(f) & np.uint32(0x1FFFF)) == 0x8000) & ok
    assert (_bf16_half_up(f) != sane)[ok].sum() == ties_to_even.sum() > 30000

    f = V.f32_boundaries_f16()
    want = V.expected_convert(f, V.F32, V.F16)
    with np.errstate(all="ignore"):
        sane = f.astype(np.float16)
    assert not V.mismatches(sane, want, V.F16)[0].any()
    ok = ~np.isnan(f)
    assert (_f16_nan_keeps_payload(f)[ok] == V.bits(sane)[ok]).all()
    for name, wrong in (("truncate", _f16_truncate), ("half_up", _f16_half_up)):
        bad, _ = V.mismatches(wrong(f).view(np.float16), want, V.F16)
        caught["f16 " + name] = int(bad.sum())
    # a payload-keeping f16 NaN is still a NaN: the rule lets it pass by design (only bf16 documents one NaN pattern); what the f16 vector
    # pins instead is the sign and quietness the hardware gives, through the exact-bits rule of everything that is not a NaN
    bad, nan_only = V.mismatches(_f16_nan_keeps_payload(f).view(np.float16), want, V.F16)
    assert not bad.any() and nan_only.sum() == np.isnan(f).sum()
    # a converter that flushes f16 subnormal results to zero
    with np.errstate(all="ignore"):
        flushed = np.where(np.abs(f) < 2.0 ** -14, np.copysign(np.float32(0), f), f).astype(np.float16)
    caught["f16 flush_subnormals"] = int(V.mismatches(flushed, want, V.F16)[0].sum())
    assert all(n > 0 for n in caught.values()), caught
    # truncation is wrong at least on every point just above a tie (one per finite pattern), half-up on every tie to an even pattern (every other one),
    # a kept payload at least on the vector's four NaNs with the sign bit set
    assert caught["bf16 truncate"] >= 2 * 0x7F80 and caught["bf16 half_up"] >= 0x7F80 - 1 and caught["bf16 nan_payload"] >= 4, caught
    assert caught["f16 truncate"] >= 2 * 0x7C00 and caught["f16 half_up"] >= 0x7C00 - 1, caught
