"""The reference of the per-tensor scaled FP8 entries (kf_fp8_amax, kf_fp8_quantize, kf_gemm_fp8, linear_fp8). numpy only.

Formats: the OCP encodings gfx950 uses. e4m3fn: bias 7, no infinity, NaN = 0x7f / 0xff, largest value 448. e5m2: bias 15, IEEE-like,
largest finite value 57344. decode is the 256-entry table; encode rounds to nearest even AFTER the explicit clamp to +-fmt_max, and a
NaN becomes 0x7f with the input's sign bit. The scale is 2^e, e the largest integer with amax 2^e <= fmt_max, clamped to [-126, 126],
e = 0 for amax 0, infinite or NaN. The product reference is the f64 product of the decoded operands times the two scale_inv values, with
mag = |A| |B|^T beside it; gemm_bound is the acceptance bound of a kf_gemm_fp8 output:

    |got - c| <= eps_out |c| + ACC_TERM mag + half a subnormal ulp

eps_out and the subnormal ulp of bf16 / f16 are oracle/checks.py's (EPS, ABS_ULP), 2^-24 and 2^-149 stand for f32. CHECKS_ACC_TERM = 1e-6
is the accumulation term of oracle/checks.gemm_ok (tests/test_fp8_ref.py probes gemm_ok and asserts the two agree): the f32 accumulation
noise relative to the sum of the terms' magnitudes. It does NOT hold for v_mfma_scale_f32_16x16x128_f8f6f4, on a kernel that passes the
whole exact tier of tests/test_gpu_gemm_fp8.py: measured on MI355X, the instruction adds the 128 products of one issue in fixed point,
aligned to the largest of them and cut no more than 16 bits below it BEFORE the sum (2^16 + 1 gives 2^16, 2^16 - 2^16 + 1 gives 0 inside one
issue; the same terms in two issues are summed exactly, subnormal operands are honoured, operands of one binade give the exact sum).
On random codes over the formats' whole range the worst |got - c| / mag is 1.87e-4 (187 times 1e-6, at (64, 64, 112); every shape's
figure is in profiles/r06_gemm_fp8_bench.json, `block_sum`). ACC_TERM is twice that, the convention of oracle/checks.py; it is still 10 times
below bf16's output rounding and rejects the mutants of tests/test_fp8_ref.py.
"""
import math

import numpy as np

from oracle import checks as CK
from oracle import oracle as O

E4M3, E5M2 = 0, 1
FMT_MAX = {E4M3: 448.0, E5M2: 57344.0}
FMT_POW = {E4M3: 9, E5M2: 16}          # fmt_max = 0.875 * 2^pow
UNIT = {E4M3: 2.0 ** -4, E5M2: 2.0 ** -3}       # half an ulp, relative: 3 and 2 mantissa bits
SUBNORMAL = {E4M3: 2.0 ** -9, E5M2: 2.0 ** -16}  # the spacing of the subnormal grid
CHECKS_ACC_TERM = 1e-6
ACC_TERM = 3.8e-4
EPS_OUT = {"f32": 2.0 ** -24, "bf16": CK.EPS[O.BF16], "f16": CK.EPS[O.F16]}
ABS_ULP = {"f32": 2.0 ** -149, "bf16": CK.ABS_ULP[O.BF16], "f16": CK.ABS_ULP[O.F16]}


def _table(fmt):
    out = np.empty(256, dtype=np.float64)
    for b in range(256):
        s = -1.0 if b & 0x80 else 1.0
        if fmt == E4M3:
            e, m = (b >> 3) & 15, b & 7
            v = math.nan if (e == 15 and m == 7) else (m / 8.0 * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7))
        else:
            e, m = (b >> 2) & 31, b & 3
            v = (math.inf if m == 0 else math.nan) if e == 31 else (m / 4.0 * 2.0 ** -14 if e == 0 else (1 + m / 4.0) * 2.0 ** (e - 15))
        out[b] = s * v
    return out


TABLE = {E4M3: _table(E4M3), E5M2: _table(E5M2)}
_NFINITE = {E4M3: 0x7f, E5M2: 0x7c}    # codes 0 .. n - 1 are the non-negative finite values, ascending
GRID = {f: TABLE[f][:_NFINITE[f]].copy() for f in (E4M3, E5M2)}


def decode(codes, fmt):
    return TABLE[fmt][np.asarray(codes, dtype=np.uint8)]


def encode(x, fmt):
    """f32 (or anything exactly convertible to f64) -> codes: clamp to +-fmt_max, round to nearest even; NaN -> 0x7f | sign."""
    x = np.asarray(x, dtype=np.float64)
    sign = np.where(np.signbit(x), 0x80, 0).astype(np.uint8)
    nan = np.isnan(x)
    a = np.minimum(np.abs(np.where(nan, 0.0, x)), FMT_MAX[fmt])
    g = GRID[fmt]
    hi = np.clip(np.searchsorted(g, a, side="left"), 1, len(g) - 1)
    lo = hi - 1
    dlo, dhi = a - g[lo], g[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    code = np.where(pick_hi, hi, lo).astype(np.uint8)
    return np.where(nan, np.uint8(0x7f), code) | sign


def amax_bits(x32):
    """The f32 bit pattern kf_fp8_amax leaves: the integer maximum of the bits of |x|, any NaN as 0x7fc00000; 0 for no elements."""
    b = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).ravel() & np.uint32(0x7fffffff)
    if b.size == 0:
        return 0
    b = np.where(b > 0x7f800000, np.uint32(0x7fc00000), b)
    return int(b.max())


def scale_exp(amax, fmt):
    amax = float(np.float32(amax))
    if amax == 0.0 or math.isinf(amax) or math.isnan(amax):
        return 0
    m, ex = math.frexp(abs(amax))
    e = FMT_POW[fmt] - ex - (1 if m > 0.875 else 0)
    return max(-126, min(126, e))


def quantize(x32, fmt, amax=None):
    """x32: f32 array [rows, cols] (the exact values of the f32 / f16 / bf16 input). Returns (q [rows, cols], qt [cols, ceil16(rows)]
    with the zero pad, scale_inv as f32, the amax bit pattern)."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    bits = amax_bits(x32) if amax is None else int(np.float32(amax).view(np.uint32))
    e = scale_exp(np.uint32(bits).view(np.float32), fmt)
    with np.errstate(over="ignore", invalid="ignore"):
        prod = x32 * np.float32(2.0 ** e)      # exact: a power of two (down to the f32 subnormals, which round to FP8 zero anyway)
    q = encode(prod, fmt)
    q = np.where(np.isnan(x32), np.uint8(0x7f) | np.where(np.signbit(x32), 0x80, 0).astype(np.uint8), q)
    rows, cols = x32.shape
    qt = np.zeros((cols, (rows + 15) // 16 * 16), dtype=np.uint8)
    qt[:, :rows] = q.T
    return q, qt, np.float32(2.0 ** -e), bits


def product(a_codes, fmt_a, b_codes, fmt_b, sa=1.0, sb=1.0):
    """(c, mag): the f64 product sa sb A B^T of the decoded operands [M, K], [N, K] and sa sb |A| |B|^T."""
    a, b = decode(a_codes, fmt_a), decode(b_codes, fmt_b)
    s = float(sa) * float(sb)
    return s * (a @ b.T), abs(s) * (np.abs(a) @ np.abs(b).T)


def gemm_bound(c, mag, out):
    return EPS_OUT[out] * np.abs(c) + ACC_TERM * mag + 0.5 * ABS_ULP[out]


def gemm_frac(got, c, mag, out):
    """Worst |got - c| as a fraction of the bound (<= 1 passes); inf when got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - c) / gemm_bound(c, mag, out)).max())


def quant_delta(v, scale, fmt):
    """Per element, the worst error of quantising v with the given scale: max(u |v|, sub / (2 scale))."""
    return np.maximum(UNIT[fmt] * np.abs(v), SUBNORMAL[fmt] / (2.0 * scale))


def end_to_end_bound(a, b, scale_a, fmt_a, scale_b, fmt_b):
    """sum_k (|a| db + |b| da + da db) for the product a [M, K] b [N, K]^T of UNQUANTISED operands."""
    da, db = quant_delta(a, scale_a, fmt_a), quant_delta(b, scale_b, fmt_b)
    return np.abs(a) @ db.T + da @ np.abs(b).T + da @ db.T


# ---- element types of the inputs and outputs ------------------------------------------------------------------------------------
def to_f32(stored, dt):
    """stored elements (f32 / f16 as their numpy types, bf16 as uint16) -> the f32 values they hold."""
    if dt == "bf16":
        return (np.ascontiguousarray(stored, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
    return np.asarray(stored).astype(np.float32)


def round_to(x, dt):
    """f64 -> stored elements of dt, round to nearest even."""
    x = np.asarray(x, dtype=np.float64)
    if dt == "f32":
        return x.astype(np.float32)
    if dt == "f16":
        return x.astype(np.float16)
    b = x.astype(np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


STORE = {"f32": np.float32, "f16": np.float16, "bf16": np.uint16}
