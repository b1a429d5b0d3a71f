"""Value vectors, lane layouts and the two references for the bit-exact kernels (kf_elementwise: arithmetic, scalar forms, copy,
convert, fill). Nothing here touches a GPU: tests/test_value_domain_reference.py holds the two references to each other on every
vector on the CPU, tests/test_gpu_ew_values.py holds the kernels to them.

The two references of every operation:
  * the project's oracle (oracle.c: the reference's loops restated in C - accumulate type of the common dtype, cast on store);
  * plain numpy written out below - f32 / f64 as is, f16 as op(float32) -> astype(float16), bf16 with the integer rounding
    (u + 0x7FFF + ((u >> 16) & 1)) >> 16 and NaN -> 0x7FC0, integer + - * in the numpy dtype with wrap, integer / truncating toward
    zero in Python ints.
The comparison rule (mismatches): bit for bit wherever the EXPECTED value is not a NaN (signed zeros, infinities, subnormals
included); where it is a NaN the result must be a NaN, and for a bf16 result exactly 0x7FC0; copies are exact bits throughout."""
import numpy as np

from oracle import oracle as O

BOOL, U8, I8, I16, I32, I64, F16, BF16, F32, F64 = range(10)   # == oracle.oracle == kfunca_amd.hip_abi
NAME = {U8: "u8", I8: "i8", I16: "i16", I32: "i32", I64: "i64", F16: "f16", BF16: "bf16", F32: "f32", F64: "f64"}
NP = O.CODE2NP
FLOATS = (F16, BF16, F32, F64)
INTS = (U8, I8, I16, I32, I64)
OPS = {"add": O.ADD, "sub": O.SUB, "mul": O.MUL, "div": O.DIV}
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def esize(code):
    return np.dtype(NP[code]).itemsize


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(_UINT[x.dtype.itemsize])


def is_nan(x, code):
    if code == BF16:
        return (np.asarray(x) & np.uint16(0x7FFF)) > np.uint16(0x7F80)
    if code in FLOATS:
        return np.isnan(x)
    return np.zeros(np.shape(x), dtype=bool)


def of_f64(values, code):
    """Python / float64 values -> an array of dtype `code` (bf16 as bits); every value given here is exact in `code` or meant to round."""
    with np.errstate(all="ignore"):
        v = np.asarray(values, dtype=np.float64)
        if code == BF16:
            return np_f32_to_bf16(v.astype(np.float32))
        if code == F16:
            return v.astype(np.float32).astype(np.float16)
        return v.astype(NP[code])


def one(code):
    return of_f64([1.0], code) if code in FLOATS else np.ones(1, dtype=NP[code])


def with_pad(vals, code):
    """The vector followed by the pad value 1: layouts index it, the pad sits at index len(vals)."""
    return np.concatenate([vals, one(code)])


# ---- value vectors ---------------------------------------------------------------------------------------
def all_patterns16(code):
    """Every bit pattern of a 16-bit float type: all subnormals, both zeros and infinities, every NaN payload of both signs."""
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    return u.view(np.float16) if code == F16 else u


# NaNs of both signs with payloads (quiet and signalling), +-inf, +-0, the f16 overflow boundary (65504 largest finite, 65520 the tie that
# rounds to inf, 65536), the f16 underflow boundary (2^-24 smallest subnormal, 2^-25 the tie that rounds to zero, and its successor),
# the largest finite f32 (-> bf16 inf), the smallest f32 subnormal
_F32_EXTRA_BITS = [0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00000, 0xFFC00000,
                   0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF]
_F32_EXTRA_VALUES = [65504.0, 65520.0, 65536.0, -65504.0, -65520.0, -65536.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -24, -2.0 ** -25]


def f32_extras():
    v = np.array(_F32_EXTRA_VALUES, dtype=np.float32)
    succ = (bits(np.array([2.0 ** -25, -2.0 ** -25], dtype=np.float32)) + np.uint32(1)).view(np.float32)
    return np.concatenate([np.array(_F32_EXTRA_BITS, dtype=np.uint32).view(np.float32), v, succ])


def _both_signs(mag):
    return np.concatenate([mag, mag | np.uint32(0x80000000)]).astype(np.uint32).view(np.float32)


def f32_boundaries_f16():
    """For every finite f16 value: the value, the midpoint to the next pattern (float64 arithmetic, exact in f32) and that midpoint's two
    f32 neighbours; the largest finite's next pattern counts as 2^16, so its midpoint is 65520. 4 x 2 x 31744 = 253952 values + extras."""
    lo = np.arange(0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    hi = np.append(lo[1:], 65536.0)
    mid64 = (lo + hi) / 2
    mid = mid64.astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    mb = bits(mid)
    mag = np.stack([bits(lo.astype(np.float32)), mb - np.uint32(1), mb, mb + np.uint32(1)], axis=1).ravel()
    return np.concatenate([_both_signs(mag), f32_extras()])


def f32_boundaries_bf16():
    """For every finite bf16 pattern b: b << 16 and the three f32 around the tie above it (+0x7FFF, +0x8000, +0x8001); the largest
    finite's tie 0x7F7F8000 is a finite f32 that rounds to inf. 4 x 2 x 32640 = 261120 values + extras."""
    b = np.arange(0x7F80, dtype=np.uint32) << np.uint32(16)
    mag = np.stack([b, b + np.uint32(0x7FFF), b + np.uint32(0x8000), b + np.uint32(0x8001)], axis=1).ravel()
    return np.concatenate([_both_signs(mag), f32_extras()])


def float_specials(code):
    """f32 / f64 arithmetic operands (21 values): +-0, +-1, +-inf, NaN, smallest and largest subnormal, smallest normal, largest finite (both signs),
    1/3 (both signs), 0.1, 1e+-20, and around the end of the exact integers 2^p - 1, 2^p and 2^p + 2 (p = 24 / 53: 2^p + 1 is not a value
    of the type - it is the tie that 2^p + 1 must round to even, and (2^p + 2) + 1 the one that rounds up)."""
    dt = NP[code]
    fi = np.finfo(dt)
    p = 24 if code == F32 else 53
    sub_max = (bits(np.array([fi.tiny], dtype=dt)) - 1).view(dt)[0]
    v = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal, sub_max, fi.tiny, fi.max, -fi.max,
         dt(1) / dt(3), -(dt(1) / dt(3)), dt(0.1), 2 ** p - 1, 2 ** p, 2 ** p + 2, dt(1e20), dt(1e-20)]
    out = np.array(v, dtype=dt)
    assert [int(x) for x in out[16:19]] == [2 ** p - 1, 2 ** p, 2 ** p + 2]
    return out


def partners16(code):
    """The 8 partners of the f16 / bf16 all-pattern sweeps: 1, -0, 3, the largest finite, the smallest subnormal, +inf, a NaN, 1/3."""
    if code == F16:
        return np.array([0x3C00, 0x8000, 0x4200, 0x7BFF, 0x0001, 0x7C00, 0x7E01, 0x3555], dtype=np.uint16).view(np.float16)
    return np.array([0x3F80, 0x8000, 0x4040, 0x7F7F, 0x0001, 0x7F80, 0x7FC1, 0x3EAB], dtype=np.uint16)


def int_specials(code):
    """MIN, MAX, MAX/2 + 1, -1, 0, 1, 3 and two full-width constants of no particular shape (for u8: MIN = 0, MAX = 255, no -1)."""
    ii = np.iinfo(NP[code])
    consts = {U8: [0x5A, 0xC7], I8: [0x35, -0x4E], I16: [12345, -23456], I32: [0x6B8B4567, -0x327B23C6],
              I64: [0x2545F4914F6CDD1D, -0x61C8864680B583EB]}[code]
    v = [ii.min, ii.max, ii.max // 2 + 1, 0, 1, 3] + ([] if code == U8 else [-1]) + consts
    return np.array(v, dtype=NP[code])


def int_domain(code):
    """All 256 values of a one-byte integer type."""
    return np.arange(256, dtype=np.uint8).view(NP[code])


def fill_scalars():
    """+-inf, NaN, -0.0, 65520 (f16: the tie that rounds to inf), 1e-8 (f16: below half the smallest subnormal), 3.4e38 (bf16: rounds to inf),
    1e39 (f32: overflows to inf), and for the f16 subnormal range 1e-7, the tie 2^-25 (to zero) and the tie 3 * 2^-25 (to even: 2 * 2^-24)."""
    return [np.inf, -np.inf, np.nan, -0.0, 65520.0, 1e-8, 3.4e38, 1e39, -1e39, 1e-7, 2.0 ** -25, 3 * 2.0 ** -25, -65519.99, 1e-40]


# ---- the numpy reference -----------------------------------------------------------------------------------
def np_f32_to_bf16(f):
    f = np.ascontiguousarray(f, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC0
    return r


def np_bf16_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def np_promote(ca, cb):
    """The common dtype of the pairs used here: float with float and signed integer with signed integer -> the later code; float with integer -> the float."""
    fa, fb = ca in FLOATS, cb in FLOATS
    if fa != fb:
        return ca if fa else cb
    assert fa or (U8 not in (ca, cb)) or ca == cb
    return max(ca, cb)


def _to_acc(x, code, acc):
    """static_cast of a stored value to the accumulate type (np.float32, np.float64 or an integer dtype that holds it)."""
    with np.errstate(all="ignore"):
        if code == BF16:
            x = np_bf16_to_f32(x).reshape(np.shape(x))
        return x.astype(acc)


def _from_f32(f, code):
    with np.errstate(all="ignore"):
        if code == BF16:
            return np_f32_to_bf16(f).reshape(np.shape(f))
        return f.astype(NP[code])


def np_convert(x, src, dst):
    """x (dtype src) -> dtype dst: through float32 for a 16- or 32-bit float result (so f64 -> f16 rounds twice, as the reference's
    cast-on-store does), through float64 for f64, through int64 with wrap for an integer result (integer sources only)."""
    if src == dst:
        return x.copy()
    if dst in (F16, BF16, F32):
        return _from_f32(_to_acc(x, src, np.float32), dst)
    if dst == F64:
        return _to_acc(x, src, np.float64)
    assert src in INTS, "float -> integer of NaN / out-of-range values is undefined: not part of these vectors"
    return x.astype(np.int64).astype(NP[dst])


def _wrap(q, dt):
    w = 8 * np.dtype(dt).itemsize
    q &= (1 << w) - 1
    return q - (1 << w) if np.dtype(dt).kind == "i" and q >> (w - 1) else q


def np_binary(op, a, b, ca, cb):
    """a (op) b with broadcasting -> (result in the common dtype, mask of DEFINED elements). Undefined: an integer division by zero
    or of MIN by -1 (the result there is 0 and is never compared)."""
    common = np_promote(ca, cb)
    shape = np.broadcast_shapes(a.shape, b.shape)
    defined = np.ones(shape, dtype=bool)
    with np.errstate(all="ignore"):
        if common in FLOATS:
            acc = np.float64 if common == F64 else np.float32
            x, y = _to_acc(a, ca, acc), _to_acc(b, cb, acc)
            r = x + y if op == "add" else x - y if op == "sub" else x * y if op == "mul" else x / y
            assert r.dtype == acc
            return (r if common == F64 else _from_f32(r, common)), defined
        dt = NP[common]
        x, y = np.broadcast_to(a.astype(dt), shape), np.broadcast_to(b.astype(dt), shape)
        if op != "div":
            r = x + y if op == "add" else x - y if op == "sub" else x * y
            assert r.dtype == dt
            return r, defined
        lo = int(np.iinfo(dt).min)
        out = np.zeros(shape, dtype=dt)
        for idx in np.ndindex(*shape):
            p, q = int(x[idx]), int(y[idx])
            if q == 0 or (lo < 0 and p == lo and q == -1):
                defined[idx] = False
                continue
            mag = abs(p) // abs(q)   # truncation toward zero
            out[idx] = _wrap(mag if (p < 0) == (q < 0) else -mag, dt)
        return out, defined


def np_fill(value, code, n=1):
    """fill_(double): the value is cast to the accumulate type of the dtype (float for f16 / bf16 / f32), then to the dtype."""
    with np.errstate(all="ignore"):
        v = np.full(n, value, dtype=np.float64)
        return v if code == F64 else _from_f32(v.astype(np.float32), code)


# ---- the comparison rule -----------------------------------------------------------------------------------
def mismatches(got, want, code, exact=False):
    """(mask of elements that break the rule, mask of elements compared by NaN-ness only). The NaN relaxation is decided from `want`
    alone; `exact` (same-dtype copies) switches it off; a bf16 NaN must be 0x7FC0 and is therefore compared bit for bit."""
    assert np.shape(got) == np.shape(want) and np.asarray(got).dtype == np.asarray(want).dtype, (np.shape(got), np.shape(want))
    g, w = bits(got), bits(want)
    bad = g != w
    if exact or code not in FLOATS:
        return bad, np.zeros(g.shape, dtype=bool)
    nan = is_nan(np.ascontiguousarray(want), code)
    if code == BF16:
        w = np.where(nan, np.uint16(0x7FC0), w)
        return g != w, np.zeros(g.shape, dtype=bool)
    return np.where(nan, ~is_nan(np.ascontiguousarray(got), code), bad), nan


def assert_match(got, want, code, what, exact=False, tally=None, key=None):
    bad, nan_only = mismatches(got, want, code, exact)
    if bad.any():
        at = np.flatnonzero(bad.ravel())[:6]
        g, w = bits(got).ravel(), bits(want).ravel()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {at.tolist()}: got "
                             f"{[hex(int(v)) for v in g[at]]}, want {[hex(int(v)) for v in w[at]]}")
    if tally is not None:
        t = tally.setdefault(key, [0, 0, 0])
        t[0] += bad.size
        t[1] += int(is_nan(np.ascontiguousarray(want), code).sum()) if code in FLOATS else 0
        t[2] += int(nan_only.sum())


# ---- expected values: both references, held to each other ------------------------------------------------------------
def expected_binary(op, avals, ca, bvals, cb, swap=False):
    """W[k, i] = avals[i] (op) bvals[k] (swap: bvals[k] (op) avals[i]) and the mask of defined pairs: computed by the oracle AND by numpy,
    which must agree under the comparison rule on every defined pair."""
    A, B = np.ascontiguousarray(avals)[None, :], np.ascontiguousarray(bvals)[:, None]
    x, y, cx, cy = (B, A, cb, ca) if swap else (A, B, ca, cb)
    w_np, defined = np_binary(op, x, y, cx, cy)
    w_or = O.binary(OPS[op], x, y, a_code=cx, b_code=cy)
    common = np_promote(cx, cy)
    assert O.promote(cx, cy) == common
    bad, _ = mismatches(w_or, w_np, common)
    bad &= defined
    assert not bad.any(), (op, NAME[ca], NAME[cb], swap, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return w_np, defined


def expected_convert(vals, src, dst):
    w_np = np_convert(vals, src, dst)
    w_or = O.convert(np.ascontiguousarray(vals), dst, src_code=src)
    bad, _ = mismatches(w_or, w_np, dst, exact=src == dst)
    assert not bad.any(), (NAME[src], NAME[dst], int(bad.sum()), np.flatnonzero(bad)[:4].tolist())
    return w_np


def expected_fill(value, code):
    w_np = np_fill(value, code)
    w_or = O.fill(np.empty(1, dtype=NP[code]), value, dst_code=code)
    bad, _ = mismatches(w_or, w_np, code)
    assert not bad.any(), (value, NAME[code], bits(w_or), bits(w_np))
    return w_np


# ---- layouts: index vectors into with_pad(vals) ---------------------------------------------------------------------
def lanes_of(*codes):
    """Positions a value must visit: the elements of a 16-byte pack (16 for one-byte types, 8 for two-byte ones) and never fewer than the
    8 elements one lane of the wide mixed-dtype and convert kernels handles."""
    return max([8] + [16 // esize(c) for c in codes])


def flat_pairs(la, lb, lanes):
    """(ia, ib): one block [pad, a_0 .. a_(la-1), pad ...] of length m + 1 (m = la rounded up to `lanes`) per b value, repeated to at least
    `lanes` blocks - block j starts one lane after block j-1, so every a value and every b value sits in every lane and every pair occurs.
    A pad pairs with a pad."""
    m = -(-la // lanes) * lanes
    nblocks = -(-max(lanes, lb) // lb) * lb
    blk = np.full(m + 1, la, dtype=np.int64)
    blk[1:la + 1] = np.arange(la)
    ia = np.tile(blk, nblocks)
    ib = np.repeat(np.arange(nblocks, dtype=np.int64) % lb, m + 1)
    ib[ia == la] = lb
    return ia, ib


def row_pairs(la, lb, lanes, mult):
    """(ia, ib) of shape [rows, cols] for a b operand that is ONE value per row (broadcast along the row): row j holds j % lanes pads, then
    the a values, then pads up to a multiple of `mult`; its b value is b_(j % lb)."""
    rows = -(-max(lanes, lb) // lb) * lb
    cols = -(-(la + lanes) // mult) * mult
    ia = np.full((rows, cols), la, dtype=np.int64)
    for j in range(rows):
        ia[j, j % lanes:j % lanes + la] = np.arange(la)
    ib = np.broadcast_to((np.arange(rows, dtype=np.int64) % lb)[:, None], (rows, cols)).copy()
    return ia, ib


def flat_single(l, lanes):
    """Index vector for a one-operand kernel: `lanes` copies of the vector, copy r one lane after copy r-1."""
    return flat_pairs(l, 1, lanes)[0]


def fit(idx, n, pad):
    """idx extended with pads to n entries."""
    assert n >= idx.size
    return np.concatenate([idx, np.full(n - idx.size, pad, dtype=np.int64)])


# ---- the cases: what is fed to which operation (shared by the CPU agreement test and the GPU test) ----------------------------------
def operand_vectors(code):
    """(a values, b values) of the same-dtype arithmetic of `code`: the full cross product is computed."""
    if code in (F32, F64):
        return float_specials(code), float_specials(code)
    if code in (F16, BF16):
        return all_patterns16(code), partners16(code)
    if code in (U8, I8):
        return int_domain(code), int_specials(code)
    return int_specials(code), int_specials(code)


SAME_DTYPE_KERNEL = (F16, BF16, F32, F64, I32, I64)   # launch_same<T>; u8 / i8 / i16 arithmetic runs in launch_cast<int64_t>


def mixed_pairs():
    """(ca, a values, cb, b values) with ca != cb: every accumulate class, results stored as bf16, f32, f64 and i64, integers beyond 2^24 /
    2^53 converted to float on load."""
    return [(F32, float_specials(F32), BF16, partners16(BF16)),
            (F16, all_patterns16(F16), F32, float_specials(F32)[:8]),
            (BF16, all_patterns16(BF16), F16, partners16(F16)),
            (F32, float_specials(F32), F64, float_specials(F64)),
            (I32, int_specials(I32), I64, int_specials(I64)),
            (I64, int_specials(I64), F32, float_specials(F32)),
            (I64, int_specials(I64), F64, float_specials(F64)),
            (I16, int_specials(I16), BF16, partners16(BF16))]


def convert_cases():
    """(source dtype, values, destination dtypes). Float -> integer is left out (NaN and out-of-range values are undefined there)."""
    b16 = f32_boundaries_f16()
    bb = f32_boundaries_bf16()
    with np.errstate(invalid="ignore"):   # (a signalling NaN is quietened by the widening)
        wide = np.concatenate([float_specials(F64), b16[::7].astype(np.float64), bb[::7].astype(np.float64)])   # (7: every fourth kind of point is kept)
    return [(F32, b16, (F16, BF16, F64, F32)),
            (F32, bb, (BF16, F16)),
            (F16, all_patterns16(F16), (F32, BF16, F64, F16)),
            (BF16, all_patterns16(BF16), (F32, F16, F64, BF16)),
            (F64, wide, (F32, F16, BF16, F64)),
            (I64, int_specials(I64), (F32, F16, BF16, F64, I32, I16, I8, U8)),
            (I32, int_specials(I32), (F32, F16, BF16, F64, I64, I16, I8, U8)),
            (U8, int_domain(U8), (F16, BF16, F32, I8, I64)),
            (I8, int_domain(I8), (F16, BF16, F32, U8, I64))]


def scalar_of(vals, code, k):
    """vals[k] as the Python float a caller would pass to a *_SCALAR operator or fill, or None when no double holds it exactly
    (or when double -> int64 would overflow)."""
    if code == BF16:
        return float(np_bf16_to_f32(vals[k:k + 1])[0])
    if code in FLOATS:
        return float(vals[k])
    v = int(vals[k])
    return float(v) if int(float(v)) == v and v < 2 ** 63 else None
