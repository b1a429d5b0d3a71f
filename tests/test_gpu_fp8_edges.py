"""-m gpu: the per-tensor FP8 entries at the grid sizes, value edges and offsets the other FP8 tests stop short of. Bit for bit against
tests/fp8_ref.py unless a test says otherwise; the shapes come from tests/fp8_geometry.py, whose claims tests/test_fp8_ref.py checks.

1. kf_fp8_amax over its whole grid: a second (and third) trip of the row loop, first trips whose u = 1..3 loads are real rows,
   blockIdx.x > 0; one larger value planted at every corner of that walk, a NaN in the last element; bf16 and f32, 16-byte and element loads.
2. kf_fp8_quantize under a caller's amax (all 65536 bf16 / f16 patterns: values beyond the bound and +-inf saturate, NaN stays NaN), the
   scale exponent's clamp to 126 with f32 subnormals, an all-subnormal bf16 matrix.
3. kf_gemm_fp8 on 8 to 161 tiles: whole groups of 8 tile rows beyond the first, ragged last groups. Exact integers.
4. kf_gemm_fp8 on every code byte: every finite code at every byte position of the instruction (ACC_TERM bound), and one NaN / infinity
   byte against the same problem without it (no tolerance).
5. Addressing: rows of A, B, C, x, q and qt that start beyond byte 2^32, and the largest legal K and leading dimension.
6. kfunca.linear_fp8 at T = 16500.

The multi-GiB cases fill their allocation once and then move kilobytes: rows go up one by one, results come back as the rows' windows and
256 bytes behind each."""
import time
import types

import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import fp8_geometry as GEO
from tests import fp8_ref as R
from tests import poison as P
from tests import test_gpu_fp8_quantize as Q
from tests import test_gpu_gemm_fp8 as G
from tests import test_gpu_linear_fp8 as L
from tests.test_gpu_norm_walk import h2d_rows

pytestmark = pytest.mark.gpu

ES = {"bf16": 2, "f16": 2, "f32": 4}
FMTS = [R.E4M3, R.E5M2]
SAT = {R.E4M3: 0x7e, R.E5M2: 0x7b}       # the code of +fmt_max
GAP_BYTES = 256                          # what the large cases read back behind each row


# ---- 1. kf_fp8_amax over its whole grid ------------------------------------------------------------------------------------------
def background(rows, cols, dt, seed):
    """|x| <= 1 everywhere (bf16 by truncation, which cannot grow a magnitude)."""
    x = np.random.default_rng(seed).random((rows, cols), dtype=np.float32) * np.float32(2) - np.float32(1)
    return (x.view(np.uint32) >> 16).astype(np.uint16) if dt == "bf16" else x


def planted_positions(rows, cols):
    gx, gy = GEO.amax_grid(rows, cols)
    rs = [r for r in (0, gy - 1, gy, 4 * gy - 1, 4 * gy, rows - 1) if 0 <= r < rows]
    return sorted({(r, c) for r in rs for c in (0, cols - 1, (gx - 1) * GEO.AMAX_STRIP)})


def put(ptr, stored):
    stored = np.ascontiguousarray(stored)
    H.check(H.lib().kf_memcpy_h2d(ptr, stored.ctypes.data, stored.nbytes, None))


def amax_of(dt, rows, cols, ld, ptr, out):
    P.fill(out.ptr, 4, 0xFF)
    H.fp8_amax(Q.CODE[dt], rows, cols, ld, ptr, out.ptr)
    H.device_sync()
    return int(out.to_numpy(1, np.uint32)[0])


def pitches(cols, dt):
    """(ld, elements the matrix starts behind the 16-byte aligned allocation): the 16-byte path, then the element path. cols + 3 can be
    a 16-byte pitch itself (4100 f32); the matrix then starts one element in, which takes the vector path away just as well."""
    per = 16 // ES[dt]
    aligned, odd = -(-cols // per) * per, cols + 3
    return [(aligned, 0), (odd, 1 if odd * ES[dt] % 16 == 0 else 0)]


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", list(GEO.AMAX_SHAPES))
def test_amax_finds_a_value_planted_anywhere_in_its_walk(rows, cols, dt):
    es = ES[dt]
    bg = background(rows, cols, dt, rows + cols)
    bg_bits = R.amax_bits(R.to_f32(bg, dt))
    assert bg_bits <= 0x3f800000
    out = H.DevBuf(4)
    for pitched, (ld, shift) in enumerate(pitches(cols, dt)):
        assert GEO.amax_vector_path(cols, ld, es, shift * es, 0) == (not pitched)
        host = np.full(rows * ld + 16, Q.GAP[dt], dtype=R.STORE[dt])
        host[shift:shift + rows * ld].reshape(rows, ld)[:, :cols] = bg
        buf = H.DevBuf.from_numpy(host)
        del host
        base = buf.ptr + shift * es
        assert amax_of(dt, rows, cols, ld, base, out) == bg_bits
        # the reference of a run is R.amax_bits of the matrix with the value in it; a maximum composes, so that is the larger of the
        # background's (computed once: it is the large array) and the planted element's
        for i, (r, c) in enumerate(planted_positions(rows, cols)):
            v = R.round_to(np.array([(2.0 + i / 64.0) * (-1) ** i]), dt)          # a different magnitude every time: no stale result passes
            want = max(bg_bits, R.amax_bits(R.to_f32(v, dt)))
            assert want > bg_bits
            at = base + (r * ld + c) * es
            put(at, v)
            got = amax_of(dt, rows, cols, ld, base, out)
            put(at, bg[r, c:c + 1])
            assert got == want, f"{rows}x{cols} {dt} ld {ld}: planted at ({r}, {c}): amax bits {got:#x}, expected {want:#x}"
        put(base + ((rows - 1) * ld + cols - 1) * es, np.array([Q.GAP[dt]]))
        assert amax_of(dt, rows, cols, ld, base, out) == 0x7fc00000, f"{rows}x{cols} {dt} ld {ld}: a NaN in the last element"
        buf.free()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", GEO.AMAX_QUANTIZED)
def test_quantize_after_an_amax_over_the_larger_grid(rows, cols, dt):
    gx, gy = GEO.amax_grid(rows, cols)
    x = background(rows, cols, dt, rows * cols)
    r, c = min(4 * gy, rows - 1), (gx - 1) * GEO.AMAX_STRIP       # a row only the u = 1..3 loads or a later block column reach
    x[r, c] = R.round_to(np.array([-3.25]), dt)[0]
    for fmt, (ld, shift) in zip(FMTS, pitches(cols, dt)):
        got = Q.check(x, dt, fmt, ld=ld + shift, what=f"{rows}x{cols} {dt} ld {ld + shift}")
        assert got[0] == 0x40500000


# ---- 2. kf_fp8_quantize with a caller's amax, and the scale's limits --------------------------------------------------------------------
@pytest.mark.parametrize("amax", [2.0 ** -20, 1.0, 448.0, 57344.0, 3e38])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_every_16_bit_pattern_under_a_callers_amax(dt, fmt, amax):
    x = Q.all_patterns(dt, False)
    amax = np.float32(amax)
    got = Q.check(x, dt, fmt, amax=amax, what=f"{dt} patterns, amax {amax}")
    # and without the reference's encoder: what lies beyond the bound is +-fmt_max, an infinity too, and a NaN is 0x7f | sign
    with np.errstate(invalid="ignore"):
        x32 = R.to_f32(x, dt).astype(np.float64)
    q = got[2][:x.size].reshape(x.shape)
    scale = 1.0 / float(got[1])
    sign = np.where(np.signbit(x32), 0x80, 0)
    beyond = ~np.isnan(x32) & (np.abs(x32) * scale >= R.FMT_MAX[fmt])
    assert np.isinf(x32).sum() == 2 and beyond[np.isinf(x32)].all() and (beyond.sum() > 2) == (amax < 1e38)
    assert np.array_equal(q[beyond], (SAT[fmt] | sign)[beyond])
    assert np.array_equal(q[np.isnan(x32)], (0x7f | sign)[np.isnan(x32)])
    inside = ~np.isnan(x32) & ~beyond
    assert ((q[inside] & 0x7f) <= SAT[fmt]).all()


LIMIT_EDGE = np.float32(0.875 * 2.0 ** -117)     # the largest amax whose e4m3 exponent is 126 without the clamp
LIMIT_AMAX = [np.float32(2.0 ** -149), np.float32(2.0 ** -127), np.float32(2.0 ** -126), np.float32(2.0 ** -118), np.float32(2.0 ** -117), LIMIT_EDGE,
              np.nextafter(LIMIT_EDGE, np.float32(1)), np.finfo(np.float32).max]


def unclamped_exp(amax, fmt):
    m, ex = np.frexp(np.float64(amax))
    return R.FMT_POW[fmt] - int(ex) - (1 if m > 0.875 else 0)


def values_around(amax, fmt):
    """32 x 48 f32 values: the format's grid and its rounding boundaries brought to amax's scale, multiples of amax on both sides of it,
    f32 subnormals; every one with both signs. Values beyond amax are meant: amax is the caller's bound."""
    g = R.GRID[fmt]
    with np.errstate(over="ignore"):
        onto = (np.concatenate([g, (g[:-1] + g[1:]) / 2]) * 2.0 ** -R.scale_exp(amax, fmt)).astype(np.float32)
        near = (np.float64(amax) * np.array([0.25, 0.5, 0.75, 1.0, 1.0625, 1.5, 2.0, 3.0, 1024.0])).astype(np.float32)
    tiny = np.array([2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -130, 2.0 ** -127, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126], dtype=np.float32)
    vals = np.concatenate([onto, near, tiny])
    vals = np.concatenate([vals, -vals])
    x = np.zeros((32, 48), dtype=np.float32)
    assert vals.size <= x.size
    x.ravel()[:vals.size] = vals
    return x


@pytest.mark.parametrize("amax", LIMIT_AMAX, ids=["2^-149", "2^-127", "2^-126", "2^-118", "2^-117", "edge", "above the edge", "largest"])
@pytest.mark.parametrize("fmt", FMTS)
def test_the_scale_exponent_stops_at_126(fmt, amax):
    """e4m3: 2^-149, 2^-127 and 2^-126 need the clamp, 2^-118 and the edge give 126 without it, 2^-117 and one step above the edge give
    125. e5m2 (seven more binades): everything but the largest finite f32 needs it."""
    x = values_around(amax, fmt)
    got = Q.check(x, "f32", fmt, amax=amax, what=f"amax {amax}")
    e = unclamped_exp(amax, fmt)
    assert (e > 126) == (amax < 1 if fmt == R.E5M2 else amax <= np.float32(2.0 ** -126))
    assert got[1].view(np.uint32) == np.float32(2.0 ** -min(e, 126)).view(np.uint32)
    if e >= 126:
        assert got[1].view(np.uint32) == 0x00800000                        # 2^-126, exactly
    if amax < 1:
        assert got[2][:x.size].any()                                       # subnormal inputs, and still codes other than zero


@pytest.mark.parametrize("fmt", FMTS)
def test_an_all_subnormal_bf16_matrix(fmt):
    n = np.arange(32 * 48, dtype=np.uint16)
    x = ((n % 127 + 1) | ((n & 1) << 15)).astype(np.uint16).reshape(32, 48)      # 0x0001 .. 0x007f, alternating sign
    assert (np.abs(R.to_f32(x, "bf16")) < 2.0 ** -126).all()
    got = Q.check(x, "bf16", fmt, what="bf16 subnormals")
    assert got[0] == 0x007f0000 and got[1].view(np.uint32) == 0x00800000 and got[2][:x.size].any()


# ---- 3. kf_gemm_fp8's tile walk -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [16, 144])
@pytest.mark.parametrize("fa,fb", [(R.E4M3, R.E4M3), (R.E5M2, R.E4M3)])
@pytest.mark.parametrize("tm,tn", GEO.TILE_COUNTS)
def test_every_tile_of_the_grouped_walk(tm, tn, fa, fb, K):
    M, N = GEO.GEMM_TILE * tm - 5, GEO.GEMM_TILE * tn - 3
    rng = np.random.default_rng(tm * 100 + tn * 10 + K + fa)
    (a, av), (b, bv) = G.int_codes(rng, (M, K), fa), G.int_codes(rng, (N, K), fb)
    sa, sb = 2.0 ** -3, 2.0 ** 2
    want = (av @ bv.T) * sa * sb
    assert (np.abs(av) @ np.abs(bv).T).max() < 2 ** 24
    got = G.run(a, fa, b, fb, "f32", sa, sb)
    bad = np.argwhere(got != want)
    tiles = sorted({(int(r) // GEO.GEMM_TILE, int(c) // GEO.GEMM_TILE) for r, c in bad})
    assert not tiles, f"{tm} x {tn} tiles, K {K}: {len(bad)} of {M * N} elements differ, in the (tile row, tile column) pairs {tiles}"


# ---- 4. kf_gemm_fp8 on every code byte ----------------------------------------------------------------------------------------------------
PERM = np.random.default_rng(256).permutation(256).astype(np.uint8)


def cyclic_codes(rows, K, step, order):
    """Row i is the 256-long cycle `order`, shifted by step * i."""
    return order[(np.arange(K)[None, :] + step * np.arange(rows)[:, None]) % 256]


def finite(codes, fmt):
    top = np.uint8(0x7f if fmt == R.E4M3 else 0x7c)
    return np.where((codes & 0x7f) >= top, (codes & 0x80) | SAT[fmt], codes).astype(np.uint8)


@pytest.mark.parametrize("out", ["f32", "bf16"])
@pytest.mark.parametrize("fa,fb", G.PAIRS)
@pytest.mark.parametrize("M,N,K", [(130, 70, 256), (64, 64, 112)])
def test_every_finite_code_at_every_byte_position(M, N, K, fa, fb, out):
    """A: row i holds code (k + i) % 256 at k, so with K = 256 and 130 rows each of the 256 codes meets each of the 128 byte positions of
    the instruction's K block (asserted). 70 rows of B cannot do that (140 blocks for 256 codes); B is a shuffled cycle stepping by 3, and
    every format is on the A side of two pairs. The non-finite codes become +-fmt_max."""
    raw = cyclic_codes(M, K, 1, np.arange(256, dtype=np.uint8))
    if K == 256:
        seen = np.zeros((128, 256), dtype=bool)
        seen[np.arange(K)[None, :] % 128, raw] = True
        assert seen.all()
    a, b = finite(raw, fa), finite(cyclic_codes(N, K, 3, PERM), fb)
    assert np.isfinite(R.decode(a, fa)).all() and np.isfinite(R.decode(b, fb)).all() and np.abs(R.decode(a, fa)).max() == R.FMT_MAX[fa]
    sa, sb = 2.0 ** -4, 2.0 ** 3
    c, mag = R.product(a, fa, b, fb, sa, sb)
    got = G.run(a, fa, b, fb, out, sa, sb)
    assert np.isfinite(got).all()
    frac, rel = R.gemm_frac(got, c, mag, out), float((np.abs(got - c) / mag).max())
    print(f"gemm_fp8 every code {M}x{N}x{K} {out} formats ({fa}, {fb}): worst fraction of the bound {frac:.3f}, worst |got - c| / mag {rel:.3e}")
    assert frac <= 1.0


SPECIAL = {"e4m3 NaN 0x7f in A": (R.E4M3, R.E4M3, "a", 0x7f), "e4m3 NaN 0xff in B": (R.E4M3, R.E4M3, "b", 0xff),
           "e5m2 NaN 0x7e in A": (R.E5M2, R.E4M3, "a", 0x7e), "e5m2 +inf in A": (R.E5M2, R.E4M3, "a", 0x7c)}
PLACE = {"first K block": (5, 17), "K tail": (37, 143), "last row of the edge tile": (-1, 40)}
_finite_runs = {}


def finite_problem(fa, fb, positive_column):
    """The finite 130 x 70 x 144 problem and its result (one run per variant, shared by the cases). positive_column: a column of B made
    strictly positive, for the infinity."""
    key = (fa, fb, positive_column)
    if key not in _finite_runs:
        rng = np.random.default_rng(41 + fa)
        a, b = G.random_codes(rng, (130, 144), fa), G.random_codes(rng, (70, 144), fb)
        if positive_column is not None:
            col = b[:, positive_column] & 0x7f
            b[:, positive_column] = np.where(col == 0, 0x30, col)
            assert (R.decode(b[:, positive_column], fb) > 0).all()
        for m in (a, b):
            m.setflags(write=False)
        base = G.run(a, fa, b, fb, "f32", 2.0 ** -2, 2.0 ** 1)
        assert np.isfinite(base).all()
        base.setflags(write=False)
        _finite_runs[key] = (a, b, base)
    return _finite_runs[key]


@pytest.mark.parametrize("place", list(PLACE))
@pytest.mark.parametrize("special", list(SPECIAL))
def test_one_special_byte_poisons_its_row_and_nothing_else(special, place):
    fa, fb, side, byte = SPECIAL[special]
    row, k = PLACE[place]
    is_inf = byte == 0x7c
    a, b, base = finite_problem(fa, fb, k if is_inf else None)
    a, b = a.copy(), b.copy()
    target = a if side == "a" else b
    row %= target.shape[0]
    target[row, k] = byte
    got = G.run(a, fa, b, fb, "f32", 2.0 ** -2, 2.0 ** 1)
    touched = np.zeros(got.shape, dtype=bool)
    if side == "a":
        touched[row, :] = True
    else:
        touched[:, row] = True
    hit = got[touched]
    print(f"gemm_fp8 {special}, {place}: the touched outputs are {sorted(set(map(str, hit)))}")
    assert not np.isfinite(hit).any()
    if is_inf:
        assert (hit == np.inf).all()          # +inf times a strictly positive column, everything else finite
    else:
        assert np.isnan(hit).all()
    same = got[~touched].astype(np.float32).view(np.uint32) == base[~touched].astype(np.float32).view(np.uint32)
    assert same.all(), f"{special}, {place}: {np.count_nonzero(~same)} outputs outside the touched row / column changed"


# ---- 5. addressing limits -------------------------------------------------------------------------------------------------------------
def beyond_4g(rows, es, multiple):
    """The smallest pitch in elements, a multiple of `multiple`, that puts the start of the last row beyond byte 2^32."""
    ld = -(-((1 << 32) // ((rows - 1) * es) + 1) // multiple) * multiple
    assert (rows - 1) * ld * es > 1 << 32 and (rows - 1) * ld * es < (1 << 32) + (1 << 28)
    return ld


class Wide:
    """[rows, width] bytes at a row pitch, with a guard band behind the last row. The WHOLE allocation is filled with `byte` once (on the
    device for 0); after that only rows move: up with h2d_rows, back as each row's window plus what follows it (GAP_BYTES, the whole gap
    where the pitch is smaller, the guard band behind the last row)."""

    def __init__(self, rows, width, pitch, byte):
        self.rows, self.width, self.pitch, self.byte = rows, width, pitch, byte
        self.nbytes = (rows - 1) * pitch + width + P.GUARD
        assert self.nbytes <= 5 << 30
        self.buf = H.DevBuf(self.nbytes)
        P.fill(self.buf.ptr, self.nbytes, byte)
        self.ptr = self.buf.ptr

    def upload(self, stored):
        stored = np.ascontiguousarray(stored)
        assert stored.shape[0] == self.rows and stored.shape[1] * stored.itemsize == self.width
        h2d_rows(self.buf, stored, 0, self.pitch)

    def window(self, dtype=np.uint8):
        """The [rows, width] window; asserts that the bytes read behind every row still hold the fill."""
        out = np.empty((self.rows, self.width), dtype=np.uint8)
        for r in range(self.rows):
            n = self.width + (P.GUARD if r == self.rows - 1 else min(self.pitch - self.width, GAP_BYTES))
            got = np.empty(n, dtype=np.uint8)
            H.check(H.lib().kf_memcpy_d2h(got.ctypes.data, self.ptr + r * self.pitch, n, None))
            assert (got[self.width:] == self.byte).all(), f"bytes behind row {r} were written"
            out[r] = got[:self.width]
        return out.view(dtype)

    def free(self):
        self.buf.free()


@pytest.mark.parametrize("big", ["a", "b", "c"])
def test_gemm_rows_beyond_byte_2_32(big):
    """One operand at a time with its last rows beyond byte 2^32: A and B at the largest legal leading dimension 2^24 (258 rows: the third
    tile row starts at byte 2^32), C at the smallest f32 ldc that does it with 130 rows. The A / B allocation is 0xFF (NaN in both
    formats) wherever no row was uploaded, so a byte from outside [rows, K] shows in the result."""
    M, N, K = (258, 70, 144) if big == "a" else (70, 258, 144) if big == "b" else (130, 70, 144)
    fa, fb = R.E5M2, R.E4M3
    rng = np.random.default_rng(M + N)
    (a, av), (b, bv) = G.int_codes(rng, (M, K), fa), G.int_codes(rng, (N, K), fb)
    sa, sb = 2.0 ** -1, 2.0 ** 3
    want = (av @ bv.T) * sa * sb
    lda, ldb = (1 << 24 if big == "a" else K + 16), (1 << 24 if big == "b" else K + 32)
    wide = []
    try:
        ops = []
        for name, codes, ld in (("a", a, lda), ("b", b, ldb)):
            if name == big:
                assert (codes.shape[0] - 1) * ld >= 1 << 32
                w = Wide(codes.shape[0], K, ld, 0xFF)
                wide.append(w)
                w.upload(codes)
                ops.append(w)
            else:
                ops.append(G.operand(codes, ld))
        bsa, bsb = G.scale(sa), G.scale(sb)
        if big == "c":
            ldc = beyond_4g(M, 4, 1)
            c = Wide(M, N * 4, ldc * 4, G.FILL)
            wide.append(c)
            H.gemm_fp8(fa, fb, H.F32, M, N, K, ops[0].ptr, lda, ops[1].ptr, ldb, bsa.ptr, bsb.ptr, c.ptr, ldc)
            H.device_sync()
            got = c.window(np.float32).astype(np.float64)
        else:
            got = G.launch(ops[0], lda, ops[1], ldb, bsa, bsb, fa, fb, "f32", M, N, K, G.default_ldc(N)).astype(np.float64)
        for w in wide[:1] if big != "c" else []:
            assert np.array_equal(w.window(), a if big == "a" else b), "the operand changed"
    finally:
        for w in wide:
            w.free()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {M * N} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, expected {want[tuple(bad[0])]}"


def test_gemm_at_the_largest_k_and_leading_dimension():
    """M = 128, N = 16, lda = ldb = 2^24, K = 2^24 - 16: num_records = 127 * 2^24 + K = 2^31 - 16 for A, the K tail's lanes ask for that
    offset, and one workgroup walks 131072 K blocks. Zero operands (filled on the device) with exact integers at a few k only - both ends
    of the first block, the seam at 2^23, the last 144 bytes - in a few rows; the product of those alone is the expected result."""
    M, N, ld = 128, 16, 1 << 24
    K = ld - 16
    fa, fb = R.E4M3, R.E5M2
    ks = np.array([0, 127, 128, (1 << 23) - 1, 1 << 23] + list(range(K - 144, K)))
    segments = [(0, 129), ((1 << 23) - 1, (1 << 23) + 1), (K - 144, K)]
    rng = np.random.default_rng(24)
    av, bv = np.zeros((M, ks.size)), np.zeros((N, ks.size))
    for vals, rows, fmt in ((av, (0, 1, 63, 64, 127), fa), (bv, (0, 7, 15), fb)):
        vals[list(rows)] = rng.choice(G.INTS[fmt][G.INTS[fmt] != 0], size=(len(rows), ks.size))
    sa, sb = 2.0 ** 1, 2.0 ** -2
    want = (av @ bv.T) * sa * sb
    assert (np.abs(av) @ np.abs(bv).T).max() < 2 ** 24 and np.count_nonzero(want) >= 10
    bufs = []
    try:
        for vals, fmt in ((av, fa), (bv, fb)):
            rows = vals.shape[0]
            buf = H.DevBuf(rows * ld)
            bufs.append(buf)
            P.fill(buf.ptr, rows * ld, 0)
            codes = R.encode(vals, fmt)
            assert np.array_equal(R.decode(codes, fmt), vals)
            for r in np.flatnonzero(vals.any(axis=1)):
                for lo, hi in segments:
                    seg = np.zeros((1, hi - lo), dtype=np.uint8)
                    inside = (ks >= lo) & (ks < hi)
                    seg[0, ks[inside] - lo] = codes[r, inside]
                    h2d_rows(types.SimpleNamespace(ptr=buf.ptr + lo), seg, int(r), ld)
        H.device_sync()
        t0 = time.perf_counter()
        got = G.launch(bufs[0], ld, bufs[1], ld, G.scale(sa), G.scale(sb), fa, fb, "f32", M, N, K, G.default_ldc(N)).astype(np.float64)
        took = time.perf_counter() - t0
    finally:
        for buf in bufs:
            buf.free()
    print(f"gemm_fp8 128x16x{K} at lda = ldb = 2^24: {took:.2f} s for the launch and the read-back")
    assert np.array_equal(got, want), f"differs at {np.argwhere(got != want)[:8].tolist()}"
    assert took < 10.0


@pytest.mark.parametrize("big", ["ld", "ldq", "ldqt"])
def test_quantize_rows_beyond_byte_2_32(big):
    """kf_fp8_amax and kf_fp8_quantize, bf16, 3 x 48 (48 x 3 for qt): the one pitch named is the smallest 16-byte multiple that puts its
    third row beyond byte 2^32. The input allocation is NaN wherever no row was uploaded."""
    rows, cols = (48, 3) if big == "ldqt" else (3, 48)
    rows16 = (rows + 15) // 16 * 16
    x = R.round_to(np.random.default_rng(len(big)).standard_normal((rows, cols)) * 3.0, "bf16")
    ld = beyond_4g(rows, 2, 8) if big == "ld" else cols + 8
    ldq = beyond_4g(rows, 1, 16) if big == "ldq" else cols + 16
    ldqt = beyond_4g(cols, 1, 16) if big == "ldqt" else rows16 + 16
    fmt = R.E4M3 if big != "ldq" else R.E5M2
    wide = []
    try:
        bx, bq, bqt = Wide(rows, cols * 2, ld * 2, 0xFF), Wide(rows, cols, ldq, Q.FILL), Wide(cols, rows16, ldqt, Q.FILL)
        wide += [bx, bq, bqt]
        bx.upload(x)
        amax, sinv = H.DevBuf(4), H.DevBuf(4)
        P.fill(amax.ptr, 4, 0xFF)
        P.fill(sinv.ptr, 4, 0xFF)
        H.fp8_amax(H.BF16, rows, cols, ld, bx.ptr, amax.ptr)
        H.fp8_quantize(H.BF16, fmt, rows, cols, ld, bx.ptr, amax.ptr, bq.ptr, ldq, sinv.ptr, bqt.ptr, ldqt)
        H.device_sync()
        got = (bq.window(), bqt.window(), sinv.to_numpy(1, np.float32)[0], int(amax.to_numpy(1, np.uint32)[0]))
    finally:
        for w in wide:
            w.free()
    q, qt, s, bits = R.quantize(R.to_f32(x, "bf16"), fmt)
    assert got[3] == bits and got[2].view(np.uint32) == s.view(np.uint32)
    assert np.array_equal(got[0], q) and np.array_equal(got[1], qt)


# ---- 6. the operator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_linear_fp8_at_16500_tokens(dt):
    """x [16500, 32] and dy [16500, 48]: kf_fp8_amax takes two trips over each, and dW contracts over ceil16(T) = 16512, 129 K blocks. The
    checks are test_output_and_gradients' own: the GEMM bound and the end-to-end bound against the reference pipeline."""
    T, K, N = 16500, 32, 48
    assert GEO.amax_trips(T, K) == GEO.amax_trips(T, N) == 2 and -(-T // 16) * 16 == 129 * 128
    L.test_output_and_gradients((T,), K, N, dt)
