"""CPU-only: tests/fp8_ref.py against torch's float8 types and against itself - the decode tables and the encode of every finite bf16
value (after the clamp) agree bit for bit with torch.float8_e4m3fn / torch.float8_e5m2, the scale rule lands amax * scale in
(fmt_max / 2, fmt_max] on both sides of every mantissa case, and the GEMM bound rejects a dropped 128-byte K block, two swapped output
rows and a missing scale_inv."""
import math

import numpy as np
import pytest
import torch

from oracle import checks as CK
from oracle import oracle as O
from tests import fp8_geometry as GEO
from tests import fp8_ref as R

TORCH = {R.E4M3: torch.float8_e4m3fn, R.E5M2: torch.float8_e5m2}
FMTS = [R.E4M3, R.E5M2]


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_table_is_torchs(fmt):
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    want = codes.view(TORCH[fmt]).to(torch.float32).numpy().astype(np.float64)
    got = R.decode(np.arange(256, dtype=np.uint8), fmt)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    assert np.nanmax(np.where(np.isinf(got), np.nan, got)) == R.FMT_MAX[fmt]


@pytest.mark.parametrize("fmt", FMTS)
def test_encode_of_every_finite_bf16_value_is_torchs(fmt):
    bits = np.arange(65536, dtype=np.uint32)
    vals = (bits << 16).astype(np.uint32).view(np.float32)
    vals = vals[np.isfinite(vals)]
    clamped = np.clip(vals, -R.FMT_MAX[fmt], R.FMT_MAX[fmt])
    want = torch.from_numpy(clamped).to(TORCH[fmt]).view(torch.uint8).numpy()
    got = R.encode(clamped, fmt)
    assert np.array_equal(got, want)
    assert np.array_equal(R.encode(vals, fmt), want)   # the reference's own clamp


@pytest.mark.parametrize("fmt", FMTS)
def test_encode_rounds_ties_to_even_and_keeps_nan_and_sign(fmt):
    g = R.GRID[fmt]
    mid = (g[:-1] + g[1:]) / 2                          # exact in f64, and in f32 (one more mantissa bit)
    got = R.encode(mid, fmt)
    assert (got % 2 == 0).all() and np.array_equal(got, np.where(np.arange(len(mid)) % 2 == 0, np.arange(len(mid)), np.arange(len(mid)) + 1))
    assert np.array_equal(R.encode(-mid, fmt), got | 0x80)
    assert R.encode(np.float32("nan"), fmt) == 0x7f and R.encode(-np.float32("nan"), fmt) == 0xff
    assert R.encode(np.float32("inf"), fmt) == R._NFINITE[fmt] - 1 and R.encode(np.float32(-0.0), fmt) == 0x80


def neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(0)), v, np.nextafter(v, np.float32(np.inf))]


@pytest.mark.parametrize("fmt", FMTS)
def test_scale_rule_on_both_sides_of_every_mantissa_case(fmt):
    fmax = R.FMT_MAX[fmt]
    amaxes = []
    for n in range(-125, 127):
        amaxes += neighbours(0.875 * 2.0 ** n) + neighbours(2.0 ** n) + [np.float32(1.3 * 2.0 ** n), np.float32(1.9999 * 2.0 ** n)]
    amaxes += [np.float32(2.0 ** -149), np.float32(3 * 2.0 ** -149), np.float32(2.0 ** -127), np.float32(0.875 * 2.0 ** -130), np.finfo(np.float32).max]
    for a in amaxes:
        e = R.scale_exp(a, fmt)
        assert -126 <= e <= 126
        prod = float(a) * 2.0 ** e
        if -126 < e < 126:
            assert fmax / 2 < prod <= fmax, (float(a), e)
            # exactly on the mantissa boundary the product IS fmt_max; one f32 step above it drops a power of two
        else:
            assert prod <= fmax
    for n in (-20, 0, 9, 30):
        lo, at, hi = neighbours(0.875 * 2.0 ** n)
        assert R.scale_exp(lo, fmt) == R.scale_exp(at, fmt) == R.scale_exp(hi, fmt) + 1
        assert float(at) * 2.0 ** R.scale_exp(at, fmt) == fmax
    for special in (0.0, math.inf, math.nan, -0.0):
        assert R.scale_exp(special, fmt) == 0
    assert R.scale_exp(np.float32(2.0 ** -149), fmt) == 126


def test_quantize_reference_shapes_pad_and_amax():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((19, 40)).astype(np.float32)
    q, qt, sinv, bits = R.quantize(x, R.E4M3)
    assert q.shape == (19, 40) and qt.shape == (40, 32) and not qt[:, 19:].any() and np.array_equal(qt[:, :19], q.T)
    assert np.uint32(bits).view(np.float32) == np.abs(x).max()
    assert np.abs(R.decode(q, R.E4M3)).max() > R.FMT_MAX[R.E4M3] / 2
    x[3, 3] = np.nan
    assert R.amax_bits(x) == 0x7fc00000 and R.quantize(x, R.E4M3)[2] == 1.0
    assert R.amax_bits(np.zeros((0, 4), np.float32)) == 0 and R.quantize(np.zeros((2, 2), np.float32), R.E5M2)[2] == 1.0


@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_under_a_callers_amax_is_torchs_after_the_clamp(fmt):
    """amax below, at and above the true maximum; infinities in x. The scale is a power of two, so x * scale is exact in f32 and torch's
    conversion of the explicitly clamped product is the whole reference; NaNs are checked apart (torch's NaN code is its own)."""
    rng = np.random.default_rng(7 + fmt)
    x = (rng.standard_normal((40, 33)) * 10.0 ** rng.integers(-6, 6, (40, 33))).astype(np.float32)
    x[0, :4] = [np.inf, -np.inf, np.nan, -np.nan]
    finite = np.isfinite(x)
    true_max = np.abs(x[finite]).max()
    for amax in (true_max / 1000, true_max / 2, np.nextafter(true_max, np.float32(0)), true_max, true_max * 2, true_max * 1e6, np.float32(3e38)):
        q, qt, sinv, bits = R.quantize(x, fmt, amax=amax)
        e = R.scale_exp(amax, fmt)
        assert bits == int(np.float32(amax).view(np.uint32)) and sinv == np.float32(2.0 ** -e) and amax * 2.0 ** e <= R.FMT_MAX[fmt] < amax * 2.0 ** (e + 1)
        with np.errstate(over="ignore", invalid="ignore"):
            clamped = np.clip(x * np.float32(2.0 ** e), -R.FMT_MAX[fmt], R.FMT_MAX[fmt])
        ok = ~np.isnan(x)
        want = torch.from_numpy(clamped[ok]).to(TORCH[fmt]).view(torch.uint8).numpy()
        assert np.array_equal(q[ok], want)
        assert q[0, 2] == 0x7f and q[0, 3] == 0xff and q[0, 0] == R._NFINITE[fmt] - 1 and q[0, 1] == (R._NFINITE[fmt] - 1) | 0x80
        assert np.array_equal(qt[:, :40], q.T) and not qt[:, 40:].any()
        beyond = finite & (np.abs(x).astype(np.float64) * 2.0 ** e > R.FMT_MAX[fmt])
        assert beyond.any() if amax <= true_max / 2 else not beyond.any() or amax < true_max
        assert ((q[beyond] & 0x7f) == R._NFINITE[fmt] - 1).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_quantize_reference_at_the_scale_limits(fmt):
    """Under the upper clamp (e = 126) x * scale is still exact, f32 subnormals included, so the codes are torch's of the clamped f64
    product; and no f32 amax reaches the lower clamp: the smallest exponent is the largest finite f32's, pow - 129."""
    tiny = np.array([2.0 ** -149, 3 * 2.0 ** -149, 2.0 ** -140, 2.0 ** -127, 2.0 ** -126, 5 * 2.0 ** -128, 2.0 ** -120], dtype=np.float32)
    x = np.concatenate([tiny, -tiny]).reshape(2, 7)
    for amax in (np.float32(2.0 ** -149), np.float32(2.0 ** -126), np.float32(2.0 ** -120)):
        q, _, sinv, _ = R.quantize(x, fmt, amax=amax)
        assert R.scale_exp(amax, fmt) == 126 and sinv == np.float32(2.0 ** -126)
        clamped = np.clip(x.astype(np.float64) * 2.0 ** 126, -R.FMT_MAX[fmt], R.FMT_MAX[fmt]).astype(np.float32)
        assert np.array_equal(q, torch.from_numpy(clamped).to(TORCH[fmt]).view(torch.uint8).numpy())
    exps = [R.scale_exp(np.float32(m * 2.0 ** n), fmt) for n in range(-149, 128) for m in (1.0, 1.9999999)]       # both ends of every f32 binade
    assert exps == sorted(exps, reverse=True) and exps[-1] == R.scale_exp(np.finfo(np.float32).max, fmt) == R.FMT_POW[fmt] - 129 > -126


def test_amax_shapes_reach_the_trips_rows_and_strips_they_claim():
    """tests/fp8_geometry.py restates kf_fp8_amax's grid. The shapes of the GPU test must still have a second trip, a first trip whose
    u = 1..3 loads are real rows, and gx > 1, each where claimed - and between them all of it."""
    assert GEO.amax_grid(300, 257) == (1, 300) and GEO.amax_trips(300, 257) == 1          # the largest shape of test_gpu_fp8_quantize.py
    for (rows, cols), claim in GEO.AMAX_SHAPES.items():
        gx, gy = GEO.amax_grid(rows, cols)
        assert gx == -(-cols // 4096) == claim["gx"] and gy == min(rows, -(-4096 // gx), 65535)
        trips = sum(1 for _ in range(0, rows, 4 * gy))                        # blockIdx.y = 0: r = 0, 4 gy, ...
        assert trips == GEO.amax_trips(rows, cols) == claim["trips"]
        assert (gy < rows) == claim["real_u"]                                 # r + u gy < rows for r = 0, u = 1
        if claim["trips"] > 1:
            assert 4 * gy < rows
    claims = list(GEO.AMAX_SHAPES.values())
    assert any(c["trips"] == 2 for c in claims) and any(c["trips"] > 2 for c in claims)
    assert any(c["gx"] == 2 and c["trips"] == 2 for c in claims) and any(c["gx"] == 3 and c["trips"] == 2 for c in claims)
    assert any(c["gx"] > 1 and c["trips"] == 1 and not c["real_u"] for c in claims) and any(c["gx"] == 1 and c["trips"] == 1 and c["real_u"] for c in claims)
    # a trip whose u = 3 row is the very last row, and one whose u = 1..3 rows all lie past it
    assert GEO.amax_grid(16384, 16)[1] * 4 == 16384 and GEO.amax_grid(16385, 16)[1] * 4 + 1 == 16385
    assert set(GEO.AMAX_QUANTIZED) <= set(GEO.AMAX_SHAPES) and sorted(GEO.AMAX_SHAPES, key=lambda s: s[0] * s[1])[:2] == sorted(GEO.AMAX_QUANTIZED, key=lambda s: s[0] * s[1])
    assert GEO.amax_trips(16500, 32) == GEO.amax_trips(16500, 48) == 2        # the operator test's x and dy


def test_gemm_fp8_block_order_is_a_bijection_with_whole_and_ragged_groups():
    """q_xcd_remap and q_grouped_tile restated: every hardware block id gets its own tile, for each tile count of the GPU test; and
    the list has what the FP8 tests lacked - a whole group of 8 tile rows beyond the first, ragged last groups of 1, 4 and 7 rows, a
    tile count that is no multiple of the 8 XCDs."""
    assert max(-(-m // 128) for m, _, _ in [(512, 512, 4096), (257, 129, 128)]) <= 4       # the other FP8 tests: at most 4 tile rows
    whole_later, ragged, uneven = False, set(), False
    for tm, tn in GEO.TILE_COUNTS:
        n = tm * tn
        ids = sorted(GEO.xcd_remap(b, n) for b in range(n))
        assert ids == list(range(n))
        tiles = [GEO.tile_of_block(b, tm, tn) for b in range(n)]
        assert sorted(tiles) == [(i, j) for i in range(tm) for j in range(tn)]
        whole_later |= tm >= 16
        if tm % 8:
            ragged.add(tm % 8)
        uneven |= n % 8 != 0
    assert whole_later and {1, 4, 7} <= ragged and uneven
    assert (1, 17) in GEO.TILE_COUNTS                                           # one ragged group only, many columns


def test_checks_acc_term_is_gemm_oks():
    # want = 0, mag = 2: gemm_ok's fraction is |got| / (term * 2 + half a subnormal ulp)
    a = O.from_float(np.array([[1.0, -1.0]], dtype=np.float32), O.BF16)
    b = O.from_float(np.array([[1.0], [1.0]], dtype=np.float32), O.BF16)
    got = O.from_float(np.array([[2.0 ** -10]], dtype=np.float32), O.BF16)
    _, frac = CK.gemm_ok(got, a, b, O.BF16)
    assert math.isclose(2.0 ** -10 / frac, 2 * R.CHECKS_ACC_TERM + 0.5 * CK.ABS_ULP[O.BF16], rel_tol=1e-12)
    assert R.ACC_TERM == 3.8e-4 and 2 * 1.87e-4 <= R.ACC_TERM < CK.EPS[O.BF16] / 8      # twice the measured worst; far below an output rounding


@pytest.mark.parametrize("out", ["f32", "bf16", "f16"])
def test_gemm_bound_accepts_a_rounded_product_and_rejects_mutants(out):
    rng = np.random.default_rng(11)
    M, N, K = 48, 40, 384
    a = rng.integers(0, 256, (M, K)).astype(np.uint8)
    b = rng.integers(0, 256, (N, K)).astype(np.uint8)
    a[(a & 0x7f) == 0x7f] = 0x30                                   # no NaN codes
    b[(b & 0x7c) == 0x7c] = 0x30                                   # no e5m2 infinity / NaN codes
    b &= 0xbf                                                      # and e5m2 magnitudes below 2: the f16 output holds the product
    sa, sb = 2.0 ** -3, 2.0 ** -2
    c, mag = R.product(a, R.E4M3, b, R.E5M2, sa, sb)
    good = R.to_f32(R.round_to(c, out), out).astype(np.float64)
    assert R.gemm_frac(good, c, mag, out) <= 1.0
    dropped, _ = R.product(a[:, 128:], R.E4M3, b[:, 128:], R.E5M2, sa, sb)      # one 128-byte K block missing
    assert R.gemm_frac(dropped, c, mag, out) > 1.0
    swapped = good.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert R.gemm_frac(swapped, c, mag, out) > 1.0
    assert R.gemm_frac(good / sb, c, mag, out) > 1.0               # scale_inv_b never applied
    assert R.gemm_frac(np.full_like(good, np.nan), c, mag, out) == math.inf
