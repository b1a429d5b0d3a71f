"""-m gpu: the fused cross-entropy kernels at the C ABI - kf_ce_fused_rows (loss and UNSCALED gradient of a block of logits in one
call), kf_ce_fused_reduce and kf_scale_cast - against the f64 reference of tests/linear_ce_ref.py on the same stored logits.

Tolerances (tests/test_gpu_cross_entropy.py's table):
  loss, lse   |got - ref| <= 1e-4 + 1e-5 |ref|
  dlogits     |got - ref| <= r |ref| + 1e-6 with r one output rounding: 2^-8 bf16, 2^-11 f16, 2^-16 f32 (the gradient is unscaled: |g| = 1)
  sums        the f32 sum of the per-row losses in a fixed order: rtol 1e-5
  scale_cast  exact: in[i] * (g / count) formed in f32 and rounded once to the output type
Ignored rows are exactly zero, an out-of-range target is NaN in its own row only, bytes past V of a strided output and behind the
buffer keep their pattern, and two runs give identical bits."""
import functools

import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests import linear_ce_ref as R
from tests import poison
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

OUT_R = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 2.0 ** -16}
NP = {H.BF16: np.uint16, H.F16: np.float16, H.F32: np.float32}
PAT = 0xAB  # what output buffers hold before the call: bf16 / f16 0xABAB and f32 0xABABABAB are small negative numbers, never zero

# (rows, V, ld): one wave per row (V <= 4096), one block per row (rows >= 1024 and V > 4096), split rows (few long rows), the pack and
# element edges (V = 1, 7, 4097, 50257) and a row stride that moves every row against the 16-byte boundaries
SHAPES = [(37, 1, None), (64, 7, None), (300, 1000, None), (5, 4096, None), (3, 4097, None), (40, 1000, 1003), (2, 50257, None),
          (1024, 4160, None), (1100, 8192, None)]
# (in dtype, out dtype, in place)
PAIRS = [(H.F32, H.BF16, False), (H.F32, H.F16, False), (H.F32, H.F32, False), (H.BF16, H.BF16, True), (H.F16, H.F16, False)]
PAIR_IDS = ["f32-bf16", "f32-f16", "f32-f32", "bf16-inplace", "f16-f16"]
# (name, ignored rows, eps, z, -inf columns, dlogits NULL, lse kept)
CASES = [("plain", False, 0.0, 0.0, False, False, True), ("ignored", True, 0.0, 0.0, False, False, True),
         ("smooth", False, 0.1, 0.0, False, False, True), ("zloss", False, 0.0, 1e-3, False, False, False),
         ("both", True, 0.1, 1e-3, False, False, True), ("neg_inf", True, 0.0, 1e-3, True, False, True),
         ("null", True, 0.1, 1e-3, False, True, True)]


@functools.lru_cache(maxsize=None)
def inputs(rows, V, ld, code, neg_inf):
    """(stored logits [rows, ld], the same as f64 [rows, V], targets with no row ignored, the first -inf column) - shared, never modified."""
    ld = V if ld is None else ld
    rng = np.random.default_rng(rows * 7 + V * 3 + code)
    x32 = rng.uniform(-3.0, 3.0, (rows, ld)).astype(np.float32)
    live = V
    if neg_inf and V > 1:   # a padded vocabulary: the last eighth of the columns (at least one), and one column inside the live part
        live = V - max(1, V // 8)
        x32[:, live:V] = -np.inf
        if live > 2:
            x32[:, live // 2] = -np.inf
    xs = O.from_float(x32, code)
    x = O.to_float(xs, code).astype(np.float64)[:, :V]
    t = rng.integers(0, live, rows)
    if neg_inf and live > 2:
        t[t == live // 2] = 0   # a target on a -inf logit is an infinite loss: not this test's subject
    for a in (xs, x, t):
        a.setflags(write=False)
    return xs, x, t


def raw(a):
    """The bytes of an array slice."""
    return np.ascontiguousarray(a).view(np.uint8)


def run(in_code, out_code, xs, t, V, eps=0.0, z=0.0, inplace=False, write=True, keep_lse=True):
    """One kf_ce_fused_rows call. Returns (rowloss, lse or None, dlogits [rows, ld] in the storage dtype or None, pads_ok)."""
    rows, ld = xs.shape
    bx, bt = H.DevBuf.from_numpy(xs), H.DevBuf.from_numpy(np.asarray(t, np.int64))
    bl, blse = H.DevBuf(4 * rows), H.DevBuf(4 * rows)
    poison.fill(bl.ptr, 4 * rows, 0xFF)
    poison.fill(blse.ptr, 4 * rows, 0xFF)
    nbytes = rows * ld * H.DTYPE_SIZE[out_code]
    bd = None
    if write and not inplace:
        bd = poison.guarded(nbytes)
        poison.fill(bd.ptr, nbytes + poison.GUARD, PAT)
    dptr = None if not write else bx.ptr if inplace else bd.ptr
    ws = H.ce_fused_rows(in_code, out_code, rows, V, bx.ptr, bt.ptr, bl.ptr, blse.ptr if keep_lse else None, dptr, label_smoothing=eps, z_loss=z,
                         ld=ld, ldd=ld)
    H.device_sync()
    del ws
    loss = bl.to_numpy((rows,), np.float32)
    lse = blse.to_numpy((rows,), np.float32) if keep_lse else None
    if not write:
        return loss, lse, None, True
    dx = (bx if inplace else bd).to_numpy((rows, ld), NP[out_code])
    if inplace:   # the columns past V still hold the uploaded logits' bytes
        pads_ok = raw(dx[:, V:]).tobytes() == raw(xs[:, V:]).tobytes()
    else:
        pads_ok = poison.guard_intact(bd, nbytes, PAT) and bool((raw(dx[:, V:]) == PAT).all())
    return loss, lse, dx, pads_ok


def check(out_code, loss, lse, dx, x, t, V, eps, z, what):
    rlse, rloss, rd = R.ce_rows(x, t, -100, eps, z)
    keep, nan = t != -100, (t != -100) & ((t < 0) | (t >= V))
    good = ~nan
    assert_close(loss[good], rloss[good], rtol=1e-5, atol=1e-4, what=f"{what}: loss")
    assert np.isnan(loss[nan]).all(), f"{what}: an out-of-range target must give a NaN loss"
    assert (loss[~keep] == 0).all(), f"{what}: an ignored row's loss must be 0"
    if lse is not None:
        assert_close(lse, rlse, rtol=1e-5, atol=1e-4, what=f"{what}: lse")
    if dx is None:
        return
    got = O.to_float(dx[:, :V], out_code).astype(np.float64)
    assert_close(got[good], rd[good], rtol=OUT_R[out_code], atol=1e-6, what=f"{what}: dlogits")
    assert np.isnan(got[nan]).all(), f"{what}: an out-of-range target must give a NaN gradient row"
    assert not raw(dx[~keep][:, :V]).any(), f"{what}: an ignored row's gradient must be exactly zero"


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("rows,V,ld", SHAPES)
def test_rows_shapes_pairs_cases(rows, V, ld, pair):
    in_code, out_code, inplace = pair
    for name, ignored, eps, z, neg_inf, null, keep_lse in CASES:
        xs, x, t0 = inputs(rows, V, ld, in_code, neg_inf)
        t = t0.copy()
        if ignored:
            t[np.random.default_rng(rows + V).random(rows) < 0.2] = -100
            t[rows // 2] = -100
        what = f"{name} ({rows}, {V}, {ld}) {in_code}->{out_code}"
        loss, lse, dx, pads_ok = run(in_code, out_code, xs, t, V, eps, z, inplace, write=not null, keep_lse=keep_lse)
        assert pads_ok, f"{what}: bytes past V or behind the buffer were written"
        check(out_code, loss, lse, dx, x, t, V, eps, z, what)
        if name == "both":   # the same call again: the same bits
            loss2, lse2, dx2, _ = run(in_code, out_code, xs, t, V, eps, z, inplace, keep_lse=keep_lse)
            assert loss.tobytes() == loss2.tobytes() and lse.tobytes() == lse2.tobytes() and dx[:, :V].tobytes() == dx2[:, :V].tobytes(), \
                f"{what}: two runs differ"
        if null:             # the loss alone equals the loss of the writing call, bit for bit
            loss3, _, _, _ = run(in_code, out_code, xs, t, V, eps, z, inplace, keep_lse=False)
            assert loss.tobytes() == loss3.tobytes(), f"{what}: the loss-only pass differs from the fused one"


@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2], PAIRS[3]], ids=[PAIR_IDS[0], PAIR_IDS[2], PAIR_IDS[3]])
@pytest.mark.parametrize("rows,V,ld", SHAPES)
def test_out_of_range_target_is_nan_in_its_row_only(rows, V, ld, pair):
    in_code, out_code, inplace = pair
    xs, x, t0 = inputs(rows, V, ld, in_code, False)
    t = t0.copy()
    t[0], t[rows - 1] = V, -5
    if rows > 3:
        t[1] = -100
    loss, lse, dx, pads_ok = run(in_code, out_code, xs, t, V, 0.1, 1e-3, inplace)
    assert pads_ok
    check(out_code, loss, lse, dx, x, t, V, 0.1, 1e-3, f"out of range ({rows}, {V}, {ld}) {in_code}->{out_code}")
    assert np.isnan(loss[[0, rows - 1]]).all() and np.isfinite(loss[1:rows - 1]).all() and np.isfinite(lse).all()
    assert np.isnan(O.to_float(dx[[0, rows - 1]][:, :V], out_code)).all() and np.isfinite(O.to_float(dx[1:rows - 1][:, :V], out_code)).all()


@pytest.mark.parametrize("rows", [1, 1000, 5000])
def test_reduce_sum_mean_count(rows):
    rng = np.random.default_rng(rows)
    rl = rng.uniform(0.0, 12.0, rows).astype(np.float32)
    t = rng.integers(0, 100, rows)
    if rows > 1:
        t[rng.random(rows) < 0.3] = -100
    rl[t == -100] = 0.0
    brl, bt, bl, bc = H.DevBuf.from_numpy(rl), H.DevBuf.from_numpy(t.astype(np.int64)), H.DevBuf(4), H.DevBuf(4)
    n = int((t != -100).sum())
    for mean in (False, True):
        poison.fill(bl.ptr, 4, 0xFF)
        poison.fill(bc.ptr, 4, 0xFF)
        H.ce_fused_reduce(brl.ptr, bt.ptr, rows, bl.ptr, bc.ptr, mean=mean)
        H.device_sync()
        got, cnt = bl.to_numpy((1,), np.float32)[0], bc.to_numpy((1,), np.float32)[0]
        want = rl.astype(np.float64).sum() / (n if mean else 1)
        assert cnt == n
        assert abs(got - want) <= 1e-5 * abs(want), (mean, got, want)
        H.ce_fused_reduce(brl.ptr, bt.ptr, rows, bl.ptr, None, mean=mean)   # count may be NULL; the same bits again
        H.device_sync()
        assert bl.to_numpy((1,), np.float32)[0].tobytes() == got.tobytes()


def test_reduce_all_rows_ignored():
    rows = 300
    brl, bt, bl, bc = H.DevBuf.from_numpy(np.zeros(rows, np.float32)), H.DevBuf.from_numpy(np.full(rows, -100, np.int64)), H.DevBuf(4), H.DevBuf(4)
    H.ce_fused_reduce(brl.ptr, bt.ptr, rows, bl.ptr, bc.ptr, mean=True)
    H.device_sync()
    assert np.isnan(bl.to_numpy((1,), np.float32)[0]) and bc.to_numpy((1,), np.float32)[0] == 0
    H.ce_fused_reduce(brl.ptr, bt.ptr, rows, bl.ptr, bc.ptr, mean=False)
    H.device_sync()
    assert bl.to_numpy((1,), np.float32)[0] == 0 and bc.to_numpy((1,), np.float32)[0] == 0


def scaled(x_store, in_code, out_code, g, count):
    """in * (g / count) in f32, rounded once to the output type: the bits kf_scale_cast must give."""
    s = np.float32(g) / np.float32(count) if count is not None else np.float32(g)
    y = O.to_float(x_store, in_code).astype(np.float32) * s
    return O.from_float(y.astype(np.float32), out_code)


@pytest.mark.parametrize("n", [1, 7, 4099, 1 << 20])
@pytest.mark.parametrize("in_code,out_code", [(H.F32, H.BF16), (H.F32, H.F16), (H.F32, H.F32), (H.BF16, H.BF16), (H.F16, H.F16)],
                         ids=["f32-bf16", "f32-f16", "f32-f32", "bf16-bf16", "f16-f16"])
def test_scale_cast_is_exact(in_code, out_code, n):
    rng = np.random.default_rng(n + in_code * 10 + out_code)
    xs = O.from_float(rng.uniform(-4.0, 4.0, n).astype(np.float32), in_code)
    es_in, es_out = H.DTYPE_SIZE[in_code], H.DTYPE_SIZE[out_code]
    bg, bc = H.DevBuf.from_numpy(np.array([0.375 * 3], np.float32)), H.DevBuf.from_numpy(np.array([3277.0], np.float32))
    g, c = np.float32(0.375 * 3), np.float32(3277.0)
    # off: both pointers moved by one element, so that neither is 16-byte aligned - the element path
    for count, off in ((c, 0), (None, 0), (c, 1)):
        if off and n < 2:
            continue
        m = n - off
        bx = H.DevBuf.from_numpy(xs)
        bo = poison.guarded(n * es_out)
        poison.fill(bo.ptr, n * es_out + poison.GUARD, PAT)
        H.scale_cast(in_code, out_code, m, bx.ptr + off * es_in, bo.ptr + off * es_out, bg.ptr, bc.ptr if count is not None else None)
        H.device_sync()
        got = bo.to_numpy((n,), NP[out_code])
        want = scaled(xs[off:], in_code, out_code, g, count)
        assert got[off:].tobytes() == want.tobytes(), (n, count, off)
        assert poison.guard_intact(bo, n * es_out, PAT) and (raw(got[:off]) == PAT).all()
        if in_code == out_code:   # in place
            H.scale_cast(in_code, out_code, m, bx.ptr + off * es_in, bx.ptr + off * es_in, bg.ptr, bc.ptr if count is not None else None)
            H.device_sync()
            assert bx.to_numpy((n,), NP[in_code])[off:].tobytes() == want.tobytes(), ("in place", n, count, off)
