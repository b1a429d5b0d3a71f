"""-m gpu: the norm backward's persistent row walk (kf_norm_bwd) at row counts where each block walks many row groups, through the C ABI.

kf_norm_bwd launches nblk = min(nrb, resident) blocks, nrb = ceil(rows / RPB) row groups (RPB = 32 / 16 / 8 / 4 rows per block for
the 8- / 16- / 32- / 64-lane plans, 1 for the 256- to 1024-thread ones), resident = occupancy x CUs of the instantiation, at most
1024. A block walks groups blockIdx.x, + gridDim.x, ..., keeps PF groups prefetched in register slots that shift every group (PF = 0
for the wave-per-row plans; 2, 1 or 0 for the block-per-row ones by dtype, packs and kind), alternates its LDS row-sum buffer with
the group's parity, accumulates dw / db in registers over every group it visits and writes one partial row; norm_fold_kernel adds
the nblk partial rows (an 8-way unrolled loop while nblk >= 29, then a remainder loop). On MI355X (256 CUs) resident can only be
256, 512, 768 or 1024; the row counts below bracket each of them instead of guessing one.

Shapes come from the plan mirror of tests/test_norm_abi.py (pinned there, without a GPU, against the library's workspace query).
Every tolerance is stated in the test that uses it; u = 2^-24 is the f32 unit roundoff, and "half an ulp" is half the spacing of the
16-bit output format at the larger of |got| and |want| (the kernels compute in f32 and round once on the store).
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.test_norm_abi import PLANS, bwd_plan, pack, plan_cols, ws_bytes

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = 1e-5
NAME = {H.F32: "f32", H.BF16: "bf16", H.F16: "f16"}
KNAME = {H.NORM_RMS: "rms", H.NORM_LAYER: "layer"}

# nrb for the exact walk test. Fold: nblk = nrb below any resident; 1..28 run only the fold's remainder loop, 29 / 31 / 32 / 33 / 61 its
# 8-way loop plus 0..3 remainder partials per wave. Resident: each of 256 / 512 / 768 / 1024 bracketed, so whichever it is, some row
# count runs exactly one round, one round plus a single group (the last block walks two), and one group short of a round. 2049 and 3001:
# two to twelve rounds per block, uneven (3001 is no multiple of 256).
NRB_FOLD = (1, 2, 3, 4, 5, 8, 28, 29, 31, 32, 33, 61)
NRB_RESIDENT = (255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2049)
NRB_MANY = (3001,)
NRB_MULTI_ROUND = 3 * 1024 + 1  # at least three rounds (four for the last blocks) at any resident


def rpb(plan):
    return 256 // plan[0] if plan[0] < 256 else 1


def prefetch(code, plan, kind):
    """PF of norm_bwd_launch: rows requested ahead of the one being worked on."""
    tpr, packs = plan
    if tpr <= 64:
        return 0
    if code != H.F32 and tpr == 1024:
        return (1 if kind == H.NORM_RMS else 0) if packs == 2 else (2 if kind == H.NORM_RMS else 1)
    return 2


def npdt(code):
    return {H.F32: np.float32, H.BF16: np.uint16, H.F16: np.float16}[code]


def to_dev(a64, code):
    """float64 values (already representable in `code`) -> the dtype's storage array."""
    return O.from_float(np.asarray(a64, dtype=np.float32), code)


def as64(a, code):
    return O.to_float(a, code).astype(np.float64)


def rounded(a, code):
    """Values of `a` rounded to `code` (round to nearest even), as float64."""
    return as64(to_dev(a, code), code)


def half_ulp(v, code):
    """Half the spacing of the 16-bit format at |v| (0 for f32 outputs)."""
    if code == H.F32:
        return np.zeros_like(v)
    mbits, emin = (7, -126) if code == H.BF16 else (10, -14)
    _, e = np.frexp(np.abs(v))
    return np.ldexp(0.5, np.maximum(e - 1, emin) - mbits)


def check_bound(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err - bound, -np.inf)), got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.size} outside the bound; worst at {i}: got {got[i]!r} want {want[i]!r} "
                             f"bound {bound[i]!r}")


def ptr(b):
    return b.ptr if b is not None else None


def h2d_rows(buf, arr, row0, ld_bytes):
    """Copy a host [n, cols] array into rows row0.. of a device matrix with a row pitch of ld_bytes."""
    arr = np.ascontiguousarray(arr)
    if arr.shape[1] * arr.itemsize == ld_bytes:
        H.check(H.lib().kf_memcpy_h2d(buf.ptr + row0 * ld_bytes, arr.ctypes.data, arr.nbytes, None))
    else:
        for i in range(arr.shape[0]):
            H.check(H.lib().kf_memcpy_h2d(buf.ptr + (row0 + i) * ld_bytes, arr[i].ctypes.data, arr[i].nbytes, None))


def d2h_rows(buf, row0, n, cols, code, ld=None):
    ld = cols if ld is None else ld
    out = np.empty((n, ld), npdt(code))
    H.check(H.lib().kf_memcpy_d2h(out.ctypes.data, buf.ptr + row0 * ld * out.itemsize, out.nbytes, None))
    return out[:, :cols]


def run_bwd(kind, code, rows, cols, bx, bw, bm, br, bdy, bdx, bdw, bdb, ld=None, ws=None):
    """kf_norm_bwd with an explicit workspace: the one given (sized for a larger call with the same cols) or one of the exact size."""
    ld = cols if ld is None else ld
    need = ws_bytes(kind, code, rows, cols, ld)
    if ws is None and need and (bdw is not None or bdb is not None):
        ws = H.DevBuf(need)
    if ws is not None:
        assert ws.nbytes >= need
    H.check(H.lib().kf_norm_bwd(kind, code, rows, cols, ld, ptr(bx), ptr(bw), ptr(bm), ptr(br), ptr(bdy), ptr(bdx), ptr(bdw), ptr(bdb),
                                ptr(ws), ws.nbytes if ws is not None else 0, None))
    return ws


def run_fwd(kind, code, rows, cols, bx, bw, bb, by, bm, br, ld=None):
    H.check(H.lib().kf_norm_fwd(kind, code, rows, cols, cols if ld is None else ld, ptr(bx), ptr(bw), ptr(bb), EPS, ptr(by), ptr(bm),
                                ptr(br), None))


# ---- 2. exact walk: mean = 0, rstd = 1, small-integer x and dy -----------------------------------------------------------------------

EXACT_CASES = [(p, c, k) for p in PLANS for c in (H.F32, H.BF16) for k in (H.NORM_RMS, H.NORM_LAYER)]
EXACT_CASES += [(p, H.F16, k) for p in ((16, 1), (64, 2), (1024, 2)) for k in (H.NORM_RMS, H.NORM_LAYER)]


@pytest.mark.parametrize("plan,code,kind", EXACT_CASES, ids=[f"{t}x{p}-{NAME[c]}-{KNAME[k]}" for (t, p), c, k in EXACT_CASES])
def test_exact_walk(plan, code, kind):
    """The walk, bit for bit. With mean = 0 and rstd = 1 passed in, xhat = x exactly; x in [-4, 4] and dy in [-2, 2] are integers, so
    every partial of dw = sum dy x and db = sum dy is an integer below 2^24 in magnitude and exact in f32 in ANY summation order.
    So f32 dw / db must equal the int64 column sums, and 16-bit ones their round-to-nearest-even; a dropped, doubled or misplaced
    row group, prefetch slot, partial row or column fails, with no tolerance. Each plan runs at its smallest column count and at a
    ragged one (npk not a multiple of TPR: lanes holding dead columns), at every nrb of NRB_FOLD, NRB_RESIDENT and NRB_MANY, with
    the last group partial (r = 1..RPB rows).

    dx in the same runs, against float64 of dx = g - mean(g) - x mean(g x) (rms: no mean(g)), g = dy w, w from {+-0.5, +-1, 1.5, 2}:
    the row sums are exact too, so the f32 result carries only the roundings of inv_n = 1 / cols, the two products and the two
    differences: |err| <= 8 u (|g| + |mean g| + |x mean(g x)|), plus half an ulp for 16-bit outputs. The group after the last row
    (sentinel-filled, never written by an earlier, smaller run: row counts ascend) must stay untouched."""
    R = rpb(plan)
    el = np.dtype(npdt(code)).itemsize
    counts = sorted(NRB_FOLD + NRB_RESIDENT + NRB_MANY)
    # the last group holds r rows, cycling through 1..RPB (r = RPB: a full group) so that partial groups meet every round count
    rows_list = [(n - 1) * R + 1 + (i * 5) % R for i, n in enumerate(counts)]
    rows_list[-1] = counts[-1] * R  # (the largest run: a full last group)
    rng = np.random.default_rng(1000 + 97 * PLANS.index(plan) + 7 * code + kind)
    lo, ragged, _ = plan_cols(code, plan)
    for cols in sorted({lo, ragged}):
        assert bwd_plan(code, cols)[:2] == plan
        maxr = max(rows_list) + R  # + one sentinel group
        x = rng.integers(-4, 5, size=(maxr, cols), dtype=np.int8)
        dy = rng.integers(-2, 3, size=(maxr, cols), dtype=np.int8)
        w = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0, 1.5, 2.0]), size=cols)
        bx, bdy, bw = H.DevBuf.from_numpy(to_dev(x, code)), H.DevBuf.from_numpy(to_dev(dy, code)), H.DevBuf.from_numpy(to_dev(w, code))
        bm, br = H.DevBuf.from_numpy(np.zeros(maxr, np.float32)), H.DevBuf.from_numpy(np.ones(maxr, np.float32))
        sentinel = np.full((maxr, cols), 0x7fc0 if code == H.BF16 else 0x7e00, dtype=np.uint16)  # a quiet NaN in the 16-bit formats
        bdx = H.DevBuf.from_numpy(sentinel if code != H.F32 else np.full((maxr, cols), np.nan, np.float32))
        bdw, bdb = H.DevBuf(cols * el), (H.DevBuf(cols * el) if kind == H.NORM_LAYER else None)
        ws = H.DevBuf(ws_bytes(kind, code, maxr, cols))  # min(nrb, 1024) partial rows: enough for every run below
        x64, g64 = x.astype(np.float64), dy.astype(np.float64) * w
        s2 = (g64 * x64).mean(1, keepdims=True)
        s1 = g64.mean(1, keepdims=True) if kind == H.NORM_LAYER else np.zeros_like(s2)
        want_dx = g64 - s1 - x64 * s2
        mag_dx = 8 * U32 * (np.abs(g64) + np.abs(s1) + np.abs(x64 * s2))
        acc_w, acc_b, done = np.zeros(cols, np.int64), np.zeros(cols, np.int64), 0
        for nrb, rows in zip(counts, rows_list):
            assert -(-rows // R) == nrb
            run_bwd(kind, code, rows, cols, bx, bw, None if kind == H.NORM_RMS else bm, br, bdy, bdx, bdw, bdb, ws=ws)
            H.device_sync()
            xs, ds = x[done:rows].astype(np.int64), dy[done:rows].astype(np.int64)
            acc_w += (xs * ds).sum(0)
            acc_b += ds.sum(0)
            assert np.abs(acc_w).max() < 2 ** 24 and np.abs(acc_b).max() < 2 ** 24
            if code == H.F16:
                assert np.abs(acc_w).max() <= 65504 and np.abs(acc_b).max() <= 65504  # (so that the expected 16-bit sums are finite)
            what = f"{NAME[code]} {KNAME[kind]} cols {cols} nrb {nrb} rows {rows}"
            got_w, want_w = as64(bdw.to_numpy((cols,), npdt(code)), code), rounded(acc_w, code)
            assert np.array_equal(got_w, want_w), f"dw {what}: columns {np.flatnonzero(got_w != want_w)[:8]} differ"
            if bdb is not None:
                got_b, want_b = as64(bdb.to_numpy((cols,), npdt(code)), code), rounded(acc_b, code)
                assert np.array_equal(got_b, want_b), f"db {what}: columns {np.flatnonzero(got_b != want_b)[:8]} differ"
            # dx: the rows this run adds to the previous one's (a row's dx does not depend on the walk: test_bitwise_properties), then
            # the sentinel group behind them
            got = as64(d2h_rows(bdx, done, rows + R - done, cols, code), code)
            want = want_dx[done:rows]
            bound = mag_dx[done:rows] + half_ulp(np.maximum(np.abs(got[:rows - done]), np.abs(want)), code)
            check_bound(got[:rows - done], want, bound, f"dx {what}")
            assert np.isnan(got[rows - done:]).all(), f"dx {what}: rows past the end were written"
            done = rows


# ---- 3. parity with float64 on random data, at multi-round shapes --------------------------------------------------------------------

def reference_check(kind, code, x, w, b, dy, y, mean, rstd, dx=None, dw=None, db=None, c_dx=48, c_sum=96, drop_groups=(), what=""):
    """Check one forward (y may be None) and backward (dx / dw / db, each may be None) against plain float64, in row chunks.

    forward, with the kernel's own f32 mean m' and rstd r':  |m' - mean(x)| <= 256 u mean|x| (per-lane sums of up to 64 terms,
      then a tree); |r' - 1 / sqrt(mean((x - m')^2) + eps)| <= 128 u r'  (rms: mean(x^2)) - the centred squares about the kernel's
      own mean, which is what an exact two-pass variance computes (a one-pass E[x^2] - E[x]^2 misses it by ~u (mean / std)^2);
      y = (x - m') r' w + b: |err| <= 8 u (|xhat w| + |b|) + half an ulp (three f32 roundings, then the store's).
    backward, evaluated with the same f32 m', r' it was given: xhat = (x - m') r', g = dy w, dx = r' (g - mean(g) - xhat mean(g xhat)):
      |err dx| <= c_dx u r' (|g| + mean|g| + |xhat| mean|g xhat|) + half an ulp: the roundings of xhat, g and the final expression
      (<= 8 u of the first terms) and of the two f32 row sums (per-lane sums of <= 16 terms, then trees over <= 1024 lanes: <= 32 u).
      dw = sum_rows dy xhat, db = sum_rows dy: |err| <= c_sum u sum_rows |term| per column, plus half an ulp: each term carries <= 3
      roundings, and the sums chain at most ~13 rows per block slot (resident 256, 3073 groups), 31 slot additions, 32 sequential
      partial rows per fold lane and two short trees: <= ~85 additions on any path. The bound scales with the magnitudes summed, not
      with the row count.
    drop_groups: (row0, row1) ranges; each must, if left out of dw (db), move the reference outside the bound in some column: the
      bound is tight enough to see a single missing row group."""
    rows, cols = x.shape
    layer = kind == H.NORM_LAYER
    wf = np.ones(cols) if w is None else as64(w, code)
    bf = np.zeros(cols) if b is None else as64(b, code)
    sw, sb, aw, ab = (np.zeros(cols) for _ in range(4))
    dropped = [[np.zeros(cols), np.zeros(cols)] for _ in drop_groups]
    step = max(1, (1 << 22) // cols)
    for r0 in range(0, rows, step):
        r1 = min(rows, r0 + step)
        xs = as64(x[r0:r1], code)
        r = rstd[r0:r1, None].astype(np.float64)
        m = np.zeros_like(r)
        if layer:
            m = mean[r0:r1, None].astype(np.float64)
            check_bound(m, xs.mean(1, keepdims=True), 256 * U32 * np.abs(xs).mean(1, keepdims=True), f"mean {what} rows {r0}..")
        r_ref = 1.0 / np.sqrt(((xs - m) ** 2).mean(1, keepdims=True) + EPS)
        check_bound(r, r_ref, 128 * U32 * r_ref, f"rstd {what} rows {r0}..")
        xh = (xs - m) * r
        if y is not None:
            ys = xh * wf + bf
            gy = as64(y[r0:r1], code)
            check_bound(gy, ys, 8 * U32 * (np.abs(xh * wf) + np.abs(bf)) + half_ulp(np.maximum(np.abs(gy), np.abs(ys)), code),
                        f"y {what} rows {r0}..")
        if dy is None:
            continue
        ds = as64(dy[r0:r1], code)
        if dx is not None:
            g = ds * wf
            s1 = g.mean(1, keepdims=True) if layer else 0.0
            s2 = (g * xh).mean(1, keepdims=True)
            want = r * (g - s1 - xh * s2)
            T = r * (np.abs(g) + (np.abs(g).mean(1, keepdims=True) if layer else 0.0) + np.abs(xh) * np.abs(g * xh).mean(1, keepdims=True))
            gd = as64(dx[r0:r1], code)
            check_bound(gd, want, c_dx * U32 * T + half_ulp(np.maximum(np.abs(gd), np.abs(want)), code), f"dx {what} rows {r0}..")
        sw += (ds * xh).sum(0)
        aw += np.abs(ds * xh).sum(0)
        sb += ds.sum(0)
        ab += np.abs(ds).sum(0)
        for (g0, g1), acc in zip(drop_groups, dropped):
            a0, a1 = max(g0, r0), min(g1, r1)
            if a0 < a1:
                acc[0] += (ds[a0 - r0:a1 - r0] * xh[a0 - r0:a1 - r0]).sum(0)
                acc[1] += ds[a0 - r0:a1 - r0].sum(0)
    for name, got, want, mag, j in (("dw", dw, sw, aw, 0), ("db", db, sb, ab, 1)):
        if got is None:
            continue
        gf = as64(got, code)
        check_bound(gf, want, c_sum * U32 * mag + half_ulp(np.maximum(np.abs(gf), np.abs(want)), code), f"{name} {what}")
        for (g0, g1), acc in zip(drop_groups, dropped):
            # sensitivity of the bound itself: the reference without rows g0..g1 must fall outside it in some column
            assert (np.abs(acc[j]) > c_sum * U32 * mag + half_ulp(np.abs(want - acc[j]), code)).any(), \
                f"{name} {what}: the bound would not notice rows {g0}..{g1} missing"


def random_case(rng, code, rows, cols, kind, with_w):
    """x ~ N(0.3, 1) with per-column offsets, dy ~ N(0, 0.1), w ~ 1 + N(0, 0.1), b ~ N(0, 0.1); all rounded to `code`."""
    f = lambda a: to_dev(a, code)  # noqa: E731
    x = f(rng.standard_normal((rows, cols), dtype=np.float32) + 0.3 + 0.2 * rng.standard_normal(cols, dtype=np.float32))
    dy = f(0.1 * rng.standard_normal((rows, cols), dtype=np.float32))
    w = f(1 + 0.1 * rng.standard_normal(cols, dtype=np.float32)) if with_w else None
    b = f(0.1 * rng.standard_normal(cols, dtype=np.float32)) if with_w and kind == H.NORM_LAYER else None
    return x, dy, w, b


def fwd_bwd(kind, code, x, w, b, dy):
    """Forward (y, f32 mean, rstd), then backward with those statistics (dx, dw, db) through the C ABI."""
    rows, cols = x.shape
    el = x.itemsize
    bx, bdy = H.DevBuf.from_numpy(x), H.DevBuf.from_numpy(dy)
    bw = H.DevBuf.from_numpy(w) if w is not None else None
    bb = H.DevBuf.from_numpy(b) if b is not None else None
    by, bm, br = H.DevBuf(x.nbytes), H.DevBuf(4 * rows), H.DevBuf(4 * rows)
    run_fwd(kind, code, rows, cols, bx, bw, bb, by, bm, br)
    bdx, bdw = H.DevBuf(x.nbytes), H.DevBuf(cols * el)
    bdb = H.DevBuf(cols * el) if kind == H.NORM_LAYER else None
    ws = run_bwd(kind, code, rows, cols, bx, bw, bm if kind == H.NORM_LAYER else None, br, bdy, bdx, bdw, bdb)
    H.device_sync()
    del ws
    y = by.to_numpy(x.shape, x.dtype)
    mean, rstd = bm.to_numpy((rows,), np.float32), br.to_numpy((rows,), np.float32)
    dx = bdx.to_numpy(x.shape, x.dtype)
    dw = bdw.to_numpy((cols,), x.dtype)
    db = bdb.to_numpy((cols,), x.dtype) if bdb is not None else None
    return y, mean, rstd, dx, dw, db


PARITY_CASES = [(p, c, k) for p in PLANS for c in (H.F32, H.BF16, H.F16) for k in (H.NORM_RMS, H.NORM_LAYER)]


@pytest.mark.parametrize("plan,code,kind", PARITY_CASES, ids=[f"{t}x{p}-{NAME[c]}-{KNAME[k]}" for (t, p), c, k in PARITY_CASES])
def test_parity_multi_round(plan, code, kind):
    """Every plan x dtype x kind, with weight (and bias for layer) and without, at nrb = 3 * 1024 + 1 groups (>= 3 rounds per block
    at any resident, an extra group for the first block) and a partial last group; ragged column count (dead lanes). Random data, the
    forward's own f32 mean / rstd fed to the backward, checked against float64 with the bounds of reference_check. The bound is
    shown, in every case, to notice a missing middle group and a missing last group."""
    R = rpb(plan)
    rows = (NRB_MULTI_ROUND - 1) * R + max(1, R // 2 + 1)
    cols = plan_cols(code, plan)[1]
    assert bwd_plan(code, cols)[:2] == plan
    rng = np.random.default_rng(2000 + 97 * PLANS.index(plan) + 7 * code + kind)
    for with_w in (True, False):
        x, dy, w, b = random_case(rng, code, rows, cols, kind, with_w)
        y, mean, rstd, dx, dw, db = fwd_bwd(kind, code, x, w, b, dy)
        mid = (NRB_MULTI_ROUND // 2) * R
        reference_check(kind, code, x, w, b, dy, y, mean, rstd, dx, dw, db, drop_groups=((mid, mid + R), ((NRB_MULTI_ROUND - 1) * R, rows)),
                        what=f"{plan} {NAME[code]} {KNAME[kind]} w={with_w} PF={prefetch(code, plan, kind)} [{rows}, {cols}]")


# ---- 4. bitwise properties -----------------------------------------------------------------------------------------------------------

# layer norm, nrb = 3073 (>= 3 rounds): 8 rows per block (PF 0), 4 rows per block (PF 0), then one row per block with PF 2, 1 (16-bit,
# 1024 threads, one pack), 0 (16-bit, 1024 threads, two packs) and 2 (f32, 1024 threads, two packs)
BITWISE_CASES = [((32, 1), H.BF16), ((64, 2), H.F32), ((256, 1), H.BF16), ((1024, 1), H.BF16), ((1024, 2), H.BF16), ((1024, 2), H.F32)]


@pytest.mark.parametrize("plan,code", BITWISE_CASES, ids=[f"{t}x{p}-{NAME[c]}" for (t, p), c in BITWISE_CASES])
def test_bitwise_properties(plan, code):
    """Layer norm at a multi-round shape (nrb = 3073; RPB 8 and 4 with PF 0, one row per block with PF 2 / 1 / 0), exact equality:
    - two runs give identical dx, dw, db (fixed fold order, no atomics);
    - dx[a:b] of the full run equals dx of a run on rows a..b alone (every row's arithmetic is the same whichever block and slot
      visits it; any row offset keeps the 16-byte alignment, as ld is a multiple of the pack, so the same plan runs);
    - rows at a pitch ld > cols (ld % V == 0: same plan): dx, dw, db equal the contiguous run's, and the ld - cols elements between
      dx's rows keep their sentinel;
    - the register-tile kernel and the fold ran (profile names), not the generic kernel."""
    kind, R = H.NORM_LAYER, rpb(plan)
    rows = (NRB_MULTI_ROUND - 1) * R + 1
    cols = plan_cols(code, plan)[1]
    rng = np.random.default_rng(3000 + PLANS.index(plan) + code)
    x, dy, w, _ = random_case(rng, code, rows, cols, kind, True)
    mean = rng.uniform(-0.5, 0.5, rows).astype(np.float32)
    rstd = rng.uniform(0.5, 2.0, rows).astype(np.float32)
    el = x.itemsize

    def run(xa, dya, ma, ra, ld=None, sentinel=None):
        n = xa.shape[0]
        ld = cols if ld is None else ld
        def up(a):
            if ld == cols:
                return H.DevBuf.from_numpy(a)
            big = np.zeros((n, ld), a.dtype)
            big[:, :cols] = a
            return H.DevBuf.from_numpy(big)
        bx, bdy, bw = up(xa), up(dya), H.DevBuf.from_numpy(w)
        bm, br = H.DevBuf.from_numpy(ma), H.DevBuf.from_numpy(ra)
        bdx = H.DevBuf.from_numpy(np.full((n, ld), sentinel, xa.dtype)) if sentinel is not None else H.DevBuf(n * ld * el)
        bdw, bdb = H.DevBuf(cols * el), H.DevBuf(cols * el)
        ws = run_bwd(kind, code, n, cols, bx, bw, bm, br, bdy, bdx, bdw, bdb, ld=ld)
        H.device_sync()
        del ws
        dxf = bdx.to_numpy((n, ld), xa.dtype)
        return dxf[:, :cols].copy(), dxf[:, cols:], bdw.to_numpy((cols,), xa.dtype), bdb.to_numpy((cols,), xa.dtype)

    H.profile_enable(True)
    H.profile_reset()
    try:
        full = run(x, dy, mean, rstd)
        prof = H.profile_results()
    finally:
        H.profile_enable(False)
    assert "norm_bwd" in prof and "norm_bwd_fold" in prof and "norm_bwd_generic" not in prof, sorted(prof)
    again = run(x, dy, mean, rstd)
    for i, name in ((0, "dx"), (2, "dw"), (3, "db")):
        assert np.array_equal(full[i].view(np.uint8), again[i].view(np.uint8)), f"{name} differs between two runs"
    a0, a1 = 517 * R + 3, 517 * R + 3 + 1500 * R + 7  # not group-aligned: rows change block, slot and round
    part = run(x[a0:a1], dy[a0:a1], mean[a0:a1], rstd[a0:a1])
    assert np.array_equal(part[0].view(np.uint8), full[0][a0:a1].view(np.uint8)), "dx of a row depends on the rows around it"
    V = pack(code)
    ld = cols + 3 * V
    sent = {H.F32: np.float32(-7.25), H.BF16: np.uint16(0x4242), H.F16: np.float16(-7.25)}[code]
    strided = run(x, dy, mean, rstd, ld=ld, sentinel=sent)
    assert np.array_equal(strided[0].view(np.uint8), full[0].view(np.uint8)), "dx with ld > cols"
    assert np.array_equal(strided[2].view(np.uint8), full[2].view(np.uint8)), "dw with ld > cols"
    assert np.array_equal(strided[3].view(np.uint8), full[3].view(np.uint8)), "db with ld > cols"
    assert (strided[1] == sent).all(), "elements between dx rows were written"


# ---- 5. statistics edges -------------------------------------------------------------------------------------------------------------

def offset_rows(rng, code, rows, cols):
    """Rows far from zero with a small spread: f32 1e4 + U(-1, 1); f16 / bf16 2^14 + k * spacing, |k| <= 4 (spacing 16 / 128 above
    2^14: the largest offset where a few steps of the format still leave a spread)."""
    if code == H.F32:
        return (1e4 + rng.uniform(-1, 1, (rows, cols))).astype(np.float32)
    step = 16.0 if code == H.F16 else 128.0
    return to_dev(16384.0 + step * rng.integers(-4, 5, (rows, cols)), code)


# per dtype, backward plans: f32 (256, 1) PF 2 and (1024, 2) PF 2; bf16 (256, 1) PF 2 and (1024, 2) PF 1 / 0; f16 (64, 2) PF 0 (four rows per
# block) and (1024, 2) PF 1 / 0. 777 rows: one round or less; these cases are about the statistics, not the walk.
EDGE_COLS = {H.F32: (1024, 4100), H.BF16: (2048, 12288), H.F16: (1024, 8200)}


@pytest.mark.parametrize("code", (H.F32, H.BF16, H.F16), ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", (H.NORM_RMS, H.NORM_LAYER), ids=["rms", "layer"])
def test_statistics_edges(kind, code):
    """Forward and backward against float64 (bounds of reference_check), on rows that stress the statistics, mixed with ordinary
    rows: a large offset with a small spread (layer: an exact two-pass variance passes, E[x^2] - E[x]^2 in f32 is off by u (mean /
    std)^2 ~ 1e-5 to 1 relatively and fails); constant rows (layer: variance 0) and all-zero rows (rms: mean square 0), where rstd =
    1 / sqrt(eps) in the forward and in dx; one spike of 1e3 (16-bit: 512) in a row of values ~1e-3."""
    rng = np.random.default_rng(4000 + 10 * kind + code)
    for cols in EDGE_COLS[code]:
        assert bwd_plan(code, cols) is not None
        rows = 777
        x, dy, w, b = random_case(rng, code, rows, cols, kind, True)
        xf = as64(x, code)
        if kind == H.NORM_LAYER:
            xf[0:200] = as64(offset_rows(rng, code, 200, cols), code)
            xf[200:210] = 3.0  # constant, dyadic: variance exactly 0
            xf[210:220] = 0.1  # constant, not dyadic
        xf[220:230] = 0.0
        small = rng.uniform(-1e-3, 1e-3, (10, cols))
        small[np.arange(10), rng.integers(0, cols, 10)] = 512.0 if code != H.F32 else 1e3
        xf[230:240] = small
        x = to_dev(xf, code)
        y, mean, rstd, dx, dw, db = fwd_bwd(kind, code, x, w, b, dy)
        assert np.isfinite(as64(y, code)).all() and np.isfinite(as64(dx, code)).all()
        r0 = 1.0 / np.sqrt(np.float32(EPS))
        zero = slice(200, 220) if kind == H.NORM_LAYER else slice(220, 230)
        assert np.allclose(rstd[zero], r0, rtol=128 * U32, atol=0), rstd[zero]
        reference_check(kind, code, x, w, b, dy, y, mean, rstd, dx, dw, db, what=f"edges {NAME[code]} {KNAME[kind]} cols {cols}")


# ---- 6. through the operator API -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bf16", (False, True), ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ("rms", "layer"))
def test_operator_api_multi_round(name, bf16):
    """kfunca.rms_norm / layer_norm with autograd at [3073, 4096] (bf16: the 512-thread plan, f32: the 1024-thread one; 3073 groups,
    >= 3 rounds at any resident), through NormGradFunction's workspace allocation. Forms: trainable weight (and bias); frozen weight
    (requires_grad False: dx still right, no weight gradient produced); layer: a trainable bias with a frozen weight. The API keeps
    its f32 statistics to itself, so they are recomputed through kf_norm_fwd on the same input (the same kernel on the same values,
    so the same bits); y, dx, dw, db are then held to reference_check's float64 bounds."""
    code = H.BF16 if bf16 else H.F32
    kind = H.NORM_RMS if name == "rms" else H.NORM_LAYER
    rows, cols = 3073, 4096
    assert bwd_plan(code, cols)[2] == 1
    rng = np.random.default_rng(5000 + bf16 + 2 * (name == "layer"))
    xn, dyn, wn, bn = random_case(rng, code, rows, cols, kind, True)
    y_abi, mean, rstd, _, _, _ = fwd_bwd(kind, code, xn, wn, bn, dyn)

    def leaf(a, grad):
        t = kfunca.from_numpy(O.to_float(a, code).astype(np.float32), 0)
        t = t.bfloat16() if bf16 else t
        t.set_requires_grad(grad)
        return t

    def get(t):  # (exact: the tensor holds values of `code`)
        return to_dev(t.float().numpy(), code)

    forms = [(True, True), (False, False)] + ([(False, True)] if kind == H.NORM_LAYER else [])
    for w_grad, b_grad in forms:
        tx, tw = leaf(xn, True), leaf(wn, w_grad)
        if kind == H.NORM_RMS:
            y = kfunca.rms_norm(tx, tw, EPS)
        else:
            tb = leaf(bn, b_grad)
            y = kfunca.layer_norm(tx, tw, tb, EPS)
        tg = kfunca.from_numpy(O.to_float(dyn, code).astype(np.float32), 0)
        y.backward(tg.bfloat16() if bf16 else tg)
        what = f"api {name} {NAME[code]} w_grad={w_grad} b_grad={b_grad}"
        assert tw.grad().defined() == w_grad, what
        if kind == H.NORM_LAYER:
            assert tb.grad().defined() == b_grad, what
        yv = get(y)
        assert np.array_equal(yv.view(np.uint8), y_abi.view(np.uint8)), f"y {what}: the API's forward differs from kf_norm_fwd"
        reference_check(kind, code, xn, wn, bn, dyn, yv, mean, rstd, dx=get(tx.grad()), dw=get(tw.grad()) if w_grad else None,
                        db=get(tb.grad()) if kind == H.NORM_LAYER and b_grad else None, what=what)


# ---- 7. beyond 2^31 elements ---------------------------------------------------------------------------------------------------------

@pytest.mark.slow
@pytest.mark.parametrize("kind", (H.NORM_RMS, H.NORM_LAYER), ids=["rms", "layer"])
def test_bf16_beyond_2_31_elements(kind):
    """bf16 [524386, 4096] (2.15e9 elements, 4.3 GB per operand; the 512-thread plan, one row per group, 512 to 2049 groups per block):
    a 63-row integer tile (x in [-4, 4], dy in [-2, 2]) repeated down the rows, uploaded with kf_memcpy_h2d. Rows 0..59 of the tile come
    in pairs (x, dy) and (x, -dy), so the tile's column sums of dy x and dy come from rows 60..62 alone (|.| <= 24 and 6): every column
    total and every partial stays below 2^24 and is exact in f32. An odd tile length also gives each block (a block walks rows b,
    b + nblk, ..., and nblk is a multiple of 64) rows from every tile row, so a block's partial row is no multiple of one tile row's
    terms and no two blocks' partials cancel. With mean = 0, rstd = 1 passed in, dw / db must equal the bf16 rounding of the int64
    totals bit for bit (the trick of test_exact_walk). dx: rows on both sides of element 2^31 and the last row, against float64 with
    test_exact_walk's bound. The forward runs first, on the same x: y / mean / rstd of those rows against float64 with
    reference_check's bounds."""
    code, cols, T = H.BF16, 4096, 63
    rows = 8323 * T + 37  # 8323 full tiles and a partial one
    assert rows * cols > 1 << 31
    rng = np.random.default_rng(6000 + kind)
    tx = rng.integers(-4, 5, size=(T, cols)).astype(np.int64)
    tdy = rng.integers(-2, 3, size=(T, cols)).astype(np.int64)
    tx[1:60:2] = tx[0:60:2]
    tdy[1:60:2] = -tdy[0:60:2]
    w = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0, 1.5, 2.0]), size=cols)
    full, rem = divmod(rows, T)
    tot_w = full * (tx * tdy).sum(0) + (tx[:rem] * tdy[:rem]).sum(0)
    tot_b = full * tdy.sum(0) + tdy[:rem].sum(0)
    assert np.abs(tot_w).max() < 2 ** 24 and np.abs(tot_b).max() < 2 ** 24
    nb = rows * cols * 2
    bx, bdy, bdx = H.DevBuf(nb), H.DevBuf(nb), H.DevBuf(nb)
    chunk_x, chunk_dy = np.tile(to_dev(tx, code), (64, 1)), np.tile(to_dev(tdy, code), (64, 1))  # 64 tiles per copy
    for r0 in range(0, rows, chunk_x.shape[0]):
        n = min(chunk_x.shape[0], rows - r0)
        h2d_rows(bx, chunk_x[:n], r0, cols * 2)
        h2d_rows(bdy, chunk_dy[:n], r0, cols * 2)
    bw = H.DevBuf.from_numpy(to_dev(w, code))
    edge = (1 << 31) // cols
    check_rows = (0, edge - 1, edge, edge + 1, rows - 1)
    # forward (y into the dx buffer), checked on the rows around element 2^31
    bm, br = H.DevBuf(4 * rows), H.DevBuf(4 * rows)
    bb = H.DevBuf.from_numpy(to_dev(np.full(cols, 0.25), code)) if kind == H.NORM_LAYER else None
    run_fwd(kind, code, rows, cols, bx, bw, bb, bdx, bm, br)
    H.device_sync()
    mean_all, rstd_all = bm.to_numpy((rows,), np.float32), br.to_numpy((rows,), np.float32)
    for t in check_rows:
        xs = to_dev(tx[t % T][None], code)
        y = d2h_rows(bdx, t, 1, cols, code)
        reference_check(kind, code, xs, to_dev(w, code), to_dev(np.full(cols, 0.25), code) if kind == H.NORM_LAYER else None, None, y,
                        mean_all[t:t + 1], rstd_all[t:t + 1], what=f"fwd row {t}")
    # backward at mean = 0, rstd = 1
    H.check(H.lib().kf_memset_zero(bm.ptr, 4 * rows, None))
    ones = np.ones(rows, np.float32)  # (bound to a name: a temporary would be freed before the copy reads it)
    H.check(H.lib().kf_memcpy_h2d(br.ptr, ones.ctypes.data, ones.nbytes, None))
    bdw, bdb = H.DevBuf(cols * 2), (H.DevBuf(cols * 2) if kind == H.NORM_LAYER else None)
    ws = run_bwd(kind, code, rows, cols, bx, bw, bm if kind == H.NORM_LAYER else None, br, bdy, bdx, bdw, bdb)
    H.device_sync()
    del ws
    assert np.array_equal(as64(bdw.to_numpy((cols,), np.uint16), code), rounded(tot_w, code)), "dw beyond 2^31"
    if bdb is not None:
        assert np.array_equal(as64(bdb.to_numpy((cols,), np.uint16), code), rounded(tot_b, code)), "db beyond 2^31"
    for t in check_rows:
        x64, g64 = tx[t % T].astype(np.float64), tdy[t % T] * w
        s2 = (g64 * x64).mean()
        s1 = g64.mean() if kind == H.NORM_LAYER else 0.0
        want = g64 - s1 - x64 * s2
        got = as64(d2h_rows(bdx, t, 1, cols, code)[0], code)
        bound = 8 * U32 * (np.abs(g64) + abs(s1) + np.abs(x64 * s2)) + half_ulp(np.maximum(np.abs(got), np.abs(want)), code)
        check_bound(got, want, bound, f"dx row {t}")
