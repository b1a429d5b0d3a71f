"""-m gpu: every kernel of the reduction engine (reduce.hip) against exact references, driven by the case table of
tests/test_reduce_plan_abi.py (each case names the kernel the planner must choose; that file checks it without a GPU, this one again
with the real pointers).

a. Sums and means of small integers in every dtype, bit for bit. Every partial sum stays far below 2^24, so f32 accumulation is exact and
   the output is the exact sum rounded once (16-bit outputs: round to nearest even); the mean is f32(S) * f32(f32(nout) / f32(numel))
   rounded once (f64: the same in f64; integers: nout / numel in integer arithmetic). Row sums stay within +-255 and every input is
   non-zero, so one dropped, duplicated or misplaced element changes the bits of a 16-bit output too.
b. Random data (magnitudes U(1, 10), random signs) against an exact float64 sum. The bound is gamma_h * sum|x| + half an ulp of the
   output, h the longest chain of additions one input goes through on the planned kernel (u = 2^-24 for f32 / 16-bit accumulation,
   2^-53 for f64). Each case asserts that twice its bound is below the smallest change one dropped input makes (the smallest |x| of the
   row, times the mean factor): a mutant's result lies within the bound of its own exact value, so it cannot pass.
c. Moments on every path against a two-pass float64 reference (bounds in `mom_bounds`), on data whose row groups differ (a trend along
   the reduced dim plus a period-64 sawtooth), each case asserting that its bounds would see one dropped row group of its plan.
   Constant rows give the mean exactly and a variance of exactly 0 on every path; the large-offset case (mean 1e4, spread 1) runs on
   every f32 / f64 path.
d. Geometry edges are cases of the table: nouter > 1024, tall grids with and without the XCD remap, rows off 16 bytes, C % vec != 0,
   outer strides off 16 bytes, several reduced dims.
e. The workspace contract on every split path; f. the operator API (profiler labels and values); g. one slow 2^31-byte case."""
import ctypes as C
import zlib

import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.gpu_util import Dev
from tests.test_reduce_plan_abi import FLOATS, MOM_CASES, NAME, SUM_CASES, multi_reduce_desc, plan_of

pytestmark = pytest.mark.gpu

U = {H.F32: 2.0 ** -24, H.BF16: 2.0 ** -24, H.F16: 2.0 ** -24, H.F64: 2.0 ** -53}
POISON = {H.BOOL: True, H.U8: 100, H.I8: 100, H.I16: 100, H.I32: 100, H.I64: 100}


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def store(v, code):
    """float64 / int64 values -> the dtype's storage array: one rounding (f32 first for 16-bit, exact when v is an f32 value)."""
    v = np.asarray(v)
    if code == H.BF16:
        return O.f32_to_bf16(v.astype(np.float32))
    if code == H.F16:
        return v.astype(np.float32).astype(np.float16)
    if code == H.BOOL:
        return v != 0
    return v.astype(H.CODE2NP[code])


def as64(a, code):
    return O.to_float(a, code).astype(np.float64) if code in FLOATS else a.astype(np.float64)


def half_ulp(v, code):
    """Half the spacing of the output format at |v| (0 for f32 / f64 outputs: the accumulator is stored as it is)."""
    if code in (H.F32, H.F64):
        return np.zeros_like(v)
    mbits, emin = (7, -126) if code == H.BF16 else (10, -14)
    _, e = np.frexp(np.abs(v))
    return np.ldexp(0.5, np.maximum(e - 1, emin) - mbits)


def from_rows(case, rows):
    """A case-shaped array from [nout, rtot] rows: output elements in the keepdim output's order, reduced elements row-major."""
    keep = [i for i in range(len(case.shape)) if i not in case.dims]
    full = rows.reshape([case.shape[i] for i in keep] + [case.shape[i] for i in case.dims])
    return np.transpose(full, np.argsort(keep + list(case.dims)))


def upload(case, rows, code=None):
    """The case's input (values given as [nout, rtot] storage rows) in its own layout; padding and the offset hold poison."""
    code = case.code if code is None else code
    dt = H.CODE2NP[code]
    poison = POISON.get(code, np.nan)
    base = np.full(case.nelem_base, poison, dtype=np.float32 if code == H.BF16 else dt)
    if code == H.BF16:
        base = O.f32_to_bf16(base)
    es = base.itemsize
    view = np.lib.stride_tricks.as_strided(base[case.offset:], case.shape, [s * es for s in case.strides])
    view[...] = from_rows(case, rows)
    return Dev(view, code, base=base)


def run(case, x, op=H.RED_SUM, mode=None, correction=1.0, eps=0.0):
    """One kf_reduce / kf_reduce_moments call on the case's geometry; returns the output(s) as [nout] storage arrays."""
    outs = [Dev.empty(case.out_shape, case.out_code) for _ in range(2 if case.op == "mom" else 1)]
    inp, views = case.views(x.view.ptr - case.offset * H.DTYPE_SIZE[case.code], [o.buf.ptr for o in outs])
    d = multi_reduce_desc(views[0], inp, case.dims, moments_out1=views[1] if case.op == "mom" else None)
    p = plan_of(d, case.op == "mom")
    assert p["kernel"] == case.kernel, (case.id, p)  # with the real pointers too
    if case.op == "mom":
        keep = H.reduce_moments(mode, d, correction, eps)
    else:
        keep = H.reduce(op, d)
    H.device_sync()
    del keep
    return [o.get().reshape(-1) for o in outs], p


def small_ints(rng, nout, n, signed=True):
    """[nout, n] non-zero integers of magnitude 1..3 whose every row sums to at most 51 in magnitude (192 for n <= 64): pairs (u, -u)
    plus a 16- or 17-element tail, shuffled along the row."""
    sign = (lambda s: rng.choice(np.array([-1, 1]), s)) if signed else (lambda s: np.ones(s, dtype=np.int64))
    if n <= 64:
        return rng.integers(1, 4, (nout, n)) * sign((nout, n))
    t = 16 + n % 2
    p = (n - t) // 2
    u = rng.integers(1, 4, (nout, p)) * sign((nout, p))
    tail = rng.integers(1, 4, (nout, t)) * sign((nout, t))
    rows = np.concatenate([u, -u if signed else u, tail], axis=1)
    return rows[:, rng.permutation(n)]


def depth(p, moments=False):
    """The longest chain of additions (sums) or Chan updates (moments) one input goes through on the planned kernel."""
    k = p["kernel"].split("+")[0]
    ns, R, vec, tx = p["nsplit"], p["R"], p["vec"], p["tx"]
    if k == "inner":
        chunk = -(-(R // vec) // ns) * vec if vec > 1 else -(-R // ns)
        ppl = -(-(-(-chunk // vec)) // tx)
        per_lane = (-(-ppl // 4) + 3) * (1 if moments else vec) + (vec if moments else 0)
        return per_lane + 2 + int(np.log2(tx)) + ns
    if k == "outer":
        chunk = -(-R // ns)
        return -(-chunk // (16 if not moments else 4)) + 3 + (4 if moments else 0) + 2 + 3 + ns
    if k == "outer_tall":
        return -(-R // 128) + 7 + 3 + 15
    return p["rtot"]  # inner_few, outer_few: one lane per output walks R; generic: rtot


def gamma(h, u):
    return h * u / (1 - h * u)


# ---- a. exact sums and means --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SUM_CASES, ids=lambda k: k.id)
def test_exact_sum_and_mean(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    code = case.code
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    if code == H.BOOL:
        ints = rng.integers(0, 2, (nout, n))
        ints[::7] = 0  # some all-false rows
    else:
        ints = small_ints(rng, nout, n, signed=code != H.U8)
    x = upload(case, store(ints, code))
    S = ints.sum(axis=1)
    numel = nout * n
    (got,), p = run(case, x, H.RED_SUM)
    want = store(S if code != H.U8 else S % 256, code)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (case.id, p, np.flatnonzero(got != want)[:8])
    (got,), _ = run(case, x, H.RED_MEAN)
    if code == H.F64:
        want = store(S.astype(np.float64) * (np.float64(nout) / np.float64(numel)), code)
    elif code in FLOATS:
        f = np.float32(np.float32(nout) / np.float32(numel))
        want = store((S.astype(np.float32) * f).astype(np.float64), code)
    else:
        want = store(S * (nout // numel), code)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (case.id, "mean", np.flatnonzero(got != want)[:8])


# ---- b. random data against an exact sum ------------------------------------------------------------------------------------
def exact_row_sums(x64):
    """Row sums of float64 values, exact to a few ulps: the values split into a part on a 2^-20 grid (summed exactly) and the rest."""
    hi = np.round(x64 * 2.0 ** 20) / 2.0 ** 20
    return hi.sum(axis=1) + (x64 - hi).sum(axis=1)


def sum_bound(case, p, mag, S, mean=False):
    """gamma_h * sum|x| (times the factor for the mean, plus its two roundings) and half an ulp of the output."""
    n = int(np.prod([case.shape[i] for i in case.dims]))
    u = U[case.code]
    b = gamma(depth(p), u) * mag + 4 * 2.0 ** -53 * np.abs(S)  # (+ the reference's own few ulps)
    if mean:
        b = b / n + 2 * u * np.abs(S / n)
        return b + half_ulp(S / n, case.code)
    return b + half_ulp(S, case.code)


def _random_ok(case):
    """Cases where an f32 / f64 accumulation bound can see one dropped input of the U(1, 10) draw (the expected sum|x| is 5.5 n): the
    longest 16-bit rows of the folds and of the tall kernel cannot be told apart from a row without one input by any such bound - they
    are held bit for bit in part a instead."""
    if case.code not in FLOATS:
        return False
    p = case.plan()
    n = p["rtot"]
    return 2 * (gamma(depth(p), U[case.code]) * 5.5 * n * 1.1 + (0.5 * 2.0 ** -8 * 60 if case.code == H.BF16 else 0)) < 1.0


RANDOM_CASES = [k for k in SUM_CASES if _random_ok(k)]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda k: k.id)
def test_random_sum_and_mean_within_an_accumulation_bound(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 1)
    code = case.code
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    # magnitudes U(1, 10) in balanced pairs (+v, -v) plus a short tail, so 16-bit outputs stay small enough to show one input
    mags = rng.uniform(1, 10, (nout, n))
    sgn = np.where(small_ints(rng, nout, n) > 0, 1.0, -1.0)
    if n > 64:
        t = 16 + n % 2
        p2 = (n - t) // 2
        mags[:, p2:2 * p2] = mags[:, :p2]
        sgn[:, :p2] = 1.0
        sgn[:, p2:2 * p2] = -1.0
        perm = rng.permutation(n)
        mags, sgn = mags[:, perm], sgn[:, perm]
    vals = store(mags * sgn, code)
    x64 = as64(vals, code)
    x = upload(case, vals)
    S = exact_row_sums(x64)
    mag = np.abs(x64).sum(axis=1)
    drop = np.abs(x64).min(axis=1)
    (got,), p = run(case, x, H.RED_SUM)
    b = sum_bound(case, p, mag, S)
    assert (2 * b < drop).all(), (case.id, "the bound cannot see one dropped input", float((2 * b / drop).max()))
    err = np.abs(as64(got, code) - S)
    assert (err <= b).all(), (case.id, p, float((err / b).max()))
    (got,), _ = run(case, x, H.RED_MEAN)
    bm = sum_bound(case, p, mag, S, mean=True)
    assert (2 * bm < drop / n).all(), (case.id, "the mean bound cannot see one dropped input")
    err = np.abs(as64(got, code) - S / n)
    assert (err <= bm).all(), (case.id, "mean", float((err / bm).max()))


def test_random_cases_cover_every_f32_and_f64_kernel():
    for code in (H.F32, H.F64):
        have = {(k.kernel, k.packed) for k in RANDOM_CASES if k.code == code}
        assert have == {(k.kernel, k.packed) for k in SUM_CASES if k.code == code}, NAME[code]


# ---- c. moments ----------------------------------------------------------------------------------------------------------------
MODES = ((H.MOM_VAR, 1.0), (H.MOM_VAR, 0.0), (H.MOM_STD, 1.0), (H.MOM_STD, 0.0), (H.MOM_INVSTD, 0.0), (H.MOM_INVSTD, 1.0))


def row_groups(p):
    """Group id of each reduced element (row-major over the reduced dims) for the units the plan folds separately: a lane's packs
    within a split (inner), a row group within a split (outer: rows r0 + g, r0 + g + 4, ...), one of 16 row groups (tall), or each
    element (generic)."""
    n = p["rtot"]
    r = np.arange(n)
    k = p["kernel"].split("+")[0]
    if k == "inner":
        vec, tx, ns = p["vec"], p["tx"], p["nsplit"]
        chunk = -(-(n // vec) // ns) * vec if vec > 1 else -(-n // ns)
        s = r // chunk
        return s * tx + ((r - s * chunk) // vec) % tx
    if k == "outer":
        chunk = -(-n // p["nsplit"])
        s = r // chunk
        return s * 4 + (r - s * chunk) % 4
    if k == "outer_tall":
        return r % 16
    return r


def drop_changes(x64, gid, correction):
    """|change| of the mean and of the variance when each row group is left out: [nout, ngroups] each (float64, centred)."""
    n = x64.shape[1]
    m = x64.mean(axis=1, keepdims=True)
    xc = x64 - m
    G = gid.max() + 1
    onehot = np.zeros((n, G))
    onehot[np.arange(n), gid] = 1.0
    cnt = onehot.sum(axis=0)
    s1, s2 = xc @ onehot, (xc * xc) @ onehot
    tot2 = (xc * xc).sum(axis=1, keepdims=True)
    n2 = n - cnt
    ok = n2 > correction
    mean2 = -s1 / np.where(n2 > 0, n2, 1)                       # (centred) mean without the group
    m2 = (tot2 - s2) - n2 * mean2 * mean2
    var = tot2 / (n - correction)
    var2 = m2 / np.where(ok, n2 - correction, 1)
    return np.abs(mean2), np.where(ok, np.abs(var2 - var), np.inf)


def mom_bounds(case, p, x64, correction):
    """Bounds on the mean and the variance from f32 (f64) Chan updates over d levels: the mean moves by at most 2 (d + 4) u max|x|
    (eps_m); M2 gathers relative error (3d + 6) u on its non-negative terms plus 4 eps_m |delta| n_a n_b / n per merge, which sums to
    at most 4 eps_m sqrt((d + 4) n M2) (Cauchy-Schwarz). Both doubled, plus half an ulp of the output."""
    u = U[case.code]
    d = depth(p, moments=True)
    n = x64.shape[1]
    m = x64.mean(axis=1)
    var = ((x64 - m[:, None]) ** 2).sum(axis=1) / max(n - correction, 1e-300)
    eps_m = 2 * (d + 4) * u * np.abs(x64).max(axis=1)
    bv = 2 * ((3 * d + 6) * u * var + 4 * eps_m * np.sqrt((d + 4) * var * n / max(n - correction, 1e-300)))
    return m, var, eps_m, bv


def group_data(rng, p, nout, n):
    """Every row group of the plan centred on its own value +-1, +-2 or +-3 (half of them negative) with +-0.1 of noise: leaving any
    one group out moves the mean by at least about n_group / n."""
    gid = row_groups(p)
    G = int(gid.max()) + 1
    v = (1 + rng.integers(0, 3, G)) * np.where(rng.permutation(G) % 2 == 0, 1.0, -1.0)
    return v[gid][None, :] + rng.uniform(-0.1, 0.1, (nout, n))


def trend_data(rng, case, nout, n, offset=0.0, spread=1.0):
    r = np.arange(n)
    return offset + spread * (4.0 * r / n + ((r % 64) - 31.5) / 8.0 + rng.uniform(-1, 1, (nout, n)))


@pytest.mark.parametrize("case", MOM_CASES, ids=lambda k: k.id)
def test_moments_every_mode_against_two_pass_float64(case):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 2)
    code, oc = case.code, case.out_code
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    p = case.plan()
    vals = store(group_data(rng, p, nout, n), code)
    x64 = as64(vals, code)
    x = upload(case, vals)
    for mode, corr in MODES:
        (gv, gm), p = run(case, x, mode=mode, correction=corr, eps=1e-5 if mode == H.MOM_INVSTD else 0.0)
        gv, gm = as64(gv, oc), as64(gm, oc)
        m, var, eps_m, bv = mom_bounds(case, p, x64, corr)
        bm = eps_m + half_ulp(m, oc)
        assert (np.abs(gm - m) <= bm).all(), (case.id, mode, corr, "mean", float((np.abs(gm - m) / bm).max()))
        if mode == H.MOM_VAR:
            want, b = var, bv + half_ulp(var, oc)
            dm, dv = drop_changes(x64, row_groups(p), corr)
            seen = (dm > 2 * bm[:, None]) | (dv > 2 * b[:, None])
            assert seen.all(), (case.id, corr, "a dropped row group could hide inside the bounds")
        elif mode == H.MOM_STD:
            want = np.sqrt(var)
            b = bv / (2 * want) + 2 * U[code] * want + half_ulp(want, oc)
        else:
            vb = var * (n - corr) / n
            want = 1 / np.sqrt(vb + 1e-5)
            bvb = bv * (n - corr) / n
            b = want * (0.5 * bvb / (vb + 1e-5) + 3 * U[code]) + half_ulp(want, oc)
        assert (np.abs(gv - want) <= b).all(), (case.id, mode, corr, float((np.abs(gv - want) / b).max()))


@pytest.mark.parametrize("case", MOM_CASES, ids=lambda k: k.id)
def test_moments_of_constant_rows_are_exact(case):
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    c = (np.arange(nout) % 13 - 6) * 0.375
    vals = store(np.repeat(c[:, None], n, axis=1), case.code)
    x = upload(case, vals)
    for mode in (H.MOM_VAR, H.MOM_STD):
        (gv, gm), p = run(case, x, mode=mode, correction=1.0)
        assert np.array_equal(as64(gm, case.out_code), c), (case.id, p)
        assert not as64(gv, case.out_code).any(), (case.id, mode)


@pytest.mark.parametrize("case", [k for k in MOM_CASES if k.code in (H.F32, H.F64)], ids=lambda k: k.id)
def test_moments_large_offset_every_path(case):
    """Mean 1e4, spread about 0.7: Chan's updates keep the variance to 1e-2 relative in f32 (ulp(1e4) is 1e-3 against the spread),
    where a sum-of-squares formula is off by O(10); the mean within mom_bounds' eps_m. The generic kernel is one lane walking all
    480 elements, each update rounding the running mean by up to u * 1e4: 4e-2 there (a float32 emulation of its chain on this
    input: 0.67 %)."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()) + 3)
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    vals = store(1e4 + 0.25 * trend_data(rng, case, nout, n), case.code)
    x64 = as64(vals, case.code)
    x = upload(case, vals)
    (gv, gm), p = run(case, x, mode=H.MOM_VAR, correction=1.0)
    m, var, eps_m, _ = mom_bounds(case, p, x64, 1.0)
    rel = (4e-2 if case.kernel == "generic" else 1e-2) if case.code == H.F32 else 1e-9
    assert (np.abs(gm - m) <= eps_m).all(), (case.id, float((np.abs(gm - m) / eps_m).max()))
    assert (np.abs(gv - var) <= rel * var).all(), (case.id, p, float((np.abs(gv - var) / var).max()))


# ---- e. the workspace contract on every split path ---------------------------------------------------------------------------
SPLIT_CASES = [k for k in SUM_CASES + MOM_CASES if k.kernel.endswith("+fold") and k.code in (H.F32, H.F64, H.BF16, H.I32, H.BOOL)]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda k: k.id)
def test_workspace_contract(case):
    rng = np.random.default_rng(5)
    nout = int(np.prod(case.out_shape))
    n = int(np.prod([case.shape[i] for i in case.dims]))
    vals = store(trend_data(rng, case, nout, n) if case.code in FLOATS else small_ints(rng, nout, n), case.code)
    x = upload(case, vals)
    mom = case.op == "mom"
    outs = [Dev.empty(case.out_shape, case.out_code) for _ in range(2 if mom else 1)]
    inp, views = case.views(x.view.ptr - case.offset * H.DTYPE_SIZE[case.code], [o.buf.ptr for o in outs])
    d = multi_reduce_desc(views[0], inp, case.dims, moments_out1=views[1] if mom else None)
    need = C.c_size_t(0)
    H.check((H.lib().kf_reduce_moments_workspace_bytes if mom else H.lib().kf_reduce_workspace_bytes)(C.byref(d), C.byref(need)))
    assert need.value == plan_of(d, mom)["ws"] > 0

    def call(ws, nbytes):
        if mom:
            return H.lib().kf_reduce_moments(H.MOM_VAR, C.byref(d), 1.0, 0.0, ws, nbytes, None)
        return H.lib().kf_reduce(H.RED_MEAN, C.byref(d), ws, nbytes, None)

    def result(ws_bytes, fill):
        for o in outs:
            o.buf.zero()
        ws = H.DevBuf(ws_bytes)
        if fill == 0xFF:
            H.check(H.lib().kf_memcpy_h2d(ws.ptr, np.full(ws_bytes, 0xFF, np.uint8).ctypes.data, ws_bytes, None))
        else:
            ws.zero()
        H.check(call(ws.ptr, ws_bytes))
        H.device_sync()
        return [o.get().tobytes() for o in outs]

    ref = result(need.value, 0)
    assert result(need.value, 0) == ref                  # run to run: the same bits
    assert result(need.value, 0xFF) == ref               # a workspace of NaNs is overwritten before it is read
    assert result(need.value + 4096, 0xFF) == ref        # a larger one: the same
    short = H.DevBuf(need.value - 1)
    assert call(short.ptr, need.value - 1) == H.KF_ERR_WORKSPACE
    assert call(None, 0) == H.KF_ERR_WORKSPACE


# ---- f. through the operator API ----------------------------------------------------------------------------------------------
def _api_tensor(a, code):
    return kfunca.from_numpy_bf16(a, 0) if code == H.BF16 else kfunca.from_numpy(a, 0)


def _api_values(t, code):
    return as64(t.numpy(), code)


def _labels(fn):
    H.profile_reset()
    H.profile_enable(True)
    try:
        out = fn()
        kfunca.synchronize()
    finally:
        H.profile_enable(False)
    return out, set(H.profile_results())


API_VIEWS = [  # (name, base shape, make the view from the base tensor, the same view of a numpy array, dim, expected path)
    ("contiguous-rows", (64, 4096), lambda t: t, lambda a: a, 1, "inner"),
    ("contiguous-cols", (4096, 64), lambda t: t, lambda a: a, 0, "outer"),
    ("permuted", (24, 40, 36), lambda t: t.permute(2, 0, 1), lambda a: a.transpose(2, 0, 1), 1, "generic"),
    ("permuted-inner", (36, 40), lambda t: t.permute(1, 0), lambda a: a.transpose(1, 0), 0, "inner"),
    ("sliced-rows", (64, 4097), lambda t: t[:, 1:], lambda a: a[:, 1:], 1, "inner"),
    ("sliced-cols", (300, 130), lambda t: t[:, 1:129], lambda a: a[:, 1:129], 0, "outer"),
    ("strided", (64, 4096), lambda t: t[::2, ::2], lambda a: a[::2, ::2], 1, "generic"),
]


@pytest.mark.parametrize("code", [H.F32, H.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("view", API_VIEWS, ids=[v[0] for v in API_VIEWS])
def test_operator_api_labels_and_values(view, code):
    name, shape, tview, aview, dim, path = view
    rng = np.random.default_rng(9)
    ints = small_ints(rng, int(np.prod(shape[:-1])), shape[-1]).reshape(shape)
    base = store(ints, code)
    t = tview(_api_tensor(base, code))
    a = aview(ints)
    S = a.sum(axis=dim, keepdims=True)
    n = a.shape[dim]
    s, lab = _labels(lambda: t.sum(dim))
    assert lab == {f"reduce_{path}"}, (name, lab)
    assert np.array_equal(s.numpy().view(np.uint8), np.ascontiguousarray(store(S, code)).view(np.uint8)), name
    mean, lab = _labels(lambda: t.mean(dim))
    assert lab == {f"reduce_{path}"}, (name, lab)
    f = np.float32(np.float32(S.size) / np.float32(a.size))
    want = np.ascontiguousarray(store((S.astype(np.float32) * f).astype(np.float64), code))
    assert np.array_equal(mean.numpy().view(np.uint8), want.view(np.uint8)), name
    # the statistics: the same bits as kf_reduce_moments on the same view through the C ABI, within the two-pass bounds
    xv = as64(store(a, code), code)
    (m, v), lab = _labels(lambda: t.mean_var(dim, False))
    assert lab == {f"moments_{path}"}, (name, lab)
    (m2, inv), lab = _labels(lambda: t.norm_stat(dim))
    assert lab == {f"moments_{path}"}, (name, lab)
    rows = np.moveaxis(xv, dim, -1).reshape(-1, n)
    wm = rows.mean(axis=1)
    wv = rows.var(axis=1, ddof=1)
    tol = 2.0 ** -7 if code == H.BF16 else 1e-5
    got_m = np.moveaxis(_api_values(m, code), dim, -1).reshape(-1)
    got_v = np.moveaxis(_api_values(v, code), dim, -1).reshape(-1)
    assert np.allclose(got_m, wm, rtol=tol, atol=tol * 4) and np.allclose(got_v, wv, rtol=tol * 4, atol=0), name
    got_m2 = np.moveaxis(m2.numpy().astype(np.float64), dim, -1).reshape(-1)
    got_inv = np.moveaxis(inv.numpy().astype(np.float64), dim, -1).reshape(-1)
    assert np.allclose(got_m2, wm, rtol=1e-5, atol=1e-5)
    assert np.allclose(got_inv, 1 / np.sqrt(rows.var(axis=1) + 1e-12), rtol=1e-4, atol=0), name


# ---- g. offsets near 2^31 bytes -----------------------------------------------------------------------------------------------
@pytest.mark.slow
def test_two_gib_input_inner_and_outer():
    """[512, 2^20] f32 is exactly 2^31 bytes, the largest input of that shape the iterator accepts: exact integer sums on the inner
    and the outer path (a wrapped 32-bit offset reads the wrong rows or faults - checked with the bounds already: every offset stays
    inside the buffer). One more row is refused by the operator API with its message."""
    rows, R = 512, 1 << 20
    x = np.empty((rows, R), dtype=np.float32)
    col = np.arange(R, dtype=np.int64)
    for i in range(rows):
        x[i] = ((col * 5 + i * 3) % 7 - 3).astype(np.float32)
    t = kfunca.from_numpy(x, 0)
    got = t.sum(1).numpy().reshape(-1)
    want = np.array([(((col * 5 + i * 3) % 7) - 3).sum() for i in range(rows)], dtype=np.float64)
    assert np.array_equal(got.astype(np.float64), want)
    got0 = t.sum(0).numpy().reshape(-1)
    want0 = np.zeros(R, dtype=np.int64)
    for i in range(rows):
        want0 += (col * 5 + i * 3) % 7 - 3
    assert np.array_equal(got0.astype(np.int64), want0)
    del t
    big = kfunca.empty([rows + 1, R], kfunca.float, 0)
    for dim in (0, 1):
        with pytest.raises(Exception, match="more than 2\\^31 bytes"):
            big.sum(dim)
