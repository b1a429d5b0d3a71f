"""-m gpu: kf_elementwise on the full value domain - every f16 / bf16 bit pattern, the exhaustive f32 rounding-boundary sets of both
narrowing conversions, infinities, NaNs, signed zeros and subnormals in arithmetic, integer operands whose sums and products wrap and
int64 quotients above 2^32 - through every geometry that selects another kernel in launch_same / launch_cast / the KF_EW_COPY branch.

Expected values come from tests/value_domain.py: the oracle and a numpy restatement, held to each other on every vector
(tests/test_value_domain_reference.py proves the same on any CPU). The rule: bit for bit wherever the expected value is not a NaN; where it
is, the result is a NaN - for a bf16 result exactly 0x7FC0; same-dtype copies are exact bits. Excluded inputs: integer x / 0 and MIN / -1
(undefined in the reference; removed by rule on the inputs) and float -> integer conversion (never fed).

Each geometry names the dispatch branch it is built for; check_desc asserts that branch's conditions on the kf_iter_desc of every launch.
Run with -s to see the count of compared elements per dtype and geometry."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import value_domain as V
from oracle import oracle as O
from tests.gpu_util import Dev, gpu_fill

pytestmark = pytest.mark.gpu
HOP = {"add": H.EW_ADD, "sub": H.EW_SUB, "mul": H.EW_MUL, "div": H.EW_DIV}
SOP = {"add": H.EW_ADD_SCALAR, "sub": H.EW_SUB_SCALAR, "mul": H.EW_MUL_SCALAR, "div": H.EW_DIV_SCALAR}
TALLY = {}   # (what, geometry) -> [elements compared, NaNs in the expected arrays, elements compared by NaN-ness only]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\n%-34s %-14s %12s %10s %10s" % ("vectors", "geometry", "compared", "exp. NaN", "NaN-only"))
    tot = [0, 0, 0]
    for (what, geom), t in sorted(TALLY.items()):
        print("%-34s %-14s %12d %10d %10d" % (what, geom, *t))
        tot = [x + y for x, y in zip(tot, t)]
    print("%-34s %-14s %12d %10d %10d" % ("total", "", *tot))
    print("(a bf16 result that is expected to be a NaN is compared bit for bit against 0x7FC0: it counts as a NaN, not as NaN-only)")


def up(n, m):
    return -(-n // m) * m


def vmax(code):
    return 16 // V.esize(code)


# ---- placing a logical array in device memory ----------------------------------------------------------------------------------
def contig(x, code):
    return Dev(np.ascontiguousarray(x), code)


def rows_view(x, code, skip):
    """x [R, C] as the first C columns of an [R, C + skip] base (the rest holds the pad value): dim 0 contiguous, rows do not collapse."""
    r, c = x.shape
    base = np.full((r, c + skip), V.one(code)[0], dtype=x.dtype)
    base[:, :c] = x
    return Dev(base[:, :c], code, base=base)


def stride2_view(x, code):
    """x [R, C] as every other column of an [R, 2C] base: the stride of dim 0 is two elements."""
    r, c = x.shape
    base = np.full((r, 2 * c), V.one(code)[0], dtype=x.dtype)
    base[:, ::2] = x
    return Dev(base[:, ::2], code, base=base)


def transposed_view(x, code):
    """x [R, C] stored as its transpose [C, R]: along the output's contiguous dim this operand strides by a whole row."""
    base = np.ascontiguousarray(x.T)
    return Dev(base.T, code, base=base)


def offset16_view(x, code):
    """x (1-D) starting 16 bytes into its base: 16-byte but not 32-byte aligned."""
    k = 16 // V.esize(code)
    base = np.concatenate([np.full(k, V.one(code)[0], dtype=x.dtype), x])
    d = Dev(base[k:], code, base=base)
    assert d.view.ptr % 32 == 16
    return d


def as_rows(idx, cols, pad, min_rows=1, row_mult=1):
    rows = up(max(min_rows, -(-idx.size // cols)), row_mult)
    return V.fit(idx, rows * cols, pad).reshape(rows, cols)


# ---- launching: every descriptor is checked against the branch its geometry is built for ------------------------------------------------
def check_desc(name, d):
    """The conditions of the dispatch branch (launch_same / launch_cast / the KF_EW_COPY branch of kf_elementwise) that the geometry `name` is
    built for, asserted on the kf_iter_desc that goes to kf_elementwise - after make_desc has dropped size-1 dims and merged what collapses."""
    nt, nd = d.ntensors, d.ndim
    es = [H.DTYPE_SIZE[d.dtype[t]] for t in range(nt)]
    s0 = [d.stride_bytes[t][0] for t in range(nt)]
    ptr = [d.data[t] for t in range(nt)]
    numel = int(np.prod([d.shape[i] for i in range(nd)]))
    vm = 16 // max(es)
    if name in ("contig16", "contig_odd", "cast8", "cast_ragged", "aligned32", "offset16", "ragged"):
        assert nd == 1 and s0 == es, (name, nd, s0)   # desc_contiguous()
        if name == "contig16":
            assert numel % vm == 0
        if name in ("contig_odd", "cast_ragged", "ragged"):
            assert numel % 2 == 1
        if name in ("cast8", "aligned32", "offset16"):
            assert numel % 8 == 0 and all(p % 16 == 0 for p in ptr)
        if name == "aligned32":
            assert all(p % 32 == 0 for p in ptr)
        if name == "offset16":
            assert any(p % 32 == 16 for p in ptr)
    elif name in ("rows16", "cast_rows", "rows"):
        assert nd >= 2 and s0 == es, (name, nd, s0)   # not contiguous; dim 0 contiguous in every operand
        assert name != "rows16" or d.shape[0] % vm == 0
    elif name == "stride2":
        # (the rows of an every-other-column view merge into one dim of stride 2: still not desc_contiguous, and pick_vec finds no pack)
        assert numel > 1 and s0[0] == es[0] and all(s0[t] == 2 * es[t] for t in range(1, nt)), (name, nd, s0)
    elif name == "bcast0":
        assert nd == 2 and s0[0] == es[0] and sorted(s0[1:]) == [0, es[1]] and d.shape[0] % vm == 0, (name, nd, s0)
    elif name == "transposed":   # the conditions in front of ew_transpose_binary_kernel
        tt = [t for t in (1, 2) if s0[t] != es[t]]
        assert nd == 2 and s0[0] == es[0] and len(tt) == 1, (name, nd, s0)
        t = tt[0]
        assert d.stride_bytes[t][1] == es[t] and s0[t] > 0 and s0[t] % 16 == 0
        assert all(d.stride_bytes[u][1] > 0 and d.stride_bytes[u][1] % 16 == 0 for u in (0, 3 - t)) and all(p % 16 == 0 for p in ptr)
        assert d.shape[0] % 64 == 0 and d.shape[1] % 64 == 0 and (d.shape[0] // 64) * (d.shape[1] // 64) >= 64
    elif name in ("copy_transposed", "copy_transposed_ragged"):   # the conditions in front of the tiled transpose copy
        assert nd == 2 and s0[0] == es[0] and s0[1] != es[1] and d.stride_bytes[1][1] == es[1] and d.shape[0] >= 16 and d.shape[1] >= 16
        whole = d.shape[0] % 64 == 0 and d.shape[1] % 64 == 0
        assert whole == (name == "copy_transposed")
    else:
        raise AssertionError(name)


def launch(op, name, out, ins, compute=0, scalar=0.0):
    d = H.make_desc([out.view], [x.view for x in ins])
    check_desc(name, d)
    H.elementwise(op, d, compute, scalar)
    H.device_sync()
    return out.get()


# ---- geometries of a two-operand launch: (ia, ib) flat index vectors -> logical index arrays + a placement per operand ---------------
# Each entry: name, shape(ia, ib, pad of a, pad of b) -> (ia, ib), place_a, place_b.
def g_flat(mult_of, odd=False):
    def shape(ia, ib, pa, pb):
        n = up(ia.size, mult_of)
        n += odd and n % 2 == 0
        return V.fit(ia, n, pa), V.fit(ib, n, pb)
    return shape


def g_rows(cols, min_rows=2, row_mult=1):   # (at least two rows: a single row collapses to a contiguous descriptor)
    def shape(ia, ib, pa, pb):
        return as_rows(ia, cols, pa, min_rows, row_mult), as_rows(ib, cols, pb, min_rows, row_mult)
    return shape


SAME_GEOMS = [
    # launch_same, desc_contiguous, numel % (16 / esize) == 0: ew_same_kernel<T, VMAX, .., CONTIG = true>
    ("contig16", g_flat(16), contig, contig),
    # launch_same, desc_contiguous, odd numel: ew_same_kernel<T, 1, .., CONTIG = true>
    ("contig_odd", g_flat(1, odd=True), contig, contig),
    # not contiguous (two dims that do not collapse), dim 0 contiguous in every operand, 256 % VMAX == 0: pick_vec -> VMAX,
    # ew_same_kernel<T, VMAX, .., CONTIG = false> (the 16-byte strided kernel)
    ("rows16", g_rows(256), lambda x, c: rows_view(x, c, vmax(c)), lambda x, c: rows_view(x, c, 2 * vmax(c))),
    # dim-0 stride of both inputs is two elements: pick_vec -> 1, ew_same_kernel<T, 1, .., CONTIG = false> (the scalar strided kernel)
    ("stride2", g_rows(256), stride2_view, stride2_view),
]
# one input transposed against the output, both extents whole 64-tiles, at least 64 tiles (512 x 512 and up), 16-byte aligned rows:
# ew_transpose_binary_kernel<T> (2- and 4-byte types); the swapped run makes the transposed operand the FIRST input (t_first)
TRANSPOSED = ("transposed", g_rows(512, min_rows=512, row_mult=64), contig, transposed_view)
CAST_GEOMS = [
    # launch_cast, desc_contiguous, numel % 8 == 0, every pointer 16-byte aligned: ew_cast8_kernel
    ("cast8", g_flat(16), contig, contig),
    # launch_cast, contiguous but an odd numel: ew_cast_kernel (one element per lane through the offset calculator)
    ("cast_ragged", g_flat(1, odd=True), contig, contig),
    # launch_cast, two dims that do not collapse: ew_cast_kernel
    ("cast_rows", g_rows(250), lambda x, c: rows_view(x, c, 1), lambda x, c: rows_view(x, c, 3)),
]


def sanitize(ia, ib, defined, pad_a):
    """The rule on the inputs: where a (op) b is undefined (integer MIN / -1; zero divisors never enter the vectors), a becomes the pad value 1."""
    ia = ia.copy()
    ia[~defined[ib, ia]] = pad_a
    assert defined[ib, ia].all()
    return ia


def run_binary(label, ca, avals, cb, bvals, ops, geoms, bcast=False):
    common = V.np_promote(ca, cb)
    assert O.promote(ca, cb) == common
    lanes = V.lanes_of(ca, cb)
    for op in ops:
        for swap in (False, True):   # swap: b (op) a, b as the first input
            av, bv = avals, bvals
            if op == "div" and common in V.INTS:   # the divisor's vector loses its zero
                av, bv = (av[av != 0], bv) if swap else (av, bv[bv != 0])
            a, b = V.with_pad(av, ca), V.with_pad(bv, cb)
            want, defined = V.expected_binary(op, a, ca, b, cb, swap)
            fa, fb = V.flat_pairs(av.size, bv.size, lanes)
            layouts = [(name, *shape(fa, fb, av.size, bv.size), pa, pb) for name, shape, pa, pb in geoms]
            if bcast:
                # as rows16, but the b operand is ONE value per row, stride 0 along dim 0 (an input: allowed by pick_vec): the 16-byte strided
                # kernel with the bcast0 bit of that operand set (a scalar load splat over the pack)
                layouts.append(("bcast0", *V.row_pairs(av.size, bv.size, lanes, vmax(ca)), contig, lambda x, c: contig(x[:, :1], c)))
            for name, ia, ib, place_a, place_b in layouts:
                ia = sanitize(ia, ib, defined, av.size)
                da, db = place_a(a[ia], ca), place_b(b[ib], cb)
                got = launch(HOP[op], name, Dev.empty(ia.shape, common), [db, da] if swap else [da, db], common)
                V.assert_match(got, want[ib, ia], common, (label, op, "b op a" if swap else "a op b", name), tally=TALLY, key=(label, name))


# ---- same-dtype arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", V.SAME_DTYPE_KERNEL, ids=lambda c: V.NAME[c])
def test_arithmetic_same_dtype(code):
    """launch_same<T, 2, 0>: f16 / bf16 every pattern against 8 partners, f32 / f64 / i32 / i64 the cross product of the specials, all four
    operators, both operand orders, every kernel of the same-dtype dispatch."""
    avals, bvals = V.operand_vectors(code)
    geoms = SAME_GEOMS + ([TRANSPOSED] if V.esize(code) in (2, 4) else [])
    run_binary(V.NAME[code] + " arith", code, avals, code, bvals, list(V.OPS), geoms, bcast=True)


@pytest.mark.parametrize("code", [V.U8, V.I8, V.I16], ids=lambda c: V.NAME[c])
def test_arithmetic_small_integers(code):
    """u8 / i8 / i16 have no same-dtype kernel: kf_elementwise sends them to launch_cast<int64_t> - int64 accumulator, truncation on store.
    The full 256-value domain of the one-byte types against the extremes; the i16 extremes against themselves."""
    avals, bvals = V.operand_vectors(code)
    run_binary(V.NAME[code] + " arith", code, avals, code, bvals, list(V.OPS), CAST_GEOMS)


def test_arithmetic_mixed_dtypes():
    """launch_cast<A>: operands of two dtypes, converted on load to the accumulate type of the common dtype, converted on store."""
    for ca, avals, cb, bvals in V.mixed_pairs():
        run_binary(f"{V.NAME[ca]} x {V.NAME[cb]} arith", ca, avals, cb, bvals, ["add", "sub", "mul"], CAST_GEOMS)


# ---- scalar forms ------------------------------------------------------------------------------------------------------------
SINGLE_GEOMS = [   # the launch_same branches of SAME_GEOMS with one input (MODE 3: scalar right operand; MODE 1: copy)
    ("contig16", lambda i, p: V.fit(i, up(i.size, 16), p), contig),
    ("contig_odd", lambda i, p: V.fit(i, i.size + (i.size % 2 == 0), p), contig),
    ("rows16", lambda i, p: as_rows(i, 256, p, 2), lambda x, c: rows_view(x, c, vmax(c))),
    ("stride2", lambda i, p: as_rows(i, 256, p, 2), stride2_view),
]


def run_scalar(label, code, a, want_row, defined_row, s, op):
    """One scalar against the whole vector, `lanes` copies of it, each one lane further: every (value, scalar) pair visits every lane."""
    n_vals = a.size - 1
    base = V.flat_single(n_vals, V.lanes_of(code))
    for name, shape, place in SINGLE_GEOMS:
        ia = shape(base, n_vals).copy()
        ia[~defined_row[ia]] = n_vals
        got = launch(SOP[op], name, Dev.empty(ia.shape, code), [place(a[ia], code)], 0, s)
        V.assert_match(got, want_row[ia], code, (label, op, s, name), tally=TALLY, key=(label, name))


@pytest.mark.parametrize("code", V.SAME_DTYPE_KERNEL, ids=lambda c: V.NAME[c])
def test_scalar_forms(code):
    """KF_EW_*_SCALAR (launch_same<T, 1, 3>): the vectors of the same-dtype test with each b value handed over as the scalar (those a double
    holds exactly), plus, for the float types, the special scalars of the fill test - expected: fill a tensor with the scalar, then the
    binary operator."""
    avals, bvals = V.operand_vectors(code)
    a, b = V.with_pad(avals, code), V.with_pad(bvals, code)
    for op in V.OPS:
        want, defined = V.expected_binary(op, a, code, b, code)
        for k in range(bvals.size):
            s = V.scalar_of(bvals, code, k)
            if s is None or (op == "div" and code in V.INTS and s == 0):
                continue
            run_scalar(V.NAME[code] + " scalar", code, a, want[k], defined[k], s, op)
        if code in V.FLOATS:
            for s in V.fill_scalars():
                filled = np.concatenate([V.expected_fill(s, code), V.one(code)])
                want, defined = V.expected_binary(op, a, code, filled, code)
                run_scalar(V.NAME[code] + " scalar", code, a, want[0], defined[0], s, op)


# ---- convert and copy ----------------------------------------------------------------------------------------------------------
def test_convert_and_copy():
    """KF_EW_COPY. Between two of f32 / f16 / bf16: `aligned32` (contiguous, numel % 8 == 0, both pointers 32-byte aligned) is
    ew_convert8_kernel; `offset16` (the same data 16 bytes further) fails the 32-byte test and falls to launch_cast, whose conditions
    (contiguous, numel % 8 == 0, 16-byte aligned) it meets: ew_cast8_kernel; `ragged` (odd numel) and `rows` (two dims that do not collapse)
    are ew_cast_kernel. Any other pair of different dtypes: aligned32 and offset16 are both ew_cast8_kernel, the rest ew_cast_kernel.
    Same dtype: launch_raw_by_size -> launch_same<U, 1, 1>, the copy form of the kernels above - exact bits, NaN payloads included."""
    for src, vals, dsts in V.convert_cases():
        v = V.with_pad(vals, src)
        for dst in dsts:
            want = V.expected_convert(v, src, dst)
            idx = V.flat_single(vals.size, V.lanes_of(src, dst))
            n8 = up(idx.size, 16)
            geoms = [("aligned32", V.fit(idx, n8, vals.size), contig), ("offset16", V.fit(idx, n8, vals.size), offset16_view),
                     ("ragged", V.fit(idx, n8 + 1, vals.size), contig), ("rows", as_rows(idx, 250, vals.size, 2), lambda x, c: rows_view(x, c, 1))]
            label = f"{V.NAME[src]} -> {V.NAME[dst]}" if src != dst else f"{V.NAME[src]} copy"
            for name, ia, place in geoms:
                got = launch(H.EW_COPY, name, Dev.empty(ia.shape, dst), [place(v[ia], src)])
                V.assert_match(got, want[ia], dst, (label, name), exact=src == dst, tally=TALLY, key=(label, name))


def test_copy_strided_and_transposed_views_exact_bits():
    """Same-dtype copies, exact bits: all f16 patterns (NaN payloads of both signs), the f32 boundary vector with its NaNs and the f64
    specials out of a stride-2 view (the scalar strided copy) and out of a transposed view of whole 64-tiles (ew_transpose_vec_kernel for the
    2- and 4-byte types, ew_transpose_kernel for f64); a 70 x 130 transposed view (ragged tiles: ew_transpose_kernel for every width) gets
    a sample of the vector: every k-th value and its last 1000, which hold the negative NaNs of f16 and the NaN / inf / zero extras of f32."""
    for code, vals in ((V.F16, V.all_patterns16(V.F16)), (V.F32, V.f32_boundaries_bf16()), (V.F64, V.float_specials(V.F64))):
        v = V.with_pad(vals, code)
        idx = V.flat_single(vals.size, V.lanes_of(code))
        n = vals.size
        sample = np.unique(np.concatenate([np.arange(0, n, -(-n // 8000)), np.arange(max(0, n - 1000), n)]))
        assert sample.size <= 9100 and V.is_nan(v[sample], code).any() and np.isin(V.bits(v[sample]) >> (8 * V.esize(code) - 1), 1).any()
        for name, ia, place in (("stride2", as_rows(idx, 256, n, 2), stride2_view),
                                ("copy_transposed", as_rows(idx, 512, n, 512, 64), transposed_view),
                                ("copy_transposed_ragged", as_rows(sample, 130, n, 70), transposed_view)):
            assert name != "copy_transposed_ragged" or ia.shape == (70, 130)
            got = launch(H.EW_COPY, name, Dev.empty(ia.shape, code), [place(v[ia], code)])
            V.assert_match(got, v[ia], code, (V.NAME[code], "copy", name), exact=True, tally=TALLY, key=(V.NAME[code] + " copy", name))


# ---- fill ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", V.FLOATS, ids=lambda c: V.NAME[c])
def test_fill_special_scalars(code):
    """KF_EW_FILL: fill_pattern rounds the double on the HOST (host_f32_to_bf16 / host_f32_to_f16) - overflow to inf, ties, subnormals, NaN,
    -0.0 - then ew_same_kernel<U, VMAX or 1, 0, 2> writes the pattern: contiguous whole packs, ragged, and a strided view."""
    for s in V.fill_scalars():
        want = V.expected_fill(s, code)
        for shape in ((5,), (1024,), (3, 5, 7)):
            got = gpu_fill(Dev.empty(shape, code), s).get()
            V.assert_match(got, np.broadcast_to(want, got.size).reshape(shape).copy(), code, (V.NAME[code], "fill", s, shape), tally=TALLY,
                           key=(V.NAME[code] + " fill", "contig"))
        base = np.full((6, 10), V.one(code)[0], dtype=V.NP[code])
        d = Dev(base[1:5:2, 2:9:3], code, base=base)
        gpu_fill(d, s)
        host = d.buf.to_numpy(base.shape, base.dtype)
        expect = base.copy()
        expect[1:5:2, 2:9:3] = want[0]
        V.assert_match(host, expect, code, (V.NAME[code], "fill", s, "strided"), tally=TALLY, key=(V.NAME[code] + " fill", "strided"))
