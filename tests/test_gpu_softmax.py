"""-m gpu: row softmax and log_softmax (kf_softmax_fwd, kf_softmax_bwd, kfunca.softmax / log_softmax) against the f64 reference of
tests/softmax_ref.py on the stored values, against torch-CPU for the special values and the operator API, bit for bit where the ABI
promises it (aliases, the element path, repeated runs, graph replay, neighbouring rows), and through an MoE router end to end.

The bounds are those of tests/softmax_ref.py (its docstring derives them; tests/test_softmax_ref.py shows on the CPU that they reject
wrong formulas on the draws used here). The backward is always fed the STORED result of the device's own forward.

No comparison here leaves elements out: every reference value of the accuracy tests is finite (asserted), so the share of masked elements
is 0, under the 1 % the project allows. The special-value test is the exception by design: there the non-finite pattern itself is compared
exactly, and the finite elements are held to the bounds.

Every buffer has guard elements of random bits in front, behind and, where ld > V, between the rows; they are compared bit for bit
after every call.
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import softmax_ref as R
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

SM, LSM = R.SOFTMAX, R.LOG_SOFTMAX
T1, T2 = R.thresholds()
GUARD = 64          # elements before and after every buffer: 128 or 256 bytes, so the base stays 16-byte aligned
WORST = {}          # (kind, direction, dtype) -> the largest fraction of the bound met in this run (printed by the last test)


class Buf:
    """rows x V elements at leading dimension ld, `off` elements past a 16-byte boundary, random bits everywhere else."""

    def __init__(self, rng, code, rows, V, ld=None, off=0):
        self.code, self.rows, self.V, self.ld = code, rows, V, V if ld is None else ld
        self.base = GUARD + off
        n = self.base + max(rows - 1, 0) * self.ld + V + GUARD
        self.host = rng.integers(0, 1 << (8 * R.ES[code]), n, dtype=np.uint64).astype(R.UINT[code])
        self.dev = None

    def idx(self):
        return self.base + np.arange(self.rows)[:, None] * self.ld + np.arange(self.V)[None, :]

    def put(self, b):
        self.host[self.idx()] = b
        return self

    def up(self):
        self.dev = H.DevBuf.from_numpy(self.host)
        return self

    def ptr(self):
        return self.dev.ptr + self.base * R.ES[self.code]

    def get(self):
        """The [rows, V] block; everything outside it must hold its old bits."""
        after = self.dev.to_numpy(self.host.shape, R.UINT[self.code])
        mask = np.ones(after.shape, bool)
        mask[self.idx()] = False
        assert np.array_equal(after[mask], self.host[mask]), "bytes outside the output were written"
        return after[self.idx()]


def labels_of(call):
    H.profile_reset()
    H.profile_enable(True)
    try:
        out = call()
        H.device_sync()
        return out, set(H.profile_results())
    finally:
        H.profile_enable(False)


def fwd(code, kind, x, scale=1.0, ld=None, off=None, inplace=False, seed=0):
    """kf_softmax_fwd on the bit patterns x [rows, V]; ld / off: {'x': .., 'y': ..} leading dimensions and base offsets in elements.
    Returns y's bits; asserts the guards and the profile label of the regime."""
    rng = np.random.default_rng(seed)
    rows, V = x.shape
    ld, off = ld or {}, off or {}
    X = Buf(rng, code, rows, V, ld.get("x"), off.get("x", 0)).put(x).up()
    Y = X if inplace else Buf(rng, code, rows, V, ld.get("y"), off.get("y", 0)).up()
    _, names = labels_of(lambda: H.softmax_fwd(kind, code, rows, V, scale, X.ptr(), X.ld, Y.ptr(), Y.ld))
    assert names == {f"softmax_fwd_{R.regime(V)}"}, (names, V)
    return Y.get()


def bwd(code, kind, y, dy, scale=1.0, ld=None, off=None, inplace=False, seed=0):
    """kf_softmax_bwd on the bit patterns y, dy; keys y, dy, dx. inplace: dx == dy. Returns dx's bits."""
    rng = np.random.default_rng(seed + 1)
    rows, V = y.shape
    ld, off = ld or {}, off or {}
    Yb = Buf(rng, code, rows, V, ld.get("y"), off.get("y", 0)).put(y).up()
    D = Buf(rng, code, rows, V, ld.get("dy"), off.get("dy", 0)).put(dy).up()
    DX = D if inplace else Buf(rng, code, rows, V, ld.get("dx"), off.get("dx", 0)).up()
    _, names = labels_of(lambda: H.softmax_bwd(kind, code, rows, V, scale, Yb.ptr(), Yb.ld, D.ptr(), D.ld, DX.ptr(), DX.ld))
    assert names == {f"softmax_bwd_{R.regime(V)}"}, (names, V)
    assert np.array_equal(Yb.get(), y), "the backward wrote to y"
    return DX.get()


def record(key, err, tol, what):
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    worst = float(frac.max()) if frac.size else 0.0
    print(f"{R.KIND_NAME[key[0]]} {key[1]} {R.CODE_NAME[key[2]]} {what}: fraction of the bound {worst:.3f}")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    bad = ~(err <= tol)
    assert not bad.any(), (key, what, int(bad.sum()), worst, np.argwhere(bad)[:3].tolist())


def check_fwd(code, kind, x, scale, y, what):
    ref, lse = R.forward(kind, R.floats(x, code), scale)
    assert np.isfinite(ref).all(), what   # nothing is left out of the comparison
    record((kind, "forward", code), np.abs(R.floats(y, code) - ref), R.forward_bound(kind, code, ref, lse), what)


def check_bwd(code, kind, y, dy, scale, dx, what):
    yf, df = R.floats(y, code), R.floats(dy, code)
    ref = R.backward(kind, yf, df, scale)
    assert np.isfinite(ref).all(), what
    record((kind, "backward", code), np.abs(R.floats(dx, code) - ref), R.backward_bound(kind, code, yf, df, scale, ref), what)


def both(code, kind, x, dy, scale=1.0, what="", **kw):
    """Forward, then the backward from the forward's stored result; both checked. kw: per-direction layouts {'fwd': {...}, 'bwd': {...}}."""
    y = fwd(code, kind, x, scale, **kw.get("fwd", {}))
    check_fwd(code, kind, x, scale, y, what)
    dx = bwd(code, kind, y, dy, scale, **kw.get("bwd", {}))
    check_bwd(code, kind, y, dy, scale, dx, what)
    return y, dx


# ---- 1. regimes and edges -------------------------------------------------------------------------------------------------------------
EDGE_V = [1, 2, 7, 63, 64, 65, 1000, T1 - 1, T1, T1 + 1, T2, T2 + 1]
# 1031 rows: 258 blocks of four waves in the wave regime; 16387 rows of a short row: more blocks than the chip holds at once
EDGE_ROWS = [1, 3, 4, 5, 1031]


@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_regimes_and_edges(code, kind):
    shapes = [(rows, V) for V in EDGE_V for rows in (EDGE_ROWS if V <= T1 else [1, 3, 5])]
    shapes += [(16387, 65), (2, 50257)]
    for rows, V in shapes:
        rng = np.random.default_rng(rows * 131 + V)
        x, dy = R.draw_logits(rng, "normal", code, rows, V), R.draw_dy(rng, "normal", code, rows, V)
        kw = {}
        if V == 50257:   # the stream regime with an odd stride: every row at another phase, in all operands alike
            kw = {"fwd": {"ld": {"x": V + 2, "y": V + 2}}, "bwd": {"ld": {"y": V + 2, "dy": V + 2, "dx": V + 2}}}
        both(code, kind, x, dy, what=f"rows {rows} V {V}", **kw)
    assert {R.regime(V) for _, V in shapes} == {"wave", "block", "stream"}


# ---- 2. layouts -------------------------------------------------------------------------------------------------------------------------
LAYOUT_V = [1000, T1 + 1, T2 + 1]   # one per regime; 1000 takes the larger of the wave regime's two tiles


@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_padded_rows_and_every_base_phase(code, kind):
    for V in LAYOUT_V:
        rng = np.random.default_rng(V + kind)
        x, dy = R.draw_logits(rng, "normal", code, 3, V), R.draw_dy(rng, "normal", code, 3, V)
        for o in range(8):   # o elements past a 16-byte boundary (f32: the phases repeat after 4), rows padded by 24 elements
            ldv = V + 24
            both(code, kind, x, dy, what=f"V {V} base + {o}", fwd={"ld": {"x": ldv, "y": ldv}, "off": {"x": o, "y": o}},
                 bwd={"ld": {"y": ldv, "dy": ldv, "dx": ldv}, "off": {"y": o, "dy": o, "dx": o}})
        # contiguous odd V: every row has another phase; an odd leading dimension likewise
        for V2 in (V | 1, V + 2 - (V & 1)):
            x2, dy2 = R.draw_logits(rng, "normal", code, 5, V2), R.draw_dy(rng, "normal", code, 5, V2)
            both(code, kind, x2, dy2, what=f"contiguous V {V2}")
            both(code, kind, x2, dy2, what=f"V {V2} ld + 3", fwd={"ld": {"x": V2 + 3, "y": V2 + 3}},
                 bwd={"ld": {"y": V2 + 3, "dy": V2 + 3, "dx": V2 + 3}})


@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_element_path_equals_pack_path_bit_for_bit(code, kind):
    """The rows of the first operand (x; y in the backward) keep their place, so the combination order is the same; the other operands
    move to another phase within 16 bytes, by their base or by their leading dimension, which takes the element path."""
    for V in [7, 64] + LAYOUT_V:
        rng = np.random.default_rng(V + 3 * kind)
        x, dy = R.draw_logits(rng, "wide", code, 5, V), R.draw_dy(rng, "normal", code, 5, V)
        ldv = V + 24
        y0 = fwd(code, kind, x, 0.125, ld={"x": ldv, "y": ldv}, off={"x": 3, "y": 3})
        check_fwd(code, kind, x, 0.125, y0, f"V {V}")
        for ld, off in (({"x": ldv, "y": ldv}, {"x": 3, "y": 4}), ({"x": ldv, "y": ldv + 1}, {"x": 3, "y": 3}), ({"x": ldv, "y": V}, {"x": 3})):
            assert np.array_equal(fwd(code, kind, x, 0.125, ld=ld, off=off), y0), (V, ld, off)
        all3 = {"y": ldv, "dy": ldv, "dx": ldv}
        dx0 = bwd(code, kind, y0, dy, 0.125, ld=all3, off={"y": 3, "dy": 3, "dx": 3})
        check_bwd(code, kind, y0, dy, 0.125, dx0, f"V {V}")
        for ld, off in ((all3, {"y": 3, "dy": 2, "dx": 3}), (all3, {"y": 3, "dy": 3, "dx": 0}), ({"y": ldv, "dy": V, "dx": ldv + 3}, {"y": 3, "dy": 1})):
            assert np.array_equal(bwd(code, kind, y0, dy, 0.125, ld=ld, off=off), dx0), (V, ld, off)


# ---- 3. value draws ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_value_draws(code, kind):
    """N(0, 1), N(0, 6^2) and 1e4 + N(0, 3^2) logits (f32 softmax is held to its bound there too) at scale 1, 0.125 and 7.5; one huge
    gradient element, so that dy - sum cancels. The very draws tests/test_softmax_ref.py runs its wrong formulas on."""
    for rows, V in R.value_shapes():
        for logits, scale, dyk in R.value_cases():
            rng = np.random.default_rng(V + 7 * code)
            x, dy = R.draw_logits(rng, logits, code, rows, V), R.draw_dy(rng, dyk, code, rows, V)
            both(code, kind, x, dy, scale, what=f"V {V} {logits} logits, scale {scale}, {dyk} dy")


# ---- 4. special values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_special_values_follow_torch_and_stay_in_their_rows(code, kind):
    import torch
    tfn = torch.softmax if kind == SM else torch.log_softmax
    for V in (70, T1 + 1, T2 + 1):
        rng = np.random.default_rng(V)
        clean = R.floats(R.draw_logits(rng, "normal", code, 7, V), code)
        x = clean.copy()
        x[1, rng.integers(0, V, max(2, V // 3))] = -np.inf   # some -inf
        x[2, :] = -np.inf                                    # only -inf
        x[3, V // 2] = np.nan
        x[5, V - 1] = np.inf
        bad = [1, 2, 3, 5]
        xb, cb = R.bits(x, code), R.bits(clean, code)
        dy = R.draw_dy(rng, "normal", code, 7, V)
        y = fwd(code, kind, xb)
        yc = fwd(code, kind, cb)
        good = [r for r in range(7) if r not in bad]
        assert np.array_equal(y[good], yc[good]), "a bad row changed a neighbouring row"
        t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        ty = tfn(t, dim=-1)
        want = ty.detach().numpy()
        got = R.floats(y, code)
        for pat in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(pat(got), pat(want)), (V, pat.__name__)
        assert np.isnan(got[[2, 3, 5]]).all() and not np.isnan(got[[0, 1, 4, 6]]).any()
        minf = np.isneginf(x[1])
        assert (got[1, minf] == (0.0 if kind == SM else -np.inf)).all() and np.isfinite(got[1, ~minf]).all()
        ref, lse = R.forward(kind, x[[0, 1, 4, 6]], 1.0)
        fin = np.isfinite(ref)
        with np.errstate(invalid="ignore"):   # (-inf - -inf at the masked elements)
            err = np.abs(got[[0, 1, 4, 6]] - ref)
        assert (err[fin] <= np.broadcast_to(R.forward_bound(kind, code, ref, lse), ref.shape)[fin]).all()
        # the backward from the stored result, against torch's autograd on that result's values
        dxb, dxc = bwd(code, kind, y, dy), bwd(code, kind, yc, dy)
        assert np.array_equal(dxb[good], dxc[good]), "a bad row changed a neighbouring row's gradient"
        dx = R.floats(dxb, code)
        ref = R.backward(kind, got, R.floats(dy, code), 1.0)   # torch's formulas (tests/test_softmax_ref.py) on the stored y
        ty.backward(torch.tensor(R.floats(dy, code)))
        tg = t.grad.numpy()
        assert np.array_equal(np.isnan(ref), np.isnan(tg)) and np.array_equal(np.isnan(dx), np.isnan(tg)), V
        assert np.isfinite(dx[~np.isnan(tg)]).all()
        if kind == SM:
            assert (dx[1, minf] == 0.0).all()   # no gradient reaches a -inf logit
        fin = np.isfinite(ref)
        tol = R.backward_bound(kind, code, got, R.floats(dy, code), 1.0, ref)
        with np.errstate(invalid="ignore"):
            err = np.abs(dx - ref)
        assert (err[fin] <= tol[fin]).all()


# ---- 5. aliases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", R.CODES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_in_place_calls_equal_the_out_of_place_call(code, kind):
    for V, off in [(7, 0), (64, 0), (1000, 1)] + [(v, o) for v in LAYOUT_V[1:] for o in (0, 3)]:
        rng = np.random.default_rng(V + off)
        x, dy = R.draw_logits(rng, "wide", code, 5, V), R.draw_dy(rng, "normal", code, 5, V)
        ld = V + 5
        y = fwd(code, kind, x, 7.5, ld={"x": ld, "y": ld}, off={"x": off, "y": off})
        assert np.array_equal(fwd(code, kind, x, 7.5, ld={"x": ld}, off={"x": off}, inplace=True), y), (V, off)
        all3, o3 = {"y": ld, "dy": ld, "dx": ld}, {"y": off, "dy": off, "dx": off}
        dx = bwd(code, kind, y, dy, 7.5, ld=all3, off=o3)
        assert np.array_equal(bwd(code, kind, y, dy, 7.5, ld=all3, off=o3, inplace=True), dx), (V, off)


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [257, T1 + 1, T2 + 1])
def test_repeated_runs_and_graph_replay_are_identical(V):
    code, rows = H.BF16, 37
    rng = np.random.default_rng(V)
    x, dy = R.draw_logits(rng, "wide", code, rows, V), R.draw_dy(rng, "normal", code, rows, V)
    eager = {}
    for kind in R.KINDS:
        y = fwd(code, kind, x)
        assert np.array_equal(fwd(code, kind, x), y)
        dx = bwd(code, kind, y, dy)
        assert np.array_equal(bwd(code, kind, y, dy), dx)
        eager[kind] = (y, dx)
    X, D = Buf(rng, code, rows, V).put(x).up(), Buf(rng, code, rows, V).put(dy).up()
    Y = {k: Buf(rng, code, rows, V).up() for k in R.KINDS}
    DX = {k: Buf(rng, code, rows, V).up() for k in R.KINDS}
    st = H.Stream()
    with H.Graph.capture(st) as graph:
        for k in R.KINDS:
            H.softmax_fwd(k, code, rows, V, 1.0, X.ptr(), V, Y[k].ptr(), V, st.handle)
            H.softmax_bwd(k, code, rows, V, 1.0, Y[k].ptr(), V, D.ptr(), V, DX[k].ptr(), V, st.handle)
    for _ in range(2):
        graph.launch()
        st.sync()
        for k in R.KINDS:
            assert np.array_equal(Y[k].get(), eager[k][0]) and np.array_equal(DX[k].get(), eager[k][1]), k
            for b in (Y[k], DX[k]):   # wipe the outputs: the next replay has to write them again
                b.host[b.idx()] = 0
                H.check(H.lib().kf_memcpy_h2d(b.dev.ptr, b.host.ctypes.data, b.host.nbytes, None))
        H.device_sync()


# ---- 7. 64-bit offsets ------------------------------------------------------------------------------------------------------------------
def test_row_offsets_beyond_2_31_elements():
    """bf16, 3 rows of 1000 at a leading dimension of 2^30 elements: the last row starts at element 2^31 (byte 2^32). Only the rows'
    own elements are touched; forward and backward of every row are checked against the reference."""
    code, rows, V, ld = H.BF16, 3, 1000, 1 << 30
    assert (rows - 1) * ld >= 1 << 31
    rng = np.random.default_rng(77)
    x, dy = R.draw_logits(rng, "normal", code, rows, V), R.draw_dy(rng, "normal", code, rows, V)
    nbytes = ((rows - 1) * ld + V) * 2
    bx, by, bdx = (H.DevBuf(nbytes) for _ in range(3))
    bd = H.DevBuf.from_numpy(dy)
    for r in range(rows):
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r * ld * 2, np.ascontiguousarray(x[r]).ctypes.data, V * 2, None))
    for kind in R.KINDS:
        H.softmax_fwd(kind, code, rows, V, 1.0, bx.ptr, ld, by.ptr, ld)
        H.softmax_bwd(kind, code, rows, V, 1.0, by.ptr, ld, bd.ptr, V, bdx.ptr, ld)
        H.device_sync()
        y, dx = np.empty((rows, V), np.uint16), np.empty((rows, V), np.uint16)
        for r in range(rows):
            H.check(H.lib().kf_memcpy_d2h(y[r].ctypes.data, by.ptr + r * ld * 2, V * 2, None))
            H.check(H.lib().kf_memcpy_d2h(dx[r].ctypes.data, bdx.ptr + r * ld * 2, V * 2, None))
        check_fwd(code, kind, x, 1.0, y, "ld 2^30")
        check_bwd(code, kind, y, dy, 1.0, dx, "ld 2^30")
        # the same values in a small buffer at the same phase (ld a multiple of the pack): the same bits
        assert np.array_equal(fwd(code, kind, x, ld={"x": V + 8, "y": V + 8}), y)


# ---- 8. the operator API ----------------------------------------------------------------------------------------------------------------
def to_t(b, code, requires_grad=False):
    f = R.floats(b, code).astype(np.float32)
    t = kfunca.from_numpy_bf16(np.ascontiguousarray(b.view(np.uint16)), 0) if code == H.BF16 else kfunca.from_numpy(f.astype(np.float16) if code == H.F16 else f, 0)
    t.set_requires_grad(requires_grad)
    return t


def t_bits(t, code):
    return np.ascontiguousarray(t.contiguous().numpy()).view(R.UINT[code])   # (a result permuted back is a view: numpy() wants it dense)


OPS = {SM: kfunca.softmax, LSM: kfunca.log_softmax}


@pytest.mark.parametrize("code", [H.F32, H.BF16])
@pytest.mark.parametrize("kind", R.KINDS)
def test_operator_over_every_dim_against_torch_cpu(code, kind):
    """softmax / log_softmax of a [2, 3, 5, 7] tensor over every dim, and the gradient of sum(y * c). The host core's sum has no grad
    function; the gradient of a sum is ones, so backward() starts at y * c with ones."""
    import torch
    tfn = torch.softmax if kind == SM else torch.log_softmax
    shape = (2, 3, 5, 7)
    rng = np.random.default_rng(11)
    xb = R.draw_logits(rng, "normal", code, 30, 7).reshape(shape)
    cb = R.draw_dy(rng, "normal", code, 30, 7).reshape(shape)
    xf, cf = R.floats(xb, code), R.floats(cb, code)
    for dim in range(-4, 4):
        for scale in (1.0, 0.125):
            x = to_t(xb, code, True)
            y = OPS[kind](x, dim=dim, scale=scale) if scale != 1.0 else OPS[kind](x, dim)
            assert y.sizes() == list(shape)
            z = y * to_t(cb, code)
            z.backward(to_t(R.bits(np.ones(shape), code), code))
            t = torch.tensor(xf, dtype=torch.float64, requires_grad=True)
            ty = tfn(t * scale, dim=dim)
            (ty * torch.tensor(cf)).sum().backward()
            yb = t_bits(y, code)
            last = lambda a: np.moveaxis(a, dim, -1).reshape(-1, shape[dim])  # noqa: E731
            ref, lse = R.forward(kind, last(xf), scale)
            assert np.abs(ref - last(ty.detach().numpy())).max() <= 1e-12
            assert (np.abs(last(R.floats(yb, code)) - ref) <= R.forward_bound(kind, code, ref, lse)).all(), (dim, scale)
            # the gradient: the reference on the stored y; torch's (from its own unrounded y) within that bound plus the f32 / 16-bit rounding of y
            ys = last(R.floats(yb, code))
            dref = R.backward(kind, ys, last(cf), scale)
            got = last(R.floats(t_bits(x.grad(), code), code))
            assert x.grad().sizes() == list(shape)
            assert (np.abs(got - dref) <= R.backward_bound(kind, code, ys, last(cf), scale, dref)).all(), (dim, scale)
            assert_close(got, last(t.grad.numpy()), rtol=1e-3 if code == H.F32 else 3e-2, atol=1e-5 if code == H.F32 else 3e-2, what=f"dx dim {dim}")


@pytest.mark.parametrize("code", [H.F32, H.BF16])
@pytest.mark.parametrize("kind", R.KINDS)
def test_operator_non_contiguous_inputs_equal_their_contiguous_twins(code, kind):
    rng = np.random.default_rng(12)
    xb = R.draw_logits(rng, "normal", code, 12, 40)
    gb = R.draw_dy(rng, "normal", code, 12, 40)
    op = OPS[kind]

    def grad_of(x, y, g):
        y.backward(g)
        return t_bits(x.grad(), code)

    base = to_t(xb, code, True)
    yb = op(base)
    dxb = grad_of(base, yb, to_t(gb, code))
    # a column slice is read in place through its leading dimension (and so is a sliced gradient)
    wide = to_t(np.concatenate([xb, xb], 1), code, True)
    sl = wide[:, 40:]
    assert sl.strides() == [80, 1] and sl.storage_offset() == 40
    ys = op(sl)
    assert np.array_equal(t_bits(ys, code), t_bits(yb, code))
    assert np.array_equal(t_bits(op(sl.contiguous()), code), t_bits(yb, code))
    ys.backward(to_t(np.concatenate([gb, gb], 1), code)[:, :40])
    assert np.array_equal(t_bits(wide.grad(), code)[:, 40:], dxb) and not t_bits(wide.grad(), code)[:, :40].any()
    # a permuted view has no unit stride along its last dim: made dense first, the same bits as its contiguous() twin
    tr = to_t(np.ascontiguousarray(xb.T), code, True)
    pv = tr.permute(1, 0)
    yp = op(pv)
    assert np.array_equal(t_bits(yp, code), t_bits(yb, code)) and np.array_equal(t_bits(op(pv.contiguous()), code), t_bits(yb, code))
    assert np.array_equal(grad_of(tr, yp, to_t(gb, code)), np.ascontiguousarray(dxb.T))
    # over dim 0 of the transposed tensor: moved last and back
    y0 = op(to_t(np.ascontiguousarray(xb.T), code), 0)
    assert y0.sizes() == [40, 12] and np.array_equal(t_bits(y0, code), np.ascontiguousarray(t_bits(yb, code).T))


def test_operator_refusals():
    f = kfunca.from_numpy(np.zeros((4, 6), np.float32), 0)
    for op in (kfunca.softmax, kfunca.log_softmax):
        with pytest.raises(RuntimeError, match="float, half and bfloat16"):
            op(kfunca.from_numpy(np.zeros((4, 6), np.int32), 0))
        with pytest.raises(RuntimeError, match="float, half and bfloat16"):
            op(kfunca.from_numpy(np.zeros((4, 6), np.float64), 0))
        for dim in (2, -3):
            with pytest.raises(RuntimeError, match="out of range"):
                op(f, dim)
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(RuntimeError, match="finite and greater than 0"):
                op(f, -1, scale)
        with pytest.raises(RuntimeError, match="at least one dimension"):
            op(kfunca.from_numpy(np.array(1.0, np.float32), 0))
        assert op(kfunca.from_numpy(np.zeros((0, 8), np.float32), 0)).sizes() == [0, 8]
        assert op(kfunca.from_numpy(np.zeros((3, 0), np.float32), 0)).sizes() == [3, 0]
        assert op(kfunca.from_numpy(np.zeros((3, 0, 2), np.float32), 0), 0).sizes() == [3, 0, 2]


def test_cross_entropy_is_minus_log_softmax_at_the_target():
    rows, V = 8, 5000
    rng = np.random.default_rng(13)
    x = rng.normal(0, 2, (rows, V)).astype(np.float32)
    t = rng.integers(0, V, rows)
    loss = kfunca.cross_entropy(kfunca.from_numpy(x, 0), kfunca.from_numpy(t, 0), reduction="none").numpy()
    lsm = kfunca.log_softmax(kfunca.from_numpy(x, 0)).numpy()
    assert_close(loss, -lsm[np.arange(rows), t], rtol=1e-5, atol=1e-4, what="cross_entropy vs -log_softmax")


def test_moe_router_end_to_end():
    """p = softmax(h w) over 8 experts, the two largest probabilities per token, and the gradient of sum(p * c) (backward() from p * c with
    ones: see test_operator_over_every_dim_against_torch_cpu) into h and w, against torch autograd in f64."""
    import torch
    rng = np.random.default_rng(14)
    T, Kd, E = 64, 32, 8
    h = rng.uniform(-1, 1, (T, Kd)).astype(np.float32)
    w = (rng.uniform(-1, 1, (Kd, E)) * (3.0 / np.sqrt(Kd))).astype(np.float32)
    c = rng.uniform(-1, 1, (T, E)).astype(np.float32)
    th, tw = kfunca.from_numpy(h, 0), kfunca.from_numpy(w, 0)
    th.set_requires_grad(True)
    tw.set_requires_grad(True)
    p = kfunca.softmax(kfunca.gemm(th, tw, 1.0, 0.0))
    vals, idx = p.topk(2, 1, True)
    z = p * kfunca.from_numpy(c, 0)
    z.backward(kfunca.from_numpy(np.ones((T, E), np.float32), 0))
    rh, rw = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (h, w))
    rp = torch.softmax(rh @ rw, dim=-1)
    (rp * torch.tensor(c, dtype=torch.float64)).sum().backward()
    rv, ri = rp.detach().topk(2, dim=1)
    assert_close(p.numpy(), rp.detach().numpy(), rtol=1e-5, atol=1e-6, what="p")
    assert_close(vals.numpy(), rv.numpy(), rtol=1e-5, atol=1e-6, what="top-2 probabilities")
    clear = (rv[:, 0] - rv[:, 1]).numpy() > 1e-4   # where the order is not a matter of rounding
    assert np.array_equal(idx.numpy()[clear], ri.numpy()[clear]) and clear.mean() > 0.9
    assert_close(th.grad().numpy(), rh.grad.numpy(), rtol=1e-3, atol=1e-5, what="dh")
    assert_close(tw.grad().numpy(), rw.grad.numpy(), rtol=1e-3, atol=1e-5, what="dw")


def test_zz_report_the_largest_fraction_of_the_bound():
    """Not a check: prints what the accuracy tests above met (run with -s), for DESIGN.md."""
    for (kind, direction, code), v in sorted(WORST.items()):
        print(f"largest fraction of the bound: {R.KIND_NAME[kind]:11s} {direction:8s} {R.CODE_NAME[code]:4s} {v:.3f}")
