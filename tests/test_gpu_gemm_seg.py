"""-m gpu: the segmented (expert) GEMM through the C ABI - kf_gemm_segmented with trans_b 0 and 1, kf_gemm_segmented_wgrad.

Exact tier (the scheme of tests/gemm_views.py): operands from {-1, 0, 1}, small integer C0, alpha and beta from {1, 0.5, 2, 0}, every
operand a window of a wider buffer with NaN poison around inputs and 0xA5 around outputs (an extra poisoned row between experts too), a
0xA5 workspace; expected values are exact in the output type (asserted on the CPU) and the whole output BUFFER is compared byte for byte,
so a wrong integer, a NaN, a row given to the wrong expert and a damaged sentinel all fail. bf16 and f16 take the matrix-core path,
f32 and N = 72 the plain kernels. Uniform tier: U(-1, 1) operands against the f64 reference of the rounded inputs within
|got - ref| <= 2^-8 |ref| + K 2^-23 sum_k |a_k b_k| (16-bit output rounding plus f32 accumulation, each doubled; f32 outputs: 2^-23 |ref|
for the first term), K the contraction length - the segment's length in wgrad."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_seg_ref as R
from tests import gemm_views as V

pytestmark = pytest.mark.gpu

CODE = {"f32": H.F32, "bf16": H.BF16, "f16": H.F16}
LAYOUTS = {
    1: (256, [0, 256]),                                       # whole tiles, one expert
    2: (300, [0, 1, 129, 129, 300]),                          # one row, exactly 128, empty, ragged
    3: (200, [0, 0, 70, 200, 200, 200]),                      # empty first and last experts
    4: (400, [37, 165, 165, 390]),                            # uncovered head and tail
    5: (96, np.concatenate([[0], np.cumsum([i % 4 for i in range(64)])]).tolist()),   # E 64, lengths 0..3: more experts than tiles
    6: (700, [0, 650, 700]),                                  # ten whole K tiles plus 10 rows in wgrad, six row tiles
    7: (400, [0, 300, 100, 9999]),                            # malformed: must equal 0, 300, 300, 400
}
CONFIGS = [("bf16", 256), ("f16", 256), ("f32", 256), ("bf16", 72)]   # (dtype, N): two on the matrix cores, two on the plain kernels
EPILOGUES = [(1.0, 0.0), (0.5, 2.0), (2.0, 1.0), (0.0, 0.5)]


def fast(dt, *extents):
    return dt != "f32" and all(x % m == 0 for x, m in extents)


def geom(is_fast):
    """(c0, gap) of a window: 16-byte aligned with a pitch that is a multiple of 8 where the matrix-core path is meant, odd otherwise."""
    return (8, 8) if is_fast else (3, 2)


def tri(rng, shape):
    v = rng.integers(0, 4, shape)
    return np.where(v >= 2, 0, 2 * v - 1).astype(np.float64)


def small(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float64)


def uniform_as(rng, shape, dt):
    return V.decode(V.encode(rng.uniform(-1, 1, shape), dt), dt)   # the rounded inputs, as f64


def mat(dt, vals, poison, g):
    return V.View(dt, vals.shape[0], vals.shape[1], g[0], g[1], poison).put(vals)


class Stack:
    """E matrices [r, c] in one window of (r + 1) rows per expert: the extra row keeps the poison."""

    def __init__(self, dt, vals, poison, g):
        self.E, self.r, self.c = vals.shape
        self.view = V.View(dt, self.E * (self.r + 1), self.c, g[0], g[1], poison)
        self.stride = (self.r + 1) * self.view.ld
        self.fill(self.view.buf, vals)

    def fill(self, buf, vals):
        w = self.view.window(buf)
        for e in range(self.E):
            w[e * (self.r + 1): e * (self.r + 1) + self.r] = V.encode(vals[e], self.view.dt).reshape(self.r, self.c)

    def read(self, buf):
        w = self.view.window(buf)
        return np.stack([V.decode(w[e * (self.r + 1): e * (self.r + 1) + self.r], self.view.dt) for e in range(self.E)])


def ptr(buf, view, row=0):
    return buf.ptr + (view.off + row * view.ld) * V.ES[view.dt]


def workspace(dt, T, E):
    n = H.gemm_segmented_workspace_bytes(CODE[dt], T, E)
    return H.DevBuf.from_numpy(np.full(n, 0xA5, dtype=np.uint8)), n


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def expect_buffer(after, expected, dt, what):
    if same_bytes(after, expected):
        return
    got, exp = V.decode(after, dt), V.decode(expected, dt)
    diff = np.flatnonzero((after.view(np.uint8).reshape(after.size, -1) != expected.view(np.uint8).reshape(after.size, -1)).any(axis=1))
    i = int(diff[0])
    raise AssertionError(f"{what}: {diff.size} elements of the output buffer differ (window or sentinel); first at flat index {i}: got {got[i]}, want {exp[i]}")


class Fwd:
    """One kf_gemm_segmented call on views. a [T, K], w [E, K, N] in math order (stored transposed per expert with trans_b)."""

    def __init__(self, dt, trans_b, offsets, a, w, c0, alpha, beta, is_fast):
        self.dt, self.tb, self.offsets, self.alpha, self.beta = dt, trans_b, offsets, alpha, beta
        self.T, self.K = a.shape
        self.E, _, self.N = w.shape
        g = geom(is_fast)
        self.a = mat(dt, a, "nan", g)
        self.w = Stack(dt, np.swapaxes(w, 1, 2) if trans_b else w, "nan", g)
        self.c = mat(dt, c0, "a5", g)
        self.d = {n: H.DevBuf.from_numpy(v.buf) for n, v in (("a", self.a), ("w", self.w.view), ("c", self.c))}
        self.off = H.DevBuf.from_numpy(np.asarray(offsets, dtype=np.int64))
        self.ws, self.ws_bytes = workspace(dt, self.T, self.E)

    def call(self, stream=None):
        H.gemm_segmented(CODE[self.dt], self.tb, self.T, self.N, self.K, self.E, self.off.ptr, self.alpha, ptr(self.d["a"], self.a), self.a.ld,
                         ptr(self.d["w"], self.w.view), self.w.view.ld, self.w.stride, self.beta, ptr(self.d["c"], self.c), self.c.ld, self.ws.ptr,
                         self.ws_bytes, stream)

    def after(self):
        H.device_sync()
        return self.d["c"].to_numpy(self.c.buf.shape, self.c.buf.dtype)

    def reset_c(self):
        H.check(H.lib().kf_memcpy_h2d(self.d["c"].ptr, self.c.buf.ctypes.data, self.c.buf.nbytes, None))

    def inputs_unchanged(self):
        for n, v in (("a", self.a), ("w", self.w.view)):
            assert same_bytes(self.d[n].to_numpy(v.buf.shape, v.buf.dtype), v.buf), f"the call changed input {n}"


class Wgrad:
    """One kf_gemm_segmented_wgrad call on views. a [T, M], b [T, N], dw0 [E, M, N]."""

    def __init__(self, dt, offsets, a, b, dw0, alpha, beta, is_fast):
        self.dt, self.offsets, self.alpha, self.beta = dt, offsets, alpha, beta
        self.T, self.M = a.shape
        self.N, self.E = b.shape[1], dw0.shape[0]
        g = geom(is_fast)
        self.a, self.b = mat(dt, a, "nan", g), mat(dt, b, "nan", (g[0], g[1] + (8 if is_fast else 1)))
        self.dw = Stack(dt, dw0, "a5", g)
        self.d = {n: H.DevBuf.from_numpy(v.buf) for n, v in (("a", self.a), ("b", self.b), ("dw", self.dw.view))}
        self.off = H.DevBuf.from_numpy(np.asarray(offsets, dtype=np.int64))
        self.ws, self.ws_bytes = workspace(dt, self.T, self.E)

    def call(self, stream=None):
        H.gemm_segmented_wgrad(CODE[self.dt], self.T, self.M, self.N, self.E, self.off.ptr, self.alpha, ptr(self.d["a"], self.a), self.a.ld,
                               ptr(self.d["b"], self.b), self.b.ld, self.beta, ptr(self.d["dw"], self.dw.view), self.dw.view.ld, self.dw.stride,
                               self.ws.ptr, self.ws_bytes, stream)

    def after(self):
        H.device_sync()
        return self.d["dw"].to_numpy(self.dw.view.buf.shape, self.dw.view.buf.dtype)

    def inputs_unchanged(self):
        for n, v in (("a", self.a), ("b", self.b)):
            assert same_bytes(self.d[n].to_numpy(v.buf.shape, v.buf.dtype), v.buf), f"the call changed input {n}"


def exact_in(want, dt):
    assert np.abs(want).max() <= V.EXACT_BOUND[dt] and np.array_equal(V.decode(V.encode(want, dt), dt), want), f"an expected value is not exact in {dt}"


def expected_c(f, want):
    exp = f.c.buf.copy()
    f.c.window(exp)[...] = V.encode(want, f.dt).reshape(want.shape)
    return exp


def expected_dw(f, want):
    exp = f.dw.view.buf.copy()
    f.dw.fill(exp, want)
    return exp


def seed(*xs):
    s = 7
    for x in xs:
        s = (s * 1000003 + int(x)) % (1 << 31)
    return s


# ---- exact tier ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,N", CONFIGS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_forward_exact(layout, dt, N):
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    owner = R.row_expert(offsets, T)
    for i, (K, tb) in enumerate([(64, 0), (64, 1), (320, 0), (320, 1)]):
        alpha, beta = EPILOGUES[(i + layout) % 4]
        rng = np.random.default_rng(seed(layout, N, K, tb, len(dt)))
        a, w, c0 = tri(rng, (T, K)), tri(rng, (E, K, N)), small(rng, (T, N))
        want = R.forward(a, w, offsets, alpha, beta, c0) + 0.0
        exact_in(want, dt)
        assert np.array_equal(want[owner < 0], (beta * c0)[owner < 0] + 0.0)
        f = Fwd(dt, tb, offsets, a, w, c0, alpha, beta, fast(dt, (N, 128), (K, 64)))
        f.call()
        after = f.after()
        expect_buffer(after, expected_c(f, want), dt, f"layout {layout} {dt} N {N} K {K} trans_b {tb} alpha {alpha} beta {beta}")
        got = V.decode(f.c.window(after), dt)
        assert np.array_equal(got[owner < 0], (beta * c0)[owner < 0] + 0.0)   # uncovered rows: beta C0
        f.inputs_unchanged()


WGRAD_SHAPES = [(64, 256), (320, 256), (128, 256), (256, 128)]   # (M, N): the issue's Din with Dout 256, and two on the matrix cores


@pytest.mark.parametrize("dt,N72", CONFIGS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_wgrad_exact(layout, dt, N72):
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    shapes = [(64, 72), (320, 72)] if N72 == 72 else WGRAD_SHAPES
    for i, (M, N) in enumerate(shapes):
        alpha, beta = EPILOGUES[(i + layout + 1) % 4]
        rng = np.random.default_rng(seed(layout, M, N, len(dt), 3))
        a, b, d0 = tri(rng, (T, M)), tri(rng, (T, N)), small(rng, (E, M, N))
        want = R.wgrad(a, b, offsets, alpha, beta, d0) + 0.0
        exact_in(want, dt)
        f = Wgrad(dt, offsets, a, b, d0, alpha, beta, fast(dt, (M, 128), (N, 128)))
        f.call()
        expect_buffer(f.after(), expected_dw(f, want), dt, f"layout {layout} {dt} M {M} N {N} alpha {alpha} beta {beta}")
        f.inputs_unchanged()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("layout", [2, 3, 6])
def test_a_neighbours_nan_rows_stay_in_their_segment(layout, dt):
    """The rows of segment e + 1 set to NaN in A: dW_e stays exact (the rows past a segment's end enter as zeros, they are not multiplied
    by zero), and so does every output row outside segment e + 1."""
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    so = R.sanitize(offsets, T)
    owner = R.row_expert(offsets, T)
    e1 = next(e for e in range(1, E) if so[e + 1] > so[e] and so[e] > so[0])   # a non-empty segment with rows before it
    rng = np.random.default_rng(seed(layout, len(dt), 11))
    M, N, K = 128, 256, 64
    a, b, d0 = tri(rng, (T, M)), tri(rng, (T, N)), small(rng, (E, M, N))
    want = R.wgrad(a, b, offsets, 1.0, 1.0, d0) + 0.0
    a_nan = a.copy()
    a_nan[owner == e1] = np.nan
    f = Wgrad(dt, offsets, a_nan, b, d0, 1.0, 1.0, fast(dt, (M, 128), (N, 128)))
    f.call()
    got = f.dw.read(f.after())
    for e in range(E):
        if e != e1:
            assert np.array_equal(got[e], want[e]), f"dW_{e} changed when segment {e1}'s rows became NaN"
    assert np.isnan(got[e1]).all()
    ax, w, c0 = tri(rng, (T, K)), tri(rng, (E, K, N)), small(rng, (T, N))
    wantc = R.forward(ax, w, offsets, 1.0, 1.0, c0) + 0.0
    ax_nan = ax.copy()
    ax_nan[owner == e1] = np.nan
    for tb in (0, 1):
        g = Fwd(dt, tb, offsets, ax_nan, w, c0, 1.0, 1.0, fast(dt, (N, 128), (K, 64)))
        g.call()
        gotc = V.decode(g.c.window(g.after()), dt)
        assert np.array_equal(gotc[owner != e1], wantc[owner != e1]), "a row outside the NaN segment changed"
        assert np.isnan(gotc[owner == e1]).all()


# ---- uniform tier ----------------------------------------------------------------------------------------------------------------------
def bound(ref, absref, K, dt):
    return (2.0 ** -23 if dt == "f32" else 2.0 ** -8) * np.abs(ref) + K * 2.0 ** -23 * absref


def uniform_fwd(dt, layout, N, K, tb, alpha=1.0, beta=0.0):
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    rng = np.random.default_rng(seed(layout, N, K, tb, len(dt), 5))
    a, w, c0 = uniform_as(rng, (T, K), dt), uniform_as(rng, (E, K, N), dt), uniform_as(rng, (T, N), dt)
    return Fwd(dt, tb, offsets, a, w, c0, alpha, beta, fast(dt, (N, 128), (K, 64))), a, w, c0


def uniform_wgrad(dt, layout, M, N, alpha=1.0, beta=0.0):
    T, offsets = LAYOUTS[layout]
    E = len(offsets) - 1
    rng = np.random.default_rng(seed(layout, M, N, len(dt), 6))
    a, b, d0 = uniform_as(rng, (T, M), dt), uniform_as(rng, (T, N), dt), uniform_as(rng, (E, M, N), dt)
    return Wgrad(dt, offsets, a, b, d0, alpha, beta, fast(dt, (M, 128), (N, 128))), a, b, d0


@pytest.mark.parametrize("dt,N", CONFIGS)
@pytest.mark.parametrize("layout", [2, 4, 6])
def test_uniform_against_f64(layout, dt, N):
    T, offsets = LAYOUTS[layout]
    for K, tb in ((64, 0), (320, 1)):
        f, a, w, c0 = uniform_fwd(dt, layout, N, K, tb)
        f.call()
        got = V.decode(f.c.window(f.after()), dt)
        ref, absref = R.forward(a, w, offsets), R.abs_forward(a, w, offsets)
        print(f"fwd layout {layout} {dt} N {N} K {K} trans_b {tb}: max excess {(np.abs(got - ref) - bound(ref, absref, K, dt)).max():.3e}")
        assert (np.abs(got - ref) <= bound(ref, absref, K, dt)).all()
    M = 128 if N == 256 else 64
    g, a, b, d0 = uniform_wgrad(dt, layout, M, N)
    g.call()
    got = g.dw.read(g.after())
    ref, absref = R.wgrad(a, b, offsets), R.abs_wgrad(a, b, offsets)
    lens = np.diff(R.sanitize(offsets, T)).astype(np.float64)[:, None, None]   # the contraction length: the segment's
    lim = (2.0 ** -23 if dt == "f32" else 2.0 ** -8) * np.abs(ref) + lens * 2.0 ** -23 * absref
    print(f"wgrad layout {layout} {dt} M {M} N {N}: max excess {(np.abs(got - ref) - lim).max():.3e}")
    assert (np.abs(got - ref) <= lim).all()


# ---- a segment alone, two runs, a captured graph ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,N", [("bf16", 256), ("f32", 256)])
def test_a_segment_equals_the_same_call_on_that_segment_alone(dt, N):
    layout, K, M = 2, 320, 128
    T, offsets = LAYOUTS[layout]
    so = R.sanitize(offsets, T)
    for tb in (0, 1):
        f, a, w, c0 = uniform_fwd(dt, layout, N, K, tb, 0.5, 2.0)
        f.call()
        full = f.c.window(f.after())
        for e in range(len(so) - 1):
            lo, hi = int(so[e]), int(so[e + 1])
            if hi > lo:
                one = Fwd(dt, tb, [0, hi - lo], a[lo:hi], w[e:e + 1], c0[lo:hi], 0.5, 2.0, fast(dt, (N, 128), (K, 64)))
                one.call()
                assert same_bytes(one.c.window(one.after()), full[lo:hi]), f"segment {e} differs from the same call with E = 1 (trans_b {tb})"
    for layout in (2, 6):
        T, offsets = LAYOUTS[layout]
        so = R.sanitize(offsets, T)
        g, a, b, d0 = uniform_wgrad(dt, layout, M, N, 0.5, 2.0)
        g.call()
        full = g.dw.read(g.after())
        for e in range(len(so) - 1):
            lo, hi = int(so[e]), int(so[e + 1])
            if hi > lo:
                one = Wgrad(dt, [0, hi - lo], a[lo:hi], b[lo:hi], d0[e:e + 1], 0.5, 2.0, fast(dt, (M, 128), (N, 128)))
                one.call()
                assert np.array_equal(one.dw.read(one.after())[0], full[e]), f"dW_{e} differs from the same call with E = 1 (layout {layout})"
            else:
                assert np.array_equal(full[e], V.decode(V.encode(2.0 * d0[e], dt), dt))   # an empty segment: beta dW_e


@pytest.mark.parametrize("dt,N", [("bf16", 256), ("f16", 256), ("f32", 72)])
def test_two_runs_and_a_captured_graph_give_the_same_bits(dt, N):
    layout, K, M = 4, 320, 128 if N == 256 else 64
    stream = H.Stream()
    for make in (lambda: uniform_fwd(dt, layout, N, K, 0)[0], lambda: uniform_fwd(dt, layout, N, K, 1)[0], lambda: uniform_wgrad(dt, layout, M, N)[0]):
        f = make()
        f.call()
        first = f.after()
        f.call()
        assert same_bytes(f.after(), first), "two runs differ"
        f.call(stream.handle)   # (every one-time setup of the launch path happens outside the capture)
        stream.sync()
        with H.Graph.capture(stream) as graph:
            f.call(stream.handle)
        for _ in range(2):
            graph.launch()
            stream.sync()
            assert same_bytes(f.after(), first), "a replayed graph differs from the direct call"
