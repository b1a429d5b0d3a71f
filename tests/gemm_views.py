"""GEMM operands that are windows of wider buffers: buffers, exact operands, the dispatch restated, and pitch-bug models. numpy only.

A view is the rows x cols window of a (rows, ld) matrix that starts at column c0, ld = c0 + cols + gap, inside an allocation of
lo + rows * ld + hi elements; lo is 1 MiB, hi at least 1 MiB and long enough that a kernel which walks the operand with ANY pitch of
the same call (the mistakes model_product imitates) stays inside the allocation. Whatever is not the window holds poison: a NaN with
a payload for inputs (one gap element in one product and the output is NaN), the byte 0xA5 for outputs (finite, and it has to come
back unchanged). Operands are drawn from {-1, 0, 1} with P(0) = 1/2, C0 / bias / mul / add are small integers and alpha, beta come
from {1, 0.5, 2, 0}: every expected output is an integer or a half that the output type holds exactly (asserted here, on the CPU),
so a kernel's result is compared bit for bit and no tolerance exists.
"""
import numpy as np

GUARD_BYTES = 1 << 20
ES = {"f32": 4, "f64": 8, "bf16": 2, "f16": 2}
STORE = {"f32": np.float32, "f64": np.float64, "bf16": np.uint16, "f16": np.uint16}
_BITS = {"f32": np.uint32, "f64": np.uint64, "bf16": np.uint16, "f16": np.uint16}
NAN_BITS = {"f32": 0x7FC0A5A5, "f64": 0x7FF8A5A5A5A5A5A5, "bf16": 0x7FE5, "f16": 0x7EA5}  # quiet NaNs with a payload
EXACT_BOUND = {"bf16": 256.0, "f16": 2048.0, "f32": float(1 << 24), "f64": float(1 << 53)}  # bf16 with halves: 128 (checked by round trip)


def encode(x, dt):
    """f64 values -> stored elements of dt (round to nearest even; exact for the integer draws)."""
    x = np.asarray(x, dtype=np.float64)
    if dt == "f64":
        return x.copy()
    if dt == "f32":
        return x.astype(np.float32)
    if dt == "f16":
        return x.astype(np.float16).view(np.uint16)
    b = x.astype(np.float32).view(np.uint32)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def decode(s, dt):
    """stored elements of dt -> f64."""
    s = np.asarray(s)
    if dt in ("f32", "f64"):
        return s.astype(np.float64)
    if dt == "f16":
        return s.view(np.float16).astype(np.float64)
    return (s.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


class View:
    """One operand: `buf` is the whole allocation (stored elements), `off` the element offset of the window's first element."""

    def __init__(self, dt, rows, cols, c0, gap, poison, reach=0):
        assert poison in ("nan", "a5") and rows > 0 and cols > 0 and c0 >= 0 and gap >= 0
        self.dt, self.rows, self.cols, self.c0, self.ld, self.poison = dt, rows, cols, c0, c0 + cols + gap, poison
        es = ES[dt]
        self.lo = GUARD_BYTES // es
        self.hi = (max(self.lo, reach - rows * self.ld) + 15) // 16 * 16
        self.off = self.lo + c0
        n = self.lo + rows * self.ld + self.hi
        if poison == "nan":
            self.buf = np.full(n, NAN_BITS[dt], dtype=_BITS[dt]).view(STORE[dt])
        else:
            self.buf = np.full(n * es, 0xA5, dtype=np.uint8).view(STORE[dt])
        assert self.lo * es >= GUARD_BYTES and self.hi * es >= GUARD_BYTES and self.off > 0

    def window(self, buf=None):
        """The rows x cols window of `buf` (default: this view's own buffer) - a numpy view, writable."""
        buf = self.buf if buf is None else buf
        assert buf.size == self.buf.size and buf.dtype == self.buf.dtype
        return buf[self.lo: self.lo + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.c0: self.c0 + self.cols]

    def put(self, values):
        self.window()[...] = encode(values, self.dt).reshape(self.rows, self.cols)
        return self

    def outside_intact(self, after):
        """Every byte of `after` outside the window equals this view's buffer (the poison)."""
        t = after.copy()
        self.window(t)[...] = self.window()
        return np.array_equal(t.view(np.uint8), self.buf.view(np.uint8))

    def packed(self):
        """The same window with no column offset and no gap (still behind its guard)."""
        v = View(self.dt, self.rows, self.cols, 0, 0, self.poison)
        v.window()[...] = self.window()
        return v


def operand_gaps(g1, g2):
    """(c0, gap) per operand from a table row's two gap values: ld - extent is g1 + g2, 2 g2 and 2 g1 for A, B and C - three different
    pitches in one call even where the extents agree, so a swapped pitch cannot cancel."""
    return {"a": (g1, g2), "b": (g2, g2), "c": (g1, g1), "mul": (g2, g1), "add": (g1, g2), "aux": (g2, g2)}


class Case:
    """One product C = alpha op(A) op(B) + beta C0 (+ bias) (then aux = that, C = that * mul + add) on views.

    draw = "int": exact operands and `want` / `want_aux` (f64); draw = "uniform": U(-1, 1) operands, no expected value (such a case is
    compared with the same call on packed copies). gaps: {operand: (c0, gap)}, operands a, b, c and with tail mul, add, aux.
    c_dt: C's dtype (f32 behind 16-bit operands)."""

    def __init__(self, dt, ta, tb, M, N, K, gaps, alpha=1.0, beta=0.0, bias=False, tail=False, c_dt=None, seed=0, draw="int"):
        self.dt, self.ta, self.tb, self.M, self.N, self.K = dt, bool(ta), bool(tb), M, N, K
        self.alpha, self.beta, self.tail, self.c_dt = float(alpha), float(beta), bool(tail), c_dt or dt
        assert self.alpha in (1.0, 0.5, 2.0, 0.0) and self.beta in (1.0, 0.5, 2.0, 0.0)
        rng = np.random.default_rng(seed)
        if draw == "int":
            a = rng.integers(0, 4, (M, K)).astype(np.float32)
            b = rng.integers(0, 4, (K, N)).astype(np.float32)
            a, b = np.where(a >= 2, 0, 2 * a - 1), np.where(b >= 2, 0, 2 * b - 1)  # -1, 1 with probability 1/4 each, 0 with 1/2
            small = lambda shp: rng.integers(-3, 4, shp, dtype=np.int8).astype(np.float32)  # noqa: E731
        else:
            a, b = rng.uniform(-1, 1, (M, K)), rng.uniform(-1, 1, (K, N))
            small = lambda shp: rng.uniform(-1, 1, shp)  # noqa: E731
        c0v, biasv = small((M, N)), small((N,))
        if tail:
            addv = small((M, N))
            mulv = np.array([-1.0, 1.0, 2.0], dtype=np.float32)[rng.integers(0, 3, (M, N), dtype=np.int8)] if draw == "int" else small((M, N))
        sa, sb = (a.T if ta else a), (b.T if tb else b)
        shapes = {"a": sa.shape, "b": sb.shape, "c": (M, N), "mul": (M, N), "add": (M, N), "aux": (M, N)}
        names = ("a", "b", "c") + (("mul", "add", "aux") if tail else ())
        reach = max(M, N, K) * max(gaps[n][0] + shapes[n][1] + gaps[n][1] for n in names) + max(gaps[n][0] for n in names)
        mk = lambda n, d, poison: View(d, shapes[n][0], shapes[n][1], gaps[n][0], gaps[n][1], poison, reach)  # noqa: E731
        self.a, self.b = mk("a", dt, "nan").put(sa), mk("b", dt, "nan").put(sb)
        self.c = mk("c", self.c_dt, "a5").put(c0v)
        self.bias = View(dt, 1, N, 5, 3, "nan").put(biasv) if bias else None
        self.mul = mk("mul", dt, "nan").put(mulv) if tail else None
        self.add = mk("add", dt, "nan").put(addv) if tail else None
        self.aux = mk("aux", dt, "a5") if tail else None
        self.want = self.want_aux = None
        if draw == "int":
            # integers and halves far below 2^23: float arithmetic is exact here in any order (and the exactness is asserted below)
            t = np.float32(self.alpha) * (a @ b) + np.float32(self.beta) * c0v + (biasv[None, :] if bias else np.float32(0))
            assert t.dtype == np.float32 and np.abs(t).max() < 1 << 20
            self.want_aux = t.astype(np.float64) + 0.0 if tail else None  # (+ 0.0: a zero is +0, as every kernel's zero-started sum is)
            self.want = (t * mulv + addv if tail else t).astype(np.float64) + 0.0
            for w, d in ((self.want, self.c_dt), (self.want_aux, dt)):
                if w is not None:
                    assert np.abs(w).max() <= EXACT_BOUND[d], (np.abs(w).max(), d)
                    assert np.array_equal(decode(encode(w, d), d), w), f"an expected value is not exact in {d}: change the seed or the density"

    def views(self):
        return [v for v in (self.a, self.b, self.c, self.bias, self.mul, self.add, self.aux) if v is not None]

    def packed(self):
        """The same call on packed copies of every operand."""
        import copy
        p = copy.copy(self)
        for n in ("a", "b", "c", "bias", "mul", "add", "aux"):
            v = getattr(self, n)
            setattr(p, n, v.packed() if v is not None else None)
        return p


def check_output(view, after, want):
    """What the GPU suite asserts about an output buffer after the call: the window holds `want` bit for bit (no NaN, no wrong integer),
    every byte outside it is still the sentinel."""
    got = view.window(after)
    exp = encode(want, view.dt).reshape(view.rows, view.cols)
    nan = np.isnan(decode(got, view.dt))
    assert not nan.any(), f"{int(nan.sum())} NaN outputs: gap elements entered a product (first at {tuple(np.argwhere(nan)[0])})"
    same = got.view(_BITS[view.dt]) == exp.view(_BITS[view.dt])
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{int((~same).sum())} outputs differ from the exact value; first at {i}: got {decode(got, view.dt)[i]}, want {want[i]}")
    assert view.outside_intact(after), "bytes outside the output window changed (0xA5 sentinel damaged)"


def model_product(case, lda=None, ldb=None, ldc=None, a_off=None, b_off=None, a_axes_swapped=False, b_axes_swapped=False):
    """C's buffer as a plain f64 evaluation of the product leaves it when it walks the buffers with THESE pitches and offsets (default:
    the true ones). `*_axes_swapped` puts the pitch on the contiguous axis of the operand and the unit stride on the other."""
    assert not case.tail and case.want is not None
    M, N, K = case.M, case.N, case.K
    lda, ldb, ldc = (case.a.ld if lda is None else lda), (case.b.ld if ldb is None else ldb), (case.c.ld if ldc is None else ldc)
    a_off, b_off = (case.a.off if a_off is None else a_off), (case.b.off if b_off is None else b_off)
    i, j, k = np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64), np.arange(K, dtype=np.int64)

    def gather(view, off, ld, rows_ix, cols_ix, stored_transposed, swapped):
        # op(X)[r, c] lies at r * ld + c, or at c * ld + r when X is stored transposed
        major, minor = (cols_ix[None, :], rows_ix[:, None]) if stored_transposed else (rows_ix[:, None], cols_ix[None, :])
        if swapped:
            major, minor = minor, major
        ix = off + major * ld + minor
        assert ix.min() >= 0 and ix.max() < view.buf.size, "the model walked out of the allocation: the guard is too short"
        return decode(view.buf[ix], view.dt)

    with np.errstate(invalid="ignore"):
        p = gather(case.a, a_off, lda, i, k, case.ta, a_axes_swapped) @ gather(case.b, b_off, ldb, k, j, case.tb, b_axes_swapped)
        out = case.c.buf.copy()
        cix = case.c.off + i[:, None] * ldc + j[None, :]
        assert cix.max() < out.size
        t = case.alpha * p
        if case.beta != 0.0:
            t = t + case.beta * decode(out[cix], case.c.dt)
        if case.bias is not None:
            t = t + decode(case.bias.window(), case.dt)
        out[cix] = encode(t, case.c.dt)
    return out


# ---- the dispatch of kf_gemm / kf_gemm_ex / kf_gemm_grouped restated (kfunca_amd/csrc/device/gemm.hip: gemm_impl, splitk_slices, pad_plan,
# grouped_single_grid): which kernel labels one call records, from its extents, pitches and base alignments ---------------------------------
H256_MIN_TILES = 100


def _h_fast(M, N, K):
    return M % 128 == 0 and N % 128 == 0 and K % 64 == 0 and min(M, N, K) > 0


def _h256(M, N, K):
    return M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and min(M, N, K) > 0 and (M // 256) * (N // 256) >= H256_MIN_TILES


def splitk_slices(dt, M, N, K):
    if dt not in ("bf16", "f16") or not _h_fast(M, N, K) or _h256(M, N, K):
        return 1
    tiles, nt = (M // 128) * (N // 128), K // 64
    if tiles > 128:
        return 1
    s = 1
    while s < 16 and tiles * (s * 2) <= 512 and nt // (s * 2) >= 8:
        s *= 2
    return s


def _pad_plan(dt, M, N, K):
    half = dt in ("bf16", "f16")
    if not (half or dt == "f32") or min(M, N, K) <= 0 or M * N * K < (1 << 24):
        return None
    tm, tk = (128, 64) if half else (64, 16)
    Mp, Np, Kp = -(-M // tm) * tm, -(-N // tm) * tm, -(-K // tk) * tk
    return None if (Mp, Np, Kp) == (M, N, K) else (Mp, Np, Kp)


def expected_labels(dt, ta, tb, M, N, K, lda, ldb, a_base16, b_base16, workspace=False, tail=False, c_f32=False):
    """The set of profile labels of one call. a_base16 / b_base16: the operand's base address is a multiple of 16 bytes; workspace: the
    caller passes what kf_gemm_workspace_bytes asks for (16-byte aligned)."""
    al16 = a_base16 and b_base16
    if dt == "f32" and M % 64 == 0 and N % 64 == 0 and K % 16 == 0 and K > 0 and al16 and lda % 4 == 0 and ldb % 4 == 0:
        t128 = M % 128 == 0 and N % 128 == 0 and (M // 128) * (N // 128) >= 192
        return {"gemm_f32_mfma" if t128 else "gemm_f32_mfma_t64"}
    if dt == "f64" and M % 64 == 0 and N % 64 == 0 and K % 16 == 0 and K > 0 and al16 and lda % 2 == 0 and ldb % 2 == 0:
        return {"gemm_f64_mfma"}
    if dt in ("bf16", "f16") and _h_fast(M, N, K) and al16 and lda % 8 == 0 and ldb % 8 == 0:
        if _h256(M, N, K):
            return {f"gemm_{dt}_mfma"}
        split = splitk_slices(dt, M, N, K) > 1 and workspace and N % 4 == 0
        return {f"gemm_{dt}_mfma_128" + ("_splitk" if split else "")}
    pp = _pad_plan(dt, M, N, K)
    if pp and workspace and not (tail or c_f32):
        Mp, Np, Kp = pp
        q = 8 if dt != "f32" else 4
        (ar, ac, arp, acp) = (K, M, Kp, Mp) if ta else (M, K, Mp, Kp)
        (br, bc, brp, bcp) = (N, K, Np, Kp) if tb else (K, N, Kp, Np)
        use_a = (ar, ac) == (arp, acp) and a_base16 and lda % q == 0
        use_b = (br, bc) == (brp, bcp) and b_base16 and ldb % q == 0
        inner = expected_labels(dt, ta, tb, Mp, Np, Kp, lda if use_a else acp, ldb if use_b else bcp, True, True, splitk_slices(dt, Mp, Np, Kp) > 1)
        return {"gemm_pad"} | inner
    return {"gemm_generic"}


def pair_is_one_grid(dt, problems):
    """problems: dicts with ta, tb, M, N, K, lda, ldb, ldc, a_base16, b_base16 - grouped_single_grid restated."""
    def ok(q):
        return (_h_fast(q["M"], q["N"], q["K"]) and _h256(q["M"], q["N"], q["K"]) and ((q["M"] // 256) * (q["N"] // 256)) % 8 == 0 and q["a_base16"] and
                q["b_base16"] and q["lda"] % 8 == 0 and q["ldb"] % 8 == 0 and q["ldc"] >= q["N"])
    p = problems
    return dt in ("bf16", "f16") and len(p) == 2 and not p[0]["ta"] and p[0]["tb"] and p[1]["ta"] and not p[1]["tb"] and ok(p[0]) and ok(p[1])
