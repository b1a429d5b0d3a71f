"""-m gpu: the mixture-of-experts routing entries (kf_moe_plan, kf_moe_gate_*, kf_moe_dispatch, kf_moe_combine, kf_moe_combine_bwd) and the
operators over them against tests/moe_ref.py.

Every device buffer is allocated under tests/poison.py (0x00, 0xFF, 0x7F: the three runs must give the same bits), operands are windows
of wider buffers whose gaps hold the pattern, and every byte outside an output's window - the guard band behind it included - must
still hold the pattern after the call.

Bit for bit: the plan; the dispatch; dys; y in bf16 and f16 (a product of two 16-bit values is exact in f32, so the f32 sum in the order
j, rounded once, is the result); the gate without normalisation; zeros where the contract says +0.
Bounded against the f64 evaluation, with h = 2^-8 (bf16), 2^-11 (f16), 2^-23 (f32) for the store:
    y in f32          |got - ref| <= k 2^-23 sum_j |g_j ys_j|                      (k products and k sums in f32)
    dgate             |got - ref| <= h |ref| + cols 2^-23 sum_c |dy ys|             (the form of tests/test_gpu_gemm_seg.py)
    gate, normalised  |got - ref| <= (h + 2^-21) |ref|                             (the store, the f32 division and a k-term sum of positives)
    dp                |got - ref| <= h |ref| + k 2^-22 sum_{j: ids[t,j] = e} m_j,   m_j = |dgate_j| without normalisation, else
                      (|dgate_j| + sum_i |dgate_i gate_i|) / S: ds_j = (dgate_j - dot) / S with dot a k-term f32 sum (error
                      <= k 2^-24 sum |dgate gate|), S a k-term f32 sum (relative error <= k 2^-24), one subtraction and one division
                      (2^-24 each), then at most k such terms added: (k + 3) 2^-24 <= k 2^-22 for every k >= 1.
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests import moe_ref as M
from tests import poison as P

pytestmark = pytest.mark.gpu

CODE = {"f32": H.F32, "bf16": H.BF16, "f16": H.F16}
DTS = ("bf16", "f16", "f32")


class Win:
    """[rows, cols] of dt at leading dimension ld, `off` elements into a device buffer allocated under the poison patch, with a guard
    band behind it. Everything outside the window holds the pattern before the call and must hold it afterwards."""

    def __init__(self, dt, rows, cols, ld=None, off=0, byte=0, slack_rows=0):
        self.dt, self.rows, self.cols, self.ld, self.off, self.byte = dt, rows, cols, cols if ld is None else ld, off, byte
        self.es = V.ES[dt]
        self.n = off + (rows + slack_rows) * self.ld + 16
        self.buf = P.guarded(self.n * self.es)

    def idx(self):
        return self.off + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]

    def image(self):
        return np.full(self.n * self.es, self.byte, dtype=np.uint8).view(V.STORE[self.dt] if self.dt != "f32" else np.uint32)

    def put(self, values=None, bits=None):
        img = self.image()
        img[self.idx()] = V.encode(values, self.dt).view(img.dtype) if bits is None else bits
        H.check(H.lib().kf_memcpy_h2d(self.buf.ptr, img.ctypes.data, img.nbytes, None))
        return self

    @property
    def ptr(self):
        return self.buf.ptr + self.off * self.es

    def bits(self):
        """The window's bits; asserts that nothing else was written."""
        img = self.image()
        after = self.buf.to_numpy(img.shape, img.dtype)
        mask = np.ones(after.shape, bool)
        mask[self.idx()] = False
        assert np.array_equal(after[mask], img[mask]), "bytes outside the window were written"
        assert P.guard_intact(self.buf, self.n * self.es, self.byte), "the guard band was written"
        return after[self.idx()]


def as_bits(values, dt):
    e = V.encode(values, dt)
    return e.view(np.uint32) if dt == "f32" else e


def dev_ints(a, dtype):
    return H.DevBuf.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def draw_ids(rng, T, k, E, bad_every=0):
    ids = rng.integers(0, E, (T, k)).astype(np.int64)
    if bad_every:
        flat = ids.reshape(-1)
        bad = [E if b is None else b for b in M.BAD_IDS]
        for i in range(1, flat.size, bad_every):
            flat[i] = bad[(i // bad_every) % len(bad)]
    return ids


def rounded(rng, shape, dt, lo=-1.0, hi=1.0):
    return M.rnd(rng.uniform(lo, hi, shape), dt)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------
def run_plan(ids, E):
    T, k = ids.shape
    n = T * k
    d_ids = dev_ints(ids, np.int64)
    off, rp, pr = P.guarded(8 * (E + 1)), P.guarded(4 * n), P.guarded(4 * n)
    need = H.moe_plan_workspace_bytes(T, k, E)
    ws = P.guarded(need)
    out = []
    for _ in range(2):   # twice into the same buffers and the same scratch: the same bits
        H.moe_plan(d_ids.ptr, T, k, E, off.ptr, rp.ptr, pr.ptr, ws.ptr if need else None, need)
        H.device_sync()
        out.append((off.to_numpy(E + 1, np.int64), rp.to_numpy(n, np.int32), pr.to_numpy(n, np.int32)))
    return out, (off, 8 * (E + 1)), (rp, 4 * n), (pr, 4 * n), (ws, need)


@pytest.mark.parametrize("T,k,E,bad_every", [(96, 2, 8, 0), (4096, 2, 8, 0), (8193, 1, 8, 0), (4099, 3, 128, 0), (40000, 1, 1, 0), (301, 3, 5, 3), (8193, 1, 300, 5),
                                             (0, 2, 4, 0)])
def test_plan_is_the_reference_bit_for_bit(monkeypatch, T, k, E, bad_every):
    rng = np.random.default_rng(T + 7 * k + E)
    ids = draw_ids(rng, T, k, E, bad_every)
    want = M.plan(ids, E)
    if bad_every:
        assert want[0][E] < T * k
    for byte in P.PATTERNS:
        P.poisoned_allocations(monkeypatch, byte)
        (first, second), *guards = run_plan(ids, E)
        for name, got, again, ref in zip(("offsets", "row_pair", "pair_row"), first, second, want):
            assert np.array_equal(got, ref), (name, hex(byte))
            assert np.array_equal(again, got), (name, "second run", hex(byte))
        for buf, nbytes in guards:
            assert P.guard_intact(buf, nbytes, byte), hex(byte)


# ---- dispatch, combine, combine_bwd ----------------------------------------------------------------------------------------------------------
# (cols, ld, off, k): 128 and 136 / 144 move 16-byte packs, 40 / 41 and 2 and an odd base take the element path; beyond 1024 columns a block
# walks the row (1160: packs; 1030 / 1031: elements, with a tail; 2312: more than one span per lane); k = 11 takes a second
# chunk of pairs
SHAPES = [(128, 128, 0, 2), (128, 128, 0, 8), (136, 144, 0, 3), (40, 41, 0, 1), (2, 2, 0, 8), (128, 128, 1, 3), (1160, 1160, 0, 2), (1030, 1031, 0, 3),
          (136, 144, 0, 11), (1160, 1168, 0, 11), (2312, 2320, 0, 2)]
T_MOVE, E_MOVE = 37, 6


def move_case(dt, cols, k, seed):
    rng = np.random.default_rng(seed)
    T, E = T_MOVE, E_MOVE
    ids = draw_ids(rng, T, k, E, bad_every=5)
    offsets, row_pair, pair_row = M.plan(ids, E)
    n, nv = T * k, int(offsets[E])
    x, ys, dy = rounded(rng, (T, cols), dt), rounded(rng, (n, cols), dt), rounded(rng, (T, cols), dt)
    gate = rounded(rng, (T, k), dt, 0.1, 1.0)
    dropped = pair_row.reshape(T, k) >= nv
    assert dropped.any() and nv > 0
    return dict(T=T, k=k, E=E, n=n, nv=nv, ids=ids, offsets=offsets, row_pair=row_pair, pair_row=pair_row, x=x, ys=ys, dy=dy, gate=gate, dropped=dropped)


def run_moves(dt, cols, ld, off, c, byte, with_gate=True):
    """One pass of the three entries on poisoned buffers; returns the outputs' bits."""
    T, k, n, code = c["T"], c["k"], c["n"], CODE[dt]
    row_pair, pair_row = c["row_pair"], c["pair_row"]
    d_rp, d_pr, d_off = dev_ints(row_pair, np.int32), dev_ints(pair_row, np.int32), dev_ints(c["offsets"], np.int64)
    n_valid = d_off.ptr + 8 * c["E"]
    w = lambda rows, width, ld_=None, off_=0: Win(dt, rows, width, ld_, off_, byte)  # noqa: E731
    # the rows and gates of dropped pairs are NaN: nothing may read them
    ys, gate = c["ys"].copy(), c["gate"].copy()
    ys[c["nv"]:] = np.nan
    gate[c["dropped"]] = np.nan
    X, XS = w(T, cols, ld, off).put(c["x"]), w(n, cols, ld, off)
    YS, Y = w(n, cols, ld, off).put(ys), w(T, cols, ld, off)
    DY, DYS = w(T, cols, ld, off).put(c["dy"]), w(n, cols, ld, off)
    G, DG = w(T, k, k + 3, 1).put(gate), w(T, k, k + 1, 0)
    H.moe_dispatch(code, T, k, cols, d_rp.ptr, X.ptr, X.ld, XS.ptr, XS.ld)
    H.moe_combine(code, T, k, cols, d_pr.ptr, n_valid, G.ptr if with_gate else None, G.ld, YS.ptr, YS.ld, Y.ptr, Y.ld)
    H.moe_combine_bwd(code, T, k, cols, d_pr.ptr, n_valid, G.ptr if with_gate else None, G.ld, YS.ptr if with_gate else None, YS.ld, DY.ptr, DY.ld,
                      DYS.ptr, DYS.ld, DG.ptr if with_gate else None, DG.ld)
    H.device_sync()
    return dict(xs=XS.bits(), y=Y.bits(), dys=DYS.bits(), dgate=DG.bits() if with_gate else None)


def floats(bits, dt):
    return V.decode(bits.view(np.float32) if dt == "f32" else bits, dt)


@pytest.mark.parametrize("cols,ld,off,k", SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_dispatch_combine_and_backward(monkeypatch, dt, cols, ld, off, k):
    c = move_case(dt, cols, k, cols * 31 + k)
    T, n, nv = c["T"], c["n"], c["nv"]
    runs = []
    for byte in P.PATTERNS:
        P.poisoned_allocations(monkeypatch, byte)
        runs.append(run_moves(dt, cols, ld, off, c, byte))
    got = runs[0]
    for other, byte in zip(runs[1:], P.PATTERNS[1:]):
        for name in got:
            assert np.array_equal(other[name], got[name]), (name, hex(byte))
    # dispatch
    assert np.array_equal(got["xs"], as_bits(M.dispatch(c["x"], c["row_pair"], k), dt))
    # combine
    y = floats(got["y"], dt)
    assert not np.isnan(y).any()
    if dt == "f32":
        ref, mag = M.combine(c["ys"], c["pair_row"], nv, c["gate"], T, k, dt, exact=True)
        lim = k * 2.0 ** -23 * mag
        print(f"y f32: max excess over the bound {(np.abs(y - ref) - lim).max():.3e}")
        assert (np.abs(y - ref) <= lim).all()
    else:
        ref, _ = M.combine(c["ys"], c["pair_row"], nv, c["gate"], T, k, dt)
        assert np.array_equal(got["y"], as_bits(ref, dt))
    # combine_bwd: the rows of dropped pairs and their dgate are +0 bit for bit
    dys, dgate, mag = M.combine_bwd(c["ys"], c["pair_row"], nv, c["gate"], c["dy"], T, k, dt, exact=False)
    assert not np.isnan(dys).any()
    assert np.array_equal(got["dys"], as_bits(dys, dt))
    assert not got["dys"][nv:].any() and not got["dgate"][c["dropped"]].any()
    gd = floats(got["dgate"], dt)
    lim = M.H[dt] * np.abs(dgate) + cols * 2.0 ** -23 * mag
    print(f"dgate {dt}: max excess over the bound {(np.abs(gd - dgate) - lim).max():.3e}")
    assert (np.abs(gd - dgate) <= lim).all()


@pytest.mark.parametrize("cols,ld,off,k", [(128, 128, 0, 2), (40, 41, 0, 3), (1160, 1160, 0, 8)])
@pytest.mark.parametrize("dt", DTS)
def test_without_a_gate(monkeypatch, dt, cols, ld, off, k):
    """gate == NULL: the combine is the dispatch's backward (a plain sum in the order j), and dys is dy bit for bit."""
    c = move_case(dt, cols, k, cols + k)
    P.poisoned_allocations(monkeypatch, 0xFF)
    got = run_moves(dt, cols, ld, off, c, 0xFF, with_gate=False)
    if dt == "f32":
        ref, mag = M.combine(c["ys"], c["pair_row"], c["nv"], None, c["T"], k, dt, exact=True)
        assert (np.abs(floats(got["y"], dt) - ref) <= k * 2.0 ** -23 * mag).all()
    else:
        ref, _ = M.combine(c["ys"], c["pair_row"], c["nv"], None, c["T"], k, dt)
        assert np.array_equal(got["y"], as_bits(ref, dt))
    dys, _, _ = M.combine_bwd(None, c["pair_row"], c["nv"], None, c["dy"], c["T"], k, dt, want_dgate=False)
    assert np.array_equal(got["dys"], as_bits(dys, dt))


def test_n_valid_null_means_every_row(monkeypatch):
    dt, cols, k = "bf16", 128, 2
    c = move_case(dt, cols, k, 9)
    P.poisoned_allocations(monkeypatch, 0x7F)
    T, n = c["T"], c["n"]
    d_pr = dev_ints(c["pair_row"], np.int32)
    YS, Y, G = Win(dt, n, cols, byte=0x7F).put(c["ys"]), Win(dt, T, cols, byte=0x7F), Win(dt, T, k, byte=0x7F).put(c["gate"])
    H.moe_combine(CODE[dt], T, k, cols, d_pr.ptr, None, G.ptr, G.ld, YS.ptr, YS.ld, Y.ptr, Y.ld)
    H.device_sync()
    ref, _ = M.combine(c["ys"], c["pair_row"], None, c["gate"], T, k, dt)
    assert np.array_equal(Y.bits(), as_bits(ref, dt))
    # a count beyond n, or below 0, is clamped by the kernel
    for count, live in ((n + 1000, n), (-3, 0)):
        d_nv = dev_ints(np.array([count]), np.int64)
        H.moe_combine(CODE[dt], T, k, cols, d_pr.ptr, d_nv.ptr, G.ptr, G.ld, YS.ptr, YS.ld, Y.ptr, Y.ld)
        H.device_sync()
        ref, _ = M.combine(c["ys"], c["pair_row"], live, c["gate"], T, k, dt)
        assert np.array_equal(Y.bits(), as_bits(ref, dt)), count


def test_malformed_tables_touch_no_memory(monkeypatch):
    """Table entries of n + 3 and -5 name no row: nothing is read or written for them. ys and dys live in allocations twice their size
    whose upper half holds the pattern (what an entry of n + 3 would reach): it stays, and the results are the reference's."""
    dt, cols, k, byte = "bf16", 128, 2, 0x7F
    c = move_case(dt, cols, k, 4)
    T, n, nv, code = c["T"], c["n"], c["nv"], CODE[dt]
    row_pair, pair_row = c["row_pair"].copy(), c["pair_row"].copy()
    row_pair[[1, 7]] = n + 3, -5
    pair_row[[0, 9, 20]] = n + 3, -5, n
    P.poisoned_allocations(monkeypatch, byte)
    d_rp, d_pr, d_off = dev_ints(row_pair, np.int32), dev_ints(pair_row, np.int32), dev_ints(c["offsets"], np.int64)
    X, XS = Win(dt, T, cols, byte=byte).put(c["x"]), Win(dt, n, cols, byte=byte)
    YS, DYS = Win(dt, n, cols, byte=byte, slack_rows=n).put(c["ys"]), Win(dt, n, cols, byte=byte, slack_rows=n)
    Y, DY, G, DG = Win(dt, T, cols, byte=byte), Win(dt, T, cols, byte=byte).put(c["dy"]), Win(dt, T, k, byte=byte).put(c["gate"]), Win(dt, T, k, byte=byte)
    H.moe_dispatch(code, T, k, cols, d_rp.ptr, X.ptr, X.ld, XS.ptr, XS.ld)
    H.moe_combine(code, T, k, cols, d_pr.ptr, d_off.ptr + 8 * c["E"], G.ptr, G.ld, YS.ptr, YS.ld, Y.ptr, Y.ld)
    H.moe_combine_bwd(code, T, k, cols, d_pr.ptr, d_off.ptr + 8 * c["E"], G.ptr, G.ld, YS.ptr, YS.ld, DY.ptr, DY.ld, DYS.ptr, DYS.ld, DG.ptr, DG.ld)
    H.device_sync()
    xs = XS.bits()
    assert np.array_equal(xs, as_bits(M.dispatch(c["x"], row_pair, k), dt)) and not xs[[1, 7]].any()
    ref, _ = M.combine(c["ys"], pair_row, nv, c["gate"], T, k, dt)
    assert np.array_equal(Y.bits(), as_bits(ref, dt))
    YS.bits()                                              # (asserts that the upper half and the guard still hold the pattern)
    got = DYS.bits()                                       # likewise
    dys, dgate, mag = M.combine_bwd(c["ys"], pair_row, nv, c["gate"], c["dy"], T, k, dt)
    named = ~np.isnan(dys).any(axis=1)
    assert (~named).sum() == 3                             # the rows whose pairs now name nothing keep the pattern
    assert np.array_equal(got[named], as_bits(dys[named], dt))
    assert (got[~named].view(np.uint8) == byte).all()
    gd = floats(DG.bits(), dt)
    assert (np.abs(gd - dgate) <= M.H[dt] * np.abs(dgate) + cols * 2.0 ** -23 * mag).all()
    assert gd.reshape(-1)[0] == 0 and gd.reshape(-1)[9] == 0 and gd.reshape(-1)[20] == 0


# ---- the gate --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,k,E,ldp", [(37, 2, 8, 8), (200, 8, 128, 128), (5, 1, 1, 1), (33, 3, 70, 73), (64, 11, 16, 16)])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("dt", DTS)
def test_gate_forward_and_backward(monkeypatch, dt, normalize, T, k, E, ldp):
    rng = np.random.default_rng(T + k + E)
    ids = draw_ids(rng, T, k, E, bad_every=7 if T * k > 7 else 0)
    if T > 20:
        ids[3, : min(k, 2)] = ids[3, 0]                  # a token that chooses one expert twice
    p, dgate = rounded(rng, (T, E), dt, 0.05, 1.0), rounded(rng, (T, k), dt)
    code = CODE[dt]
    runs = []
    for byte in P.PATTERNS:
        P.poisoned_allocations(monkeypatch, byte)
        d_ids = dev_ints(ids, np.int64)
        Pw, G = Win(dt, T, E, ldp, 0, byte).put(p), Win(dt, T, k, k + 2, 1, byte)
        H.moe_gate_fwd(code, T, k, E, d_ids.ptr, Pw.ptr, Pw.ld, normalize, G.ptr, G.ld)
        H.device_sync()
        gate_bits = G.bits()
        DGw, DP = Win(dt, T, k, k, 0, byte).put(dgate), Win(dt, T, E, ldp, 0, byte)
        H.moe_gate_bwd(code, T, k, E, d_ids.ptr, Pw.ptr, Pw.ld, normalize, G.ptr, G.ld, DGw.ptr, DGw.ld, DP.ptr, DP.ld)
        H.device_sync()
        runs.append((gate_bits, DP.bits()))
    for other in runs[1:]:
        assert np.array_equal(other[0], runs[0][0]) and np.array_equal(other[1], runs[0][1])
    gate_bits, dp_bits = runs[0]
    gate, dp = floats(gate_bits, dt), floats(dp_bits, dt)
    ok = (ids >= 0) & (ids < E)
    if not normalize:
        assert np.array_equal(gate_bits, as_bits(M.gate_fwd(p, ids, E, False, dt), dt))
    else:
        ref = M.gate_fwd(p, ids, E, True, dt, exact=True)
        assert np.isfinite(ref).all()                    # every token keeps a live pair here
        assert (np.abs(gate - ref) <= (M.H[dt] + 2.0 ** -21) * np.abs(ref)).all()
    assert not gate_bits[~ok].any()                      # a dropped pair's gate is +0
    # the backward from the device's stored gate
    ref = M.gate_bwd(p, ids, E, normalize, gate, dgate, dt, exact=True)
    s = np.where(ok, np.take_along_axis(p, np.where(ok, ids, 0), 1), 0.0)
    m = np.abs(dgate) if not normalize else (np.abs(dgate) + (np.abs(dgate * gate) * ok).sum(1, keepdims=True)) / s.sum(1, keepdims=True)
    mag, chosen = np.zeros((T, E)), np.zeros((T, E), bool)
    for j in range(k):
        rows = np.flatnonzero(ok[:, j])
        np.add.at(mag, (rows, ids[rows, j]), m[rows, j])
        chosen[rows, ids[rows, j]] = True
    lim = M.H[dt] * np.abs(ref) + k * 2.0 ** -22 * mag
    print(f"dp {dt} normalize={normalize}: max excess over the bound {(np.abs(dp - ref) - lim).max():.3e}")
    assert (np.abs(dp - ref) <= lim).all()
    assert not dp_bits[~chosen].any()                    # exactly zero off the chosen columns


# ---- the operators ---------------------------------------------------------------------------------------------------------------------------
def to_t(vals, dt, requires_grad=False):
    if dt == "bf16":
        t = kfunca.from_numpy_bf16(np.ascontiguousarray(V.encode(vals, "bf16")), 0)
    else:
        t = kfunca.from_numpy(np.ascontiguousarray(vals, dtype=np.float32), 0)
    t.set_requires_grad(requires_grad)
    return t


def bits_of(t, dt):
    a = np.ascontiguousarray(t.numpy())
    return a.view(np.uint16) if dt == "bf16" else a.view(np.uint32)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_operators_equal_the_abi(monkeypatch, dt):
    cols, k = 136, 3
    c = move_case(dt, cols, k, 77)
    T, E, n, nv, ids = c["T"], c["E"], c["n"], c["nv"], c["ids"]
    rng = np.random.default_rng(1)
    P.poisoned_allocations(monkeypatch, 0x00)   # the ABI side's buffers (Win) check their surroundings against the pattern
    plan = kfunca.moe_plan(kfunca.from_numpy(ids, 0), E)
    assert (plan.T, plan.k, plan.E) == (T, k, E) and plan.pair_row.sizes() == [T, k] and plan.row_pair.sizes() == [n]
    assert np.array_equal(plan.offsets.numpy(), c["offsets"]) and np.array_equal(plan.row_pair.numpy(), c["row_pair"])
    assert np.array_equal(plan.pair_row.numpy().reshape(-1), c["pair_row"]) and np.array_equal(plan.ids.numpy(), ids)
    code = CODE[dt]
    d_pr, d_off, d_ids = dev_ints(c["pair_row"], np.int32), dev_ints(c["offsets"], np.int64), dev_ints(ids, np.int64)

    def abi(values, rows, width):
        return Win(dt, rows, width).put(values)

    # dispatch and its backward; a row-pitched x is read in place
    wide = rounded(rng, (T, cols + 24), dt)
    tx = to_t(wide, dt, True)
    xs = kfunca.moe_dispatch(tx[:, 16:16 + cols], plan)
    assert np.array_equal(bits_of(xs, dt), as_bits(M.dispatch(wide[:, 16:16 + cols], c["row_pair"], k), dt))
    dxs = rounded(rng, (n, cols), dt)
    xs.backward(to_t(dxs, dt))
    DXS, DX = abi(dxs, n, cols), Win(dt, T, cols)
    H.moe_combine(code, T, k, cols, d_pr.ptr, None, None, 0, DXS.ptr, DXS.ld, DX.ptr, DX.ld)
    H.device_sync()
    assert np.array_equal(bits_of(tx.grad(), dt)[:, 16:16 + cols], DX.bits()) and not bits_of(tx.grad(), dt)[:, :16].any()

    # gate and its backward
    p, dgate = rounded(rng, (T, E), dt, 0.05, 1.0), rounded(rng, (T, k), dt)
    tp = to_t(p, dt, True)
    gate = kfunca.moe_gate(tp, plan, True)
    Pw, G, DGw, DP = abi(p, T, E), Win(dt, T, k), abi(dgate, T, k), Win(dt, T, E)
    H.moe_gate_fwd(code, T, k, E, d_ids.ptr, Pw.ptr, Pw.ld, 1, G.ptr, G.ld)
    H.moe_gate_bwd(code, T, k, E, d_ids.ptr, Pw.ptr, Pw.ld, 1, G.ptr, G.ld, DGw.ptr, DGw.ld, DP.ptr, DP.ld)
    H.device_sync()
    assert np.array_equal(bits_of(gate, dt), G.bits())
    gate.backward(to_t(dgate, dt))
    assert np.array_equal(bits_of(tp.grad(), dt), DP.bits())

    # combine and its backward in ys and gate
    tys, tg = to_t(c["ys"], dt, True), to_t(c["gate"], dt, True)
    y = kfunca.moe_combine(tys, plan, tg)
    YS, Y, Gw = abi(c["ys"], n, cols), Win(dt, T, cols), abi(c["gate"], T, k)
    DY, DYS, DG = abi(c["dy"], T, cols), Win(dt, n, cols), Win(dt, T, k)
    H.moe_combine(code, T, k, cols, d_pr.ptr, d_off.ptr + 8 * E, Gw.ptr, Gw.ld, YS.ptr, YS.ld, Y.ptr, Y.ld)
    H.moe_combine_bwd(code, T, k, cols, d_pr.ptr, d_off.ptr + 8 * E, Gw.ptr, Gw.ld, YS.ptr, YS.ld, DY.ptr, DY.ld, DYS.ptr, DYS.ld, DG.ptr, DG.ld)
    H.device_sync()
    assert np.array_equal(bits_of(y, dt), Y.bits())
    y.backward(to_t(c["dy"], dt))
    assert np.array_equal(bits_of(tys.grad(), dt), DYS.bits()) and np.array_equal(bits_of(tg.grad(), dt), DG.bits())
    # without a gate, and with a gate that needs no gradient
    tys2 = to_t(c["ys"], dt, True)
    y2 = kfunca.moe_combine(tys2, plan)
    ref, _ = M.combine(c["ys"], c["pair_row"], nv, None, T, k, dt)
    if dt == "bf16":
        assert np.array_equal(bits_of(y2, dt), as_bits(ref, dt))
    y2.backward(to_t(c["dy"], dt))
    dys, _, _ = M.combine_bwd(None, c["pair_row"], nv, None, c["dy"], T, k, dt, want_dgate=False)
    assert np.array_equal(bits_of(tys2.grad(), dt), as_bits(dys, dt))
    tys3, tg3 = to_t(c["ys"], dt, True), to_t(c["gate"], dt)
    kfunca.moe_combine(tys3, plan, tg3).backward(to_t(c["dy"], dt))
    assert np.array_equal(bits_of(tys3.grad(), dt), DYS.bits()) and not tg3.requires_grad()


def test_operators_refuse():
    T, k, E, d = 8, 2, 4, 16
    rng = np.random.default_rng(0)
    ids = kfunca.from_numpy(rng.integers(0, E, (T, k)).astype(np.int64), 0)
    plan = kfunca.moe_plan(ids, E)
    f32 = lambda *shape: kfunca.from_numpy(np.zeros(shape, np.float32), 0)  # noqa: E731
    assert kfunca.moe_dispatch(f32(T, d), plan).sizes() == [T * k, d] and kfunca.moe_combine(f32(T * k, d), plan, f32(T, k)).sizes() == [T, d]
    assert kfunca.moe_gate(f32(T, E), plan).sizes() == [T, k]
    other = kfunca.moe_plan(kfunca.from_numpy(rng.integers(0, E, (T, k + 1)).astype(np.int64), 0), E)
    bad = [
        lambda: kfunca.moe_plan(kfunca.from_numpy(np.zeros((T, k), np.int32), 0), E),          # ids are Long
        lambda: kfunca.moe_plan(kfunca.from_numpy(np.zeros(T * k, np.int64), 0), E),            # [T, k]
        lambda: kfunca.moe_plan(ids, 0),
        lambda: kfunca.moe_dispatch(f32(T + 1, d), plan),                                        # another T
        lambda: kfunca.moe_dispatch(f32(T, d, 1), plan),                                         # rank
        lambda: kfunca.moe_dispatch(kfunca.from_numpy(np.zeros((T, d), np.float64), 0), plan),  # dtype
        lambda: kfunca.moe_dispatch(f32(T, d), ids),                                             # not a plan
        lambda: kfunca.moe_combine(f32(T * k, d), other),                                        # a plan of another k
        lambda: kfunca.moe_combine(f32(T * k, d), plan, f32(T, k + 1)),
        lambda: kfunca.moe_combine(f32(T * k, d), plan, f32(T, k).bfloat16()),
        lambda: kfunca.moe_combine(f32(T * k + 1, d), plan),
        lambda: kfunca.moe_gate(f32(T, E + 1), plan),                                            # another E
        lambda: kfunca.moe_gate(f32(T + 1, E), plan),
        lambda: kfunca.moe_gate(kfunca.from_numpy(np.zeros((T, E), np.int64), 0), plan),
    ]
    for i, call in enumerate(bad):
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            call()
            pytest.fail(f"case {i} was accepted")
    with pytest.raises(AttributeError):
        plan.pair_row = plan.row_pair          # the tables are read-only
