"""-m gpu: the fused per-head QK-norm + rotary embedding (kf_qk_norm_rope_fwd / _bwd, kfunca.qk_norm_rope) against the f64 numpy reference
of tests/qk_norm_ref.py on the same stored inputs, against torch-CPU autograd, through attention end to end, and against the composition
of today's rms_norm and rope.

Bounds (tests/qk_norm_ref.py derives them; r = one output rounding: 2^-8 bf16, 2^-11 f16, 0 f32; r |ref| is at least half the subnormal
spacing of the type, 2^-25 in f16):
  forward   |got - ref| <= r |ref| + 2^-20 (|n_a| + |n_b|); v heads bit-exact
  dx        r |ref| + 2^-20 rstd (|gw_d| + |xhat_d| mean_d |gw xhat|)
  dw        r |ref| + (N + 8) 2^-24 sum |g_d xhat_d| over the N (token, head) rows summed
  end to end (gemm -> qk_norm_rope -> attention_qkv -> sum), as tests/test_gpu_rope.py states for its model: f32 loss 1e-5 relative,
            gradients rtol 1e-3 / atol 1e-5; bf16 operands: loss 2e-2 relative, gradients 6 % of each tensor's max |grad|
  composition (f32)  rms_norm's stated forward bound (rtol = atol = 1e-5, tests/test_gpu_norm.py) on both elements of a pair, carried through
            the rotation, plus rope's 2^-22 (|n_a| + |n_b|) (tests/test_gpu_rope.py)
Bitwise: pack and element access on the same lane map, in place and out of place, repeated runs, poisoned scratch and outputs, graph replay.
Every test prints the worst fraction of each bound it met (pytest -s shows them).
"""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests import poison
from tests import qk_norm_ref as R
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

NAME = {H.BF16: "bf16", H.F16: "f16", H.F32: "f32"}
NP = {H.BF16: np.uint16, H.F16: np.float16, H.F32: np.float32}
ES = {H.BF16: 2, H.F16: 2, H.F32: 4}
PAD = 0xA5   # what the columns W .. ld and the buffers behind an output hold before a call


def tables(P, rot, base=10000.0):
    if rot == 0:
        return None, None
    i = np.arange(rot // 2, dtype=np.float64)
    th = np.arange(P, dtype=np.float64)[:, None] * base ** (-2 * i / rot)[None, :]
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


def store(vals, code):
    return O.from_float(np.asarray(vals, np.float32), code)


def fl(a, code):
    return O.to_float(np.ascontiguousarray(a), code).astype(np.float64)


class Case:
    """One geometry with its weights, tables and positions on the host (storage arrays) and on the device."""

    def __init__(self, code, B, S, Hq, Hk, Hv, D, rot, interleaved=False, P=64, pos=None, wq=True, wk=True, eps=1e-6, seed=0):
        self.code, self.B, self.S, self.Hq, self.Hk, self.Hv, self.D, self.rot = code, B, S, Hq, Hk, Hv, D, rot
        self.interleaved, self.eps, self.P = interleaved, eps, P
        self.T, self.W = B * S, (Hq + Hk + Hv) * D
        rng = np.random.default_rng(seed)
        self.wq = store(rng.uniform(0.5, 1.5, D), code) if wq else None
        self.wk = store(rng.uniform(-1.5, 1.5, D), code) if wk else None
        self.cos, self.sin = tables(P, rot)
        self.pos = None if pos is None else np.asarray(pos, np.int64)
        up = lambda a: None if a is None else H.DevBuf.from_numpy(a)  # noqa: E731
        self.d_wq, self.d_wk, self.d_cos, self.d_sin, self.d_pos = up(self.wq), up(self.wk), up(self.cos), up(self.sin), up(self.pos)
        self.rng = rng

    def ref_args(self):
        f = lambda w: None if w is None else fl(w, self.code)  # noqa: E731
        return (f(self.wq), f(self.wk), self.cos, self.sin, self.pos, self.B, self.S, self.Hq, self.Hk, self.Hv, self.D, self.rot, self.interleaved,
                self.eps)

    def geom(self):
        return (self.code, self.B, self.S, self.Hq, self.Hk, self.Hv, self.D)

    def common(self):
        p = lambda b: b.ptr if b is not None else None  # noqa: E731
        return dict(wq=p(self.d_wq), wk=p(self.d_wk), cos=p(self.d_cos), sin=p(self.d_sin), table_rows=self.P if self.rot else 0, rotary_dim=self.rot,
                    positions=p(self.d_pos), interleaved=self.interleaved, eps=self.eps)

    def values(self, scale=2.0):
        """[T, W] storage of random values and their f64 floats."""
        s = store(self.rng.uniform(-scale, scale, (self.T, self.W)), self.code)
        return s, fl(s, self.code)


def padded(vals, ld, code, shift=0):
    """The [T, W] storage `vals` as rows of ld elements behind `shift` elements, everything else holding the PAD byte."""
    T, W = vals.shape
    flat = np.frombuffer(bytes([PAD]) * ((shift + T * ld) * ES[code]), dtype=NP[code]).copy()
    rows = flat[shift:].reshape(T, ld)
    rows[:, :W] = vals
    return flat


def out_buffer(T, ld, code, shift=0, fill=True):
    b = H.DevBuf((shift + T * ld) * ES[code] + poison.GUARD)
    if fill:
        poison.fill(b.ptr, b.nbytes, PAD)
    return b


def read(buf, T, ld, W, code, shift=0, pad=PAD):
    """-> the [T, W] storage of a result; asserts that nothing else of the buffer (pad columns, the shift, the guard band) was written."""
    raw = buf.to_numpy((buf.nbytes,), np.uint8)
    n = (shift + T * ld) * ES[code]
    rows = raw[shift * ES[code]:n].view(NP[code]).reshape(T, ld)
    if pad is not None:
        assert (raw[:shift * ES[code]] == pad).all() and (raw[n:] == pad).all(), "bytes around the result were written"
        assert (rows[:, W:].view(np.uint8) == pad).all(), "columns W .. ld were written"
    return rows[:, :W].copy()


def run_fwd(c, xs, ld=None, shift=0, in_place=False, stream=None, fill=True, pad=PAD):
    ld = c.W if ld is None else ld
    es = ES[c.code]
    bx = H.DevBuf.from_numpy(padded(xs, ld, c.code, shift))
    if in_place:
        H.qk_norm_rope_fwd(*c.geom(), bx.ptr + shift * es, ld, None, None, stream=stream, **c.common())
        H.device_sync()
        rows = bx.to_numpy(((shift + c.T * ld),), NP[c.code])[shift:].reshape(c.T, ld)
        assert (rows[:, c.W:].view(np.uint8) == PAD).all(), "in place: columns W .. ld were written"
        return rows[:, :c.W].copy()
    by = out_buffer(c.T, ld, c.code, shift, fill)
    H.qk_norm_rope_fwd(*c.geom(), bx.ptr + shift * es, ld, by.ptr + shift * es, ld, stream=stream, **c.common())
    H.device_sync()
    return read(by, c.T, ld, c.W, c.code, shift, pad)


def run_bwd(c, xs, dys, ld=None, shift=0, in_place=False, want=(True, True), fill=True, pad=PAD):
    """-> (dx [T, W], dwq [D] or None, dwk [D] or None) storage."""
    ld = c.W if ld is None else ld
    es = ES[c.code]
    bx, bg = H.DevBuf.from_numpy(padded(xs, ld, c.code, shift)), H.DevBuf.from_numpy(padded(dys, ld, c.code, shift))
    bq = out_buffer(1, c.D, c.code, 0, fill) if want[0] else None
    bk = out_buffer(1, c.D, c.code, 0, fill) if want[1] else None
    kw = dict(dwq=bq.ptr if bq else None, dwk=bk.ptr if bk else None, **c.common())
    if in_place:
        ws = H.qk_norm_rope_bwd(*c.geom(), bx.ptr + shift * es, ld, bg.ptr + shift * es, ld, None, None, **kw)
        H.device_sync()
        rows = bg.to_numpy(((shift + c.T * ld),), NP[c.code])[shift:].reshape(c.T, ld)
        assert (rows[:, c.W:].view(np.uint8) == PAD).all(), "in place: columns W .. ld were written"
        dx = rows[:, :c.W].copy()
    else:
        bd = out_buffer(c.T, ld, c.code, shift, fill)
        ws = H.qk_norm_rope_bwd(*c.geom(), bx.ptr + shift * es, ld, bg.ptr + shift * es, ld, bd.ptr + shift * es, ld, **kw)
        H.device_sync()
        dx = read(bd, c.T, ld, c.W, c.code, shift, pad)
    del ws
    dq = read(bq, 1, c.D, c.D, c.code, 0, pad)[0] if bq else None
    dk = read(bk, 1, c.D, c.D, c.code, 0, pad)[0] if bk else None
    return dx, dq, dk


FRACTIONS = {}


def check(what, got, ref, tol, code):
    ok, frac = R.within(fl(got, code), ref, tol, R.ROUNDING[NAME[code]], R.SUBNORMAL_ROUNDING[NAME[code]])
    FRACTIONS[what] = max(FRACTIONS.get(what, 0.0), frac)
    print(f"{what}: worst fraction of the bound {frac:.3f}")
    assert ok, (what, frac)


def check_all(c, xs, x, dys, dy, got_y, got_b, tag):
    nv = (c.Hq + c.Hk) * c.D
    y, tol = R.forward(x, *c.ref_args())
    check(f"forward {NAME[c.code]}", got_y, y, tol, c.code)
    assert np.array_equal(got_y[:, nv:], xs[:, nv:]), f"{tag}: v heads are not the input's bits"
    rb = R.backward(x, dy, *c.ref_args())
    dx, dq, dk = got_b
    check(f"dx {NAME[c.code]}", dx, rb["dx"], rb["dx_tol"], c.code)
    assert np.array_equal(dx[:, nv:], dys[:, nv:]), f"{tag}: dx of the v heads is not dy's bits"
    if dq is not None:
        check(f"dw {NAME[c.code]}", dq, rb["dwq"], rb["dwq_tol"], c.code)
    if dk is not None:
        check(f"dw {NAME[c.code]}", dk, rb["dwk"], rb["dwk_tol"], c.code)


@pytest.mark.parametrize("code", [H.F32, H.BF16, H.F16])
@pytest.mark.parametrize("D", [64, 128, 80, 256])
@pytest.mark.parametrize("rsel", ["D", "D/2", "32", "0"])
def test_parity_with_f64(code, D, rsel):
    """Each (dtype, D, R): both pair conventions x the three leading dimensions, with and without positions in turn."""
    rot = {"D": D, "D/2": D // 2, "32": 32, "0": 0}[rsel]
    B, S, Hq, Hk, Hv = 2, 19, 5, 2, 2
    W = (Hq + Hk + Hv) * D
    n = 0
    for interleaved in (False, True):
        for ld in (W, W + 24, W + 3):
            n += 1
            rng = np.random.default_rng(D * 7 + rot + n + code)
            pos = rng.integers(0, 64, B * S) if n % 2 else None
            c = Case(code, B, S, Hq, Hk, Hv, D, rot, interleaved, pos=pos, seed=D + rot + n)
            (xs, x), (dys, dy) = c.values(), c.values()
            check_all(c, xs, x, dys, dy, run_fwd(c, xs, ld), run_bwd(c, xs, dys, ld), f"il {interleaved} ld {ld}")


@pytest.mark.parametrize("code", [H.F32, H.BF16])
@pytest.mark.parametrize("heads,wq,wk", [((5, 2, 2), False, True), ((5, 2, 2), True, False), ((5, 2, 2), False, False), ((4, 0, 0), True, True),
                                         ((0, 3, 1), True, True), ((3, 1, 0), True, True)])
def test_missing_weights_and_missing_kinds_of_heads(code, heads, wq, wk):
    for D, rot, ld_extra in ((128, 128, 0), (80, 40, 3)):
        c = Case(code, 2, 19, *heads, D, rot, pos=np.arange(38)[::-1] % 64, wq=wq, wk=wk, seed=D + wq + 2 * wk + sum(heads))
        (xs, x), (dys, dy) = c.values(), c.values()
        got_b = run_bwd(c, xs, dys, c.W + ld_extra, want=(wq, wk))
        check_all(c, xs, x, dys, dy, run_fwd(c, xs, c.W + ld_extra), got_b, f"heads {heads}")
        if heads[1] == 0 and wk:
            assert not fl(got_b[2], code).any()   # no k head: dwk is a sum over nothing
        # a weight sum that is not wanted changes nothing else
        only_dx = run_bwd(c, xs, dys, c.W + ld_extra, want=(False, False))
        assert np.array_equal(only_dx[0], got_b[0])


@pytest.mark.parametrize("code", [H.F32, H.BF16, H.F16])
@pytest.mark.parametrize("interleaved", [False, True])
def test_pack_and_element_access_agree_bit_for_bit(code, interleaved):
    """The same values at an aligned base (16-byte packs) and at a base shifted by one element (element loads and stores on the same lane
    map): the same bits, forward and backward, weight sums included. D = 80 has a group of 8 (bf16) or 16 (f32) lanes with idle ones."""
    for D, rot in ((128, 128), (128, 64), (80, 32), (64, 0)):
        c = Case(code, 2, 19, 5, 2, 2, D, rot, interleaved, pos=np.arange(38) * 5 % 64, seed=D + rot)
        (xs, _), (dys, _) = c.values(), c.values()
        H.profile_reset()
        H.profile_enable(True)
        try:
            ya, ba = run_fwd(c, xs), run_bwd(c, xs, dys)
            names_a = set(H.profile_results())
            H.profile_reset()
            ye, be = run_fwd(c, xs, shift=1), run_bwd(c, xs, dys, shift=1)
            names_e = set(H.profile_results())
        finally:
            H.profile_enable(False)
        assert {"qk_norm_rope_fwd_packed", "qk_norm_rope_bwd_packed"} <= names_a, names_a
        assert {"qk_norm_rope_fwd_lanes", "qk_norm_rope_bwd_lanes"} <= names_e, names_e
        assert np.array_equal(ya, ye)
        for a, e in zip(ba, be):
            assert np.array_equal(a, e)


@pytest.mark.parametrize("code", [H.F32, H.BF16])
@pytest.mark.parametrize("D,rot,extra", [(128, 128, 0), (128, 64, 24), (80, 40, 3), (64, 2, 0)])
def test_in_place_equals_out_of_place(code, D, rot, extra):
    c = Case(code, 2, 19, 5, 2, 2, D, rot, pos=np.arange(38) * 3 % 64, seed=D + rot + extra)
    (xs, _), (dys, _) = c.values(), c.values()
    ld = c.W + extra
    nv = (c.Hq + c.Hk) * D
    y, y_ip = run_fwd(c, xs, ld), run_fwd(c, xs, ld, in_place=True)
    assert np.array_equal(y, y_ip) and np.array_equal(y_ip[:, nv:], xs[:, nv:])
    b, b_ip = run_bwd(c, xs, dys, ld), run_bwd(c, xs, dys, ld, in_place=True)
    assert np.array_equal(b_ip[0][:, nv:], dys[:, nv:])
    for a, e in zip(b, b_ip):
        assert np.array_equal(a, e)


@pytest.mark.parametrize("code", [H.BF16, H.F32])
def test_many_tokens_per_block(code):
    """T = 4099 is more tokens than the backward's grid has waves: waves walk several tokens and the weight sums cross blocks."""
    T, Hq, Hk, Hv, D = 4099, 2, 1, 1, 64
    c = Case(code, 1, T, Hq, Hk, Hv, D, D, P=T, seed=41)
    (xs, x), (dys, dy) = c.values(), c.values()
    got = run_bwd(c, xs, dys)
    again = run_bwd(c, xs, dys)
    rb = R.backward(x, dy, *c.ref_args())
    check(f"dx {NAME[code]}", got[0], rb["dx"], rb["dx_tol"], code)
    check(f"dw {NAME[code]}, 4099 tokens", got[1], rb["dwq"], rb["dwq_tol"], code)
    check(f"dw {NAME[code]}, 4099 tokens", got[2], rb["dwk"], rb["dwk_tol"], code)
    for a, e in zip(got, again):
        assert np.array_equal(a, e), "two runs differ"
    # dy one-hot at a single (token, head, dim) of a head of +-1 (rstd = 1 with eps = 0, no rotation): dw there is x exactly, 0 elsewhere
    c0 = Case(code, 1, T, Hq, Hk, Hv, D, 0, wq=False, wk=False, eps=0.0, seed=42)
    for t0, h0, d0 in ((T - 1, 1, 5), (2049, 2, 63), (0, 0, 0)):
        xv = c0.rng.uniform(-2, 2, (T, Hq + Hk + Hv, D))
        xv[t0, h0] = np.where(c0.rng.integers(0, 2, D) > 0, 1.0, -1.0)
        g = np.zeros_like(xv)
        g[t0, h0, d0] = 1.0
        _, dq, dk = run_bwd(c0, store(xv.reshape(T, -1), code), store(g.reshape(T, -1), code))
        want = np.zeros((2, D))
        want[0 if h0 < Hq else 1, d0] = xv[t0, h0, d0]
        assert np.array_equal(np.stack([fl(dq, code), fl(dk, code)]), want), (t0, h0, d0)


def test_poisoned_workspace_and_outputs(monkeypatch):
    """Scratch and pure outputs filled with each pattern of tests/poison.py before the call: the bits of the zero-filled run."""
    base = {}
    for byte in poison.PATTERNS:
        state = poison.poisoned_allocations(monkeypatch, byte)
        for code, D, rot, extra in ((H.BF16, 128, 128, 0), (H.F32, 64, 32, 0), (H.F16, 80, 40, 3), (H.BF16, 64, 2, 0)):
            c = Case(code, 2, 19, 5, 2, 2, D, rot, pos=np.arange(38) % 64, seed=D + rot)
            (xs, _), (dys, _) = c.values(), c.values()
            ld = c.W + extra
            # (with pad columns the result's surroundings hold the pattern itself)
            got = (run_fwd(c, xs, ld, fill=False, pad=byte),) + run_bwd(c, xs, dys, ld, fill=False, pad=byte)
            key = (code, D, rot)
            if byte == poison.PATTERNS[0]:
                base[key] = got
            for a, e in zip(got, base[key]):
                assert np.array_equal(a, e), (hex(byte), key)
        assert state.allocations > 0


def test_special_values():
    code, B, S, Hq, Hk, Hv, D = H.F32, 1, 6, 2, 1, 1, 64
    c = Case(code, B, S, Hq, Hk, Hv, D, D, seed=7)
    xs, x = c.values()
    xv = x.reshape(S, Hq + Hk + Hv, D).copy()
    xv[0, 1] = 0.0                       # an all-zero head
    xv[1, 0, 7] = np.inf                 # one Inf, one NaN: they stay inside their heads
    xv[2, 2, 40] = np.nan
    xv[3, :3] *= 1e-20 / 2.0             # tiny: eps decides the scale
    xv[4, :3] *= 1e18 / 2.0              # huge but the f32 sum of squares still fits (64 * 1e36 < 3.4e38)
    xv[5, :3] = np.where(xv[5, :3] < 0, -3e19, 3e19)   # x^2 = 9e38 overflows f32: rstd = 0, y = 0 by the stated f32 formula
    xs = store(xv.reshape(S, -1), code)
    x = fl(xs, code)
    dys, dy = c.values()
    y = fl(run_fwd(c, xs), code).reshape(S, Hq + Hk + Hv, D)
    dx, dq, dk = run_bwd(c, xs, dys)
    dx = fl(dx, code).reshape(S, Hq + Hk + Hv, D)
    with np.errstate(all="ignore"):
        ry, tol = R.forward(x, *c.ref_args())
        rb = R.backward(x, dy, *c.ref_args())
    ry, tol = ry.reshape(y.shape), tol.reshape(y.shape)
    rdx, rdx_tol = rb["dx"].reshape(y.shape), rb["dx_tol"].reshape(y.shape)
    assert not y[0, 1].any(), "an all-zero head must give zeros"
    # Inf: sum = inf, rstd = 0, so the head is 0 except the Inf's own pair (inf * 0); NaN: the whole head. Nothing leaves the head, and the
    # backward's m is NaN in both, so all of the head's dx. (R.within wants the NaN pattern of the f64 reference.)
    assert np.isnan(y[1, 0]).sum() == 2 and np.isnan(y[2, 2]).all() and np.isnan(dx[1, 0]).all() and np.isnan(dx[2, 2]).all()
    clean = np.ones(y.shape[:2], bool)
    clean[5, :3] = False
    for t, h in zip(*np.nonzero(clean)):
        assert R.within(y[t, h], ry[t, h], tol[t, h], 0.0)[0], ("forward", t, h)
        assert R.within(dx[t, h], rdx[t, h], rdx_tol[t, h], 0.0)[0], ("dx", t, h)
    # 1e-20: mean(x^2) ~ 1e-40 vanishes beside eps = 1e-6, so y = x * 1000 * w (checked against the reference above); the scale shows
    assert 1e-18 < np.abs(y[3, :3]).max() < 1e-16
    assert 0.1 < np.abs(y[4, :3]).max() < 10.0
    # overflow: the stated formula in f32 gives rstd = 1 / sqrt(inf) = 0, so y = 0, xhat = 0 and dx = 0
    assert not y[5, :3].any() and not dx[5, :3].any()
    # the weight sums: what the reference gives with xhat = 0 in the overflowed token, NaN where a NaN or Inf head reaches them
    xz = x.reshape(y.shape).copy()
    xz[5, :3] = 0.0
    with np.errstate(all="ignore"):
        rz = R.backward(xz.reshape(S, -1), dy, *c.ref_args())
    assert R.within(fl(dq, code), rz["dwq"], rz["dwq_tol"], 0.0)[0] and R.within(fl(dk, code), rz["dwk"], rz["dwk_tol"], 0.0)[0]
    assert np.isnan(rz["dwq"]).sum() == 1 and np.isnan(rz["dwk"]).all()


def test_bad_position_is_nan_in_that_token_only():
    code, B, S, Hq, Hk, Hv, D, P = H.BF16, 2, 19, 5, 2, 2, 128, 16
    for rot, interleaved in ((128, False), (64, True), (34, False)):
        pos = np.arange(B * S) % P
        pos[4], pos[30] = P, -1
        c = Case(code, B, S, Hq, Hk, Hv, D, rot, interleaved, P=P, pos=pos, seed=rot)
        (xs, x), (dys, dy) = c.values(), c.values()
        y = fl(run_fwd(c, xs), code)
        dx, dq, dk = run_bwd(c, xs, dys)
        ry, tol = R.forward(x, *c.ref_args())
        rb = R.backward(x, dy, *c.ref_args())
        bad = np.zeros((B * S, Hq + Hk + Hv, D), bool)
        bad[[4, 30], :Hq + Hk, :rot] = True
        assert np.array_equal(np.isnan(y), bad.reshape(B * S, -1)), "exactly the rotated elements of the two tokens"
        bad[[4, 30], :Hq + Hk, :] = True
        assert np.array_equal(np.isnan(fl(dx, code)), bad.reshape(B * S, -1)), "exactly the q and k heads of the two tokens"
        # everything else within the bounds (R.within wants NaN where the reference has NaN)
        check(f"forward {NAME[code]}", store(y, code), ry, tol, code)
        check(f"dx {NAME[code]}", dx, rb["dx"], rb["dx_tol"], code)
        for got, name in ((dq, "dwq"), (dk, "dwk")):
            g = fl(got, code)
            assert np.isnan(g[:rot]).all() and np.array_equal(np.isnan(g), np.isnan(rb[name]))
    # (a read outside the table would fault or pull garbage into other tokens: the table above has exactly P rows and the buffer ends there)


def test_graph_capture_and_replay():
    code, B, S, Hq, Hk, Hv, D = H.BF16, 2, 64, 4, 2, 2, 128
    c = Case(code, B, S, Hq, Hk, Hv, D, D, P=S, seed=3)
    (xs, _), (dys, _) = c.values(), c.values()
    want_y, want_b = run_fwd(c, xs), run_bwd(c, xs, dys)
    bx, bg = H.DevBuf.from_numpy(xs), H.DevBuf.from_numpy(dys)
    by, bd = H.DevBuf(xs.nbytes), H.DevBuf(xs.nbytes)
    bq, bk = H.DevBuf(D * ES[code]), H.DevBuf(D * ES[code])
    ws = H.DevBuf(H.qk_norm_rope_bwd_workspace_bytes(*c.geom()))
    st = H.Stream()
    with H.Graph.capture(st) as graph:
        H.qk_norm_rope_fwd(*c.geom(), bx.ptr, c.W, by.ptr, c.W, stream=st.handle, **c.common())
        H.qk_norm_rope_bwd(*c.geom(), bx.ptr, c.W, bg.ptr, c.W, bd.ptr, c.W, dwq=bq.ptr, dwk=bk.ptr, workspace=ws.ptr, workspace_bytes=ws.nbytes,
                           stream=st.handle, **c.common())
    for _ in range(2):
        for b in (by, bd, bq, bk, ws):
            poison.fill(b.ptr, b.nbytes, 0xFF)
        H.device_sync()
        graph.launch()
        st.sync()
        assert np.array_equal(by.to_numpy(xs.shape, NP[code]), want_y)
        assert np.array_equal(bd.to_numpy(xs.shape, NP[code]), want_b[0])
        assert np.array_equal(bq.to_numpy((D,), NP[code]), want_b[1]) and np.array_equal(bk.to_numpy((D,), NP[code]), want_b[2])


# ---- the operator -------------------------------------------------------------------------------------------------------------------------
def torch_qk_norm_rope(x, wq, wk, cos, sin, pos, B, S, Hq, Hk, D, rot, interleaved, eps):
    """torch f64 on [T, (Hq + 2 Hk) D]: the manual RMS norm per head and HF's rotate_half / GPT-J's rotate_every_two."""
    import torch
    T = B * S
    h = x.reshape(T, Hq + 2 * Hk, D)
    qk, v = h[:, :Hq + Hk], h[:, Hq + Hk:]
    one = torch.ones(D, dtype=torch.float64)
    w = torch.cat([(one if wq is None else wq).expand(Hq, D), (one if wk is None else wk).expand(Hk, D)], 0)
    n = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + eps) * w
    if rot:
        p = torch.arange(T) % S if pos is None else torch.as_tensor(pos)
        c, s = cos[p][:, None, :], sin[p][:, None, :]
        z = n[..., :rot]
        if interleaved:
            c, s = c.repeat_interleave(2, -1), s.repeat_interleave(2, -1)
            zr = torch.stack([-z[..., 1::2], z[..., ::2]], -1).flatten(-2)
        else:
            c, s = torch.cat([c, c], -1), torch.cat([s, s], -1)
            zr = torch.cat([-z[..., rot // 2:], z[..., :rot // 2]], -1)
        n = torch.cat([z * c + zr * s, n[..., rot:]], -1)
    return torch.cat([n, v], 1).reshape(T, -1)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("rot,interleaved,kv,with_pos", [(64, False, 2, True), (32, True, 4, False), (0, False, 1, False)])
def test_operator_against_torch_autograd(bf16, rot, interleaved, kv, with_pos):
    import torch
    B, S, Hh, D = 2, 10, 4, 64
    code = H.BF16 if bf16 else H.F32
    rng = np.random.default_rng(rot + kv)
    W = (Hh + 2 * kv) * D
    rnd = lambda a: fl(store(a, code), code)  # noqa: E731
    x, g = rnd(rng.uniform(-2, 2, (B * S, W))), rnd(rng.uniform(-1, 1, (B * S, W)))
    wq, wk = rnd(rng.uniform(0.5, 1.5, D)), rnd(rng.uniform(0.5, 1.5, D))
    c, s = tables(S + 3, rot)
    pos = rng.integers(0, S + 3, B * S) if with_pos else None
    dev = lambda a: kfunca.from_numpy(a.astype(np.float32), 0).bfloat16() if bf16 else kfunca.from_numpy(a.astype(np.float32), 0)  # noqa: E731
    tx, tq, tk = dev(x), dev(wq), dev(wk)
    for t in (tx, tq, tk):
        t.set_requires_grad(True)
    tc, ts = (kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)) if rot else (None, None)
    tp = kfunca.from_numpy(pos.astype(np.int64), 0) if with_pos else None
    y = kfunca.qk_norm_rope(tx, tq, tk, tc, ts, B, S, Hh, kv_heads=kv, positions=tp, interleaved=interleaved)
    assert y.sizes() == [B * S, W]
    y.backward(dev(g))
    num = lambda t: (t.float() if bf16 else t).numpy().astype(np.float64)  # noqa: E731
    # torch f64 on the same stored values
    px, pq, pk = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, wq, wk))
    tt = (torch.tensor(c, dtype=torch.float64), torch.tensor(s, dtype=torch.float64)) if rot else (None, None)
    py = torch_qk_norm_rope(px, pq, pk, *tt, pos, B, S, Hh, kv, D, rot, interleaved, 1e-6)
    py.backward(torch.tensor(g))
    args = (wq, wk, c, s, pos, B, S, Hh, kv, kv, D, rot, interleaved, 1e-6)
    _, tol = R.forward(x, *args)
    rb = R.backward(x, g, *args)
    r = R.ROUNDING[NAME[code]]
    for what, got, want, t in (("y", y, py, tol), ("dqkv", tx.grad(), px.grad, rb["dx_tol"]), ("dwq", tq.grad(), pq.grad, rb["dwq_tol"]),
                               ("dwk", tk.grad(), pk.grad, rb["dwk_tol"])):
        ok, frac = R.within(num(got), want.detach().numpy(), t, r, R.SUBNORMAL_ROUNDING[NAME[code]])
        print(f"operator {what} {NAME[code]}: worst fraction of the bound {frac:.3f}")
        assert ok, (what, frac)
    # a weight that is None: 1, and no gradient for it; the tables get none either
    y1 = kfunca.qk_norm_rope(tx, None, tk, tc, ts, B, S, Hh, kv_heads=kv, positions=tp, interleaved=interleaved)
    p1 = torch_qk_norm_rope(px, None, pk, *tt, pos, B, S, Hh, kv, D, rot, interleaved, 1e-6)
    _, tol1 = R.forward(x, None, *args[1:])
    assert R.within(num(y1), p1.detach().numpy(), tol1, r)[0]
    before = num(tq.grad()).copy()
    y1.backward(dev(g))
    assert np.array_equal(num(tq.grad()), before), "a weight that was not given got a gradient"


def test_operator_refusals():
    B, S, Hh, D = 2, 10, 4, 64
    rng = np.random.default_rng(1)
    qkv = kfunca.from_numpy(rng.uniform(-1, 1, (B * S, 3 * Hh * D)).astype(np.float32), 0)
    w = kfunca.from_numpy(np.ones(D, np.float32), 0)
    c, s = tables(S, 32)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    with pytest.raises(RuntimeError, match="shape does not match"):
        kfunca.qk_norm_rope(qkv, w, w, tc, ts, B, S, Hh + 2)
    with pytest.raises(RuntimeError, match="shape does not match"):
        kfunca.qk_norm_rope(qkv, w, w, tc, ts, B, S + 1, Hh)
    with pytest.raises(RuntimeError, match="q_weight / k_weight"):
        kfunca.qk_norm_rope(qkv, kfunca.from_numpy(np.ones(D + 1, np.float32), 0), w, tc, ts, B, S, Hh)
    with pytest.raises(RuntimeError, match="q_weight / k_weight"):
        kfunca.qk_norm_rope(qkv, w, w.bfloat16(), tc, ts, B, S, Hh)
    with pytest.raises(RuntimeError, match="given together"):
        kfunca.qk_norm_rope(qkv, w, w, tc, None, B, S, Hh)
    with pytest.raises(RuntimeError, match="rotary_dim"):
        kfunca.qk_norm_rope(qkv, w, w, *(kfunca.from_numpy(np.zeros((S, 40), np.float32), 0),) * 2, B, S, Hh)
    with pytest.raises(RuntimeError, match="float tables"):
        kfunca.qk_norm_rope(qkv, w, w, tc.bfloat16(), ts.bfloat16(), B, S, Hh)
    with pytest.raises(RuntimeError, match="Long"):
        kfunca.qk_norm_rope(qkv, w, w, tc, ts, B, S, Hh, positions=kfunca.from_numpy(np.zeros(B * S, np.float32), 0))
    with pytest.raises(RuntimeError, match="B\\*S"):
        kfunca.qk_norm_rope(qkv, w, w, tc, ts, B, S, Hh, positions=kfunca.from_numpy(np.zeros(B * S - 1, np.int64), 0))
    with pytest.raises(RuntimeError, match="rows"):   # S = 10 rows needed, the tables have 4
        kfunca.qk_norm_rope(qkv, w, w, kfunca.from_numpy(c[:4], 0), kfunca.from_numpy(s[:4], 0), B, S, Hh)
    with pytest.raises(RuntimeError, match="eps"):
        kfunca.qk_norm_rope(qkv, w, w, tc, ts, B, S, Hh, eps=-1.0)
    with pytest.raises(RuntimeError, match="float, half and bfloat16"):
        kfunca.qk_norm_rope(kfunca.from_numpy(np.zeros((B * S, 3 * Hh * D), np.int64), 0), w, w, tc, ts, B, S, Hh)


@pytest.mark.parametrize("bf16", [False, True])
def test_end_to_end_through_attention(bf16):
    """gemm -> qk_norm_rope -> attention_qkv (causal, GQA) -> sum, against torch-CPU f64 on the same weights, with rope's end-to-end tolerances."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(23)
    B, S, Hh, kv, D, d = 2, 64, 4, 2, 64, 96
    W = (Hh + 2 * kv) * D
    w = {"h": rng.uniform(-1, 1, (B * S, d)), "wqkv": rng.uniform(-1, 1, (d, W)) / np.sqrt(d), "wq": rng.uniform(0.5, 1.5, D),
         "wk": rng.uniform(0.5, 1.5, D)}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    if bf16:
        w = {k: O.bf16_to_f32(O.f32_to_bf16(v)) for k, v in w.items()}
    c, s = tables(S, D)
    pos = np.tile(np.arange(S), B)[::-1].copy()
    ps = {k: kfunca.from_numpy(v, 0) for k, v in w.items()}
    if bf16:
        ps = {k: v.bfloat16() for k, v in ps.items()}
    for p in ps.values():
        p.set_requires_grad(True)
    tc, ts, tpos = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0), kfunca.from_numpy(pos, 0)
    qkv = kfunca.qk_norm_rope(kfunca.gemm(ps["h"], ps["wqkv"], 1.0, 0.0), ps["wq"], ps["wk"], tc, ts, B, S, Hh, kv_heads=kv, positions=tpos)
    a = kfunca.attention_qkv(qkv, B, S, Hh, kv_heads=kv, causal=True)
    ones = kfunca.from_numpy(np.ones((B * S, Hh * D), np.float32), 0)
    a.backward(ones.bfloat16() if bf16 else ones)   # the loss is the sum of the attention output
    got = float((a.float() if bf16 else a).numpy().astype(np.float64).sum())
    kg = {k: (p.grad().float() if bf16 else p.grad()).numpy() for k, p in ps.items()}

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    y = torch_qk_norm_rope(t["h"] @ t["wqkv"], t["wq"], t["wk"], torch.tensor(c, dtype=torch.float64), torch.tensor(s, dtype=torch.float64), pos, B, S,
                           Hh, kv, D, D, False, 1e-6).reshape(B, S, Hh + 2 * kv, D).permute(0, 2, 1, 3)
    q, k, v = y[:, :Hh], y[:, Hh:Hh + kv], y[:, Hh + kv:]
    rl = F.scaled_dot_product_attention(q, k.repeat_interleave(Hh // kv, 1), v.repeat_interleave(Hh // kv, 1), is_causal=True).sum()
    rl.backward()
    tg = {k: v.grad.numpy() for k, v in t.items()}
    want = rl.item()
    if not bf16:
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
        for k in kg:
            assert_close(kg[k], tg[k], rtol=1e-3, atol=1e-5, what=f"d {k}")
    else:
        assert abs(got - want) <= 2e-2 * abs(want), (got, want)
        for k in kg:
            scale = np.abs(tg[k]).max()
            assert np.abs(kg[k] - tg[k]).max() <= 0.06 * scale, (k, float(np.abs(kg[k] - tg[k]).max()), float(scale))


def test_f32_against_the_composition_of_rms_norm_and_rope():
    """Split q and k out, rms_norm each over its heads, rope each: today's route. f32, so the one extra rounding of the composition is an f32
    one and the two results agree within the sum of the two operators' stated bounds."""
    B, S, Hh, kv, D, rot = 2, 19, 4, 2, 64, 64
    rng = np.random.default_rng(9)
    W = (Hh + 2 * kv) * D
    x = rng.uniform(-2, 2, (B * S, W)).astype(np.float32)
    wq, wk = rng.uniform(0.5, 1.5, D).astype(np.float32), rng.uniform(0.5, 1.5, D).astype(np.float32)
    c, s = tables(S, rot)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    fused = kfunca.qk_norm_rope(kfunca.from_numpy(x, 0), kfunca.from_numpy(wq, 0), kfunca.from_numpy(wk, 0), tc, ts, B, S, Hh, kv_heads=kv).numpy()
    xh = x.reshape(B, S, Hh + 2 * kv, D)
    parts = []
    for sl, w in ((slice(0, Hh), wq), (slice(Hh, Hh + kv), wk)):
        heads = np.ascontiguousarray(xh[:, :, sl].transpose(0, 2, 1, 3))                     # [B, H, S, D], contiguous
        n = kfunca.rms_norm(kfunca.from_numpy(heads, 0), kfunca.from_numpy(w, 0), 1e-6)
        parts.append(kfunca.rope(n, tc, ts).numpy().transpose(0, 2, 1, 3))
    comp = np.concatenate(parts + [xh[:, :, Hh + kv:]], 2).reshape(B * S, W)
    f = lambda a: a.astype(np.float64)  # noqa: E731
    ry, _ = R.forward(f(x), f(wq), f(wk), None, None, None, B, S, Hh, kv, kv, D, 0, False, 1e-6)   # n: the norm alone
    n = np.abs(ry.reshape(B * S, Hh + 2 * kv, D))
    pair = n[..., :rot // 2] + n[..., rot // 2:rot]
    tol = np.zeros_like(n)
    tol[..., :rot // 2] = tol[..., rot // 2:rot] = 1e-5 * (pair + 2.0) + 2.0 ** -22 * pair
    tol[:, Hh + kv:] = 0.0
    err = np.abs(f(fused) - f(comp)).reshape(n.shape)
    print(f"fused vs composition: worst fraction of the bound {float((err[:, :Hh + kv] / tol[:, :Hh + kv]).max()):.3f}")
    assert (err <= tol).all()
    assert np.array_equal(fused.reshape(n.shape)[:, Hh + kv:], xh.reshape(n.shape)[:, Hh + kv:])
