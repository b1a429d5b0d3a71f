"""-m gpu: rotary position embeddings (kf_rope, kf_rope_table, kfunca.rope / rope_qkv / rope_table) against an f64 numpy reference on
the same rounded inputs and tables, against torch-CPU's HF `apply_rotary_pos_emb` / GPT-J `rotate_every_two`, and through a small
attention model end to end.

Tolerances (stated):
  rotation       |got - ref| <= r |ref| + 2^-22 (|x_a| + |x_b|), r one output rounding: 2^-8 bf16, 2^-11 f16, 0 f32 (the f32 product and FMA
                 round twice relative to |x_a| + |x_b|; the stored output rounds once more); copied heads and dims are bit-exact
  torch parity   twice that bound in f32, 2^-21 (|x_a| + |x_b|): both sides round (torch three times: x_a c, x_b s and their sum, each
                 within 2^-24 (|x_a| + |x_b|); this kernel's product and FMA about as much)
  tables         within 1 f32 ulp of numpy's f64, plus |theta| 2^-50 where cos or sin sits near a zero and the f64 angle's own last bit
                 shows (libm pow may differ from numpy's in the last f64 bit)
  algebra        <rope(x), g> = <x, rope_inv(g)> to 1e-6 of sum |x| |g| (f32); rope_inv(rope(x)) = x within 2^-21 (|x_a| + |x_b|) in f32,
                 2^-7 (|x_a| + |x_b|) in bf16
  end to end     f32: loss 1e-5 relative, gradients rtol 1e-3 / atol 1e-5; bf16 operands: loss 2e-2 relative, gradients 6 % of each
                 tensor's max |grad| (bf16 rounding of every operand and of attention's probabilities)
Bitwise: in place equals out of place, rope_qkv equals rope on the split heads, repeated runs, graph replay.
"""
import ctypes as C

import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

OUT_R = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 0.0}
NP = {H.BF16: np.uint16, H.F16: np.float16, H.F32: np.float32}
ES = {H.BF16: 2, H.F16: 2, H.F32: 4}


def tables(P, R, base=10000.0):
    """f32 tables rounded from f64 (the test's own; the device's kf_rope_table is checked separately)."""
    i = np.arange(R // 2, dtype=np.float64)
    th = np.arange(P, dtype=np.float64)[:, None] * base ** (-2 * i / R)[None, :]
    return np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)


def ref(x, c, s, R, h_rot, pos=None, interleaved=False, inverse=False):
    """f64 of x [B, H, S, D] (float values of the stored elements). Returns (y, bound without the output rounding, rotated mask)."""
    x = np.asarray(x, np.float64)
    B, Hh, S, D = x.shape
    p = np.tile(np.arange(S), B) if pos is None else np.asarray(pos)
    ok = (p >= 0) & (p < c.shape[0])
    pc = np.where(ok, p, 0)
    cc = c.astype(np.float64)[pc].reshape(B, 1, S, R // 2)
    ss = s.astype(np.float64)[pc].reshape(B, 1, S, R // 2) * (-1.0 if inverse else 1.0)
    bad = (~ok).reshape(B, 1, S, 1)
    cc, ss = np.where(bad, np.nan, cc), np.where(bad, np.nan, ss)
    y = x.copy()
    ia = np.arange(0, R, 2) if interleaved else np.arange(R // 2)
    ib = ia + 1 if interleaved else ia + R // 2
    xa, xb = x[:, :h_rot, :, ia], x[:, :h_rot, :, ib]
    y[:, :h_rot, :, ia] = xa * cc - xb * ss
    y[:, :h_rot, :, ib] = xb * cc + xa * ss
    bound = np.zeros_like(x)
    mag = 2.0 ** -22 * (np.abs(xa) + np.abs(xb))
    bound[:, :h_rot, :, ia] = mag
    bound[:, :h_rot, :, ib] = mag
    rot = np.zeros(x.shape, bool)
    rot[:, :h_rot, :, ia] = rot[:, :h_rot, :, ib] = True
    return y, bound, rot


def check(got, want, bound, code, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    tol = OUT_R[code] * np.abs(want) + bound
    bad = ~(err <= tol)
    assert not bad.any(), (what, int(bad.sum()), float(err[bad].max()), np.argwhere(bad)[:3].tolist())


def contiguous_layout(Hh, S, D):
    return (Hh * S * D, S * D, D)


def run(code, xs, c, s, R, h_rot, pos=None, interleaved=False, inverse=False, lay=None, out_lay=None, out_elems=None, in_place=False):
    """Through the C ABI on contiguous storage (or the given layouts). xs: storage array holding x; returns the storage of y."""
    B, Hh, S, D = xs.shape if lay is None else lay[0]
    lx = contiguous_layout(Hh, S, D) if lay is None else lay[1]
    bx = H.DevBuf.from_numpy(xs)
    bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    bp = H.DevBuf.from_numpy(np.asarray(pos, np.int64)) if pos is not None else None
    if in_place:
        H.rope(code, B, Hh, S, D, bx.ptr, lx, None, None, bc.ptr, bs.ptr, c.shape[0], R, h_rot, bp.ptr if bp else None, interleaved, inverse)
        H.device_sync()
        return bx.to_numpy(xs.shape, xs.dtype)
    ly = lx if out_lay is None else out_lay
    n = xs.size if out_elems is None else out_elems
    by = H.DevBuf(n * ES[code])
    by.zero()
    H.rope(code, B, Hh, S, D, bx.ptr, lx, by.ptr, ly, bc.ptr, bs.ptr, c.shape[0], R, h_rot, bp.ptr if bp else None, interleaved, inverse)
    H.device_sync()
    return by.to_numpy((n,), xs.dtype)


def make(rng, code, shape, scale=2.0):
    xs = O.from_float(rng.uniform(-scale, scale, shape).astype(np.float32), code)
    return xs, O.to_float(xs, code).astype(np.float64)


def fl(a, code):
    return O.to_float(a, code).astype(np.float64)


@pytest.mark.parametrize("code", [H.F32, H.BF16, H.F16])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("D", [64, 128, 80, 256])
@pytest.mark.parametrize("rsel", ["D", "D/2", "32"])
@pytest.mark.parametrize("with_pos", [False, True])
def test_parity_with_f64(code, interleaved, D, rsel, with_pos):
    R = {"D": D, "D/2": D // 2, "32": 32}[rsel]
    B, Hh, S = 2, 5, 19
    h_rot = 3 if (D + R) % 3 else Hh  # partial h_rot on most cases
    rng = np.random.default_rng(D * 7 + R + 13 * with_pos + 2 * interleaved + code)
    xs, x = make(rng, code, (B, Hh, S, D))
    P = 64
    c, s = tables(P, R)
    pos = rng.integers(0, P, B * S) if with_pos else None
    want, bound, _ = ref(x, c, s, R, h_rot, pos, interleaved)
    got = run(code, xs, c, s, R, h_rot, pos, interleaved).reshape(xs.shape)
    check(fl(got, code), want, bound, code, "forward")
    # copied heads and dims: exact bits
    assert np.array_equal(got[:, h_rot:], xs[:, h_rot:])
    assert np.array_equal(got[:, :h_rot, :, R:], xs[:, :h_rot, :, R:])
    # the inverse, and in place equals out of place bit for bit
    want_i, bound_i, _ = ref(x, c, s, R, h_rot, pos, interleaved, inverse=True)
    got_i = run(code, xs, c, s, R, h_rot, pos, interleaved, inverse=True).reshape(xs.shape)
    check(fl(got_i, code), want_i, bound_i, code, "inverse")
    got_ip = run(code, xs, c, s, R, h_rot, pos, interleaved, in_place=True)
    assert np.array_equal(got_ip, got)


@pytest.mark.parametrize("interleaved", [False, True])
def test_parity_with_torch_hf_and_gptj(interleaved):
    import torch
    B, Hh, S, D, R = 2, 4, 33, 128, 128
    rng = np.random.default_rng(3 + interleaved)
    x = rng.uniform(-3, 3, (B, Hh, S, D)).astype(np.float32)
    c, s = tables(S, R)
    pos = rng.integers(0, S, (B, S))
    xt, ct, st = torch.tensor(x), torch.tensor(c)[torch.tensor(pos)][:, None], torch.tensor(s)[torch.tensor(pos)][:, None]  # [B, 1, S, R/2]
    if not interleaved:  # transformers' apply_rotary_pos_emb with rotate_half; its cos / sin are the tables repeated: cat(freqs, freqs)
        cos, sin = torch.cat([ct, ct], -1), torch.cat([st, st], -1)
        x1, x2 = xt[..., : D // 2], xt[..., D // 2:]
        want = xt * cos + torch.cat([-x2, x1], -1) * sin
    else:  # GPT-J's rotate_every_two with repeat_interleave'd tables
        cos, sin = ct.repeat_interleave(2, -1), st.repeat_interleave(2, -1)
        x1, x2 = xt[..., ::2], xt[..., 1::2]
        want = xt * cos + torch.stack([-x2, x1], -1).flatten(-2) * sin
    got = run(H.F32, x, c, s, R, Hh, pos.reshape(-1), interleaved).reshape(x.shape)
    _, bound, _ = ref(x, c, s, R, Hh, pos.reshape(-1), interleaved)
    err = np.abs(got.astype(np.float64) - want.numpy().astype(np.float64))
    assert (err <= 2 * bound + 1e-30).all(), float(err.max())


@pytest.mark.parametrize("base", [1e4, 5e5])
def test_table_within_one_ulp_of_f64(base):
    P, R = 131072, 128
    c32, s32 = H.DevBuf(P * R // 2 * 4), H.DevBuf(P * R // 2 * 4)
    H.rope_table(base, R, P, c32.ptr, s32.ptr)
    H.device_sync()
    gc, gs = c32.to_numpy((P, R // 2), np.float32), s32.to_numpy((P, R // 2), np.float32)
    i = np.arange(R // 2, dtype=np.float64)
    th = np.arange(P, dtype=np.float64)[:, None] * base ** (-2 * i / R)[None, :]
    for got, want in ((gc, np.cos(th)), (gs, np.sin(th))):
        tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + np.abs(th) * 2.0 ** -50
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= tol).all(), float((err / tol).max())
    # the operator API returns the same table
    tc, ts = kfunca.rope_table(P, R, base)
    assert tc.sizes() == [P, R // 2] and np.array_equal(tc.numpy(), gc) and np.array_equal(ts.numpy(), gs)


@pytest.mark.parametrize("code", [H.F32, H.BF16])
def test_adjoint_and_round_trip(code):
    B, Hh, S, D, R = 2, 6, 40, 128, 96
    rng = np.random.default_rng(11)
    c, s = tables(64, R)
    pos = rng.integers(0, 64, B * S)
    xs, x = make(rng, H.F32, (B, Hh, S, D))
    gs_, g = make(rng, H.F32, (B, Hh, S, D))
    y = run(H.F32, xs, c, s, R, 4, pos).astype(np.float64)
    gi = run(H.F32, gs_, c, s, R, 4, pos, inverse=True).astype(np.float64)
    lhs, rhs = np.dot(y, g.reshape(-1)), np.dot(x.reshape(-1), gi)
    assert abs(lhs - rhs) <= 1e-6 * np.dot(np.abs(x.reshape(-1)), np.abs(g.reshape(-1))), (lhs, rhs)
    xs, x = make(rng, code, (B, Hh, S, D))
    y = run(code, xs, c, s, R, 4, pos).reshape(xs.shape)
    back = fl(run(code, y, c, s, R, 4, pos, inverse=True).reshape(xs.shape), code)
    _, bound, _ = ref(x, c, s, R, 4, pos)
    k = 2.0 ** -21 / 2.0 ** -22 if code == H.F32 else 2.0 ** -7 / 2.0 ** -22
    assert (np.abs(back - x) <= k * bound).all()


def test_rope_qkv_equals_rope_on_split_heads_and_gqa():
    rng = np.random.default_rng(21)
    for Hq, Hkv in ((4, 4), (8, 2)):
        B, S, D, R = 2, 24, 64, 64
        W = (Hq + 2 * Hkv) * D
        xs, x = make(rng, H.BF16, (B * S, W))
        c, s = tables(S, R)
        qkv = kfunca.from_numpy_bf16(xs, 0)
        tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
        out = kfunca.rope_qkv(qkv, tc, ts, B, S, Hq, kv_heads=Hkv)
        got = out.numpy()
        heads = x.reshape(B, S, Hq + 2 * Hkv, D).transpose(0, 2, 1, 3)
        want, bound, _ = ref(heads, c, s, R, Hq + Hkv)
        check(fl(got, H.BF16).reshape(B, S, -1, D).transpose(0, 2, 1, 3), want, bound, H.BF16, f"qkv {Hq}/{Hkv}")
        # the same bits as kfunca.rope on the split heads: on a strided [B, H, S, D] view of the packed tensor (every head rotated there),
        # and on the q and k blocks split out contiguously
        Ht = Hq + 2 * Hkv
        mine = out.numpy().reshape(B, S, Ht, D).transpose(0, 2, 1, 3)
        allrot = kfunca.rope(qkv.view(B, S, Ht, D).permute(0, 2, 1, 3), tc, ts).numpy()
        assert np.array_equal(allrot[:, :Hq + Hkv], mine[:, :Hq + Hkv])
        assert np.array_equal(mine[:, Hq + Hkv:], xs.reshape(B, S, Ht, D).transpose(0, 2, 1, 3)[:, Hq + Hkv:])
        for h0, h1 in ((0, Hq), (Hq, Hq + Hkv)):
            part = np.ascontiguousarray(xs.reshape(B, S, Ht, D).transpose(0, 2, 1, 3)[:, h0:h1])
            split = kfunca.rope(kfunca.from_numpy_bf16(part, 0), tc, ts).numpy()
            assert np.array_equal(split, mine[:, h0:h1]), (Hq, Hkv, h0)


def test_packed_and_element_paths_are_both_taken_and_agree():
    B, Hh, S, D, R = 2, 4, 16, 128, 128
    rng = np.random.default_rng(5)
    xs, x = make(rng, H.BF16, (B, Hh, S, D))
    c, s = tables(S, R)
    H.profile_reset()
    H.profile_enable(True)
    try:
        aligned = run(H.BF16, xs, c, s, R, Hh)
        names_a = set(H.profile_results())
        H.profile_reset()
        # the same values at a base one element past a 16-byte boundary with a padded row stride: the element path
        big = np.zeros(1 + B * Hh * S * (D + 1), np.uint16)
        lx = (Hh * S * (D + 1), S * (D + 1), D + 1)
        for b in range(B):
            for h in range(Hh):
                for t in range(S):
                    o = 1 + b * lx[0] + h * lx[1] + t * lx[2]
                    big[o:o + D] = xs[b, h, t]
        bx = H.DevBuf.from_numpy(big)
        by = H.DevBuf(xs.nbytes)
        bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
        H.rope(H.BF16, B, Hh, S, D, bx.ptr + 2, lx, by.ptr, contiguous_layout(Hh, S, D), bc.ptr, bs.ptr, S)
        H.device_sync()
        names_e = set(H.profile_results())
    finally:
        H.profile_enable(False)
    assert "rope_packed" in names_a and "rope_elem" in names_e, (names_a, names_e)
    assert np.array_equal(by.to_numpy((xs.size,), np.uint16), aligned)


@pytest.mark.parametrize("code", [H.F32, H.BF16, H.F16])
@pytest.mark.parametrize("interleaved", [False, True])
def test_odd_strides_and_unaligned_bases(code, interleaved):
    B, Hh, S, D, R = 3, 3, 11, 80, 48
    rng = np.random.default_rng(code + 3 * interleaved)
    lx = (Hh * (S * (D + 3) + 1) + 7, S * (D + 3) + 1, D + 3)   # x: padded, odd strides, base 3 elements in
    ly = (Hh * S * (D + 1) + 5, S * (D + 1), D + 1)             # y: another odd layout, base 1 element in
    nx = 3 + (B - 1) * lx[0] + (Hh - 1) * lx[1] + (S - 1) * lx[2] + D
    ny = 1 + (B - 1) * ly[0] + (Hh - 1) * ly[1] + (S - 1) * ly[2] + D
    big, bigf = make(rng, code, (nx,))
    idx = lambda l, off: off + (np.arange(B)[:, None, None, None] * l[0] + np.arange(Hh)[None, :, None, None] * l[1]  # noqa: E731
                               + np.arange(S)[None, None, :, None] * l[2] + np.arange(D)[None, None, None, :])
    x = bigf[idx(lx, 3)]
    c, s = tables(S + 5, R)
    pos = rng.integers(0, S + 5, B * S)
    bx, by = H.DevBuf.from_numpy(big), H.DevBuf(ny * ES[code])
    by.zero()
    bc, bs, bp = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s), H.DevBuf.from_numpy(pos)
    H.rope(code, B, Hh, S, D, bx.ptr + 3 * ES[code], lx, by.ptr + ES[code], ly, bc.ptr, bs.ptr, S + 5, R, 2, bp.ptr, interleaved)
    H.device_sync()
    out = by.to_numpy((ny,), NP[code])
    got = fl(out[idx(ly, 1)], code)
    want, bound, _ = ref(x, c, s, R, 2, pos, interleaved)
    check(got, want, bound, code, "odd layout")
    # nothing outside y's elements was written
    mask = np.ones(ny, bool)
    mask[idx(ly, 1).reshape(-1)] = False
    assert not out[mask].astype(np.float64).any()


def test_in_place_on_packed_qkv_touches_only_rotated_elements_with_guard_bands():
    B, S, Hq, D, R = 2, 32, 4, 128, 64
    W = 3 * Hq * D
    rng = np.random.default_rng(8)
    xs, x = make(rng, H.BF16, (B * S, W))
    guard = 65536 // 2
    pattern = rng.integers(0, 65536, 2 * guard + xs.size).astype(np.uint16)
    pattern[guard:guard + xs.size] = xs.reshape(-1)
    buf = H.DevBuf.from_numpy(pattern)
    c, s = tables(S, R)
    bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    lay = (S * W, D, W)
    H.rope(H.BF16, B, 3 * Hq, S, D, buf.ptr + 2 * guard, lay, None, None, bc.ptr, bs.ptr, S, R, 2 * Hq)
    H.device_sync()
    after = buf.to_numpy(pattern.shape, np.uint16)
    assert np.array_equal(after[:guard], pattern[:guard]) and np.array_equal(after[guard + xs.size:], pattern[guard + xs.size:])
    y = after[guard:guard + xs.size].reshape(B, S, 3 * Hq, D)
    x4 = xs.reshape(B, S, 3 * Hq, D)
    assert np.array_equal(y[:, :, 2 * Hq:], x4[:, :, 2 * Hq:])            # v heads
    assert np.array_equal(y[:, :, :2 * Hq, R:], x4[:, :, :2 * Hq, R:])    # dims >= R
    want, bound, _ = ref(fl(x4, H.BF16).transpose(0, 2, 1, 3), c, s, R, 2 * Hq)
    check(fl(y, H.BF16).transpose(0, 2, 1, 3), want, bound, H.BF16, "in place")


@pytest.mark.parametrize("code,D,stride,R", [(H.BF16, 84, 88, 64), (H.BF16, 84, 88, 80), (H.F32, 82, 84, 40), (H.F16, 100, 104, 96)])
def test_packed_path_with_a_ragged_head_tail(code, D, stride, R):
    """D not a multiple of the pack with 16-byte aligned (padded) strides: the packed path, including its per-head copy of the last
    D % V elements. The padding of y is never written."""
    B, Hh, S, h_rot = 2, 5, 12, 3
    rng = np.random.default_rng(D + stride + R + code)
    lay = (Hh * S * stride, S * stride, stride)
    xs_pad, xpad = make(rng, code, (B, Hh, S, stride))
    x, xs = xpad[..., :D], xs_pad[..., :D]
    c, s = tables(S, R)
    bx, by = H.DevBuf.from_numpy(xs_pad), H.DevBuf(xs_pad.nbytes)
    by.zero()
    bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    H.profile_reset()
    H.profile_enable(True)
    try:
        H.rope(code, B, Hh, S, D, bx.ptr, lay, by.ptr, lay, bc.ptr, bs.ptr, S, R, h_rot)
        H.device_sync()
        names = set(H.profile_results())
    finally:
        H.profile_enable(False)
    assert "rope_packed" in names, names
    out = by.to_numpy(xs_pad.shape, NP[code])
    want, bound, _ = ref(x, c, s, R, h_rot)
    check(fl(out[..., :D], code), want, bound, code, "packed, ragged tail")
    assert np.array_equal(out[:, h_rot:, :, :D], xs[:, h_rot:])
    assert np.array_equal(out[:, :h_rot, :, R:D], xs[:, :h_rot, :, R:])
    assert not out[..., D:].astype(np.float64).any()


def test_strided_positions_views():
    """positions given as strided Long views (pos2d[:, 1:] of a [B, S + 1] tensor, pos[::2]) are read in token order, forward and
    backward, through kfunca.rope and kfunca.rope_qkv."""
    B, Hh, S, D, R = 2, 3, 16, 64, 64
    rng = np.random.default_rng(29)
    P = 40
    c, s = tables(P, R)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    pos2d = rng.integers(0, P, (B, S + 1))
    pos_long = rng.integers(0, P, 2 * B * S)
    views = ((kfunca.from_numpy(pos2d, 0)[:, 1:], pos2d[:, 1:].reshape(-1)), (kfunca.from_numpy(pos_long, 0)[::2], pos_long[::2]))
    x = rng.uniform(-1, 1, (B, Hh, S, D)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, Hh, S, D)).astype(np.float32)
    for tpos, npos in views:
        tx = kfunca.from_numpy(x, 0)
        tx.set_requires_grad(True)
        y = kfunca.rope(tx, tc, ts, positions=tpos)
        want, bound, _ = ref(x, c, s, R, Hh, npos)
        check(y.numpy(), want, bound, H.F32, "rope, strided positions")
        y.backward(kfunca.from_numpy(g, 0))
        gw, gb, _ = ref(g, c, s, R, Hh, npos, inverse=True)
        check(tx.grad().numpy(), gw, gb, H.F32, "rope backward, strided positions")
        qkv = x.transpose(0, 2, 1, 3).reshape(B * S, Hh * D)  # q = k = v = x: one head group per third
        packed = np.ascontiguousarray(np.concatenate([qkv, qkv, qkv], 1))
        out = kfunca.rope_qkv(kfunca.from_numpy(packed, 0), tc, ts, B, S, Hh, positions=tpos)
        got = out.numpy().reshape(B, S, 3 * Hh, D).transpose(0, 2, 1, 3)
        wq, bq, _ = ref(np.concatenate([x, x, x], 1), c, s, R, 2 * Hh, npos)
        check(got, wq, bq, H.F32, "rope_qkv, strided positions")


def test_repeated_runs_are_bitwise_identical():
    rng = np.random.default_rng(2)
    xs, _ = make(rng, H.BF16, (4, 12, 64, 128))
    c, s = tables(64, 128)
    pos = rng.integers(0, 64, 4 * 64)
    a, b = run(H.BF16, xs, c, s, 128, 8, pos), run(H.BF16, xs, c, s, 128, 8, pos)
    assert np.array_equal(a, b)


def test_out_of_range_positions_are_nan_rows_only():
    B, Hh, S, D, R = 2, 3, 8, 64, 32
    rng = np.random.default_rng(4)
    xs, x = make(rng, H.BF16, (B, Hh, S, D))
    P = 16
    c, s = tables(P, R)
    pos = rng.integers(0, P, B * S)
    pos[3], pos[12] = -1, P
    for in_place in (False, True):
        got = fl(run(H.BF16, xs, c, s, R, 2, pos, in_place=in_place).reshape(xs.shape), H.BF16)
        want, bound, rot = ref(x, c, s, R, 2, pos)
        badtok = np.zeros((B, 1, S, 1), bool)
        badtok.reshape(-1)[[3, 12]] = True
        nanmask = rot & badtok
        assert np.isnan(got[nanmask]).all() and not np.isnan(got[~nanmask]).any()
        check(np.where(nanmask, 0, got), np.where(nanmask, 0, want), np.where(nanmask, 0, bound), H.BF16, "other tokens")
    # the process is healthy: an ordinary call afterwards is right
    pos2 = rng.integers(0, P, B * S)
    want, bound, _ = ref(x, c, s, R, 2, pos2)
    check(fl(run(H.BF16, xs, c, s, R, 2, pos2).reshape(xs.shape), H.BF16), want, bound, H.BF16, "after")


def test_graph_replay_follows_positions_written_in_place():
    B, S, Hq, D, R = 2, 64, 4, 128, 128
    W = 3 * Hq * D
    rng = np.random.default_rng(6)
    xs, _ = make(rng, H.BF16, (B * S, W))
    P = 256
    c, s = tables(P, R)
    bx, by = H.DevBuf.from_numpy(xs), H.DevBuf(xs.nbytes)
    bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    p1, p2 = rng.integers(0, P, B * S), rng.integers(0, P, B * S)
    bp = H.DevBuf.from_numpy(p1)
    st = H.Stream()
    lay = (S * W, D, W)

    def call():
        H.rope(H.BF16, B, 3 * Hq, S, D, bx.ptr, lay, by.ptr, lay, bc.ptr, bs.ptr, P, R, 2 * Hq, bp.ptr, stream=st.handle)

    def eager(pos):
        H.check(H.lib().kf_memcpy_h2d(bp.ptr, np.ascontiguousarray(pos).ctypes.data, pos.nbytes, None))
        H.device_sync()
        call()
        st.sync()
        return by.to_numpy(xs.shape, np.uint16).copy()

    want1, want2 = eager(p1), eager(p2)
    assert not np.array_equal(want1, want2)
    H.check(H.lib().kf_memcpy_h2d(bp.ptr, p1.ctypes.data, p1.nbytes, None))
    H.device_sync()
    with H.Graph.capture(st) as graph:
        call()
    for pos, want in ((p1, want1), (p2, want2)):
        H.check(H.lib().kf_memcpy_h2d(bp.ptr, np.ascontiguousarray(pos).ctypes.data, pos.nbytes, None))
        by.zero()
        H.device_sync()
        graph.launch()
        st.sync()
        assert np.array_equal(by.to_numpy(xs.shape, np.uint16), want)


def test_operator_api_autograd_and_refusals():
    B, Hh, S, D = 2, 3, 10, 64
    rng = np.random.default_rng(12)
    x = rng.uniform(-1, 1, (B, S, Hh, D)).astype(np.float32)
    g = rng.uniform(-1, 1, (B, Hh, S, D)).astype(np.float32)
    c, s = tables(S, 32)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    base = kfunca.from_numpy(x, 0)
    base.set_requires_grad(True)
    xv = base.permute(0, 2, 1, 3)  # [B, H, S, D] with non-contiguous strides
    y = kfunca.rope(xv, tc, ts)
    assert y.sizes() == [B, Hh, S, D]
    want, bound, _ = ref(x.transpose(0, 2, 1, 3), c, s, 32, Hh)
    check(y.numpy(), want, bound, H.F32, "rope on a permuted view")
    y.backward(kfunca.from_numpy(g, 0))
    gw, gb, _ = ref(g, c, s, 32, Hh, inverse=True)
    assert base.grad().sizes() == [B, S, Hh, D]
    check(base.grad().contiguous().numpy().transpose(0, 2, 1, 3), gw, gb, H.F32, "rope backward")
    with pytest.raises(RuntimeError, match="unit stride"):
        kfunca.rope(xv.permute(0, 1, 3, 2), tc, ts)
    with pytest.raises(RuntimeError, match="rotary_dim"):
        kfunca.rope(xv, *(kfunca.from_numpy(np.zeros((S, 40), np.float32), 0),) * 2)
    with pytest.raises(RuntimeError, match="float tables"):
        kfunca.rope(xv, tc.bfloat16(), ts.bfloat16())
    with pytest.raises(RuntimeError, match="Long"):
        kfunca.rope(xv, tc, ts, positions=kfunca.from_numpy(np.zeros(B * S, np.float32), 0))
    with pytest.raises(RuntimeError, match="B\\*S"):
        kfunca.rope(xv, tc, ts, positions=kfunca.from_numpy(np.zeros(B * S - 1, np.int64), 0))
    with pytest.raises(RuntimeError, match="positions"):  # S = 10 rows needed, the tables have 4
        kfunca.rope(xv, kfunca.from_numpy(c[:4], 0), kfunca.from_numpy(s[:4], 0))
    qkv = kfunca.from_numpy(rng.uniform(-1, 1, (B * S, 3 * Hh * D)).astype(np.float32), 0)
    with pytest.raises(RuntimeError, match="shape does not match"):
        kfunca.rope_qkv(qkv, tc, ts, B, S, Hh + 2)
    with pytest.raises(RuntimeError, match="shape does not match"):
        kfunca.rope_qkv(qkv, tc, ts, B, S + 1, Hh)


def attention_model(dtype_bf16, seed=17):
    """embedding -> rms_norm -> qkv_linear -> rope_qkv -> causal_attention_qkv -> gemm_fused(Wo, add=x) -> logits -> cross_entropy -> backward,
    through kfunca and through torch-CPU f32 on the same weights and tables. Returns (kf loss, kf grads, torch loss, torch grads, params, batch)."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(seed)
    B, S, Hh, D, vocab = 2, 64, 2, 64, 97
    d = Hh * D
    w = {"table": rng.uniform(-1, 1, (vocab, d)), "norm": rng.uniform(0.5, 1.5, d), "wqkv": rng.uniform(-1, 1, (d, 3 * d)) / np.sqrt(d),
         "wo": rng.uniform(-1, 1, (d, d)) / np.sqrt(d), "head": rng.uniform(-1, 1, (d, vocab)) / np.sqrt(d)}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    if dtype_bf16:
        w = {k: O.bf16_to_f32(O.f32_to_bf16(v)) for k, v in w.items()}
    tokens = rng.integers(0, vocab, B * S)
    target = np.r_[tokens[1:], -100]
    c, s = tables(S, D)
    pos = np.tile(np.arange(S), B)[::-1].copy()  # positions given explicitly, reversed within the batch: they must be used as given

    ps = {k: kfunca.from_numpy(v, 0) for k, v in w.items()}
    if dtype_bf16:
        ps = {k: v.bfloat16() for k, v in ps.items()}
    for p in ps.values():
        p.set_requires_grad(True)
    tc, ts = kfunca.from_numpy(c, 0), kfunca.from_numpy(s, 0)
    tpos, ttok, ttgt = kfunca.from_numpy(pos, 0), kfunca.from_numpy(tokens, 0), kfunca.from_numpy(target, 0)

    def forward():
        e = kfunca.embedding(ps["table"], ttok)
        h = kfunca.rms_norm(e, ps["norm"], 1e-5)
        qkv = kfunca.rope_qkv(kfunca.qkv_linear(h, ps["wqkv"]), tc, ts, B, S, Hh, positions=tpos)
        a = kfunca.causal_attention_qkv(qkv, B, S, Hh)
        x2 = kfunca.gemm_fused(a, ps["wo"], add=e)
        logits = kfunca.gemm(x2, ps["head"], 1.0, 0.0)
        return kfunca.cross_entropy(logits, ttgt)

    loss = forward()
    loss.backward(kfunca.from_numpy(np.ones(1, np.float32), 0))
    kgrads = {k: p.grad().float().numpy() if dtype_bf16 else p.grad().numpy() for k, p in ps.items()}

    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    e = t["table"][torch.tensor(tokens)]
    h = e * torch.rsqrt((e * e).mean(-1, keepdim=True) + 1e-5) * t["norm"]
    q, k, v = (z.reshape(B, S, Hh, D).permute(0, 2, 1, 3) for z in (h @ t["wqkv"]).split(d, -1))
    cc = torch.tensor(c, dtype=torch.float64)[torch.tensor(pos)].reshape(B, 1, S, D // 2)
    ss = torch.tensor(s, dtype=torch.float64)[torch.tensor(pos)].reshape(B, 1, S, D // 2)
    cos, sin = torch.cat([cc, cc], -1), torch.cat([ss, ss], -1)
    rot = lambda z: z * cos + torch.cat([-z[..., D // 2:], z[..., :D // 2]], -1) * sin  # noqa: E731
    a = F.scaled_dot_product_attention(rot(q), rot(k), v, is_causal=True)
    x2 = a.permute(0, 2, 1, 3).reshape(B * S, d) @ t["wo"] + e
    rl = F.cross_entropy(x2 @ t["head"], torch.tensor(target))
    rl.backward()
    tgrads = {k: v.grad.numpy() for k, v in t.items()}
    return float(loss.numpy()[0]), kgrads, rl.item(), tgrads, ps, forward


@pytest.mark.parametrize("bf16", [False, True])
def test_attention_model_end_to_end_and_one_adamw_step(bf16):
    loss, kg, rloss, tg, ps, forward = attention_model(bf16)
    if not bf16:
        assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
        for k in kg:
            assert_close(kg[k], tg[k], rtol=1e-3, atol=1e-5, what=f"d {k}")
    else:
        assert abs(loss - rloss) <= 2e-2 * abs(rloss), (loss, rloss)
        for k in kg:
            scale = np.abs(tg[k]).max()
            assert np.abs(kg[k] - tg[k]).max() <= 0.06 * scale, (k, float(np.abs(kg[k] - tg[k]).max()), float(scale))
    opt = kfunca.AdamW(list(ps.values()), lr=3e-3, weight_decay=0.0)
    opt.step()
    after = float(forward().numpy()[0])
    assert after < loss, (loss, after)


@pytest.mark.slow
def test_packed_bf16_beyond_2_31_elements():
    """Packed bf16 [176128, 12288] (2.16e9 elements, 4.3 GB each way): B 43 x S 4096, H 32, D 128, no positions. The input is a 61-row
    random tile repeated down the rows; tokens on both sides of element 2^31 are checked, in both directions of the ABI."""
    B, S, Hq, D = 43, 4096, 32, 128
    W, T = 3 * Hq * D, 43 * 4096
    assert T * W > 1 << 31
    rng = np.random.default_rng(41)
    tile, tile64 = make(rng, H.BF16, (61, W))
    bx, by = H.DevBuf(T * W * 2), H.DevBuf(T * W * 2)
    for r0 in range(0, T, 61):
        n = min(61, T - r0)
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r0 * W * 2, tile.ctypes.data, n * W * 2, None))
    c, s = tables(S, D)
    bc, bs = H.DevBuf.from_numpy(c), H.DevBuf.from_numpy(s)
    lay = (S * W, D, W)
    H.rope(H.BF16, B, 3 * Hq, S, D, bx.ptr, lay, by.ptr, lay, bc.ptr, bs.ptr, S, D, 2 * Hq)
    H.device_sync()
    edge = (1 << 31) // W
    for t in (0, edge - 1, edge, edge + 1, T - 1):
        row = np.empty(W, np.uint16)
        H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, by.ptr + t * W * 2, W * 2, None))
        x = tile64[t % 61].reshape(1, 3 * Hq, 1, D)
        cc, ss = c[t % S:t % S + 1], s[t % S:t % S + 1]
        want, bound, _ = ref(x, cc, ss, D, 2 * Hq)
        check(fl(row, H.BF16).reshape(1, 3 * Hq, 1, D), want, bound, H.BF16, f"token {t}")
