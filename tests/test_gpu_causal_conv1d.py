"""-m gpu: kf_causal_conv1d_fwd / _bwd against the float64 reference of tests/causal_conv1d_ref.py on the inputs as stored. Every output
lies between 64 guard elements in a buffer filled with 0xA5 (the workspace too), and the guards and the padding columns C..ld of y and dx
must come back untouched. R = 64 is the rows a wave walks, 4 R the rows of a workgroup.

Bounds |got - ref| <= u |ref| + n 2^-23 (absref + |ref|) (+ the measured SiLU term of the reference module), u = 2^-8 / 2^-11 / 0, with n
counted from the f32 operations the kernel issues, each rounding at most 2^-24 of the running absolute sum:
  y         n = K + 1: K fused multiply-adds from the bias up (K / 2), carried through SiLU with slope <= 1.1, and SiLU's own product
  dx, d_h0  n = K + 2: the K fused multiply-adds on d_hT (K / 2), the product dy act' (1 / 2), and pre's K / 2 through act' (in absref)
  dw, dbias n = R + 3 + W + K + 2: one fused multiply-add per row of a wave's walk (R), the three additions of the four waves, the W - 1
            additions over the W = B ceil(S / 4R) workgroup partials, and every term's own dpre (K + 2, as for dx)
hT is copies and is compared bit for bit."""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V
from tests.causal_conv1d_ref import ROWS as R, bound, reference, stored

pytestmark = pytest.mark.gpu
CODE, ES, GUARD = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}, {"bf16": 2, "f16": 2, "f32": 4}, 64
ALL = ("bias", "h0", "hT", "d_hT", "d_h0", "dbias")
value = lambda bits, dt: V.decode(bits.view(np.float32) if dt == "f32" else bits, dt)   # an output's stored bits -> float64


def put(a, dt, ld=None):
    """a [..., C] -> a device buffer of rows at leading dimension ld, 0xA5 in the padding columns"""
    rows = a.reshape(-1, a.shape[-1])
    host = np.full((rows.shape[0], ld or rows.shape[1]), 0xA5A5A5A5 if ES[dt] == 4 else 0xA5A5, np.uint32 if ES[dt] == 4 else np.uint16)
    host[:, :rows.shape[1]] = V.encode(rows, dt).view(host.dtype)
    return H.DevBuf.from_numpy(host)


class Out:
    """[rows, C] at leading dimension ld between guards, all of it 0xA5 before the call"""

    def __init__(self, rows, C, ld, dt):
        self.rows, self.C, self.ld, self.dt = rows, C, ld, dt
        self.buf = H.DevBuf.from_numpy(np.full((2 * GUARD + rows * ld) * ES[dt], 0xA5, np.uint8))
        self.ptr = self.buf.ptr + GUARD * ES[dt]

    def bits(self):
        raw = self.buf.to_numpy((2 * GUARD + self.rows * self.ld,), np.uint32 if ES[self.dt] == 4 else np.uint16)
        poison = 0xA5A5A5A5 if ES[self.dt] == 4 else 0xA5A5
        body = raw[GUARD:-GUARD].reshape(self.rows, self.ld)
        assert (raw[:GUARD] == poison).all() and (raw[-GUARD:] == poison).all() and (body[:, self.C:] == poison).all(), "guard or padding written"
        return body[:, :self.C].copy()


def draw(dt, K, B, S, C, seed=0):
    rng = np.random.default_rng(seed + 1000 * K + S)
    u = lambda *shape: stored(rng.uniform(-2, 2, shape), dt)
    return dict(x=u(B, S, C), w=u(K, C), bias=u(C), h0=u(B, K - 1, C), dy=u(B, S, C), d_hT=u(B, K - 1, C))


def run(dt, K, silu, a, ldx=None, ldo=None, have=ALL, h0=None, d_hT=None):
    """forward and backward through the C ABI -> the outputs' stored bits; h0 / d_hT: device pointers that replace the drawn ones"""
    (B, S, C), code, act = a["x"].shape, CODE[dt], H.CONV1D_ACT_SILU if silu else H.CONV1D_ACT_NONE
    ldx, ldo = ldx or C, ldo or C
    dev = {n: put(a[n], dt, ldx if n in ("x", "dy") else None) for n in a}
    opt = lambda n: dev[n].ptr if n in have else None
    h0, d_hT = h0 or opt("h0"), d_hT or opt("d_hT")
    out = dict(y=Out(B * S, C, ldo, dt), dx=Out(B * S, C, ldo, dt), dw=Out(K, C, C, dt), **{n: Out(B * (K - 1), C, C, dt) for n in ("hT", "d_h0")},
               dbias=Out(1, C, C, dt))
    need = H.causal_conv1d_bwd_workspace_bytes(code, B, S, C, K)
    ws = H.DevBuf.from_numpy(np.full(need, 0xA5, np.uint8))
    o = lambda n: out[n].ptr if n in have or n in ("y", "dx", "dw") else None
    H.causal_conv1d_fwd(code, act, B, S, C, K, dev["x"].ptr, ldx, dev["w"].ptr, opt("bias"), h0, out["y"].ptr, ldo, o("hT"))
    H.causal_conv1d_bwd(code, act, B, S, C, K, dev["x"].ptr, ldx, dev["w"].ptr, opt("bias"), h0, dev["dy"].ptr, ldx, d_hT, out["dx"].ptr, ldo,
                        out["dw"].ptr, o("dbias"), o("d_h0"), ws.ptr, need)
    H.device_sync()
    got = {n: b.bits() for n, b in out.items()}
    assert all((got[n].view(np.uint8) == 0xA5).all() for n in ("hT", "d_h0", "dbias") if n not in have), "an output that was not asked for was written"
    return got, out


def check(dt, K, silu, a, got, have=ALL):
    (B, S, C), dec = a["x"].shape, lambda n, shape: value(got[n], dt).reshape(shape)
    ref, absref = reference(a["x"], a["w"], a["bias"] if "bias" in have else None, a["h0"] if "h0" in have else None, silu, a["dy"],
                            a["d_hT"] if "d_hT" in have else None)
    W = B * -(-S // (4 * R))
    for n, key, shape, count in (("y", "y", (B, S, C), K + 1), ("dx", "dx", (B, S, C), K + 2), ("d_h0", "dh0", (B, K - 1, C), K + 2),
                                 ("dw", "dw", (K, C), R + 3 + W + K + 2), ("dbias", "dbias", (C,), R + 3 + W + K + 2)):
        if n in have or n in ("y", "dx", "dw"):
            excess = np.abs(dec(n, shape) - ref[key]) - bound(ref[key], absref[key], dt, count, silu)
            assert excess.max() <= 0, (n, np.unravel_index(excess.argmax(), shape), excess.max())
    if "hT" in have:
        assert np.array_equal(got["hT"], V.encode(ref["hT"], dt).view(got["hT"].dtype).reshape(got["hT"].shape)), "hT is not a copy"


def sizes(K):   # shorter than the state, the state, one wave less one / exactly / plus one, a workgroup seam with a tail
    return sorted({1, max(K - 2, 1), K - 1, K, R - 1, R, R + 1, 4 * R + K - 2})


def shape(dt, which):   # one pack, one lane's worth; or more than a wave row of packs with a tail pack, and a row stride
    pack = 16 // ES[dt]
    return (1, pack, pack) if which == 0 else (3, 65 * pack, 67 * pack)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_every_variant_twice(dt, K, silu):
    B, C, ld = shape(dt, 1)
    a = draw(dt, K, B, 4 * R + K - 2, C)
    got, _ = run(dt, K, silu, a, ld, ld)
    check(dt, K, silu, a, got)
    again, _ = run(dt, K, silu, a, ld, ld)
    assert all(np.array_equal(got[n], again[n]) for n in got), "a second call gave other bits"


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("dt,silu", [("bf16", True), ("f32", False)])
@pytest.mark.parametrize("K,S", [(K, S) for K in (2, 3, 4) for S in sizes(K)])
def test_sequence_lengths(K, S, dt, silu, which):
    B, C, ld = shape(dt, which)
    a = draw(dt, K, B, S, C)
    check(dt, K, silu, a, run(dt, K, silu, a, ld, ld)[0])


@pytest.mark.parametrize("have", [(), ("bias",), ("h0",), ("hT",), ("d_hT",), ("h0", "d_h0"), ("dbias",)])
def test_optional_operands(have):
    B, C, ld = shape("bf16", 1)
    a = draw("bf16", 3, B, R + 1, C)
    check("bf16", 3, True, a, run("bf16", 3, True, a, ld, ld, have)[0], have)


def test_the_step_in_place_equals_the_call_out_of_place():
    """S = 3 <= R: hT may be h0 and y may be x"""
    dt, K, code = "bf16", 4, H.BF16
    B, C, ld = shape(dt, 1)
    a = draw(dt, K, B, 3, C)
    want, _ = run(dt, K, True, a, ld, ld)
    x, w, bias, state = put(a["x"], dt, ld), put(a["w"], dt), put(a["bias"], dt), put(a["h0"], dt)
    H.causal_conv1d_fwd(code, H.CONV1D_ACT_SILU, B, 3, C, K, x.ptr, ld, w.ptr, bias.ptr, state.ptr, x.ptr, ld, state.ptr)
    H.device_sync()
    assert np.array_equal(x.to_numpy((B * 3, ld), np.uint16)[:, :C], want["y"]) and np.array_equal(state.to_numpy((B * 3, C), np.uint16), want["hT"])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_two_segments_chained_through_the_state(dt):
    """hT -> h0 forward, d_h0 -> d_hT backward. y has the bits of one call. So has dx in f32, where a segment's d_h0 is exactly the head of
    the chain the whole sequence runs; in 16 bits d_h0 is rounded on its way to the first segment, so the K - 1 rows in front of the cut
    carry that one rounding more (u |d_h0|) and every other row has the bits of one call. dw adds up within the sum of the two bounds."""
    K, silu, cut = 4, True, R + 1
    B, C, ld = shape(dt, 1)
    S = 4 * R + 2
    a = draw(dt, K, B, S, C)
    whole, _ = run(dt, K, silu, a, ld, ld)
    part = lambda lo, hi: dict(a, x=a["x"][:, lo:hi], dy=a["dy"][:, lo:hi])
    one, out1 = run(dt, K, silu, part(0, cut), ld, ld)                      # forward of the first segment (its backward waits for d_h0)
    two, out2 = run(dt, K, silu, part(cut, S), ld, ld, h0=out1["hT"].ptr)
    one, _ = run(dt, K, silu, part(0, cut), ld, ld, d_hT=out2["d_h0"].ptr)
    rows = lambda g, n, s: g[n].reshape(B, s, C)
    assert np.array_equal(np.concatenate([rows(one, "y", cut), rows(two, "y", S - cut)], 1), rows(whole, "y", S))
    assert np.array_equal(two["hT"], whole["hT"]) and (dt != "f32" or np.array_equal(one["d_h0"], whole["d_h0"]))
    dx, want = np.concatenate([rows(one, "dx", cut), rows(two, "dx", S - cut)], 1), rows(whole, "dx", S)
    near = slice(cut - (K - 1), cut)
    if dt == "f32":
        assert np.array_equal(dx, want)
    else:
        far = np.ones(S, bool)
        far[near] = False
        assert np.array_equal(dx[:, far], want[:, far])
    hT1 = value(one["hT"], dt).reshape(B, K - 1, C)
    dh0_2 = value(two["d_h0"], dt).reshape(B, K - 1, C)
    ref, absref = reference(a["x"], a["w"], a["bias"], a["h0"], silu, a["dy"], a["d_hT"])
    r1, a1 = reference(a["x"][:, :cut], a["w"], a["bias"], a["h0"], silu, a["dy"][:, :cut], dh0_2)
    r2, a2 = reference(a["x"][:, cut:], a["w"], a["bias"], hT1, silu, a["dy"][:, cut:], a["d_hT"])
    lim = bound(ref["dx"], absref["dx"], dt, K + 2, silu)[:, near] + (2.0 ** -8 if dt == "bf16" else 0) * np.abs(dh0_2)
    assert (np.abs(value(dx, dt)[:, near] - ref["dx"][:, near]) <= lim).all()
    n1, n2 = R + 3 + B + K + 2, R + 3 + B + K + 2   # each segment lies within one workgroup per batch row
    for n, shp in (("dw", (K, C)), ("dbias", (C,))):
        both = value(one[n], dt).reshape(shp) + value(two[n], dt).reshape(shp)
        assert (np.abs(both - ref[n]) <= bound(r1[n], a1[n], dt, n1, silu) + bound(r2[n], a2[n], dt, n2, silu)).all(), n
