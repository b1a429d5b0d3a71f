"""CPU-only: the fused QK-norm + rotary entries of the C ABI (kf_qk_norm_rope_fwd, kf_qk_norm_rope_bwd_workspace_bytes, kf_qk_norm_rope_bwd)
are declared and exported, every invalid argument is refused with KF_ERR_INVALID and a message that names the entry and the reason before
any device call, zero extents are KF_OK without a launch, the allowed aliases pass and every other overlap is refused, the workspace
query answers without a device, a valid call without a device reports an error instead of falling back to a CPU path, and the operator
surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_qk_norm_rope_fwd", "kf_qk_norm_rope_bwd_workspace_bytes", "kf_qk_norm_rope_bwd")
B, S, HQ, HK, HV, D, P = 2, 3, 2, 1, 1, 8, 4
T, W, LD = B * S, (HQ + HK + HV) * D, (HQ + HK + HV) * D + 8
INF, NAN = float("inf"), float("nan")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("x", "y", "dy", "dx"):
            setattr(self, n, (C.c_float * (T * LD + 16))())
        for n in ("wq", "wk", "dwq", "dwk"):
            setattr(self, n, (C.c_float * (D + 4))())
        self.cos, self.sin = (C.c_float * (P * D))(), (C.c_float * (P * D))()
        self.pos = (C.c_int64 * T)()
        self.ws = (C.c_float * (T * 2 * D + 4))()

    def p(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off


def fwd(b, dtype=H.F32, Bn=B, Sn=S, hq=HQ, hk=HK, hv=HV, d=D, R=D, il=0, eps=1e-6, wq="wq", wk="wk", cos="cos", sin="sin", rows=P, pos="pos",
        x="x", ldx=LD, y="y", ldy=LD, off=None):
    off = off or {}
    o = lambda role, n: b.p(n, off.get(role, 0))  # noqa: E731  (an offset belongs to the argument, whichever buffer stands in for it)
    return H.lib().kf_qk_norm_rope_fwd(dtype, Bn, Sn, hq, hk, hv, d, R, il, eps, o("wq", wq), o("wk", wk), o("cos", cos), o("sin", sin), rows,
                                       o("pos", pos), o("x", x), ldx, o("y", y), ldy, None)


def bwd(b, dtype=H.F32, Bn=B, Sn=S, hq=HQ, hk=HK, hv=HV, d=D, R=D, il=0, eps=1e-6, wq="wq", wk="wk", cos="cos", sin="sin", rows=P, pos="pos",
        x="x", ldx=LD, dy="dy", lddy=LD, dx="dx", lddx=LD, dwq="dwq", dwk="dwk", ws="ws", ws_bytes=None, off=None):
    off = off or {}
    o = lambda role, n: b.p(n, off.get(role, 0))  # noqa: E731
    nbytes = C.sizeof(b.ws) if ws_bytes is None else ws_bytes
    return H.lib().kf_qk_norm_rope_bwd(dtype, Bn, Sn, hq, hk, hv, d, R, il, eps, o("wq", wq), o("wk", wk), o("cos", cos), o("sin", sin), rows,
                                       o("pos", pos), o("x", x), ldx, o("dy", dy), lddy, o("dx", dx), lddx, o("dwq", dwq), o("dwk", dwk), o("ws", ws),
                                       nbytes, None)


COMMON = [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(Bn=-1), "negative extents"), (dict(Sn=-2), "negative extents"), (dict(hq=-1), "negative extents"), (dict(hk=-1), "negative extents"),
    (dict(hv=-3), "negative extents"), (dict(d=-8), "negative extents"),
    (dict(hq=0, hk=0), "Hq + Hk"),
    (dict(R=7), "rotary_dim"), (dict(R=D + 2), "rotary_dim"), (dict(R=-2), "rotary_dim"),
    (dict(il=2), "interleaved"),
    (dict(eps=-1e-6), "eps"), (dict(eps=INF), "eps"), (dict(eps=NAN), "eps"),
    (dict(ldx=W - 1), "leading dimension of x"),
    (dict(x=None), "null x"),
    (dict(cos=None), "tables"), (dict(sin=None), "tables"),
    (dict(rows=0), "table_rows"), (dict(rows=-3), "table_rows"),
    (dict(pos=None, rows=S - 1), "positions"),
    (dict(off={"x": 2}), "x not aligned"), (dict(off={"wq": 1}), "aligned"), (dict(off={"cos": 2}), "aligned"), (dict(off={"pos": 4}), "aligned"),
]


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(ldy=W - 1), "leading dimension of y"), (dict(ldy=0), "leading dimension of y"),
    (dict(y=None), "null y"),
    (dict(off={"y": 3}), "y not aligned"),
    (dict(y="x", ldy=LD + 8), "overlaps"),              # in place with another leading dimension
    (dict(y="x", off={"y": 4}), "overlaps"),            # shifted into the input's rows
    (dict(y="x", off={"y": 4 * LD}, Bn=1), "overlaps"),  # one row further down
])
def test_forward_refuses(kw, what):
    rc = fwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_qk_norm_rope_fwd:" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(lddy=W - 1), "leading dimension of dy"), (dict(lddx=1), "leading dimension of dx"),
    (dict(dy=None), "null dy"), (dict(dx=None), "null dx"),
    (dict(off={"dy": 2}), "dy not aligned"), (dict(off={"dx": 1}), "dx not aligned"), (dict(off={"dwk": 2}), "aligned"),
    (dict(dx="x"), "dx overlaps x"), (dict(dx="x", off={"dx": 4 * (LD + 2)}, Bn=1), "dx overlaps x"),
    (dict(dx="dy", lddx=LD + 4), "dx overlaps dy"), (dict(dx="dy", off={"dx": 8}), "dx overlaps dy"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=T * 2 * D * 4 - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
    (dict(off={"ws": 2}), "workspace"),
])
def test_backward_refuses(kw, what):
    rc = bwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_qk_norm_rope_bwd:" in last_error() and what in last_error(), last_error()


def test_16_bit_bases_need_two_byte_alignment_only():
    b = Bufs()
    assert fwd(b, dtype=H.BF16, Bn=0, off={"x": 2, "y": 6, "wq": 2}) == H.KF_OK
    assert bwd(b, dtype=H.F16, Bn=0, off={"x": 2, "dy": 10, "dx": 14, "dwq": 2}) == H.KF_OK
    assert fwd(b, dtype=H.BF16, off={"x": 1}) == H.KF_ERR_INVALID and "aligned" in last_error()
    assert bwd(b, dtype=H.F16, off={"dx": 3}) == H.KF_ERR_INVALID and "aligned" in last_error()


@pytest.mark.parametrize("kw", [dict(Bn=0), dict(Sn=0), dict(d=0, R=0), dict(Bn=0, Sn=0)])
def test_zero_extents_are_ok_without_a_launch(kw):
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        assert fwd(b, dtype=dtype, **kw) == H.KF_OK, last_error()
        assert bwd(b, dtype=dtype, **kw) == H.KF_OK, last_error()
    # the checks still come first
    assert fwd(b, dtype=H.F64, **kw) == H.KF_ERR_INVALID
    assert fwd(b, eps=-1.0, **kw) == H.KF_ERR_INVALID
    assert bwd(b, dx=None, **kw) == H.KF_ERR_INVALID
    assert bwd(b, hq=0, hk=0, **kw) == H.KF_ERR_INVALID


def test_norm_only_ignores_tables_and_positions():
    b = Bufs()
    kw = dict(R=0, cos=None, sin=None, pos=None, rows=0, Bn=0)
    assert fwd(b, **kw) == H.KF_OK, last_error()
    assert bwd(b, **kw) == H.KF_OK, last_error()
    if H.device_count() == 0:
        kw.pop("Bn")
        assert fwd(b, **kw) not in (H.KF_OK, H.KF_ERR_INVALID) and bwd(b, **kw) not in (H.KF_OK, H.KF_ERR_INVALID)


def test_optional_operands_may_be_null():
    b = Bufs()
    assert fwd(b, Bn=0, wq=None, wk=None) == H.KF_OK, last_error()
    assert bwd(b, Bn=0, wq=None, wk=None, dwq=None, dwk=None, ws=None, ws_bytes=0) == H.KF_OK, last_error()   # no weight sums: no workspace
    assert bwd(b, Bn=0, dwq=None) == H.KF_OK and bwd(b, Bn=0, dwk=None) == H.KF_OK
    assert bwd(b, Bn=0, hk=0, hv=0) == H.KF_OK and fwd(b, Bn=0, hq=0, hk=2) == H.KF_OK   # a lone q; no q at all


def test_allowed_aliases_pass_validation():
    b = Bufs()
    assert fwd(b, Bn=0, y="x") == H.KF_OK
    assert bwd(b, Bn=0, dx="dy") == H.KF_OK
    if H.device_count() == 0:
        # with extents: past validation (no KF_ERR_INVALID), and then no device to launch on
        assert fwd(b, y="x") not in (H.KF_OK, H.KF_ERR_INVALID), last_error()
        assert bwd(b, dx="dy") not in (H.KF_OK, H.KF_ERR_INVALID), last_error()


def test_workspace_query():
    need = C.c_size_t(1)
    q = H.lib().kf_qk_norm_rope_bwd_workspace_bytes
    assert q(H.F32, B, S, HQ, HK, HV, D, C.byref(need)) == H.KF_OK and need.value == T * 2 * D * 4
    assert H.qk_norm_rope_bwd_workspace_bytes(H.BF16, B, S, HQ, HK, HV, D) == T * 2 * D * 4
    # bounded in the number of tokens: one f32 row [2][D] per block of the backward's grid
    big = H.qk_norm_rope_bwd_workspace_bytes(H.BF16, 8, 4096, 32, 8, 8, 128)
    assert 0 < big <= 4096 * 2 * 128 * 4 and big % (2 * 128 * 4) == 0
    assert H.qk_norm_rope_bwd_workspace_bytes(H.BF16, 64, 4096, 32, 8, 8, 128) == big
    assert H.qk_norm_rope_bwd_workspace_bytes(H.F32, 0, S, HQ, HK, HV, D) == 0
    for args, what in (((H.F64, B, S, HQ, HK, HV, D), "dtype"), ((H.F32, -1, S, HQ, HK, HV, D), "negative extents"),
                       ((H.F32, B, S, 0, 0, HV, D), "Hq + Hk")):
        assert q(*args, C.byref(need)) == H.KF_ERR_INVALID
        assert "kf_qk_norm_rope_bwd_workspace_bytes" in last_error() and what in last_error(), last_error()
    assert q(H.F32, B, S, HQ, HK, HV, D, None) == H.KF_ERR_INVALID and "null" in last_error()


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        return  # (host pointers: never launched on a machine that has a device)
    b = Bufs()
    for il in (0, 1):
        assert fwd(b, il=il) != H.KF_OK and last_error()
        assert bwd(b, il=il) != H.KF_OK and last_error()
    assert fwd(b, dtype=H.BF16, R=4) != H.KF_OK and last_error()
    assert bwd(b, dtype=H.BF16, dwq=None, dwk=None, ws=None, ws_bytes=0) != H.KF_OK and last_error()


def test_operator_surface():
    assert "qk_norm_rope" in kfunca.__all__ and callable(kfunca.qk_norm_rope)
    doc = kfunca.qk_norm_rope.__doc__
    for what in ("rstd = 1 / sqrt(mean(x^2) + eps)", "single rounding", "keeps only its input", "1 + w", "kv_heads", "positions", "interleaved"):
        assert what in doc, what
    for n in ("qk_norm_rope_fwd", "qk_norm_rope_bwd", "qk_norm_rope_bwd_workspace_bytes"):
        assert callable(getattr(H, n)) and getattr(H, n).__doc__
