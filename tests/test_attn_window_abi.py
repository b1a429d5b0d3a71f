"""CPU-only: the sliding-window attention entries of the C ABI (kf_attn_window_fwd, kf_attn_window_bwd) are declared and exported, refuse
what kf_attn_full_* refuses - the INVALID table of tests/test_attn_full_abi.py, restated - with the same statuses and their own name in
the message, before any device call; a window side below -1 is refused before anything is dereferenced; zero extents are KF_OK without a
launch; the workspace is the full family's; the operators' docstrings name window."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_attn_window_fwd", "kf_attn_window_bwd")
B, HQ, HKV, SQ, SKV, D = 2, 4, 2, 5, 7, 64
SCALE = 0.125
OPS = ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        m = re.search(rf"\bint {n}\s*\(([^;]*)\);", text)
        assert m, f"{n} not declared"
        assert re.search(r"const int64_t \*kv_len,\s*int64_t window_left,\s*int64_t window_right,\s*const void \*q", m.group(1)), m.group(1)
        assert "prefix_len" not in m.group(1)
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert H.lib().kf_abi_version() == 7          # entries were added, none changed
    for n in ("attn_window_fwd", "attn_window_bwd"):
        assert callable(getattr(H, n))


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in OPS + ("lse", "ws", "kv_len"):
            setattr(self, n, (C.c_double * (B * HQ * SKV * D // 2 + 8))())

    def p(self, name, off=0):
        if name is None:
            return None
        a = C.addressof(getattr(self, name))
        return (a + 15) // 16 * 16 + off


def lay(t):
    return None if t is None else C.byref(H.AttnLayout(*t))


CONTIG = {n: None for n in OPS}
W = (HQ + 2 * HKV) * D
PACKED = dict(q=(SKV * W, D, W), k=(SKV * W, D, W), v=(SKV * W, D, W), o=(SKV * HQ * D, D, HQ * D), d_o=(SKV * HQ * D, D, HQ * D),
              dq=(SKV * W, D, W), dk=(SKV * W, D, W), dv=(SKV * W, D, W))


def fwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, sq=SQ, skv=SKV, d=D, scale=SCALE, lays=None, null=(), off=None, lse="lse", wl=2, wr=0):
    lays, off = lays or CONTIG, off or {}
    a = []
    for n in ("q", "k", "v", "o"):
        a += [b.p(None if n in null else n, off.get(n, 0)), lay(lays[n])]
    return H.lib().kf_attn_window_fwd(dtype, Bn, hq, hkv, sq, skv, d, scale, b.p("kv_len"), wl, wr, *a, b.p(lse), None)


def bwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, sq=SQ, skv=SKV, d=D, scale=SCALE, lays=None, null=(), off=None, ws="ws", ws_bytes=1 << 16, lse="lse",
        wl=2, wr=0):
    lays, off = lays or CONTIG, off or {}
    p = lambda n: b.p(None if n in null else n, off.get(n, 0))  # noqa: E731
    return H.lib().kf_attn_window_bwd(dtype, Bn, hq, hkv, sq, skv, d, scale, b.p("kv_len"), wl, wr, p("q"), lay(lays["q"]), p("k"),
                                      lay(lays["k"]), p("v"), lay(lays["v"]), p("o"), lay(lays["o"]), b.p(lse), p("d_o"), lay(lays["d_o"]), p("dq"),
                                      lay(lays["dq"]), p("dk"), lay(lays["dk"]), p("dv"), lay(lays["dv"]), b.p(ws), ws_bytes, None)


def mixed(names):
    return {n: (PACKED[n] if n in names else None) for n in OPS}


def bad_stride(name, t):
    return dict(PACKED, **{name: t})


INVALID = [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(d=0), "head size"), (dict(d=257), "head size"), (dict(d=-8), "head size"),
    (dict(hkv=0), "Hkv"), (dict(hkv=8), "Hkv"), (dict(hkv=3), "Hkv"), (dict(hkv=-1), "Hkv"),
    (dict(skv=0), "Skv"), (dict(skv=-3), "negative extent"),
    (dict(Bn=-1), "negative extent"), (dict(hq=-4), "negative extent"), (dict(sq=-1), "negative extent"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(null=("q",)), "null"), (dict(null=("v",)), "null"), (dict(null=("o",)), "null"),
    (dict(lays=mixed(("q",))), "all NULL"), (dict(lays=mixed(("q", "k", "v"))), "all NULL"),
    (dict(lays=bad_stride("k", (SKV * W, D, W + 4))), "multiples of 8"), (dict(lays=bad_stride("q", (-8, D, W))), "multiples of 8"),
    (dict(lays=PACKED, off={"v": 8}), "16-byte aligned"), (dict(off={"q": 1}), "aligned to its element"),
]
# the table holds for every kind of window, the two that are served by the older families' kernels included
WINDOWS = [(2, 0), (3, 3), (-1, 0), (-1, -1), (0, -1)]


@pytest.mark.parametrize("wl,wr", WINDOWS)
@pytest.mark.parametrize("kw,what", INVALID)
def test_forward_refuses(kw, what, wl, wr):
    rc = fwd(Bufs(), wl=wl, wr=wr, **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_window_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("wl,wr", WINDOWS)
@pytest.mark.parametrize("kw,what", INVALID + [
    (dict(null=("d_o",)), "null"), (dict(null=("dq",)), "null"), (dict(null=("dk",)), "null"), (dict(null=("dv",)), "null"), (dict(lse=None), "null"),
    (dict(lays=mixed(("q", "k", "v", "o"))), "all NULL"),
    (dict(lays=bad_stride("dk", (SKV * W, D + 2, W))), "multiples of 8"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=B * HQ * SQ * 4 - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
])
def test_backward_refuses(kw, what, wl, wr):
    rc = bwd(Bufs(), wl=wl, wr=wr, **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_window_bwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("wl,wr", [(-2, 0), (0, -2), (-2, -2), (-1, -5), (-(2 ** 62), 3), (4, -(2 ** 40))])
def test_a_window_side_below_minus_one_is_invalid(wl, wr):
    """refused with otherwise valid arguments, host pointers for every operand (nothing may be dereferenced or launched), and first: with
    a zero extent, which would otherwise be KF_OK, and with NULL operands, which would otherwise be the refusal"""
    for call, name in ((fwd, "kf_attn_window_fwd"), (bwd, "kf_attn_window_bwd")):
        for kw in ({}, dict(Bn=0), dict(sq=0), dict(null=OPS), dict(lays=PACKED)):
            rc = call(Bufs(), wl=wl, wr=wr, **kw)
            assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
            assert name in last_error() and "window" in last_error() and "null" not in last_error(), last_error()


@pytest.mark.parametrize("kw", [dict(dtype=H.F32), dict(d=80), dict(d=256), dict(dtype=H.F16, d=8)])
def test_strided_layouts_off_the_matrix_core_path_are_unsupported(kw):
    for call, name in ((fwd, "kf_attn_window_fwd"), (bwd, "kf_attn_window_bwd")):
        rc = call(Bufs(), lays=PACKED, **kw)
        assert rc == H.KF_ERR_UNSUPPORTED, (kw, rc, last_error())
        assert "matrix-core" in last_error() and name in last_error()


@pytest.mark.parametrize("kw", [dict(Bn=0), dict(hq=0, hkv=0), dict(hq=0), dict(sq=0)])
def test_zero_extents_are_ok_without_a_launch(kw):
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for wl, wr in WINDOWS:
            assert fwd(b, dtype=dtype, wl=wl, wr=wr, **kw) == H.KF_OK, last_error()
            assert bwd(b, dtype=dtype, wl=wl, wr=wr, **kw) == H.KF_OK, last_error()
            assert fwd(b, dtype=dtype, lays=PACKED, d=64, wl=wl, wr=wr, **kw) == H.KF_OK, last_error()
    # the checks of the arguments themselves still come first
    assert fwd(b, dtype=H.I64, **kw) == H.KF_ERR_INVALID
    assert bwd(b, skv=0, **kw) == H.KF_ERR_INVALID
    assert fwd(b, d=300, **kw) == H.KF_ERR_INVALID


def test_the_workspace_is_the_full_family_s():
    """no second query: the backward accepts exactly what kf_attn_full_bwd_workspace_bytes states, and names it in its refusal"""
    need = H.attn_full_bwd_workspace_bytes(H.BF16, B, HQ, HKV, SQ, SKV, D)
    assert not hasattr(H.lib(), "kf_attn_window_bwd_workspace_bytes")
    assert "kf_attn_window_bwd_workspace_bytes" not in H.EXPORTS
    assert bwd(Bufs(), ws_bytes=need - 256) == H.KF_ERR_INVALID and "kf_attn_full_bwd_workspace_bytes" in last_error()


def test_operator_docstrings():
    for n in ("attention", "attention_qkv"):
        doc = getattr(kfunca, n).__doc__
        assert "window" in doc and "causal" in doc and "prefix_len" in doc and "kv_len" in doc, doc
    doc = kfunca.attention.__doc__
    assert "(left, right)" in doc and "unbounded" in doc and "right = 0" in doc and "refused" in doc, doc
