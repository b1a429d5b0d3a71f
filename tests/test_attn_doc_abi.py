"""CPU-only: the document-mask entries of the C ABI (kf_attn_doc_table, kf_attn_doc_fwd, kf_attn_doc_bwd) are declared and exported
and the ABI version is still 7; the attention entries refuse what kf_attn_full_* refuses - the INVALID table of
tests/test_attn_full_abi.py, restated for Sq = Skv = S - with the same statuses and their own name in the message, before any device
call; null tables, a causal flag outside {0, 1} and n_docs < 1 are refused; strided layouts off the matrix-core path are UNSUPPORTED;
zero extents are KF_OK without a launch; the workspace is the full family's; the operators' docstrings name doc_mask."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_attn_doc_table", "kf_attn_doc_fwd", "kf_attn_doc_bwd")
B, HQ, HKV, S, D = 2, 4, 2, 7, 64
SCALE = 0.125
OPS = ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        m = re.search(rf"\bint {n}\s*\(([^;]*)\);", text)
        assert m, f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
        if n != "kf_attn_doc_table":
            assert re.search(r"int64_t S,\s*int64_t D,\s*float scale,\s*int causal,\s*const int64_t \*kv_len,\s*const int32_t \*doc_start,\s*"
                             r"const int32_t \*doc_end,\s*const void \*q", m.group(1)), m.group(1)
            assert "Skv" not in m.group(1) and "prefix_len" not in m.group(1) and "window" not in m.group(1)
    m = re.search(r"\bint kf_attn_doc_table\s*\(([^;]*)\);", text)
    assert re.search(r"int64_t B,\s*int64_t S,\s*int64_t n_docs,\s*const int64_t \*cu_doclens,\s*int64_t \*kv_len,\s*int32_t \*doc_start,\s*"
                     r"int32_t \*doc_end,\s*void \*stream", m.group(1)), m.group(1)
    assert H.lib().kf_abi_version() == 7          # entries were added, none changed
    for n in ("attn_doc_table", "attn_doc_fwd", "attn_doc_bwd"):
        assert callable(getattr(H, n))


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in OPS + ("lse", "ws", "kv_len", "doc_start", "doc_end", "cu"):
            setattr(self, n, (C.c_double * (B * HQ * S * D // 2 + 8))())

    def p(self, name, off=0):
        if name is None:
            return None
        a = C.addressof(getattr(self, name))
        return (a + 15) // 16 * 16 + off


def lay(t):
    return None if t is None else C.byref(H.AttnLayout(*t))


CONTIG = {n: None for n in OPS}
W = (HQ + 2 * HKV) * D
PACKED = dict(q=(S * W, D, W), k=(S * W, D, W), v=(S * W, D, W), o=(S * HQ * D, D, HQ * D), d_o=(S * HQ * D, D, HQ * D),
              dq=(S * W, D, W), dk=(S * W, D, W), dv=(S * W, D, W))


def fwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, s=S, d=D, scale=SCALE, lays=None, null=(), off=None, lse="lse", causal=0, kv_len="kv_len",
        doc_start="doc_start", doc_end="doc_end"):
    lays, off = lays or CONTIG, off or {}
    a = []
    for n in ("q", "k", "v", "o"):
        a += [b.p(None if n in null else n, off.get(n, 0)), lay(lays[n])]
    return H.lib().kf_attn_doc_fwd(dtype, Bn, hq, hkv, s, d, scale, causal, b.p(kv_len), b.p(doc_start), b.p(doc_end), *a, b.p(lse), None)


def bwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, s=S, d=D, scale=SCALE, lays=None, null=(), off=None, ws="ws", ws_bytes=1 << 16, lse="lse", causal=0,
        kv_len="kv_len", doc_start="doc_start", doc_end="doc_end"):
    lays, off = lays or CONTIG, off or {}
    p = lambda n: b.p(None if n in null else n, off.get(n, 0))  # noqa: E731
    return H.lib().kf_attn_doc_bwd(dtype, Bn, hq, hkv, s, d, scale, causal, b.p(kv_len), b.p(doc_start), b.p(doc_end), p("q"), lay(lays["q"]), p("k"),
                                   lay(lays["k"]), p("v"), lay(lays["v"]), p("o"), lay(lays["o"]), b.p(lse), p("d_o"), lay(lays["d_o"]), p("dq"),
                                   lay(lays["dq"]), p("dk"), lay(lays["dk"]), p("dv"), lay(lays["dv"]), b.p(ws), ws_bytes, None)


def mixed(names):
    return {n: (PACKED[n] if n in names else None) for n in OPS}


def bad_stride(name, t):
    return dict(PACKED, **{name: t})


# the full family's table with Sq = Skv = S: S = 0 is its "Skv must be positive", a negative S its "negative extent"
INVALID = [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(d=0), "head size"), (dict(d=257), "head size"), (dict(d=-8), "head size"),
    (dict(hkv=0), "Hkv"), (dict(hkv=8), "Hkv"), (dict(hkv=3), "Hkv"), (dict(hkv=-1), "Hkv"),
    (dict(s=0), "Skv"), (dict(s=-3), "negative extent"),
    (dict(Bn=-1), "negative extent"), (dict(hq=-4), "negative extent"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(null=("q",)), "null"), (dict(null=("v",)), "null"), (dict(null=("o",)), "null"),
    (dict(lays=mixed(("q",))), "all NULL"), (dict(lays=mixed(("q", "k", "v"))), "all NULL"),
    (dict(lays=bad_stride("k", (S * W, D, W + 4))), "multiples of 8"), (dict(lays=bad_stride("q", (-8, D, W))), "multiples of 8"),
    (dict(lays=PACKED, off={"v": 8}), "16-byte aligned"), (dict(off={"q": 1}), "aligned to its element"),
    # this family's own
    (dict(doc_start=None), "doc_start"), (dict(doc_end=None), "doc_end"), (dict(doc_start=None, doc_end=None, lays=PACKED), "doc_start"),
]


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("kw,what", INVALID)
def test_forward_refuses(kw, what, causal):
    rc = fwd(Bufs(), causal=causal, **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_doc_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("kw,what", INVALID + [
    (dict(null=("d_o",)), "null"), (dict(null=("dq",)), "null"), (dict(null=("dk",)), "null"), (dict(null=("dv",)), "null"), (dict(lse=None), "null"),
    (dict(lays=mixed(("q", "k", "v", "o"))), "all NULL"),
    (dict(lays=bad_stride("dk", (S * W, D + 2, W))), "multiples of 8"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=B * HQ * S * 4 - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
])
def test_backward_refuses(kw, what, causal):
    rc = bwd(Bufs(), causal=causal, **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_doc_bwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("causal", [2, -1, 7, 1 << 20])
def test_a_causal_flag_outside_0_1_is_invalid(causal):
    """refused first: with a zero extent, which would otherwise be KF_OK, and with NULL operands, which would otherwise be the refusal"""
    for call, name in ((fwd, "kf_attn_doc_fwd"), (bwd, "kf_attn_doc_bwd")):
        for kw in ({}, dict(Bn=0), dict(null=OPS), dict(lays=PACKED)):
            rc = call(Bufs(), causal=causal, **kw)
            assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
            assert name in last_error() and "causal" in last_error() and "null" not in last_error(), last_error()


def table(b, Bn=B, s=S, n=3, cu="cu", kv_len="kv_len", doc_start="doc_start", doc_end="doc_end"):
    return H.lib().kf_attn_doc_table(Bn, s, n, b.p(cu), b.p(kv_len), b.p(doc_start), b.p(doc_end), None)


@pytest.mark.parametrize("kw,what", [
    (dict(n=0), "n_docs"), (dict(n=-1), "n_docs"), (dict(Bn=-1), "negative extent"), (dict(s=-2), "negative extent"),
    (dict(cu=None), "null"), (dict(kv_len=None), "null"), (dict(doc_start=None), "null"), (dict(doc_end=None), "null"),
    (dict(n=0, Bn=0), "n_docs"), (dict(cu=None, s=0), "null"),
])
def test_table_refuses(kw, what):
    rc = table(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_doc_table" in last_error() and what in last_error(), last_error()


def test_table_zero_extents_are_ok_without_a_launch():
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    assert table(b, Bn=0) == H.KF_OK, last_error()
    assert table(b, s=0) == H.KF_OK, last_error()
    assert table(b, Bn=0, s=0, n=1) == H.KF_OK, last_error()


@pytest.mark.parametrize("kw", [dict(dtype=H.F32), dict(d=80), dict(d=256), dict(dtype=H.F16, d=8)])
def test_strided_layouts_off_the_matrix_core_path_are_unsupported(kw):
    for call, name in ((fwd, "kf_attn_doc_fwd"), (bwd, "kf_attn_doc_bwd")):
        rc = call(Bufs(), lays=PACKED, **kw)
        assert rc == H.KF_ERR_UNSUPPORTED, (kw, rc, last_error())
        assert "matrix-core" in last_error() and name in last_error()


@pytest.mark.parametrize("kw", [dict(Bn=0), dict(hq=0, hkv=0), dict(hq=0)])
def test_zero_extents_are_ok_without_a_launch(kw):
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for causal in (0, 1):
            assert fwd(b, dtype=dtype, causal=causal, **kw) == H.KF_OK, last_error()
            assert bwd(b, dtype=dtype, causal=causal, **kw) == H.KF_OK, last_error()
            assert fwd(b, dtype=dtype, lays=PACKED, d=64, causal=causal, **kw) == H.KF_OK, last_error()
            # nothing to launch: the tables are not looked at either, as the operands are not
            assert fwd(b, dtype=dtype, causal=causal, doc_start=None, doc_end=None, null=OPS, **kw) == H.KF_OK, last_error()
    # the checks of the arguments themselves still come first
    assert fwd(b, dtype=H.I64, **kw) == H.KF_ERR_INVALID
    assert bwd(b, s=0, **kw) == H.KF_ERR_INVALID
    assert fwd(b, d=300, **kw) == H.KF_ERR_INVALID


def test_the_workspace_is_the_full_family_s():
    """no second query: the backward accepts exactly what kf_attn_full_bwd_workspace_bytes states for (S, S), and names it in its refusal"""
    need = H.attn_full_bwd_workspace_bytes(H.BF16, B, HQ, HKV, S, S, D)
    assert not hasattr(H.lib(), "kf_attn_doc_bwd_workspace_bytes")
    assert "kf_attn_doc_bwd_workspace_bytes" not in H.EXPORTS
    assert bwd(Bufs(), ws_bytes=need - 256) == H.KF_ERR_INVALID and "kf_attn_full_bwd_workspace_bytes" in last_error()


def test_operator_docstrings():
    for n in ("attention", "attention_qkv"):
        doc = getattr(kfunca, n).__doc__
        assert "doc_mask" in doc and "window" in doc and "causal" in doc and "prefix_len" in doc and "kv_len" in doc, doc
    doc = kfunca.attention.__doc__
    assert "DocMask" in doc and "same document" in doc and "refused" in doc and "Sq = Skv" in doc, doc
    assert "cu_doclens" in kfunca.doc_mask.__doc__ and "doc_mask" in kfunca.__all__ and callable(kfunca.doc_mask)
    for n in ("kv_len", "doc_start", "doc_end", "B", "S"):
        assert hasattr(kfunca.DocMask, n), n
