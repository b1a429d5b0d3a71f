"""CPU-only: the descriptor-based attention entries with score modifiers (kf_attn_ext_fwd, kf_attn_ext_bwd_workspace_bytes,
kf_attn_ext_bwd) are declared and exported, the ABI version stays 7, every invalid argument - kf_attn_full_*'s table (tests/
test_attn_full_abi.py, restated), a softcap that is negative or not finite, an unknown mask kind, mask fields that contradict the kind,
dsink without sink and sink without dsink - is KF_ERR_INVALID with the entry's name in the message before any device call (the operands
are host memory: nothing may be dereferenced or launched), and zero extents are KF_OK without a launch, with and without modifiers."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_attn_ext_fwd", "kf_attn_ext_bwd_workspace_bytes", "kf_attn_ext_bwd")
B, HQ, HKV, S, D = 2, 4, 2, 7, 64
SCALE = 0.125
OPS = ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        m = re.search(rf"\bint {n}\s*\(([^;]*)\);", text)
        assert m, f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
        if n != "kf_attn_ext_bwd_workspace_bytes":
            assert re.search(r"const kf_attn_mask \*mask,\s*float softcap,\s*const float \*sink,\s*const void \*q", m.group(1)), m.group(1)
    assert re.search(r"float \*dsink,\s*void \*workspace", re.search(r"\bint kf_attn_ext_bwd\s*\(([^;]*)\);", text).group(1))
    struct = re.search(r"typedef struct kf_attn_mask \{(.*?)\} kf_attn_mask;", text, flags=re.S).group(1)
    for field in ("kind", "kv_len", "prefix_len", "window_left", "window_right", "doc_start", "doc_end", "causal"):
        assert re.search(rf"\b{field}\b", struct), field
    assert H.lib().kf_abi_version() == 7          # entries were added, none changed
    for n in ("attn_ext_fwd", "attn_ext_bwd_workspace_bytes", "attn_ext_bwd", "attn_mask", "AttnMask"):
        assert callable(getattr(H, n))
    assert (H.ATTN_MASK_FULL, H.ATTN_MASK_PREFIX, H.ATTN_MASK_WINDOW, H.ATTN_MASK_DOC) == (0, 1, 2, 3)


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in OPS + ("lse", "ws", "kv_len", "prefix_len", "doc_start", "doc_end", "sink", "dsink"):
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


def mask_of(b, of_kind, **over):
    """a valid mask of the kind, host pointers for its arrays; `over` replaces fields"""
    kind = of_kind
    f = dict(kind=kind, kv_len=b.p("kv_len"), prefix_len=None, window_left=-1, window_right=-1, doc_start=None, doc_end=None, causal=0)
    if kind == H.ATTN_MASK_PREFIX:
        f["prefix_len"] = b.p("prefix_len")
    elif kind == H.ATTN_MASK_WINDOW:
        f.update(window_left=2, window_right=0)
    elif kind == H.ATTN_MASK_DOC:
        f.update(doc_start=b.p("doc_start"), doc_end=b.p("doc_end"), causal=1)
    f.update(over)
    return H.attn_mask(**f)


def fwd(b, kind=H.ATTN_MASK_FULL, mask=None, no_mask=False, softcap=0.0, sink=None, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, sq=S, skv=S, d=D, scale=SCALE,
        lays=None, null=(), off=None, lse="lse", **_):
    lays, off = lays or CONTIG, off or {}
    m = mask_of(b, kind, **(mask or {}))
    a = []
    for n in ("q", "k", "v", "o"):
        a += [b.p(None if n in null else n, off.get(n, 0)), lay(lays[n])]
    return H.lib().kf_attn_ext_fwd(dtype, Bn, hq, hkv, sq, skv, d, scale, None if no_mask else C.byref(m), softcap, b.p(sink), *a, b.p(lse), None)


def bwd(b, kind=H.ATTN_MASK_FULL, mask=None, no_mask=False, softcap=0.0, sink=None, dsink="same", dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, sq=S, skv=S, d=D,
        scale=SCALE, lays=None, null=(), off=None, ws="ws", ws_bytes=1 << 16, lse="lse"):
    lays, off = lays or CONTIG, off or {}
    m = mask_of(b, kind, **(mask or {}))
    p = lambda n: b.p(None if n in null else n, off.get(n, 0))  # noqa: E731
    ds = ("dsink" if sink else None) if dsink == "same" else dsink
    return H.lib().kf_attn_ext_bwd(dtype, Bn, hq, hkv, sq, skv, d, scale, None if no_mask else C.byref(m), softcap, b.p(sink), p("q"), lay(lays["q"]),
                                   p("k"), lay(lays["k"]), p("v"), lay(lays["v"]), p("o"), lay(lays["o"]), b.p(lse), p("d_o"), lay(lays["d_o"]),
                                   p("dq"), lay(lays["dq"]), p("dk"), lay(lays["dk"]), p("dv"), lay(lays["dv"]), b.p(ds), b.p(ws), ws_bytes, None)


def mixed(names):
    return {n: (PACKED[n] if n in names else None) for n in OPS}


def bad_stride(name, t):
    return dict(PACKED, **{name: t})


INVALID = [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(d=0), "head size"), (dict(d=257), "head size"), (dict(d=-8), "head size"),
    (dict(hkv=0), "Hkv"), (dict(hkv=8), "Hkv"), (dict(hkv=3), "Hkv"), (dict(hkv=-1), "Hkv"),
    (dict(sq=0, skv=0), "Skv"), (dict(sq=-3, skv=-3), "negative extent"),
    (dict(Bn=-1), "negative extent"), (dict(hq=-4), "negative extent"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=float("inf")), "scale"), (dict(scale=float("nan")), "scale"),
    (dict(null=("q",)), "null"), (dict(null=("v",)), "null"), (dict(null=("o",)), "null"),
    (dict(lays=mixed(("q",))), "all NULL"), (dict(lays=mixed(("q", "k", "v"))), "all NULL"),
    (dict(lays=bad_stride("k", (S * W, D, W + 4))), "multiples of 8"), (dict(lays=bad_stride("q", (-8, D, W))), "multiples of 8"),
    (dict(lays=PACKED, off={"v": 8}), "16-byte aligned"), (dict(off={"q": 1}), "aligned to its element"),
    # the modifiers
    (dict(softcap=-1.0), "softcap"), (dict(softcap=float("inf")), "softcap"), (dict(softcap=float("nan")), "softcap"), (dict(softcap=-0.5, sink="sink"), "softcap"),
    # the mask
    (dict(no_mask=True), "null mask"), (dict(mask=dict(kind=4)), "unknown mask kind"), (dict(mask=dict(kind=-1)), "unknown mask kind"),
]
BWD_ONLY = [
    (dict(null=("d_o",)), "null"), (dict(null=("dq",)), "null"), (dict(null=("dk",)), "null"), (dict(null=("dv",)), "null"), (dict(lse=None), "null"),
    (dict(lays=mixed(("q", "k", "v", "o"))), "all NULL"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=B * HQ * S * 4 - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
    (dict(sink="sink", dsink=None), "dsink"), (dict(sink=None, dsink="dsink"), "dsink"), (dict(softcap=2.0, sink="sink", dsink=None), "dsink"),
]
KINDS = [H.ATTN_MASK_FULL, H.ATTN_MASK_PREFIX, H.ATTN_MASK_WINDOW, H.ATTN_MASK_DOC]
MODS = [dict(), dict(softcap=2.0), dict(sink="sink"), dict(softcap=0.5, sink="sink")]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kw,what", INVALID)
def test_forward_refuses(kw, what, kind):
    for mod in MODS:
        rc = fwd(Bufs(), kind=kind, **{**mod, **kw})
        assert rc == H.KF_ERR_INVALID, (kw, mod, rc, last_error())
        assert "kf_attn_ext_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("kw,what", INVALID + BWD_ONLY)
def test_backward_refuses(kw, what, kind):
    for mod in MODS:
        rc = bwd(Bufs(), kind=kind, **{**mod, **kw})
        assert rc == H.KF_ERR_INVALID, (kw, mod, rc, last_error())
        assert "kf_attn_ext_bwd" in last_error() and what in last_error(), last_error()


CONTRADICTIONS = [
    (H.ATTN_MASK_FULL, dict(prefix_len="prefix_len"), "prefix_len"), (H.ATTN_MASK_WINDOW, dict(prefix_len="prefix_len"), "prefix_len"),
    (H.ATTN_MASK_DOC, dict(prefix_len="prefix_len"), "prefix_len"),
    (H.ATTN_MASK_FULL, dict(window_left=3), "window"), (H.ATTN_MASK_PREFIX, dict(window_right=0), "window"), (H.ATTN_MASK_DOC, dict(window_left=0, window_right=0), "window"),
    (H.ATTN_MASK_FULL, dict(doc_start="doc_start"), "doc_start"), (H.ATTN_MASK_PREFIX, dict(doc_end="doc_end"), "doc_start"),
    (H.ATTN_MASK_WINDOW, dict(causal=1), "causal"), (H.ATTN_MASK_FULL, dict(causal=1), "causal"),
    (H.ATTN_MASK_WINDOW, dict(window_left=-2), "window side"), (H.ATTN_MASK_WINDOW, dict(window_right=-(2 ** 40)), "window side"),
    (H.ATTN_MASK_DOC, dict(causal=2), "causal is 0 or 1"), (H.ATTN_MASK_DOC, dict(causal=-1), "causal is 0 or 1"),
    (H.ATTN_MASK_DOC, dict(doc_start=None), "doc_start"), (H.ATTN_MASK_DOC, dict(doc_end=None), "doc_start"),
]


@pytest.mark.parametrize("kind,fields,what", CONTRADICTIONS)
def test_mask_fields_that_contradict_the_kind_are_invalid(kind, fields, what):
    b = Bufs()
    over = {n: (b.p(v) if isinstance(v, str) else v) for n, v in fields.items()}
    for call, name in ((fwd, "kf_attn_ext_fwd"), (bwd, "kf_attn_ext_bwd")):
        for mod in MODS:
            rc = call(b, kind=kind, mask=over, **mod)
            assert rc == H.KF_ERR_INVALID, (fields, mod, rc, last_error())
            assert name in last_error() and what in last_error(), last_error()


def test_a_document_mask_is_self_attention():
    for call, name in ((fwd, "kf_attn_ext_fwd"), (bwd, "kf_attn_ext_bwd")):
        rc = call(Bufs(), kind=H.ATTN_MASK_DOC, sq=5, softcap=1.0)
        assert rc == H.KF_ERR_INVALID and name in last_error() and "Sq" in last_error(), last_error()


@pytest.mark.parametrize("kw", [dict(dtype=H.F32), dict(d=80), dict(d=256), dict(dtype=H.F16, d=8)])
def test_strided_layouts_off_the_matrix_core_path_are_unsupported(kw):
    for call, name in ((fwd, "kf_attn_ext_fwd"), (bwd, "kf_attn_ext_bwd")):
        for mod in MODS:
            rc = call(Bufs(), lays=PACKED, **mod, **kw)
            assert rc == H.KF_ERR_UNSUPPORTED, (kw, rc, last_error())
            assert "matrix-core" in last_error() and name in last_error()


@pytest.mark.parametrize("kw", [dict(Bn=0), dict(hq=0, hkv=0), dict(hq=0), dict(sq=0)])
def test_zero_extents_are_ok_without_a_launch(kw):
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for kind in KINDS:
            if kind == H.ATTN_MASK_DOC and "sq" in kw:
                continue    # Sq = 0 with Skv = 7 is no self-attention: refused
            for mod in MODS:
                assert fwd(b, kind=kind, dtype=dtype, **mod, **kw) == H.KF_OK, last_error()
                assert bwd(b, kind=kind, dtype=dtype, **mod, **kw) == H.KF_OK, last_error()
                assert fwd(b, kind=kind, dtype=dtype, lays=PACKED, d=64, **mod, **kw) == H.KF_OK, last_error()
    # the checks of the arguments themselves still come first
    assert fwd(b, dtype=H.I64, **kw) == H.KF_ERR_INVALID
    assert bwd(b, softcap=-1.0, **kw) == H.KF_ERR_INVALID
    assert fwd(b, mask=dict(kind=9), **kw) == H.KF_ERR_INVALID


def test_the_workspace_query():
    assert H.attn_ext_bwd_workspace_bytes(H.BF16, B, HQ, HKV, S, S, D) == H.attn_full_bwd_workspace_bytes(H.BF16, B, HQ, HKV, S, S, D)
    need = C.c_size_t(0)
    assert H.lib().kf_attn_ext_bwd_workspace_bytes(H.BF16, B, HQ, 3, S, S, D, C.byref(need)) == H.KF_ERR_INVALID
    assert "kf_attn_ext_bwd_workspace_bytes" in last_error()
    assert H.lib().kf_attn_ext_bwd_workspace_bytes(H.BF16, B, HQ, HKV, S, S, D, None) == H.KF_ERR_INVALID


def test_operator_docstrings():
    for n in ("attention", "attention_qkv"):
        doc = getattr(kfunca, n).__doc__
        assert "softcap" in doc and "sinks" in doc, doc
    doc = kfunca.attention.__doc__
    assert "tanh" in doc and "denominator" in doc and "refused" in doc and "[Hq]" in doc, doc
