"""CPU-only: the span entries of the C ABI (kf_attn_span_table, kf_attn_span_fwd, kf_attn_span_bwd: the document mask with a causal
rule, per-document prefixes and a window) are declared and exported and the ABI version is still 7; the attention entries refuse what
kf_attn_doc_* refuses - the INVALID table of tests/test_attn_doc_abi.py - with the same statuses and their own name in the message,
before any device call, and the modifiers are refused as kf_attn_ext_* refuses them; the table entry refuses n_docs < 1, negative
extents, null pointers (doc_prefix may be NULL), a causal flag outside {0, 1}, a window side below -1 and prefixes without causal;
zero extents are KF_OK without a launch; the workspace is the full family's; doc_mask and the operators' docstrings name the new form."""
import ctypes as C
import re

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests.test_attn_doc_abi import B, CONTIG, D, HKV, HQ, INVALID, OPS, PACKED, ROOT, S, SCALE, W, bad_stride, last_error, lay, mixed

ENTRIES = ("kf_attn_span_table", "kf_attn_span_fwd", "kf_attn_span_bwd")
TABLES = ("key_lo", "key_hi", "query_lo", "query_hi")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    decl = {}
    for n in ENTRIES:
        m = re.search(rf"\bint {n}\s*\(([^;]*)\);", text)
        assert m, f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
        decl[n] = m.group(1)
    assert re.search(r"int64_t B,\s*int64_t S,\s*int64_t n_docs,\s*const int64_t \*cu_doclens,\s*const int64_t \*doc_prefix,\s*int causal,\s*"
                     r"int64_t window_left,\s*int64_t window_right,\s*int64_t \*kv_len,\s*int32_t \*key_lo,\s*int32_t \*key_hi,\s*"
                     r"int32_t \*query_lo,\s*int32_t \*query_hi,\s*void \*stream", decl["kf_attn_span_table"]), decl["kf_attn_span_table"]
    assert re.search(r"int64_t S,\s*int64_t D,\s*float scale,\s*const int64_t \*kv_len,\s*const int32_t \*key_lo,\s*const int32_t \*key_hi,\s*"
                     r"float softcap,\s*const float \*sink,\s*const void \*q", decl["kf_attn_span_fwd"]), decl["kf_attn_span_fwd"]
    assert re.search(r"int64_t S,\s*int64_t D,\s*float scale,\s*const int64_t \*kv_len,\s*const int32_t \*key_lo,\s*const int32_t \*key_hi,\s*"
                     r"const int32_t \*query_lo,\s*const int32_t \*query_hi,\s*float softcap,\s*const float \*sink,\s*const void \*q",
                     decl["kf_attn_span_bwd"]), decl["kf_attn_span_bwd"]
    assert re.search(r"float \*dsink,\s*void \*workspace,\s*size_t workspace_bytes,\s*void \*stream", decl["kf_attn_span_bwd"])
    for n in ENTRIES[1:]:       # self-attention, and no mask descriptor: kf_attn_mask and its kinds are unchanged
        assert "Skv" not in decl[n] and "kf_attn_mask" not in decl[n] and "causal" not in decl[n] and "window" not in decl[n]
    assert re.search(r"enum \{ KF_ATTN_MASK_FULL = 0, KF_ATTN_MASK_PREFIX = 1, KF_ATTN_MASK_WINDOW = 2, KF_ATTN_MASK_DOC = 3 \};", text)
    assert H.lib().kf_abi_version() == 7          # entries were added, none changed
    for n in ("attn_span_table", "attn_span_fwd", "attn_span_bwd"):
        assert callable(getattr(H, n))


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in OPS + ("lse", "ws", "kv_len", "cu", "prefix", "sink", "dsink") + TABLES:
            setattr(self, n, (C.c_double * (B * HQ * S * D // 2 + 8))())

    def p(self, name, off=0):
        if name is None:
            return None
        a = C.addressof(getattr(self, name))
        return (a + 15) // 16 * 16 + off


def fwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, s=S, d=D, scale=SCALE, lays=None, null=(), off=None, lse="lse", kv_len="kv_len", key_lo="key_lo",
        key_hi="key_hi", softcap=0.0, sink=None):
    lays, off = lays or CONTIG, off or {}
    a = []
    for n in ("q", "k", "v", "o"):
        a += [b.p(None if n in null else n, off.get(n, 0)), lay(lays[n])]
    return H.lib().kf_attn_span_fwd(dtype, Bn, hq, hkv, s, d, scale, b.p(kv_len), b.p(key_lo), b.p(key_hi), softcap, b.p(sink), *a, b.p(lse), None)


def bwd(b, dtype=H.BF16, Bn=B, hq=HQ, hkv=HKV, s=S, d=D, scale=SCALE, lays=None, null=(), off=None, ws="ws", ws_bytes=1 << 16, lse="lse",
        kv_len="kv_len", key_lo="key_lo", key_hi="key_hi", query_lo="query_lo", query_hi="query_hi", softcap=0.0, sink=None, dsink=None):
    lays, off = lays or CONTIG, off or {}
    p = lambda n: b.p(None if n in null else n, off.get(n, 0))  # noqa: E731
    return H.lib().kf_attn_span_bwd(dtype, Bn, hq, hkv, s, d, scale, b.p(kv_len), b.p(key_lo), b.p(key_hi), b.p(query_lo), b.p(query_hi), softcap,
                                    b.p(sink), p("q"), lay(lays["q"]), p("k"), lay(lays["k"]), p("v"), lay(lays["v"]), p("o"), lay(lays["o"]), b.p(lse),
                                    p("d_o"), lay(lays["d_o"]), p("dq"), lay(lays["dq"]), p("dk"), lay(lays["dk"]), p("dv"), lay(lays["dv"]), b.p(dsink),
                                    b.p(ws), ws_bytes, None)


# the document family's table without its own three rows (this family names its tables otherwise), then this family's
SHARED = [(kw, what) for kw, what in INVALID if not any(k.startswith("doc_") for k in kw)]
FWD_INVALID = SHARED + [
    (dict(key_lo=None), "key_lo"), (dict(key_hi=None), "key_hi"), (dict(key_lo=None, key_hi=None, lays=PACKED), "kf_attn_span_table"),
    (dict(softcap=-1.0), "softcap"), (dict(softcap=float("inf")), "softcap"), (dict(softcap=float("nan")), "softcap"),
    (dict(softcap=-1.0, Bn=0), "softcap"),        # the modifier is checked first, as in kf_attn_ext_*
]


@pytest.mark.parametrize("mods", [dict(), dict(softcap=30.0), dict(sink="sink")])
@pytest.mark.parametrize("kw,what", FWD_INVALID)
def test_forward_refuses(kw, what, mods):
    rc = fwd(Bufs(), **dict(mods, **kw))
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_span_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("mods", [dict(), dict(softcap=30.0), dict(sink="sink", dsink="dsink")])
@pytest.mark.parametrize("kw,what", FWD_INVALID + [
    (dict(null=("d_o",)), "null"), (dict(null=("dq",)), "null"), (dict(null=("dk",)), "null"), (dict(null=("dv",)), "null"), (dict(lse=None), "null"),
    (dict(lays=mixed(("q", "k", "v", "o"))), "all NULL"),
    (dict(lays=bad_stride("dk", (S * W, D + 2, W))), "multiples of 8"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=B * HQ * S * 4 - 1), "workspace"), (dict(ws_bytes=0), "workspace"),
    (dict(query_lo=None), "query_lo"), (dict(query_hi=None), "query_hi"), (dict(query_lo=None, query_hi=None, lays=PACKED), "kf_attn_span_table"),
])
def test_backward_refuses(kw, what, mods):
    rc = bwd(Bufs(), **dict(mods, **kw))
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_span_bwd" in last_error() and what in last_error(), last_error()


def test_dsink_is_required_exactly_with_a_sink():
    for kw in (dict(sink="sink"), dict(dsink="dsink"), dict(sink="sink", softcap=2.0), dict(dsink="dsink", Bn=0)):
        rc = bwd(Bufs(), **kw)
        assert rc == H.KF_ERR_INVALID and "kf_attn_span_bwd" in last_error() and "dsink" in last_error(), (kw, rc, last_error())


def table(b, Bn=B, s=S, n=3, cu="cu", prefix=None, causal=0, wl=-1, wr=-1, kv_len="kv_len", key_lo="key_lo", key_hi="key_hi", query_lo="query_lo",
          query_hi="query_hi"):
    return H.lib().kf_attn_span_table(Bn, s, n, b.p(cu), b.p(prefix), causal, wl, wr, b.p(kv_len), b.p(key_lo), b.p(key_hi), b.p(query_lo),
                                      b.p(query_hi), None)


@pytest.mark.parametrize("kw,what", [
    (dict(n=0), "n_docs"), (dict(n=-1), "n_docs"), (dict(Bn=-1), "negative extent"), (dict(s=-2), "negative extent"),
    (dict(cu=None), "null"), (dict(kv_len=None), "null"), (dict(key_lo=None), "null"), (dict(key_hi=None), "null"), (dict(query_lo=None), "null"),
    (dict(query_hi=None), "null"), (dict(n=0, Bn=0), "n_docs"), (dict(cu=None, s=0), "null"),
    (dict(causal=2), "causal"), (dict(causal=-1), "causal"), (dict(causal=2, Bn=0), "causal"),
    (dict(wl=-2), "window"), (dict(wr=-2), "window"), (dict(wl=-9, wr=3, causal=1), "window"), (dict(wr=-2, s=0), "window"),
    (dict(prefix="prefix"), "doc_prefix"), (dict(prefix="prefix", wl=4, wr=0), "doc_prefix"), (dict(prefix="prefix", Bn=0), "doc_prefix"),
])
def test_table_refuses(kw, what):
    rc = table(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_attn_span_table" in last_error() and what in last_error(), last_error()


def test_table_zero_extents_are_ok_without_a_launch():
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for kw in (dict(), dict(causal=1, wl=5, wr=0), dict(causal=1, prefix="prefix"), dict(wl=0, wr=0)):
        assert table(b, Bn=0, **kw) == H.KF_OK, last_error()
        assert table(b, s=0, **kw) == H.KF_OK, last_error()
        assert table(b, Bn=0, s=0, n=1, **kw) == H.KF_OK, last_error()


def test_a_row_of_2_to_the_31_tokens_is_unsupported():
    rc = table(Bufs(), Bn=1, s=1 << 31)
    assert rc == H.KF_ERR_UNSUPPORTED and "kf_attn_span_table" in last_error(), (rc, last_error())


@pytest.mark.parametrize("kw", [dict(dtype=H.F32), dict(d=80), dict(d=256), dict(dtype=H.F16, d=8)])
def test_strided_layouts_off_the_matrix_core_path_are_unsupported(kw):
    for call, name in ((fwd, "kf_attn_span_fwd"), (bwd, "kf_attn_span_bwd")):
        rc = call(Bufs(), lays=PACKED, **kw)
        assert rc == H.KF_ERR_UNSUPPORTED, (kw, rc, last_error())
        assert "matrix-core" in last_error() and name in last_error()


@pytest.mark.parametrize("kw", [dict(Bn=0), dict(hq=0, hkv=0), dict(hq=0)])
def test_zero_extents_are_ok_without_a_launch(kw):
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for mods in (dict(), dict(softcap=30.0), dict(sink="sink")):
            back = dict(mods, dsink="dsink") if "sink" in mods else mods
            assert fwd(b, dtype=dtype, **mods, **kw) == H.KF_OK, last_error()
            assert bwd(b, dtype=dtype, **back, **kw) == H.KF_OK, last_error()
            assert fwd(b, dtype=dtype, lays=PACKED, d=64, **mods, **kw) == H.KF_OK, last_error()
            # nothing to launch: the tables are not looked at either, as the operands are not
            assert fwd(b, dtype=dtype, key_lo=None, key_hi=None, null=OPS, **mods, **kw) == H.KF_OK, last_error()
            assert bwd(b, dtype=dtype, key_lo=None, key_hi=None, query_lo=None, query_hi=None, null=OPS, **back, **kw) == H.KF_OK, last_error()
    # the checks of the arguments themselves still come first
    assert fwd(b, dtype=H.I64, **kw) == H.KF_ERR_INVALID
    assert bwd(b, s=0, **kw) == H.KF_ERR_INVALID
    assert fwd(b, d=300, **kw) == H.KF_ERR_INVALID


def test_the_workspace_is_the_full_family_s():
    """no second query: the backward accepts exactly what kf_attn_full_bwd_workspace_bytes states for (S, S), and names it in its refusal"""
    need = H.attn_full_bwd_workspace_bytes(H.BF16, B, HQ, HKV, S, S, D)
    for n in ("kf_attn_span_bwd_workspace_bytes", "kf_attn_span_workspace_bytes"):
        assert not hasattr(H.lib(), n) and n not in H.EXPORTS
    for mods in (dict(), dict(softcap=2.0), dict(sink="sink", dsink="dsink")):
        assert bwd(Bufs(), ws_bytes=need - 256, **mods) == H.KF_ERR_INVALID and "kf_attn_full_bwd_workspace_bytes" in last_error()


def test_operator_surface_and_docstrings():
    doc = kfunca.doc_mask.__doc__
    for word in ("cu_doclens", "window", "prefix_lens", "causal", "n_docs", "query_lo", "key_lo"):
        assert word in doc, (word, doc)
    for n in ("kv_len", "doc_start", "doc_end", "B", "S", "key_lo", "key_hi", "query_lo", "query_hi", "window", "causal"):
        assert hasattr(kfunca.DocMask, n), n
    for n in ("attention", "attention_qkv"):
        assert "doc_mask" in getattr(kfunca, n).__doc__
    doc = kfunca.attention.__doc__
    assert "prefix_lens" in doc and "doc_mask(cu_doclens, S, window=" in doc and "must equal the mask's" in doc, doc
