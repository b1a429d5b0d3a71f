"""CPU-only: the grouped-query attention entries of the C ABI (kf_attn_fwd_gqa, kf_attn_bwd_gqa_workspace_bytes, kf_attn_bwd_gqa) are
declared and exported, every invalid argument is refused with KF_ERR_INVALID and a message before any device call, the workspace query
adds exactly the two partial dK / dV arrays to the multi-head numbers, and a valid call without a device reports an error."""
import ctypes as C
import re
from pathlib import Path

import pytest

from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_attn_fwd_gqa", "kf_attn_bwd_gqa_workspace_bytes", "kf_attn_bwd_gqa")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    declared = sorted(set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", text)))
    assert sorted(H.EXPORTS) == declared
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


def align256(n):
    return (n + 255) // 256 * 256


def stats_bytes(nbh, Sq):  # delta [B H, Sq] + two row-constant arrays [B H, ceil32(Sq)], each 256-aligned (include/kfunca_hip.h)
    return align256(nbh * Sq * 4) + 2 * align256(nbh * ((Sq + 31) // 32 * 32) * 4)


class Bufs:
    """16-byte aligned host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self, B=1, Hq=4, Hkv=2, S=256, D=128, es=2):
        self._keep = []
        nq, nkv = B * Hq * S * D * es, B * Hkv * S * D * es
        for name, n in (("q", nq), ("k", nkv), ("v", nkv), ("o", nq), ("do", nq), ("dq", nq), ("dk", nkv), ("dv", nkv), ("lse", B * Hq * S * 4)):
            raw = (C.c_char * (n + 16))()
            self._keep.append(raw)
            setattr(self, name, (C.addressof(raw) + 15) // 16 * 16)
        self.ws_bytes = stats_bytes(B * Hq, S) + 2 * align256(nq) + (1 << 16)
        raw = (C.c_char * (self.ws_bytes + 16))()
        self._keep.append(raw)
        self.ws = (C.addressof(raw) + 15) // 16 * 16


def lay(t):
    return C.byref(H.AttnLayout(*t))


def contiguous(Hh, S, D):
    return (Hh * S * D, S * D, D)


def fwd(b, dtype=H.BF16, B=1, Hq=4, Hkv=2, S=256, D=128, scale=0.125, lays=None, drop=None):
    ptr = {n: getattr(b, n) for n in ("q", "k", "v", "o", "lse")}
    if drop:
        ptr[drop] = None
    L = [None] * 4 if lays is None else [None if t is None else lay(t) for t in lays]
    return H.lib().kf_attn_fwd_gqa(dtype, B, Hq, Hkv, S, S, D, scale, ptr["q"], L[0], ptr["k"], L[1], ptr["v"], L[2], ptr["o"], L[3], ptr["lse"], None)


def bwd(b, dtype=H.BF16, B=1, Hq=4, Hkv=2, S=256, D=128, scale=0.125, lays=None, drop=None, ws_bytes=None):
    ptr = {n: getattr(b, n) for n in ("q", "k", "v", "o", "lse", "do", "dq", "dk", "dv", "ws")}
    if drop:
        ptr[drop] = None
    L = [None] * 8 if lays is None else [None if t is None else lay(t) for t in lays]
    wsb = b.ws_bytes if ws_bytes is None else ws_bytes
    return H.lib().kf_attn_bwd_gqa(dtype, B, Hq, Hkv, S, S, D, scale, ptr["q"], L[0], ptr["k"], L[1], ptr["v"], L[2], ptr["o"], L[3], ptr["lse"],
                                   ptr["do"], L[4], ptr["dq"], L[5], ptr["dk"], L[6], ptr["dv"], L[7], ptr["ws"], wsb, None)


QL, KL = contiguous(4, 256, 128), contiguous(2, 256, 128)
FWD_LAYS = [QL, KL, KL, QL]
BWD_LAYS = [QL, KL, KL, QL, QL, QL, KL, KL]


@pytest.mark.parametrize("kw,what", [
    (dict(Hkv=0), "Hkv"), (dict(Hkv=-2), "Hkv"), (dict(Hkv=8), "Hkv"), (dict(Hkv=3), "Hkv"), (dict(Hq=6, Hkv=4), "Hkv"),
    (dict(drop="q"), "null"), (dict(drop="k"), "null"), (dict(drop="v"), "null"), (dict(drop="o"), "null"),
    (dict(lays=[QL, None, KL, QL]), "layouts"), (dict(lays=[None, None, None, QL]), "layouts"), (dict(lays=[QL, KL, KL, None]), "layouts"),
    (dict(lays=[QL, (2 * 256 * 128, 128, 132), KL, QL]), "strides"), (dict(lays=[QL, KL, KL, (-1, 128, 128)]), "strides"),
    (dict(lays=[(4 * 256 * 128, 129, 128), KL, KL, QL]), "strides"),
])
def test_fwd_refuses_invalid_arguments(kw, what):
    b = Bufs()
    assert fwd(b, **kw) == H.KF_ERR_INVALID, what
    assert last_error(), what


@pytest.mark.parametrize("kw,what", [
    (dict(Hkv=0), "Hkv"), (dict(Hkv=5), "Hkv"), (dict(Hkv=3), "Hkv"),
    (dict(drop="q"), "null"), (dict(drop="lse"), "null"), (dict(drop="do"), "null"), (dict(drop="dq"), "null"), (dict(drop="dk"), "null"),
    (dict(drop="dv"), "null"), (dict(drop="ws"), "null"),
    (dict(lays=BWD_LAYS[:6] + [None, KL]), "layouts"), (dict(lays=[None] * 7 + [KL]), "layouts"),
    (dict(lays=BWD_LAYS[:6] + [(2 * 256 * 128, 128, 130), KL]), "strides"),
    (dict(ws_bytes=0), "workspace"), (dict(ws_bytes=stats_bytes(4, 256)), "workspace"),
    (dict(ws_bytes=stats_bytes(4, 256) + 2 * align256(4 * 256 * 128 * 2) - 1), "workspace"),
])
def test_bwd_refuses_invalid_arguments(kw, what):
    b = Bufs()
    assert bwd(b, **kw) == H.KF_ERR_INVALID, what
    assert last_error(), what


def test_strided_off_the_matrix_core_path_is_unsupported():
    b = Bufs(es=4)
    f32 = [contiguous(4, 256, 128), contiguous(2, 256, 128), contiguous(2, 256, 128), contiguous(4, 256, 128)]
    assert fwd(b, dtype=H.F32, lays=f32) == H.KF_ERR_UNSUPPORTED
    assert "strided" in last_error()


def query(dtype, B, Hq, Hkv, Sq, Skv, D):
    rec, mn = C.c_size_t(0), C.c_size_t(0)
    rc = H.lib().kf_attn_bwd_gqa_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D, C.byref(rec), C.byref(mn))
    assert rc == H.KF_OK, last_error()
    rec_only = C.c_size_t(0)  # minimum may be NULL
    assert H.lib().kf_attn_bwd_gqa_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D, C.byref(rec_only), None) == H.KF_OK
    assert rec_only.value == rec.value
    return rec.value, mn.value


SHAPES = [(H.BF16, 8, 32, 4096, 4096, 128), (H.BF16, 2, 8, 1000, 1000, 64), (H.F16, 1, 8, 384, 128, 128), (H.F32, 2, 6, 256, 256, 128),
          (H.BF16, 2, 8, 65, 33, 96), (H.F32, 1, 4, 65, 33, 40)]


@pytest.mark.parametrize("dtype,B,Hq,Sq,Skv,D", SHAPES)
def test_workspace_multi_head_equals_the_existing_query(dtype, B, Hq, Sq, Skv, D):
    rec, mn = query(dtype, B, Hq, Hq, Sq, Skv, D)
    assert rec == H.attn_bwd_workspace_bytes(dtype, B, Hq, Sq, Skv, D)
    assert mn == stats_bytes(B * Hq, Sq)


@pytest.mark.parametrize("dtype,B,Hq,Sq,Skv,D", SHAPES)
def test_workspace_grows_by_the_two_partial_arrays(dtype, B, Hq, Sq, Skv, D):
    es = 4 if dtype == H.F32 else 2
    parts = 2 * align256(B * Hq * Skv * D * es)
    rec1, mn1 = query(dtype, B, Hq, Hq, Sq, Skv, D)
    for Hkv in [h for h in (Hq // 2, Hq // 4, 1) if h >= 1 and Hq % h == 0 and h < Hq]:
        rec, mn = query(dtype, B, Hq, Hkv, Sq, Skv, D)
        assert mn == mn1 + parts and rec == rec1 + parts, (Hkv, rec, mn)
    if (dtype, B, Hq, Skv, D) == (H.BF16, 8, 32, 4096, 128):
        assert parts == 512 << 20


def test_workspace_query_refuses_bad_heads():
    rec = C.c_size_t(0)
    for Hq, Hkv in ((8, 0), (8, 3), (4, 8), (8, -1)):
        assert H.lib().kf_attn_bwd_gqa_workspace_bytes(H.BF16, 1, Hq, Hkv, 256, 256, 128, C.byref(rec), None) == H.KF_ERR_INVALID
        assert last_error()
    assert H.lib().kf_attn_bwd_gqa_workspace_bytes(H.BF16, 1, 8, 2, 256, 256, 128, None, None) == H.KF_ERR_INVALID


def test_valid_calls_without_a_device_report_an_error():
    if H.device_count() > 0:
        return
    b = Bufs()
    assert fwd(b) != H.KF_OK and last_error()
    assert fwd(b, lays=FWD_LAYS) != H.KF_OK and last_error()
    assert bwd(b) != H.KF_OK and last_error()
    assert bwd(b, lays=BWD_LAYS) != H.KF_OK and last_error()
