"""CPU-only: the rotary-embedding entries of the C ABI (kf_rope, kf_rope_table) are declared and exported, every invalid argument is
refused with KF_ERR_INVALID and a message before any device call, a valid call without a device reports an error instead of falling
back to a CPU path, and the operator API refuses bad table arguments before it touches a device."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_rope", "kf_rope_table")


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


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self, B=2, Hh=3, S=4, D=8, P=16):
        n = B * Hh * S * D
        self.x = (C.c_float * n)()
        self.y = (C.c_float * n)()
        self.cos = (C.c_float * (P * D))()
        self.sin = (C.c_float * (P * D))()
        self.pos = (C.c_int64 * (B * S))()


def call(b, dtype=H.F32, B=2, Hh=3, S=4, D=8, h_rot=3, R=8, il=0, inv=0, cos="cos", sin="sin", P=16, pos="pos", x="x", y="y", lx=None, ly=None,
         null_lx=False, null_ly=False):
    p = lambda n: C.addressof(getattr(b, n)) if n else None  # noqa: E731
    lx = H.AttnLayout(*(lx or (Hh * S * D, S * D, D)))
    ly = H.AttnLayout(*(ly or (Hh * S * D, S * D, D)))
    return H.lib().kf_rope(dtype, B, Hh, S, D, h_rot, R, il, inv, p(cos), p(sin), P, p(pos), p(x), None if null_lx else C.byref(lx), p(y),
                           None if null_ly else C.byref(ly), None)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I64), "dtype"),
    (dict(R=7), "rotary_dim"), (dict(R=0), "rotary_dim"), (dict(R=10), "rotary_dim"), (dict(R=-2), "rotary_dim"),
    (dict(h_rot=-1), "h_rot"), (dict(h_rot=4), "h_rot"),
    (dict(cos=None), "null"), (dict(sin=None), "null"), (dict(x=None), "null"), (dict(y=None), "null"), (dict(null_lx=True), "null"),
    (dict(null_ly=True), "null"),
    (dict(P=0), "table_rows"), (dict(P=-3), "table_rows"),
    (dict(pos=None, P=3), "positions"),
    (dict(y="x", lx=(96, 8, 24), ly=(96, 32, 8)), "in place"), (dict(y="x", ly=(96, 32, 9)), "in place"),
    (dict(il=2), "interleaved"), (dict(inv=-1), "inverse"), (dict(D=0, R=2), "extents"),
])
def test_rope_refuses(kw, what):
    rc = call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(base=0.0), "base"), (dict(base=-1.0), "base"), (dict(base=float("inf")), "base"), (dict(base=float("nan")), "base"),
    (dict(R=7), "rotary_dim"), (dict(R=0), "rotary_dim"), (dict(rows=0), "rows"), (dict(c=None), "null"), (dict(s=None), "null"),
])
def test_rope_table_refuses(kw, what):
    b = Bufs()
    c = kw.get("c", "cos")
    s = kw.get("s", "sin")
    rc = H.lib().kf_rope_table(kw.get("base", 1e4), kw.get("R", 8), kw.get("rows", 16), C.addressof(b.cos) if c else None,
                               C.addressof(b.sin) if s else None, None)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        return  # (host pointers: never launched on a machine that has a device)
    b = Bufs()
    assert call(b) != H.KF_OK and last_error()
    assert call(b, y="x") != H.KF_OK and last_error()
    assert H.lib().kf_rope_table(1e4, 8, 16, C.addressof(b.cos), C.addressof(b.sin), None) != H.KF_OK and last_error()


@pytest.mark.parametrize("args,what", [((0, 128), "max_positions"), ((4096, 127), "rotary_dim"), ((4096, 0), "rotary_dim"),
                                       ((4096, 128, -1.0), "base"), ((4096, 128, 0.0), "base")])
def test_rope_table_operator_refuses_before_the_device(args, what):
    with pytest.raises(RuntimeError, match=what):
        kfunca.rope_table(*args)


def test_operator_surface():
    for n in ("rope_table", "rope", "rope_qkv"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))
