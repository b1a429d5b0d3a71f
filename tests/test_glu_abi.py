"""CPU-only: the gated-activation entries of the C ABI (kf_glu_fwd, kf_glu_bwd) are declared and exported, every invalid argument is
refused with KF_ERR_INVALID and a message before any device call, zero extents are KF_OK without a launch, a valid call without a
device reports an error instead of falling back to a CPU path, and the operator surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_glu_fwd", "kf_glu_bwd")
ROWS, F, LD = 3, 8, 16


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    for name, value in (("KF_ACT_SILU", 0), ("KF_ACT_GELU_TANH", 1), ("KF_ACT_GELU_ERF", 2)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert (H.ACT_SILU, H.ACT_GELU_TANH, H.ACT_GELU_ERF) == (0, 1, 2)
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("gate", "up", "h", "dh", "dgate", "dup"):
            setattr(self, n, (C.c_float * (ROWS * LD + 4))())

    def p(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off


def fwd(b, act=H.ACT_SILU, dtype=H.F32, rows=ROWS, f=F, gate="gate", ldg=LD, up="up", ldu=LD, h="h", ldh=LD, off=None):
    off = off or {}
    return H.lib().kf_glu_fwd(act, dtype, rows, f, b.p(gate, off.get("gate", 0)), ldg, b.p(up, off.get("up", 0)), ldu, b.p(h, off.get("h", 0)), ldh, None)


def bwd(b, act=H.ACT_SILU, dtype=H.F32, rows=ROWS, f=F, gate="gate", ldg=LD, up="up", ldu=LD, dh="dh", lddh=LD, dgate="dgate", lddg=LD,
        dup="dup", lddu=LD, off=None):
    off = off or {}
    return H.lib().kf_glu_bwd(act, dtype, rows, f, b.p(gate), ldg, b.p(up), ldu, b.p(dh, off.get("dh", 0)), lddh, b.p(dgate), lddg, b.p(dup), lddu, None)


@pytest.mark.parametrize("kw,what", [
    (dict(act=3), "act"), (dict(act=-1), "act"),
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(rows=-1), "extents"), (dict(f=-2), "extents"),
    (dict(ldg=F - 1), "leading dimension of gate"), (dict(ldu=F - 1), "leading dimension of up"), (dict(ldh=0), "leading dimension of h"),
    (dict(gate=None), "null"), (dict(h=None), "null"),
    (dict(h="gate", ldh=LD + 8), "alias h == gate"), (dict(h="up", ldh=F), "alias h == up"),
    (dict(off={"gate": 2}), "aligned"), (dict(off={"h": 1}), "aligned"), (dict(off={"up": 3}), "aligned"),
])
def test_forward_refuses(kw, what):
    rc = fwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_glu_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(act=7), "act"), (dict(dtype=H.U8), "dtype"), (dict(dtype=H.F64), "dtype"),
    (dict(rows=-5), "extents"), (dict(f=-1), "extents"),
    (dict(ldg=F - 1), "leading dimension of gate"), (dict(ldu=1), "leading dimension of up"), (dict(lddh=F - 1), "leading dimension of dh"),
    (dict(lddg=F - 1), "leading dimension of dgate"), (dict(lddu=F - 1), "leading dimension of dup"),
    (dict(gate=None), "null"), (dict(dh=None), "null"), (dict(dgate=None), "null"),
    (dict(up=None), "dup goes with up"), (dict(dup=None), "dup goes with up"),
    (dict(dgate="gate", lddg=LD + 4), "alias dgate == gate"), (dict(dup="up", lddu=F), "alias dup == up"),
    (dict(off={"dh": 2}), "aligned"),
])
def test_backward_refuses(kw, what):
    rc = bwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_glu_bwd" in last_error() and what in last_error(), last_error()


def test_16_bit_bases_need_two_byte_alignment_only():
    b = Bufs()
    assert fwd(b, dtype=H.BF16, rows=0, off={"gate": 2, "h": 2, "up": 2}) == H.KF_OK
    assert fwd(b, dtype=H.BF16, off={"gate": 1}) == H.KF_ERR_INVALID and "aligned" in last_error()


@pytest.mark.parametrize("rows,f", [(0, F), (ROWS, 0), (0, 0)])
def test_zero_extents_are_ok_without_a_launch(rows, f):
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        assert fwd(b, dtype=dtype, rows=rows, f=f) == H.KF_OK
        assert fwd(b, dtype=dtype, rows=rows, f=f, up=None) == H.KF_OK
        assert bwd(b, dtype=dtype, rows=rows, f=f) == H.KF_OK
        assert bwd(b, dtype=dtype, rows=rows, f=f, up=None, dup=None) == H.KF_OK
    # the checks still come first
    assert fwd(b, rows=rows, f=f, act=5) == H.KF_ERR_INVALID
    assert bwd(b, rows=rows, f=f, dgate=None) == H.KF_ERR_INVALID


def test_allowed_aliases_pass_validation():
    b = Bufs()
    assert fwd(b, rows=0, h="gate") == H.KF_OK and fwd(b, rows=0, h="up") == H.KF_OK
    assert bwd(b, rows=0, dgate="gate", dup="up") == H.KF_OK
    assert fwd(b, rows=0, up=None, ldu=-7) == H.KF_OK   # ldu is ignored without up


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        pytest.skip("a device is present: host pointers are never launched on one")
    b = Bufs()
    assert fwd(b) != H.KF_OK and last_error()
    assert fwd(b, up=None) != H.KF_OK and last_error()
    assert bwd(b) != H.KF_OK and last_error()


def test_operator_surface():
    for n in ("swiglu", "geglu", "silu", "gelu"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))
    for fn in (kfunca.geglu, kfunca.gelu):
        assert "approximate" in fn.__doc__
