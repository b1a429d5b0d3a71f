"""CPU-only: the softmax entries of the C ABI (kf_softmax_fwd, kf_softmax_bwd) are declared and exported, every invalid argument is
refused with KF_ERR_INVALID and a message before any device call, zero extents are KF_OK without a launch, the allowed aliases pass and
every other overlap is refused, a valid call without a device reports an error instead of falling back to a CPU path, and the operator
surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_softmax_fwd", "kf_softmax_bwd")
ROWS, V, LD = 3, 8, 16
INF, NAN = float("inf"), float("nan")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    for name, value in (("KF_SOFTMAX", 0), ("KF_LOG_SOFTMAX", 1)):
        assert re.search(rf"\b{name} = {value}\b", text), name
    assert (H.SOFTMAX, H.LOG_SOFTMAX) == (0, 1)
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("x", "y", "dy", "dx"):
            setattr(self, n, (C.c_float * (ROWS * LD + 4))())

    def p(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off


def fwd(b, kind=H.SOFTMAX, dtype=H.F32, rows=ROWS, v=V, scale=1.0, x="x", ldx=LD, y="y", ldy=LD, off=None):
    off = off or {}
    return H.lib().kf_softmax_fwd(kind, dtype, rows, v, scale, b.p(x, off.get("x", 0)), ldx, b.p(y, off.get("y", 0)), ldy, None)


def bwd(b, kind=H.SOFTMAX, dtype=H.F32, rows=ROWS, v=V, scale=1.0, y="y", ldy=LD, dy="dy", lddy=LD, dx="dx", lddx=LD, off=None):
    off = off or {}
    return H.lib().kf_softmax_bwd(kind, dtype, rows, v, scale, b.p(y, off.get("y", 0)), ldy, b.p(dy, off.get("dy", 0)), lddy,
                                  b.p(dx, off.get("dx", 0)), lddx, None)


@pytest.mark.parametrize("kw,what", [
    (dict(kind=2), "kind"), (dict(kind=-1), "kind"),
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I64), "dtype"), (dict(dtype=99), "dtype"),
    (dict(rows=-1), "extents"), (dict(v=-2), "extents"),
    (dict(scale=0.0), "scale"), (dict(scale=-1.0), "scale"), (dict(scale=INF), "scale"), (dict(scale=NAN), "scale"),
    (dict(ldx=V - 1), "leading dimension of x"), (dict(ldy=0), "leading dimension of y"),
    (dict(x=None), "null"), (dict(y=None), "null"),
    (dict(off={"x": 2}), "aligned"), (dict(off={"y": 1}), "aligned"),
    (dict(y="x", ldy=LD + 8), "alias"),                 # in place with another leading dimension
    (dict(y="x", off={"y": 4}), "alias"),               # shifted into the input's rows
    (dict(y="x", off={"y": 4 * LD}, rows=2), "alias"),  # one row further down
])
def test_forward_refuses(kw, what):
    rc = fwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_softmax_fwd" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(kind=7), "kind"), (dict(dtype=H.U8), "dtype"), (dict(dtype=H.F64), "dtype"),
    (dict(rows=-5), "extents"), (dict(v=-1), "extents"),
    (dict(scale=0.0), "scale"), (dict(scale=-INF), "scale"), (dict(scale=NAN), "scale"),
    (dict(ldy=V - 1), "leading dimension of y"), (dict(lddy=1), "leading dimension of dy"), (dict(lddx=V - 1), "leading dimension of dx"),
    (dict(y=None), "null"), (dict(dy=None), "null"), (dict(dx=None), "null"),
    (dict(off={"y": 2}), "aligned"), (dict(off={"dy": 3}), "aligned"), (dict(off={"dx": 1}), "aligned"),
    (dict(dx="dy", lddx=LD + 4), "alias"), (dict(dx="dy", off={"dx": 8}), "alias"),
    (dict(dx="y"), "alias"), (dict(dx="y", off={"dx": 4 * (LD + 2)}, rows=2), "alias"),
])
def test_backward_refuses(kw, what):
    rc = bwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_softmax_bwd" in last_error() and what in last_error(), last_error()


def test_16_bit_bases_need_two_byte_alignment_only():
    b = Bufs()
    assert fwd(b, dtype=H.BF16, rows=0, off={"x": 2, "y": 6}) == H.KF_OK
    assert bwd(b, dtype=H.F16, rows=0, off={"y": 2, "dy": 10, "dx": 14}) == H.KF_OK
    assert fwd(b, dtype=H.BF16, off={"x": 1}) == H.KF_ERR_INVALID and "aligned" in last_error()
    assert bwd(b, dtype=H.F16, off={"dx": 3}) == H.KF_ERR_INVALID and "aligned" in last_error()


@pytest.mark.parametrize("rows,v", [(0, V), (ROWS, 0), (0, 0)])
def test_zero_extents_are_ok_without_a_launch(rows, v):
    # (host pointers and, on a machine without a device, no device either: KF_OK means nothing was launched)
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for kind in (H.SOFTMAX, H.LOG_SOFTMAX):
            assert fwd(b, kind=kind, dtype=dtype, rows=rows, v=v) == H.KF_OK
            assert bwd(b, kind=kind, dtype=dtype, rows=rows, v=v) == H.KF_OK
    # the checks still come first
    assert fwd(b, rows=rows, v=v, kind=5) == H.KF_ERR_INVALID
    assert fwd(b, rows=rows, v=v, scale=0.0) == H.KF_ERR_INVALID
    assert bwd(b, rows=rows, v=v, dx=None) == H.KF_ERR_INVALID


def test_allowed_aliases_pass_validation():
    b = Bufs()
    assert fwd(b, rows=0, y="x") == H.KF_OK
    assert bwd(b, rows=0, dx="dy") == H.KF_OK
    if H.device_count() == 0:
        # with extents: past validation (no KF_ERR_INVALID), and then no device to launch on
        assert fwd(b, y="x") not in (H.KF_OK, H.KF_ERR_INVALID) and bwd(b, dx="dy") not in (H.KF_OK, H.KF_ERR_INVALID)
        # two column blocks of one wider buffer interleave without sharing an element
        assert fwd(b, y="x", off={"y": 4 * V}) not in (H.KF_OK, H.KF_ERR_INVALID)


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        pytest.skip("a device is present: host pointers are never launched on one")
    b = Bufs()
    for kind in (H.SOFTMAX, H.LOG_SOFTMAX):
        assert fwd(b, kind=kind) != H.KF_OK and last_error()
        assert bwd(b, kind=kind) != H.KF_OK and last_error()
    assert fwd(b, dtype=H.BF16, v=2 * V, scale=0.125) != H.KF_OK and last_error()


def test_operator_surface():
    for n in ("softmax", "log_softmax"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))
        doc = getattr(kfunca, n).__doc__
        assert "dim" in doc and "scale" in doc and "-inf" in doc and "backward keeps the result" in doc
    for n in ("softmax_fwd", "softmax_bwd"):
        assert callable(getattr(H, n)) and getattr(H, n).__doc__
