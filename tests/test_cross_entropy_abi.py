"""CPU-only: the softmax cross-entropy entries of the C ABI (kf_cross_entropy_*) are declared and exported, the workspace query follows
the documented partition of (rows, V), every invalid argument is refused with KF_ERR_INVALID and a message before any device call, and
a valid call without a device reports an error instead of falling back to a CPU path."""
import ctypes as C
import re
from pathlib import Path

import pytest

from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_cross_entropy_workspace_bytes", "kf_cross_entropy_fwd", "kf_cross_entropy_bwd")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    for name, value in (("KF_CE_NONE", H.CE_NONE), ("KF_CE_SUM", H.CE_SUM), ("KF_CE_MEAN", H.CE_MEAN)):
        assert re.search(rf"\b{name} = {value}\b", text)


def ws(dtype, rows, V, reduction):
    return H.ce_workspace_bytes(dtype, rows, V, reduction)


def test_workspace_follows_the_regimes():
    # one wave per row (V <= 4096) and one block per row (rows >= 1024): no partials; the sums keep one f32 loss per row (256-B rounded)
    assert ws(H.BF16, 4, 4096, H.CE_NONE) == 0
    assert ws(H.BF16, 32768, 128256, H.CE_NONE) == 0
    assert ws(H.BF16, 32768, 128256, H.CE_MEAN) == 32768 * 4
    assert ws(H.BF16, 8192, 50257, H.CE_SUM) == 8192 * 4
    assert ws(H.F32, 8192, 32000, H.CE_MEAN) == 8192 * 4
    assert ws(H.F16, 3, 1000, H.CE_MEAN) == 256
    # few long rows split into chunks: 16 x 128256 -> 32 chunks of 4032 elements, three f32 partials each
    assert ws(H.BF16, 16, 128256, H.CE_NONE) == 16 * 32 * 3 * 4
    assert ws(H.BF16, 16, 128256, H.CE_MEAN) == 16 * 32 * 3 * 4 + 256
    # 1023 rows of 8192: two chunks of 4096 (aiming at 2048 blocks in all, chunks of at least 4096 elements)
    assert ws(H.F32, 1023, 8192, H.CE_NONE) == -(-1023 * 2 * 3 * 4 // 256) * 256
    # the partition depends on (rows, V) only: the dtype does not enter
    assert ws(H.F32, 16, 128256, H.CE_SUM) == ws(H.BF16, 16, 128256, H.CE_SUM) == ws(H.F16, 16, 128256, H.CE_SUM)
    assert ws(H.BF16, 0, 128256, H.CE_NONE) == 0


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self, rows=4, V=16):
        self.x = (C.c_float * (rows * V))()
        self.t = (C.c_int64 * rows)()
        self.loss = (C.c_float * rows)()
        self.lse = (C.c_float * rows)()
        self.count = (C.c_float * 1)()
        self.g = (C.c_float * rows)()
        self.dx = (C.c_float * (rows * V))()
        self.ws = (C.c_char * 4096)()


def fwd(b, dtype=H.F32, rows=4, V=16, ld=16, x="x", t="t", eps=0.0, red=H.CE_MEAN, loss="loss", ws="ws", ws_bytes=4096):
    p = lambda n: C.addressof(getattr(b, n)) if n else None  # noqa: E731
    return H.lib().kf_cross_entropy_fwd(dtype, rows, V, ld, p(x), p(t), -100, eps, red, p(loss), p("lse"), p("count"), p(ws), ws_bytes, None)


def bwd(b, dtype=H.F32, rows=4, V=16, ld=16, x="x", t="t", eps=0.0, red=H.CE_MEAN, lse="lse", count="count", g="g", dx="dx", ldd=16):
    p = lambda n: C.addressof(getattr(b, n)) if n else None  # noqa: E731
    return H.lib().kf_cross_entropy_bwd(dtype, rows, V, ld, p(x), p(t), -100, eps, red, p(lse), p(count), p(g), p(dx), ldd, None)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.I32), "dtype"), (dict(dtype=H.F64), "dtype"), (dict(red=3), "reduction"), (dict(red=-1), "reduction"),
    (dict(V=0, ld=0), "V"), (dict(ld=15), "stride"), (dict(rows=-1), "rows"), (dict(eps=-0.1), "label_smoothing"),
    (dict(eps=1.5), "label_smoothing"), (dict(eps=float("nan")), "label_smoothing"), (dict(x=None), "null"), (dict(t=None), "null"),
    (dict(loss=None), "null loss"), (dict(ws=None), "workspace"), (dict(ws_bytes=16), "workspace"),
])
def test_forward_refuses_invalid_arguments(kw, what):
    rc = fwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def test_forward_refuses_misaligned_logits():
    b = Bufs()
    rc = H.lib().kf_cross_entropy_fwd(H.BF16, 4, 16, 16, C.addressof(b.x) + 1, C.addressof(b.t), -100, 0.0, H.CE_NONE, C.addressof(b.loss),
                                      None, None, None, 0, None)
    assert rc == H.KF_ERR_INVALID and "aligned" in last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.I64), "dtype"), (dict(red=7), "reduction"), (dict(V=0, ld=0, ldd=0), "V"), (dict(ld=8), "stride"), (dict(ldd=8), "stride"),
    (dict(eps=2.0), "label_smoothing"), (dict(lse=None), "null"), (dict(g=None), "null"), (dict(dx=None), "null"), (dict(x=None), "null"),
    (dict(t=None), "null"), (dict(count=None), "count"),
])
def test_backward_refuses_invalid_arguments(kw, what):
    rc = bwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def test_workspace_query_refuses_invalid_arguments():
    n = C.c_size_t(0)
    lib = H.lib()
    assert lib.kf_cross_entropy_workspace_bytes(H.F32, 4, 16, H.CE_MEAN, None) == H.KF_ERR_INVALID
    for args in ((H.I32, 4, 16, H.CE_MEAN), (H.F32, 4, 0, H.CE_MEAN), (H.F32, -1, 16, H.CE_MEAN), (H.F32, 4, 16, 9)):
        assert lib.kf_cross_entropy_workspace_bytes(*args, C.byref(n)) == H.KF_ERR_INVALID and last_error()


def test_valid_calls_without_a_device_fail_loudly():
    if H.device_count() > 0:
        return  # the device path is covered by tests/test_gpu_cross_entropy.py
    b = Bufs()
    need = ws(H.F32, 4, 16, H.CE_MEAN)
    assert 0 < need <= 4096
    for red in (H.CE_NONE, H.CE_SUM, H.CE_MEAN):
        assert fwd(b, red=red) != H.KF_OK and last_error()
    assert bwd(b) != H.KF_OK and last_error()
    assert bwd(b, red=H.CE_NONE, count=None) != H.KF_OK and last_error()
