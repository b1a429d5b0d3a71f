"""CPU-only: the fused cross-entropy entries of the C ABI (kf_ce_fused_rows, its workspace query, kf_ce_fused_reduce, kf_scale_cast) are
declared and exported, the ABI version is still 7, the workspace query follows the documented partition of (rows, V), every invalid
argument is refused with KF_ERR_INVALID and a message before any device call, the operator refuses a chunk_rows that is not a multiple
of 128, and a valid call without a device reports an error instead of falling back to a CPU path."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_ce_fused_rows_workspace_bytes", "kf_ce_fused_rows", "kf_ce_fused_reduce", "kf_scale_cast")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    for n in ("ce_fused_rows_workspace_bytes", "ce_fused_rows", "ce_fused_reduce", "scale_cast"):
        assert callable(getattr(H, n))
    assert H.lib().kf_abi_version() == 7 and re.search(r"#define KF_ABI_VERSION 7\b", text)
    assert "linear_cross_entropy" in kfunca.__all__ and callable(kfunca.linear_cross_entropy)


def test_workspace_follows_the_regimes():
    ws = H.ce_fused_rows_workspace_bytes
    # one wave per row (V <= 4096) and one block per row (rows >= 1024): one launch, no scratch
    assert ws(4, 4096) == 0 and ws(100000, 7) == 0 and ws(1024, 4097) == 0 and ws(8192, 128256) == 0 and ws(0, 128256) == 0
    # few long rows split into chunks: three f32 partials per chunk and one f32 lse per row, each part rounded to 256 bytes
    assert ws(16, 128256) == 16 * 32 * 3 * 4 + 256           # 32 chunks of 4032 elements
    assert ws(1023, 8192) == -(-1023 * 2 * 3 * 4 // 256) * 256 + 1023 * 4 // 256 * 256 + 256
    assert ws(2, 50257) == -(-2 * 13 * 3 * 4 // 256) * 256 + 256


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self, rows=4, V=16):
        self.x = (C.c_float * (rows * V))()
        self.t = (C.c_int64 * rows)()
        self.rowloss = (C.c_float * rows)()
        self.lse = (C.c_float * rows)()
        self.dx = (C.c_float * (rows * V))()
        self.loss = (C.c_float * 1)()
        self.count = (C.c_float * 1)()
        self.g = (C.c_float * 1)()
        self.ws = (C.c_char * 4096)()


def p(b, n):
    return C.addressof(getattr(b, n)) if n else None


def rows_call(b, ind=H.F32, outd=H.F32, rows=4, V=16, ld=16, x="x", t="t", eps=0.0, z=0.0, rowloss="rowloss", lse="lse", dx="dx", ldd=16,
              ws="ws", ws_bytes=4096):
    return H.lib().kf_ce_fused_rows(ind, outd, rows, V, ld, p(b, x), p(b, t), -100, eps, z, p(b, rowloss), p(b, lse), p(b, dx), ldd, p(b, ws),
                                    ws_bytes, None)


@pytest.mark.parametrize("kw,what", [
    (dict(ind=H.I32), "dtype pair"), (dict(ind=H.F64, outd=H.F64), "dtype pair"), (dict(outd=H.I64), "dtype pair"),
    (dict(ind=H.BF16, outd=H.F32), "dtype pair"), (dict(ind=H.BF16, outd=H.F16), "dtype pair"), (dict(ind=H.F16, outd=H.BF16), "dtype pair"),
    (dict(ind=H.BF16, outd=H.F32, dx=None), "dtype pair"),
    (dict(V=0, ld=0, ldd=0), "V"), (dict(V=-3), "V"), (dict(rows=-1), "rows"), (dict(ld=15), "stride"), (dict(ldd=15), "gradient row stride"),
    (dict(eps=-0.1), "label_smoothing"), (dict(eps=1.5), "label_smoothing"), (dict(eps=float("nan")), "label_smoothing"),
    (dict(z=-1.0), "z_loss"), (dict(z=float("inf")), "z_loss"), (dict(z=float("nan")), "z_loss"),
    (dict(x=None), "null"), (dict(t=None), "null"), (dict(rowloss=None), "null"),
    (dict(dx="x", outd=H.BF16), "overlaps"),              # in place with differing dtypes
    (dict(dx="x", ld=20, ldd=16, V=12), "overlaps"),      # in place with differing strides
])
def test_rows_refuses_invalid_arguments(kw, what):
    rc = rows_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def test_rows_refuses_partial_overlap_and_misalignment():
    b = Bufs()
    lib = H.lib()
    x = C.addressof(b.x)
    # the gradient starts inside the logits: neither disjoint nor in place
    rc = lib.kf_ce_fused_rows(H.F32, H.F32, 2, 16, 16, x, p(b, "t"), -100, 0.0, 0.0, p(b, "rowloss"), None, x + 64, 16, None, 0, None)
    assert rc == H.KF_ERR_INVALID and "overlaps" in last_error()
    rc = lib.kf_ce_fused_rows(H.F32, H.BF16, 4, 16, 16, x + 2, p(b, "t"), -100, 0.0, 0.0, p(b, "rowloss"), None, p(b, "dx"), 16, None, 0, None)
    assert rc == H.KF_ERR_INVALID and "aligned" in last_error()
    rc = lib.kf_ce_fused_rows(H.F32, H.BF16, 4, 16, 16, x, p(b, "t"), -100, 0.0, 0.0, p(b, "rowloss"), None, C.addressof(b.dx) + 1, 16, None, 0, None)
    assert rc == H.KF_ERR_INVALID and "aligned" in last_error()


def test_rows_refuses_a_small_workspace():
    # 2 x 50257 is the split regime: it needs scratch, for the loss alone too (dlogits NULL: the stand-in buffers are far smaller than the
    # extents named here, and two of them would be seen to overlap). The buffers are never touched: the refusal comes first.
    need = H.ce_fused_rows_workspace_bytes(2, 50257)
    assert need > 0
    b = Bufs()
    for ws, nbytes in ((None, need), ("ws", need - 1), ("ws", 0)):
        rc = rows_call(b, rows=2, V=50257, ld=50257, dx=None, ws=ws, ws_bytes=nbytes)
        assert rc == H.KF_ERR_INVALID and "workspace" in last_error(), (ws, nbytes, rc)


def test_workspace_query_refuses_invalid_arguments():
    n = C.c_size_t(0)
    lib = H.lib()
    assert lib.kf_ce_fused_rows_workspace_bytes(4, 16, None) == H.KF_ERR_INVALID
    for args in ((4, 0), (-1, 16), (4, 1 << 31), (1 << 31, 16)):
        assert lib.kf_ce_fused_rows_workspace_bytes(*args, C.byref(n)) == H.KF_ERR_INVALID and last_error()


def reduce_call(b, rowloss="rowloss", t="t", rows=4, mean=1, loss="loss", count="count"):
    return H.lib().kf_ce_fused_reduce(p(b, rowloss), p(b, t), rows, -100, mean, p(b, loss), p(b, count), None)


@pytest.mark.parametrize("kw,what", [(dict(rowloss=None), "null"), (dict(t=None), "null"), (dict(loss=None), "null loss"), (dict(rows=-1), "rows"),
                                     (dict(mean=2), "mean"), (dict(mean=-1), "mean")])
def test_reduce_refuses_invalid_arguments(kw, what):
    rc = reduce_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def scale_call(b, ind=H.F32, outd=H.F32, n=16, src="x", dst="dx", g="g", count="count"):
    return H.lib().kf_scale_cast(ind, outd, n, p(b, src), p(b, dst), p(b, g), p(b, count), None)


@pytest.mark.parametrize("kw,what", [
    (dict(ind=H.I32), "dtype pair"), (dict(ind=H.BF16, outd=H.F32), "dtype pair"), (dict(ind=H.F16, outd=H.BF16), "dtype pair"),
    (dict(outd=H.F64), "dtype pair"), (dict(n=-1), "n"), (dict(n=(1 << 38) + 1), "n"), (dict(g=None), "null g"), (dict(src=None), "null"),
    (dict(dst=None), "null"), (dict(dst="x", outd=H.BF16), "overlaps"),
])
def test_scale_cast_refuses_invalid_arguments(kw, what):
    rc = scale_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def test_scale_cast_refuses_partial_overlap():
    b = Bufs()
    x = C.addressof(b.x)
    rc = H.lib().kf_scale_cast(H.F32, H.F32, 8, x, x + 16, p(b, "g"), None, None)
    assert rc == H.KF_ERR_INVALID and "overlaps" in last_error()


@pytest.mark.parametrize("chunk_rows", [1, 100, 127, 129, 192, -128, 1000])
def test_operator_refuses_a_chunk_that_is_not_a_multiple_of_128(chunk_rows):
    with pytest.raises(Exception, match="multiple of 128"):
        kfunca._linear_ce_chunk_rows(chunk_rows)


def test_operator_chunk_default_and_multiples():
    assert kfunca._linear_ce_chunk_rows(0) == kfunca._linear_ce_chunk_rows() > 0 and kfunca._linear_ce_chunk_rows(0) % 128 == 0
    for c in (128, 256, 1024, 8192):
        assert kfunca._linear_ce_chunk_rows(c) == c


def test_empty_calls_are_ok_without_a_launch():
    b = Bufs()
    assert rows_call(b, rows=0) == H.KF_OK
    assert scale_call(b, n=0) == H.KF_OK


def test_valid_calls_without_a_device_fail_loudly():
    if H.device_count() > 0:
        return  # the device path is covered by tests/test_gpu_ce_fused.py
    b = Bufs()
    assert rows_call(b) != H.KF_OK and last_error()
    assert rows_call(b, dx=None) != H.KF_OK and last_error()
    assert rows_call(b, dx="x") != H.KF_OK and last_error()   # in place: accepted by the checks, refused by the missing device
    assert reduce_call(b) != H.KF_OK and last_error()
    assert scale_call(b) != H.KF_OK and last_error()
    assert scale_call(b, dst="x", count=None) != H.KF_OK and last_error()
