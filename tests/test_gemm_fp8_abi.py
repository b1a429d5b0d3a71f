"""CPU-only: the FP8 entries of the C ABI (kf_fp8_amax, kf_fp8_quantize, kf_gemm_fp8) are declared and exported, the ABI version is still
7, every invalid argument is refused with KF_ERR_INVALID and a message before any device call (host buffers stand in for device pointers,
as in tests/test_ce_fused_abi.py), linear_fp8 refuses a K or N that is not a multiple of 16, and a valid call without a device reports an
error instead of falling back to a CPU path."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_fp8_amax", "kf_fp8_quantize", "kf_gemm_fp8")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
        assert callable(getattr(H, n[3:]))
    assert H.FP8_E4M3 == 0 and H.FP8_E5M2 == 1
    assert H.lib().kf_abi_version() == 7 and re.search(r"#define KF_ABI_VERSION 7\b", text)
    for n in ("fp8_quantize", "gemm_fp8", "linear_fp8"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        self.x = (C.c_float * 1024)()
        self.amax = (C.c_float * 1)()
        self.sinv = (C.c_float * 1)()
        self.sinv2 = (C.c_float * 1)()
        self.q = (C.c_char * 4096)()
        self.qt = (C.c_char * 4096)()
        self.a = (C.c_char * 4096)()
        self.b = (C.c_char * 4096)()
        self.c = (C.c_float * 1024)()


def p(b, n, off=0):
    if n is None:
        return None
    a = C.addressof(getattr(b, n))
    a += (-a) % 16          # ctypes arrays are 8- or 16-byte aligned: make every base 16-byte aligned, then apply the asked offset
    return a + off


def amax_call(b, dtype=H.F32, rows=4, cols=16, ld=16, x="x", amax="amax", xoff=0):
    return H.lib().kf_fp8_amax(dtype, rows, cols, ld, p(b, x, xoff), p(b, amax), None)


def quant_call(b, dtype=H.F32, fmt=H.FP8_E4M3, rows=4, cols=16, ld=16, x="x", amax="amax", q="q", ldq=16, qt="qt", ldqt=16, sinv="sinv"):
    return H.lib().kf_fp8_quantize(dtype, fmt, rows, cols, ld, p(b, x), p(b, amax), p(b, q), ldq, p(b, qt), ldqt, p(b, sinv), None)


def gemm_call(b, fa=H.FP8_E4M3, fb=H.FP8_E4M3, out=H.F32, M=4, N=4, K=16, a="a", lda=16, bb="b", ldb=16, sa="sinv", sb="sinv2", c="c", ldc=4, aoff=0,
              boff=0):
    return H.lib().kf_gemm_fp8(fa, fb, out, M, N, K, p(b, a, aoff), lda, p(b, bb, boff), ldb, p(b, sa), p(b, sb), p(b, c), ldc, None)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I32), "dtype"), (dict(rows=-1), "negative"), (dict(cols=-1, ld=0), "negative"),
    (dict(ld=15), "ld"), (dict(x=None), "null x"), (dict(amax=None), "null amax"), (dict(xoff=2), "aligned"),
])
def test_amax_refuses_invalid_arguments(kw, what):
    rc = amax_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert "kf_fp8_amax" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(fmt=2), "format"), (dict(fmt=-1), "format"), (dict(rows=-1), "negative"), (dict(ld=15), "ld"),
    (dict(ldq=15), "ldq"), (dict(ldqt=15), "ldqt"), (dict(rows=17, ldqt=31), "ldqt"), (dict(x=None), "null x"), (dict(amax=None), "null"),
    (dict(q=None), "null"), (dict(sinv=None), "null"),
])
def test_quantize_refuses_invalid_arguments(kw, what):
    rc = quant_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert "kf_fp8_quantize" in last_error() and what in last_error(), last_error()


def test_quantize_accepts_a_short_ldqt_without_qt():
    # ldqt is only read with qt; the call then fails on the missing device, or runs on a box that has one
    if H.device_count() == 0:
        assert quant_call(Bufs(), qt=None, ldqt=0) not in (H.KF_OK, H.KF_ERR_INVALID)


@pytest.mark.parametrize("kw,what", [
    (dict(K=8, lda=16, ldb=16), "multiple of 16"), (dict(K=24, lda=32, ldb=32), "multiple of 16"), (dict(K=0), "multiple of 16"),
    (dict(K=-16), "multiple of 16"), (dict(lda=24, K=16), "multiples of 16"), (dict(ldb=40, K=16), "multiples of 16"),
    (dict(K=32, lda=16, ldb=32), "below K"), (dict(K=32, lda=32, ldb=16), "below K"), (dict(lda=(1 << 24) + 16), "2^24"),
    (dict(aoff=8), "16-byte aligned"), (dict(boff=4), "16-byte aligned"), (dict(fa=2), "format"), (dict(fb=-1), "format"),
    (dict(out=H.F64), "out_dtype"), (dict(out=H.U8), "out_dtype"), (dict(out=H.I32), "out_dtype"), (dict(M=-1), "negative"),
    (dict(N=-2, ldc=0), "negative"), (dict(ldc=3), "ldc"), (dict(a=None), "null"), (dict(bb=None), "null"), (dict(c=None), "null"),
    (dict(sa=None), "null"), (dict(sb=None), "null"),
])
def test_gemm_refuses_invalid_arguments(kw, what):
    rc = gemm_call(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert "kf_gemm_fp8" in last_error() and what in last_error(), last_error()


def test_empty_products_are_ok_without_a_launch():
    b = Bufs()
    assert gemm_call(b, M=0) == H.KF_OK and gemm_call(b, N=0, ldc=0) == H.KF_OK


@pytest.mark.parametrize("K,N", [(8, 16), (24, 16), (16, 8), (16, 40), (0, 16), (16, 0), (100, 100)])
def test_linear_fp8_refuses_dims_that_are_no_multiple_of_16(K, N):
    with pytest.raises(Exception, match="multiple of 16"):
        kfunca._linear_fp8_check_dims(K, N)


def test_linear_fp8_accepts_multiples_of_16():
    for K, N in ((16, 16), (48, 80), (4096, 14336)):
        kfunca._linear_fp8_check_dims(K, N)


def test_valid_calls_without_a_device_fail_loudly():
    if H.device_count() > 0:
        return  # the device path is covered by tests/test_gpu_fp8_quantize.py and tests/test_gpu_gemm_fp8.py
    b = Bufs()
    assert amax_call(b) != H.KF_OK and last_error()
    assert quant_call(b) != H.KF_OK and last_error()
    assert gemm_call(b) != H.KF_OK and last_error()
