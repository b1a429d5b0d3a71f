"""CPU-only: the segmented-GEMM entries of the C ABI (kf_segment_offsets, kf_gemm_segmented_workspace_bytes, kf_gemm_segmented,
kf_gemm_segmented_wgrad) are declared and exported, every invalid argument is refused with KF_ERR_INVALID and the entry's name in the
message before any device call (the pointers here are host memory), zero extents are KF_OK without a launch, the workspace query says
what the kernels' plan needs, a valid call without a device reports an error, and the operator surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_segment_offsets", "kf_gemm_segmented_workspace_bytes", "kf_gemm_segmented", "kf_gemm_segmented_wgrad")
T, N, K, E = 6, 8, 4, 3


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


def need(dtype=H.BF16, t=T, e=E):
    return H.gemm_segmented_workspace_bytes(dtype, t, e)


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("a", "w", "c", "b", "dw"):
            setattr(self, n, (C.c_float * 1024)())
        self.off = (C.c_int64 * 16)()
        self.ids = (C.c_int64 * 16)()
        self.ws = (C.c_char * (need() + 64))()

    def p(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off

    def ws16(self, off=0):
        return (C.addressof(self.ws) + 15) // 16 * 16 + off


def fwd(b, dtype=H.F32, trans_b=0, t=T, n=N, k=K, e=E, off="off", a="a", lda=K, w="w", ldw=None, w_stride=None, c="c", ldc=N, ws=True, ws_bytes=None,
        ws_off=0, a_off=0):
    ldw = (k if trans_b == 1 else n) if ldw is None else ldw
    w_stride = n * k if w_stride is None else w_stride
    return H.lib().kf_gemm_segmented(dtype, trans_b, t, n, k, e, b.p(off), 1.0, b.p(a, a_off), lda, b.p(w), ldw, w_stride, 0.0, b.p(c), ldc,
                                     b.ws16(ws_off) if ws else None, need() if ws_bytes is None else ws_bytes, None)


def wgrad(b, dtype=H.F32, t=T, m=K, n=N, e=E, off="off", a="a", lda=K, bb="b", ldb=N, dw="dw", lddw=N, dw_stride=None, ws=True, ws_bytes=None, ws_off=0,
          b_off=0):
    dw_stride = m * n if dw_stride is None else dw_stride
    return H.lib().kf_gemm_segmented_wgrad(dtype, t, m, n, e, b.p(off), 1.0, b.p(a), lda, b.p(bb, b_off), ldb, 0.0, b.p(dw), lddw, dw_stride,
                                           b.ws16(ws_off) if ws else None, need() if ws_bytes is None else ws_bytes, None)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I32), "dtype"), (dict(dtype=99), "dtype"),
    (dict(trans_b=2), "trans_b"), (dict(trans_b=-1), "trans_b"),
    (dict(t=-1), "extents"), (dict(n=-1), "extents"), (dict(k=-2), "extents"), (dict(e=0), "extents"), (dict(e=-3), "extents"),
    (dict(off=None), "null"), (dict(a=None), "null"), (dict(w=None), "null"), (dict(c=None), "null"),
    (dict(lda=K - 1), "pitch of A"), (dict(ldw=N - 1), "pitch of W"), (dict(trans_b=1, ldw=K - 1), "pitch of W"), (dict(ldc=N - 1), "pitch of C"),
    (dict(w_stride=N * K - 1), "w_stride"),
    (dict(a_off=2), "aligned"),
    (dict(ws=False), "workspace"), (dict(ws_bytes=need() - 1), "workspace too small"), (dict(ws_bytes=0), "workspace too small"),
    (dict(ws_off=8), "workspace not 16-byte aligned"),
])
def test_forward_refuses(kw, what):
    rc = fwd(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_gemm_segmented:" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(dtype=H.U8), "dtype"),
    (dict(t=-1), "extents"), (dict(m=-1), "extents"), (dict(n=-4), "extents"), (dict(e=0), "extents"),
    (dict(off=None), "null"), (dict(a=None), "null"), (dict(bb=None), "null"), (dict(dw=None), "null"),
    (dict(lda=K - 1), "pitch of A"), (dict(ldb=N - 1), "pitch of B"), (dict(lddw=N - 1), "pitch of dW"),
    (dict(dw_stride=K * N - 1), "dw_stride"),
    (dict(b_off=1), "aligned"),
    (dict(ws=False), "workspace"), (dict(ws_bytes=need() - 1), "workspace too small"), (dict(ws_off=4), "workspace not 16-byte aligned"),
])
def test_wgrad_refuses(kw, what):
    rc = wgrad(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc, last_error())
    assert "kf_gemm_segmented_wgrad:" in last_error() and what in last_error(), last_error()


def test_segment_offsets_refuses():
    b = Bufs()
    f = H.lib().kf_segment_offsets
    for args, what in (((b.p("ids"), -1, 3, b.p("off"), None), "extents"), ((b.p("ids"), 4, 0, b.p("off"), None), "extents"),
                       ((None, 4, 3, b.p("off"), None), "null"), ((b.p("ids"), 4, 3, None, None), "null"),
                       ((b.p("ids", 4), 4, 3, b.p("off"), None), "aligned")):
        rc = f(*args)
        assert rc == H.KF_ERR_INVALID and "kf_segment_offsets" in last_error() and what in last_error(), (args, rc, last_error())


def test_workspace_query():
    f = H.lib().kf_gemm_segmented_workspace_bytes
    out = C.c_size_t(0)
    for args in ((H.F64, 8, 2), (H.I64, 8, 2), (H.F32, -1, 2), (H.F32, 8, 0)):
        assert f(*args, C.byref(out)) == H.KF_ERR_INVALID and "kf_gemm_segmented_workspace_bytes" in last_error(), args
    assert f(H.F32, 8, 2, None) == H.KF_ERR_INVALID and "null" in last_error()
    for dtype in (H.F32, H.BF16, H.F16):
        for t, e in ((0, 1), (1, 1), (300, 4), (1 << 18, 128), (96, 64)):
            n = H.gemm_segmented_workspace_bytes(dtype, t, e)
            # the sanitised offsets and one 32-byte entry for each of the T / 128 + E + 2 row tiles the grid is launched on
            assert n % 16 == 0 and n >= 8 * (e + 1) + 32 * (t // 128 + e + 2), (dtype, t, e, n)
            assert n <= 8 * (e + 1) + 32 + 32 * (t // 128 + e + 2)
    assert H.gemm_segmented_workspace_bytes(H.BF16, 512, 8) > H.gemm_segmented_workspace_bytes(H.BF16, 256, 8)


@pytest.mark.parametrize("zero", ["t", "n", "k"])
def test_forward_zero_extents_are_ok_without_a_launch(zero):
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for tb in (0, 1):
            assert fwd(b, dtype=dtype, trans_b=tb, **{zero: 0}) == H.KF_OK, last_error()
    assert fwd(b, **{zero: 0}, c=None) == H.KF_ERR_INVALID   # the checks still come first
    assert fwd(b, **{zero: 0}, ws=False) == H.KF_ERR_INVALID


@pytest.mark.parametrize("zero", ["t", "m", "n"])
def test_wgrad_zero_extents_are_ok_without_a_launch(zero):
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        assert wgrad(b, dtype=dtype, **{zero: 0}) == H.KF_OK, last_error()
    assert wgrad(b, **{zero: 0}, dw=None) == H.KF_ERR_INVALID
    assert wgrad(b, **{zero: 0}, e=0) == H.KF_ERR_INVALID


def test_one_expert_needs_no_stride():
    b = Bufs()
    assert fwd(b, e=1, t=0, w_stride=0) == H.KF_OK and wgrad(b, e=1, t=0, dw_stride=0) == H.KF_OK


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        pytest.skip("a device is present: host pointers are never launched on one")
    b = Bufs()
    assert fwd(b) != H.KF_OK and last_error()
    assert wgrad(b) != H.KF_OK and last_error()
    assert H.lib().kf_segment_offsets(b.p("ids"), 4, 3, b.p("off"), None) != H.KF_OK and last_error()


def test_operator_surface():
    for n in ("segment_offsets", "expert_linear"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))
    doc = kfunca.expert_linear.__doc__
    for word in ("softmax", "topk", "sort", "embedding", "swiglu", "inverse permutation", "segment_offsets"):
        assert word in doc, word


def test_the_committed_bench_profile_was_measured_on_these_sources():
    import json

    import bench
    obj = json.loads((ROOT / "profiles" / "r06_expert_gemm_bench.json").read_text())
    sources = ("gemm_seg.hip", "gemm.hip", "common.h")
    assert bench.stamp_is_current(obj, sources), "profiles/r06_expert_gemm_bench.json is stale: re-run tools/expert_gemm_bench.py --check"
    assert len(obj["cases"]) == 45 and all(k["ok"] for c in obj["cases"] for k in c["check"])
