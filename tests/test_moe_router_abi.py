"""CPU-only: the router entries of the C ABI (kf_moe_router_fwd, kf_moe_router_bwd, kf_moe_aux_loss_workspace_bytes, kf_moe_aux_loss_fwd,
kf_moe_aux_loss_bwd) are declared and exported, kf_abi_version() is still 7, every invalid argument is refused with KF_ERR_INVALID and
the entry's name in the message before any device call (the pointers here are host memory), E > 1024 and k > min(E, 64) are
KF_ERR_UNSUPPORTED, T == 0 is KF_OK without a launch, the workspace query is monotone in T and 16-byte granular, a valid call without a
device reports an error, and the operator surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_moe_router_fwd", "kf_moe_router_bwd", "kf_moe_aux_loss_workspace_bytes", "kf_moe_aux_loss_fwd", "kf_moe_aux_loss_bwd")
T, E, K = 6, 8, 2


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert re.search(r"KF_MOE_SCORE_SOFTMAX = 0, KF_MOE_SCORE_SIGMOID = 1", text)
    assert (H.MOE_SCORE_SOFTMAX, H.MOE_SCORE_SIGMOID) == (0, 1)
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


def need(t=T, e=E):
    return H.moe_aux_loss_workspace_bytes(t, e)


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("logits", "gate", "dgate", "dlogits"):
            setattr(self, n, (C.c_float * 4096)())
        for n in ("ids", "off"):
            setattr(self, n, (C.c_int64 * 2048)())
        for n in ("loss", "parts", "dloss"):
            setattr(self, n, (C.c_float * 4)())
        self.ws = (C.c_char * (need(64, 1024) + 64))()

    def p_(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off

    def ws16(self, off=0):
        return (C.addressof(self.ws) + 15) // 16 * 16 + off


def fwd(b, dtype=H.F32, t=T, e=E, k=K, score=0, normalize=1, logits="logits", ldl=None, ids="ids", gate="gate", ldg=None, l_off=0, ids_off=0, g_off=0):
    return H.lib().kf_moe_router_fwd(dtype, t, e, k, score, normalize, b.p_(logits, l_off), e if ldl is None else ldl, b.p_(ids, ids_off), b.p_(gate, g_off),
                                     k if ldg is None else ldg, None)


def bwd(b, dtype=H.F32, t=T, e=E, k=K, score=0, normalize=1, logits="logits", ldl=None, ids="ids", dgate="dgate", lddg=None, dlogits="dlogits", lddl=None,
        l_off=0, ids_off=0, dl_off=0):
    return H.lib().kf_moe_router_bwd(dtype, t, e, k, score, normalize, b.p_(logits, l_off), e if ldl is None else ldl, b.p_(ids, ids_off), b.p_(dgate),
                                     k if lddg is None else lddg, b.p_(dlogits, dl_off), e if lddl is None else lddl, None)


def aux_fwd(b, dtype=H.F32, t=T, e=E, k=K, logits="logits", ldl=None, off="off", loss="loss", parts="parts", ws=True, ws_bytes=None, ws_off=0, l_off=0,
            off_off=0, loss_off=0, parts_off=0):
    return H.lib().kf_moe_aux_loss_fwd(dtype, t, e, k, b.p_(logits, l_off), e if ldl is None else ldl, b.p_(off, off_off), 1e-2, 1e-3, b.p_(loss, loss_off),
                                       b.p_(parts, parts_off), b.ws16(ws_off) if ws else None, need(max(t, 0), min(max(e, 1), 1024)) if ws_bytes is None else ws_bytes,
                                       None)


def aux_bwd(b, dtype=H.F32, t=T, e=E, k=K, logits="logits", ldl=None, off="off", dloss="dloss", dlogits="dlogits", lddl=None, l_off=0, off_off=0, dloss_off=0,
            dl_off=0):
    return H.lib().kf_moe_aux_loss_bwd(dtype, t, e, k, b.p_(logits, l_off), e if ldl is None else ldl, b.p_(off, off_off), 1e-2, 1e-3, b.p_(dloss, dloss_off),
                                       b.p_(dlogits, dl_off), e if lddl is None else lddl, None)


def refused(rc, entry, what, code=H.KF_ERR_INVALID):
    assert rc == code, (rc, last_error())
    assert entry + ":" in last_error() and what in last_error(), last_error()


COMMON = [(dict(dtype=H.F64), "dtype"), (dict(dtype=H.I32), "dtype"), (dict(dtype=99), "dtype"), (dict(t=-1), "extents"), (dict(e=0), "extents"),
          (dict(k=0), "extents"), (dict(k=-2), "extents"), (dict(t=1 << 62), "overflows"), (dict(logits=None), "null logits"),
          (dict(ldl=E - 1), "leading dimension of logits"), (dict(l_off=2), "logits not aligned")]
LIMITS = [dict(e=1025, k=2), dict(e=4096, k=2), dict(k=E + 1), dict(e=128, k=65), dict(e=1024, k=1000)]


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(score=2), "score"), (dict(score=-1), "score"), (dict(normalize=2), "normalize"), (dict(normalize=-1), "normalize"),
    (dict(ids=None), "null ids"), (dict(gate=None), "null gate"), (dict(ldg=K - 1), "leading dimension of gate"), (dict(ids_off=4), "ids not aligned"),
    (dict(g_off=1), "gate not aligned"),
])
def test_router_fwd_refuses(kw, what):
    refused(fwd(Bufs(), **kw), "kf_moe_router_fwd", what)


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(score=2), "score"), (dict(normalize=3), "normalize"), (dict(ids=None), "null ids"), (dict(dgate=None), "null dgate"),
    (dict(dlogits=None), "null dlogits"), (dict(lddg=K - 1), "leading dimension of dgate"), (dict(lddl=E - 1), "leading dimension of dlogits"),
    (dict(ids_off=4), "ids not aligned"), (dict(dl_off=2), "dlogits not aligned"),
])
def test_router_bwd_refuses(kw, what):
    refused(bwd(Bufs(), **kw), "kf_moe_router_bwd", what)


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(off=None), "null offsets"), (dict(off_off=4), "offsets not aligned"), (dict(loss=None), "null loss"), (dict(loss_off=2), "loss not aligned"),
    (dict(parts_off=2), "parts not aligned"), (dict(ws=False), "workspace too small or missing"), (dict(ws_bytes=need() - 1), "workspace too small"),
    (dict(ws_bytes=0), "workspace too small"), (dict(ws_off=8), "workspace not 16-byte aligned"),
])
def test_aux_fwd_refuses(kw, what):
    refused(aux_fwd(Bufs(), **kw), "kf_moe_aux_loss_fwd", what)


@pytest.mark.parametrize("kw,what", COMMON + [
    (dict(off=None), "null offsets"), (dict(off_off=4), "offsets not aligned"), (dict(dloss=None), "null dloss"), (dict(dloss_off=2), "dloss not aligned"),
    (dict(dlogits=None), "null dlogits"), (dict(lddl=E - 1), "leading dimension of dlogits"), (dict(dl_off=2), "dlogits not aligned"),
])
def test_aux_bwd_refuses(kw, what):
    refused(aux_bwd(Bufs(), **kw), "kf_moe_aux_loss_bwd", what)


@pytest.mark.parametrize("kw", LIMITS)
def test_more_than_a_wave_holds_is_unsupported(kw):
    b = Bufs()
    for f, entry in ((fwd, "kf_moe_router_fwd"), (bwd, "kf_moe_router_bwd"), (aux_fwd, "kf_moe_aux_loss_fwd"), (aux_bwd, "kf_moe_aux_loss_bwd")):
        refused(f(b, **kw), entry, "one wave holds", H.KF_ERR_UNSUPPORTED)
    assert fwd(b, dtype=H.F64, **kw) == H.KF_ERR_INVALID and fwd(b, t=-1, **kw) == H.KF_ERR_INVALID    # the dtype and the extents come first


def test_the_limits_themselves_are_supported():
    b = Bufs()
    for kw in (dict(e=1024, k=64), dict(e=64, k=64), dict(e=1, k=1), dict(e=1000, k=1)):
        for f in (fwd, bwd, aux_fwd, aux_bwd):
            assert f(b, t=0, **kw) == H.KF_OK, (f.__name__, kw, last_error())


def test_workspace_query():
    f = H.lib().kf_moe_aux_loss_workspace_bytes
    out = C.c_size_t(0)
    for args in ((-1, 8), (8, 0), (8, -1)):
        assert f(*args, C.byref(out)) == H.KF_ERR_INVALID and "kf_moe_aux_loss_workspace_bytes" in last_error(), args
    assert f(8, 8, None) == H.KF_ERR_INVALID and "null" in last_error()
    assert f(8, 1025, C.byref(out)) == H.KF_ERR_UNSUPPORTED and "kf_moe_aux_loss_workspace_bytes" in last_error()
    assert need(0, 8) == 0
    for e in (1, 8, 127, 128, 1000, 1024):
        sizes = [need(t, e) for t in (1, 2, 4, 5, 63, 64, 1027, 4099, 32768, 1 << 20, 1 << 40)]
        assert all(s % 16 == 0 and s >= 4 * (e + 1) for s in sizes), (e, sizes)
        assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (e, sizes)          # monotone in T, and it does grow
        assert sizes[-1] == sizes[-2] <= 2 << 20, (e, sizes)                        # bounded: the blocks walk the rows beyond that


def test_zero_tokens_are_ok_without_a_launch():
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        for f in (fwd, bwd, aux_fwd, aux_bwd):
            assert f(b, dtype=dtype, t=0) == H.KF_OK, (f.__name__, last_error())
    assert aux_fwd(b, t=0, ws=False, ws_bytes=0) == H.KF_OK and aux_fwd(b, t=0, parts=None) == H.KF_OK, last_error()
    # the checks still come first
    assert fwd(b, t=0, gate=None) == H.KF_ERR_INVALID and bwd(b, t=0, dlogits=None) == H.KF_ERR_INVALID
    assert aux_fwd(b, t=0, loss=None) == H.KF_ERR_INVALID and aux_bwd(b, t=0, dloss=None) == H.KF_ERR_INVALID
    assert fwd(b, t=0, e=2000) == H.KF_ERR_UNSUPPORTED


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        pytest.skip("a device is present: host pointers are never launched on one")
    b = Bufs()
    for f in (fwd, bwd, aux_fwd, aux_bwd):
        assert f(b) != H.KF_OK and last_error(), f.__name__
    assert aux_fwd(b, parts=None) != H.KF_OK


def test_operator_surface():
    for n in ("moe_route", "moe_aux_loss"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n)) and getattr(kfunca, n).__doc__
    assert "topk" in kfunca.moe_route.__doc__ and "sigmoid" in kfunca.moe_route.__doc__ and "normalize" in kfunca.moe_route.__doc__
    assert "balance_coef" in kfunca.moe_aux_loss.__doc__ and "return_parts" in kfunca.moe_aux_loss.__doc__ and "Mixtral" in kfunca.moe_aux_loss.__doc__


def test_the_committed_bench_profile_was_measured_on_this_source():
    import json

    import bench
    obj = json.loads((ROOT / "profiles" / "r06_moe_router_bench.json").read_text())
    assert bench.stamp_is_current(obj, ("moe_router.hip", "float_pack.h", "common.h")), \
        "profiles/r06_moe_router_bench.json is stale: re-run tools/moe_router_bench.py --check"
    assert len(obj["cases"]) == 4 and all(k["ok"] for c in obj["cases"] for k in c["check"])
