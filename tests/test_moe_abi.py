"""CPU-only: the mixture-of-experts routing entries of the C ABI (kf_moe_plan_workspace_bytes, kf_moe_plan, kf_moe_gate_fwd, kf_moe_gate_bwd,
kf_moe_dispatch, kf_moe_combine, kf_moe_combine_bwd) are declared and exported, kf_abi_version() is still 7, every invalid argument is
refused with KF_ERR_INVALID and the entry's name in the message before any device call (the pointers here are host memory), T k >= 2^31
is KF_ERR_UNSUPPORTED, zero extents are KF_OK without a launch, the workspace query says what the plan needs, a valid call without a
device reports an error, and the operator surface exists."""
import ctypes as C
import re
from pathlib import Path

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_moe_plan_workspace_bytes", "kf_moe_plan", "kf_moe_gate_fwd", "kf_moe_gate_bwd", "kf_moe_dispatch", "kf_moe_combine", "kf_moe_combine_bwd")
T, K, E, D = 6, 2, 3, 8


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert H.lib().kf_abi_version() == 7


def last_error():
    return H.lib().kf_last_error().decode()


def need(t=T, k=K, e=E):
    return H.moe_plan_workspace_bytes(t, k, e)


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self):
        for n in ("x", "xs", "ys", "y", "dy", "dys", "gate", "dgate", "p", "dp"):
            setattr(self, n, (C.c_float * 1024)())
        for n in ("ids", "off", "nv"):
            setattr(self, n, (C.c_int64 * 64)())
        for n in ("rp", "pr"):
            setattr(self, n, (C.c_int32 * 64)())
        self.ws = (C.c_char * (need() + 64))()

    def p_(self, name, off=0):
        return None if name is None else C.addressof(getattr(self, name)) + off

    def ws16(self, off=0):
        return (C.addressof(self.ws) + 15) // 16 * 16 + off


def plan(b, t=T, k=K, e=E, ids="ids", off="off", rp="rp", pr="pr", ws=True, ws_bytes=None, ws_off=0, ids_off=0, rp_off=0, off_off=0):
    return H.lib().kf_moe_plan(b.p_(ids, ids_off), t, k, e, b.p_(off, off_off), b.p_(rp, rp_off), b.p_(pr), b.ws16(ws_off) if ws else None,
                               need() if ws_bytes is None else ws_bytes, None)


def gate_fwd(b, dtype=H.F32, t=T, k=K, e=E, ids="ids", p="p", ldp=E, normalize=0, gate="gate", ldg=K, p_off=0, ids_off=0):
    return H.lib().kf_moe_gate_fwd(dtype, t, k, e, b.p_(ids, ids_off), b.p_(p, p_off), ldp, normalize, b.p_(gate), ldg, None)


def gate_bwd(b, dtype=H.F32, t=T, k=K, e=E, ids="ids", p="p", ldp=E, normalize=1, gate="gate", ldg=K, dgate="dgate", lddg=K, dp="dp", lddp=E, dp_off=0):
    return H.lib().kf_moe_gate_bwd(dtype, t, k, e, b.p_(ids), b.p_(p), ldp, normalize, b.p_(gate), ldg, b.p_(dgate), lddg, b.p_(dp, dp_off), lddp, None)


def dispatch(b, dtype=H.F32, t=T, k=K, cols=D, rp="rp", x="x", ldx=D, xs="xs", ldxs=D, x_off=0, rp_off=0):
    return H.lib().kf_moe_dispatch(dtype, t, k, cols, b.p_(rp, rp_off), b.p_(x, x_off), ldx, b.p_(xs), ldxs, None)


def combine(b, dtype=H.F32, t=T, k=K, cols=D, pr="pr", nv="nv", gate="gate", ldg=K, ys="ys", ldys=D, y="y", ldy=D, y_off=0, nv_off=0, pr_off=0):
    return H.lib().kf_moe_combine(dtype, t, k, cols, b.p_(pr, pr_off), b.p_(nv, nv_off), b.p_(gate), ldg, b.p_(ys), ldys, b.p_(y, y_off), ldy, None)


def combine_bwd(b, dtype=H.F32, t=T, k=K, cols=D, pr="pr", nv="nv", gate="gate", ldg=K, ys="ys", ldys=D, dy="dy", lddy=D, dys="dys", lddys=D,
                dgate="dgate", lddg=K, dy_off=0, nv_off=0):
    return H.lib().kf_moe_combine_bwd(dtype, t, k, cols, b.p_(pr), b.p_(nv, nv_off), b.p_(gate), ldg, b.p_(ys), ldys, b.p_(dy, dy_off), lddy, b.p_(dys),
                                      lddys, b.p_(dgate), lddg, None)


def refused(rc, entry, what):
    assert rc == H.KF_ERR_INVALID, (rc, last_error())
    assert entry + ":" in last_error() and what in last_error(), last_error()


@pytest.mark.parametrize("kw,what", [
    (dict(t=-1), "extents"), (dict(k=0), "extents"), (dict(k=-2), "extents"), (dict(e=0), "extents"), (dict(e=-1), "extents"),
    (dict(ids=None), "null ids"), (dict(off=None), "null offsets"), (dict(rp=None), "null row_pair"), (dict(pr=None), "null pair_row"),
    (dict(ids_off=4), "ids not aligned"), (dict(rp_off=2), "row_pair not aligned"), (dict(off_off=4), "offsets not aligned"),
    (dict(ws=False), "workspace too small or missing"), (dict(ws_bytes=need() - 1), "workspace too small"), (dict(ws_bytes=0), "workspace too small"),
    (dict(ws_off=8), "workspace not 16-byte aligned"),
])
def test_plan_refuses(kw, what):
    refused(plan(Bufs(), **kw), "kf_moe_plan", what)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(dtype=H.I32), "dtype"), (dict(dtype=99), "dtype"),
    (dict(t=-1), "extents"), (dict(k=0), "extents"), (dict(e=0), "extents"),
    (dict(ids=None), "null ids"), (dict(p=None), "null p"), (dict(gate=None), "null gate"),
    (dict(ldp=E - 1), "leading dimension of p"), (dict(ldg=K - 1), "leading dimension of gate"),
    (dict(normalize=2), "normalize"), (dict(normalize=-1), "normalize"),
    (dict(p_off=2), "p not aligned"), (dict(ids_off=4), "ids not aligned"),
])
def test_gate_fwd_refuses(kw, what):
    refused(gate_fwd(Bufs(), **kw), "kf_moe_gate_fwd", what)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.U8), "dtype"), (dict(t=-1), "extents"), (dict(k=0), "extents"), (dict(e=-5), "extents"),
    (dict(ids=None), "null ids"), (dict(p=None), "null p"), (dict(gate=None), "null gate"), (dict(dgate=None), "null dgate"), (dict(dp=None), "null dp"),
    (dict(ldp=E - 1), "leading dimension of p"), (dict(ldg=K - 1), "leading dimension of gate"), (dict(lddg=0), "leading dimension of dgate"),
    (dict(lddp=E - 1), "leading dimension of dp"), (dict(normalize=3), "normalize"), (dict(dp_off=1), "dp not aligned"),
])
def test_gate_bwd_refuses(kw, what):
    refused(gate_bwd(Bufs(), **kw), "kf_moe_gate_bwd", what)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.F64), "dtype"), (dict(t=-1), "extents"), (dict(k=0), "extents"), (dict(cols=-1), "extents"),
    (dict(rp=None), "null row_pair"), (dict(x=None), "null x"), (dict(xs=None), "null xs"),
    (dict(ldx=D - 1), "leading dimension of x"), (dict(ldxs=D - 1), "leading dimension of xs"),
    (dict(x_off=2), "x not aligned"), (dict(rp_off=2), "row_pair not aligned"),
])
def test_dispatch_refuses(kw, what):
    refused(dispatch(Bufs(), **kw), "kf_moe_dispatch", what)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.I64), "dtype"), (dict(t=-1), "extents"), (dict(k=-1), "extents"), (dict(cols=-3), "extents"),
    (dict(pr=None), "null pair_row"), (dict(ys=None), "null ys"), (dict(y=None), "null y"),
    (dict(ldys=D - 1), "leading dimension of ys"), (dict(ldy=D - 1), "leading dimension of y"), (dict(ldg=K - 1), "leading dimension of gate"),
    (dict(y_off=3), "y not aligned"), (dict(nv_off=4), "n_valid not aligned"), (dict(pr_off=1), "pair_row not aligned"),
])
def test_combine_refuses(kw, what):
    refused(combine(Bufs(), **kw), "kf_moe_combine", what)


@pytest.mark.parametrize("kw,what", [
    (dict(dtype=H.BOOL), "dtype"), (dict(t=-1), "extents"), (dict(k=0), "extents"), (dict(cols=-1), "extents"),
    (dict(pr=None), "null pair_row"), (dict(dy=None), "null dy"), (dict(dys=None), "null dys"), (dict(ys=None), "null ys"),
    (dict(gate=None), "dgate without a gate"),
    (dict(lddy=D - 1), "leading dimension of dy"), (dict(lddys=D - 1), "leading dimension of dys"), (dict(ldys=D - 1), "leading dimension of ys"),
    (dict(ldg=K - 1), "leading dimension of gate"), (dict(lddg=K - 1), "leading dimension of dgate"),
    (dict(dy_off=2), "dy not aligned"), (dict(nv_off=4), "n_valid not aligned"),
])
def test_combine_bwd_refuses(kw, what):
    refused(combine_bwd(Bufs(), **kw), "kf_moe_combine_bwd", what)


def test_more_pairs_than_the_tables_index_are_unsupported():
    b = Bufs()
    big = dict(t=1 << 30, k=2)
    for f, entry in ((plan, "kf_moe_plan"), (gate_fwd, "kf_moe_gate_fwd"), (gate_bwd, "kf_moe_gate_bwd"), (dispatch, "kf_moe_dispatch"),
                     (combine, "kf_moe_combine"), (combine_bwd, "kf_moe_combine_bwd")):
        rc = f(b, **big)
        assert rc == H.KF_ERR_UNSUPPORTED and entry + ":" in last_error() and "32-bit" in last_error(), (entry, rc, last_error())
    out = C.c_size_t(0)
    assert H.lib().kf_moe_plan_workspace_bytes(1 << 30, 2, 4, C.byref(out)) == H.KF_ERR_UNSUPPORTED
    assert H.lib().kf_moe_plan_workspace_bytes(1 << 40, 1 << 40, 4, C.byref(out)) == H.KF_ERR_UNSUPPORTED    # T k overflows int64
    assert dispatch(b, t=1 << 30, k=2, x=None) == H.KF_ERR_INVALID                                            # the checks still come first
    assert H.lib().kf_moe_plan_workspace_bytes((1 << 31) - 1, 1, 4, C.byref(out)) == H.KF_OK


def test_workspace_query():
    f = H.lib().kf_moe_plan_workspace_bytes
    out = C.c_size_t(0)
    for args in ((-1, 2, 2), (8, 0, 2), (8, 2, 0), (8, -1, 2)):
        assert f(*args, C.byref(out)) == H.KF_ERR_INVALID and "kf_moe_plan_workspace_bytes" in last_error(), args
    assert f(8, 2, 2, None) == H.KF_ERR_INVALID and "null" in last_error()
    assert need(0, 2, 4) == 0
    for t, k, e in ((1, 1, 1), (96, 2, 8), (4096, 2, 8), (4097, 2, 8), (4099, 3, 128), (40000, 1, 1)):
        n = t * k
        got = need(t, k, e)
        # the keys, the sorted keys and the positions (int64 each) and kf_sort's own scratch (none up to 8192 keys)
        sort = H.lib().kf_sort_workspace_bytes(H.I64, 1, n)
        assert got % 16 == 0 and 3 * 8 * n + sort <= got <= 3 * (8 * n + 15) + sort + 15, (t, k, e, got)
        assert (sort == 0) == (n <= 8192)
    assert need(8193, 1, 8) > need(8192, 1, 8)


def test_zero_extents_are_ok_without_a_launch():
    b = Bufs()
    for dtype in (H.F32, H.BF16, H.F16):
        assert gate_fwd(b, dtype=dtype, t=0) == H.KF_OK and gate_bwd(b, dtype=dtype, t=0) == H.KF_OK, last_error()
        for f in (dispatch, combine, combine_bwd):
            assert f(b, dtype=dtype, t=0) == H.KF_OK, last_error()
        assert dispatch(b, dtype=dtype, cols=0) == H.KF_OK and combine(b, dtype=dtype, cols=0) == H.KF_OK, last_error()
        assert combine_bwd(b, dtype=dtype, cols=0, dgate=None) == H.KF_OK, last_error()
    # the checks still come first
    assert dispatch(b, t=0, xs=None) == H.KF_ERR_INVALID and combine(b, cols=0, y=None) == H.KF_ERR_INVALID
    assert combine_bwd(b, t=0, k=0) == H.KF_ERR_INVALID and gate_fwd(b, t=0, e=0) == H.KF_ERR_INVALID
    assert plan(b, t=0, ids=None, rp=None, pr=None, off=None) == H.KF_ERR_INVALID    # zero tokens still write the offsets


def test_optional_operands():
    b = Bufs()
    # no gate, no n_valid, no dgate (and then no ys): accepted as far as validation goes (T = 0: nothing is launched)
    assert combine(b, t=0, gate=None, nv=None) == H.KF_OK, last_error()
    assert combine_bwd(b, t=0, gate=None, dgate=None, ys=None, nv=None) == H.KF_OK, last_error()
    assert combine_bwd(b, t=0, dgate=None, ys=None) == H.KF_OK, last_error()


def test_valid_calls_fail_loudly_without_a_device():
    if H.device_count() > 0:
        pytest.skip("a device is present: host pointers are never launched on one")
    b = Bufs()
    for f in (plan, gate_fwd, gate_bwd, dispatch, combine, combine_bwd):
        assert f(b) != H.KF_OK and last_error(), f.__name__
    assert plan(b, t=0) != H.KF_OK and last_error()     # n == 0 still launches the offsets


def test_operator_surface():
    for n in ("moe_plan", "moe_gate", "moe_dispatch", "moe_combine", "MoePlan"):
        assert n in kfunca.__all__ and hasattr(kfunca, n)
    for n in ("moe_plan", "moe_gate", "moe_dispatch", "moe_combine"):
        assert callable(getattr(kfunca, n)) and getattr(kfunca, n).__doc__
    for field in ("offsets", "row_pair", "pair_row", "ids", "T", "k", "E"):
        assert hasattr(kfunca.MoePlan, field), field
    assert "expert_linear" in kfunca.moe_plan.__doc__ and "topk" in kfunca.moe_plan.__doc__
    assert "pair_row" in kfunca.moe_combine.__doc__ and "row_pair" in kfunca.moe_dispatch.__doc__


def test_the_committed_bench_profile_was_measured_on_these_sources():
    import json

    import bench
    obj = json.loads((ROOT / "profiles" / "r06_moe_route_bench.json").read_text())
    sources = ("moe.hip", "float_pack.h", "common.h", "sort.hip")
    assert bench.stamp_is_current(obj, sources), "profiles/r06_moe_route_bench.json is stale: re-run tools/moe_route_bench.py --check"
    assert len(obj["cases"]) == 6 and all(k["ok"] for c in obj["cases"] for k in c["check"])
