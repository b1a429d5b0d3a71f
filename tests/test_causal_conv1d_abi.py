"""CPU-only: the three kf_causal_conv1d_* entries are exported and typed as the header declares them, the constants have their values,
every refusal comes back with its status and the entry's name before any device call (host buffers stand in for device pointers; no GPU
is needed), and the two operators are public with docstrings."""
import ctypes as C

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

BUF = (C.c_float * (1 << 16))()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 16
Q = lambda i: P + i * 16384   # sixteen disjoint 16 KiB operands
GOOD = dict(dtype=H.BF16, act=H.CONV1D_ACT_SILU, B=2, S=100, C=16, K=4, x=Q(0), ldx=24, w=Q(1), bias=Q(2), h0=Q(3), y=Q(4), ldy=16, hT=Q(5), dy=Q(6),
            lddy=16, d_hT=Q(7), dx=Q(8), lddx=32, dw=Q(9), dbias=Q(10), d_h0=Q(11), ws=Q(12), wsb=16384)
ENTRIES = ("kf_causal_conv1d_fwd", "kf_causal_conv1d_bwd", "kf_causal_conv1d_bwd_workspace_bytes")
INV, UNS = H.KF_ERR_INVALID, H.KF_ERR_UNSUPPORTED
REFUSALS = [   # (change, status, the entries it applies to: f forward, b backward, w workspace query)
    (dict(x=None), INV, "fb"), (dict(w=None), INV, "fb"), (dict(y=None), INV, "f"), (dict(dy=None), INV, "b"), (dict(dx=None), INV, "b"),
    (dict(dw=None), INV, "b"), (dict(K=1), UNS, "fbw"), (dict(K=5), UNS, "fbw"), (dict(C=12), UNS, "fbw"), (dict(dtype=H.F32, C=6), UNS, "fbw"),
    (dict(ldx=8), INV, "fb"), (dict(ldy=15), INV, "f"), (dict(lddx=8), INV, "b"), (dict(ldx=20), UNS, "fb"), (dict(lddy=20), UNS, "b"),
    (dict(x=Q(0) + 2), INV, "fb"), (dict(w=Q(1) + 8), INV, "fb"), (dict(hT=Q(5) + 4), INV, "f"), (dict(d_h0=Q(11) + 4), INV, "b"),
    (dict(dtype=H.F64), UNS, "fbw"), (dict(dtype=99), UNS, "fbw"), (dict(act=2), INV, "fb"), (dict(act=-1), INV, "fb"),
    (dict(S=0), INV, "fbw"), (dict(B=-1), INV, "fbw"),
    # aliasing: in place only within one wave's rows (S <= KF_CONV1D_STEP_MAX), never otherwise
    (dict(y=Q(0), ldy=24), INV, "f"), (dict(hT=Q(3)), INV, "f"), (dict(S=3, y=Q(0), ldy=16), INV, "f"), (dict(y=Q(1)), INV, "f"),
    (dict(hT=Q(3) + 16), INV, "f"), (dict(dx=Q(6), lddx=16), INV, "b"), (dict(dx=Q(0), lddx=24), INV, "b"), (dict(d_h0=Q(7)), INV, "b"),
    (dict(dw=Q(1)), INV, "b"),
]


def call(entry, a):
    head = (a["dtype"], a["act"], a["B"], a["S"], a["C"], a["K"])
    if entry == "kf_causal_conv1d_fwd":
        return H.lib().kf_causal_conv1d_fwd(*head, a["x"], a["ldx"], a["w"], a["bias"], a["h0"], a["y"], a["ldy"], a["hT"], None)
    if entry == "kf_causal_conv1d_bwd":
        return H.lib().kf_causal_conv1d_bwd(*head, a["x"], a["ldx"], a["w"], a["bias"], a["h0"], a["dy"], a["lddy"], a["d_hT"], a["dx"], a["lddx"],
                                            a["dw"], a["dbias"], a["d_h0"], a["ws"], a["wsb"], None)
    return H.lib().kf_causal_conv1d_bwd_workspace_bytes(a["dtype"], a["B"], a["S"], a["C"], a["K"], C.byref(C.c_size_t(0)))


@pytest.mark.parametrize("entry,change,status", [(e, c, s) for c, s, who in REFUSALS for e, k in zip(ENTRIES, "fbw") if k in who])
def test_refusals(entry, change, status):
    assert call(entry, {**GOOD, **change}) == status and entry in H.lib().kf_last_error().decode()


@pytest.mark.parametrize("change", [dict(ws=None), dict(wsb=2 * 5 * 16 * 4 - 1), dict(ws=Q(12) + 4)])   # missing, one byte short, misaligned
def test_workspace_refusals(change):
    assert call("kf_causal_conv1d_bwd", {**GOOD, **change}) == H.KF_ERR_WORKSPACE and "kf_causal_conv1d_bwd" in H.lib().kf_last_error().decode()
    assert H.lib().kf_causal_conv1d_bwd_workspace_bytes(H.BF16, 2, 100, 16, 4, None) == INV


def test_exported_typed_and_sized():
    assert (H.CONV1D_ACT_NONE, H.CONV1D_ACT_SILU, H.CONV1D_STEP_MAX) == (0, 1, 64)
    assert all(n in H.CONSTANTS for n in ("CONV1D_ACT_NONE", "CONV1D_ACT_SILU", "CONV1D_STEP_MAX"))
    for n in ENTRIES:
        fn, (restype, argtypes) = getattr(H.lib(), n), H.HEADER.prototypes[n]
        assert n in H.EXPORTS and fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and callable(getattr(H, n[3:]))
    # one f32 row of K + 1 sums per workgroup of 256 rows and batch row
    assert H.causal_conv1d_bwd_workspace_bytes(H.BF16, 2, 100, 16, 4) == 2 * 1 * 5 * 16 * 4
    assert H.causal_conv1d_bwd_workspace_bytes(H.F32, 3, 257, 8, 2) == 3 * 2 * 3 * 8 * 4


def test_the_operators_are_public_and_documented():
    for n in ("causal_conv1d", "causal_conv1d_step"):
        assert n in kfunca.__all__ and "state" in getattr(kfunca, n).__doc__
