"""CPU-only: the three kf_linear_attn_* entries are exported and typed as the header declares them, and every refusal comes back with its
status and the entry's name before any device call (host buffers stand in for device pointers; no GPU is needed)."""
import ctypes as C

import pytest

from kfunca_amd import hip_abi as H

BUF = (C.c_float * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 16
GOOD = dict(dtype=H.BF16, B=1, H=1, S=8, Dk=64, Dv=64, scale=0.125, q=P, k=P, v=P, g=P, d_o=P, o=P, dq=P, dk=P, dv=P, dg=P, ws=P, wsb=1 << 20)
REFUSALS = [
    (dict(q=None), H.KF_ERR_INVALID), (dict(g=None), H.KF_ERR_INVALID), (dict(S=0), H.KF_ERR_INVALID), (dict(B=-1), H.KF_ERR_INVALID),
    (dict(scale=0.0), H.KF_ERR_INVALID), (dict(scale=float("inf")), H.KF_ERR_INVALID), (dict(scale=float("nan")), H.KF_ERR_INVALID),
    (dict(k=P + 2), H.KF_ERR_INVALID), (dict(dtype=H.F32), H.KF_ERR_UNSUPPORTED), (dict(dtype=H.F64), H.KF_ERR_UNSUPPORTED),
    (dict(Dv=128), H.KF_ERR_UNSUPPORTED), (dict(Dk=32, Dv=32), H.KF_ERR_UNSUPPORTED), (dict(Dk=256, Dv=256), H.KF_ERR_UNSUPPORTED),
]


def call(entry, a):
    head = (a["dtype"], a["B"], a["H"], a["S"], a["Dk"], a["Dv"])
    if entry == "kf_linear_attn_fwd":
        return H.lib().kf_linear_attn_fwd(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["o"], None)
    if entry == "kf_linear_attn_bwd":
        return H.lib().kf_linear_attn_bwd(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["d_o"], a["dq"], a["dk"], a["dv"], a["dg"], a["ws"],
                                          a["wsb"], None)
    return H.lib().kf_linear_attn_bwd_workspace_bytes(*head, C.byref(C.c_size_t(0)))


# (the workspace query takes neither pointers nor a scale)
@pytest.mark.parametrize("entry,change,status", [(e, c, s) for e in ("kf_linear_attn_fwd", "kf_linear_attn_bwd", "kf_linear_attn_bwd_workspace_bytes")
                                                 for c, s in REFUSALS if not (e.endswith("bytes") and set(c) & {"q", "g", "k", "scale"})])
def test_refusals(entry, change, status):
    assert call(entry, {**GOOD, **change}) == status and entry in H.lib().kf_last_error().decode()


@pytest.mark.parametrize("change", [dict(ws=None), dict(wsb=15)])
def test_workspace_refusals(change):
    assert call("kf_linear_attn_bwd", {**GOOD, **change}) == H.KF_ERR_WORKSPACE and "kf_linear_attn_bwd" in H.lib().kf_last_error().decode()
    assert H.lib().kf_linear_attn_bwd_workspace_bytes(H.BF16, 1, 1, 8, 64, 64, None) == H.KF_ERR_INVALID


def test_exported_typed_and_sized():
    for n in ("kf_linear_attn_fwd", "kf_linear_attn_bwd_workspace_bytes", "kf_linear_attn_bwd"):
        fn, (restype, argtypes) = getattr(H.lib(), n), H.HEADER.prototypes[n]
        assert n in H.EXPORTS and fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and callable(getattr(H, n[3:]))
    for shape in [(1, 1, 1, 64, 64), (2, 3, 65, 128, 128), (8, 32, 4096, 128, 128)]:
        n = H.linear_attn_bwd_workspace_bytes(H.F16, *shape)
        assert n > 0 and n % 16 == 0
