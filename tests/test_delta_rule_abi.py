"""CPU-only: the three entries of the gated delta rule (kf_delta_rule_fwd, its workspace query, kf_delta_rule_step) are exported and typed
as the header declares them, every refusal comes back with its status and the entry's name before any device call (host buffers stand
in for device pointers; no GPU is needed), the workspace has the size the header states, and the two operators are public."""
import ctypes as C

import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

BUF = (C.c_float * 8192)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 16
GOOD = dict(dtype=H.BF16, B=1, H=1, S=8, Dk=64, Dv=64, scale=0.125, q=P, k=P, v=P, g=P, beta=P, h0=P, o=P, hT=P, ws=P, wsb=1 << 20, state=P)
ENTRIES = ("kf_delta_rule_fwd", "kf_delta_rule_fwd_workspace_bytes", "kf_delta_rule_step")
REFUSALS = [   # S is T for the step entry
    (dict(q=None), H.KF_ERR_INVALID), (dict(beta=None), H.KF_ERR_INVALID), (dict(o=None), H.KF_ERR_INVALID), (dict(S=0), H.KF_ERR_INVALID),
    (dict(S=-3), H.KF_ERR_INVALID), (dict(B=-1), H.KF_ERR_INVALID), (dict(scale=0.0), H.KF_ERR_INVALID), (dict(scale=float("nan")), H.KF_ERR_INVALID),
    (dict(k=P + 2), H.KF_ERR_INVALID), (dict(g=P + 4), H.KF_ERR_INVALID), (dict(dtype=H.F32), H.KF_ERR_UNSUPPORTED),
    (dict(dtype=H.F64), H.KF_ERR_UNSUPPORTED), (dict(Dv=128), H.KF_ERR_UNSUPPORTED), (dict(Dk=32, Dv=32), H.KF_ERR_UNSUPPORTED),
    (dict(Dk=256, Dv=256), H.KF_ERR_UNSUPPORTED),
]
OWN_REFUSALS = [   # a misaligned or missing state, a missing, short or misaligned workspace
    ("kf_delta_rule_fwd", dict(h0=P + 4), H.KF_ERR_INVALID), ("kf_delta_rule_fwd", dict(hT=P + 8), H.KF_ERR_INVALID),
    ("kf_delta_rule_step", dict(state=None), H.KF_ERR_INVALID), ("kf_delta_rule_step", dict(state=P + 4), H.KF_ERR_INVALID),
    ("kf_delta_rule_fwd", dict(ws=None), H.KF_ERR_WORKSPACE), ("kf_delta_rule_fwd", dict(wsb=2 * 64 * 64 * 2 - 1), H.KF_ERR_WORKSPACE),
    ("kf_delta_rule_fwd", dict(ws=P + 8), H.KF_ERR_WORKSPACE),
]


def call(entry, a):
    head = (a["dtype"], a["B"], a["H"], a["S"], a["Dk"], a["Dv"])
    if entry == "kf_delta_rule_fwd":
        return H.lib().kf_delta_rule_fwd(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["beta"], a["h0"], a["o"], a["hT"], a["ws"], a["wsb"], None)
    if entry == "kf_delta_rule_step":
        return H.lib().kf_delta_rule_step(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["beta"], a["state"], a["o"], None)
    return H.lib().kf_delta_rule_fwd_workspace_bytes(*head, C.byref(C.c_size_t(0)))


# (the workspace query takes neither pointers nor a scale)
@pytest.mark.parametrize("entry,change,status", [(e, c, s) for e in ENTRIES for c, s in REFUSALS
                                                 if not (e.endswith("bytes") and set(c) & {"q", "beta", "o", "k", "g", "scale"})] + OWN_REFUSALS)
def test_refusals(entry, change, status):
    assert call(entry, {**GOOD, **change}) == status and entry in H.lib().kf_last_error().decode()


def test_exported_typed_and_sized():
    for n in ENTRIES:
        fn, (restype, argtypes) = getattr(H.lib(), n), H.HEADER.prototypes[n]
        assert n in H.EXPORTS and fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and callable(getattr(H, n[3:]))
    assert H.lib().kf_delta_rule_fwd_workspace_bytes(H.BF16, 1, 1, 8, 64, 64, None) == H.KF_ERR_INVALID
    for B, Hh, S, D in [(1, 1, 1, 64), (2, 3, 65, 128), (8, 32, 4096, 128), (1, 2, 64, 64)]:
        assert H.delta_rule_fwd_workspace_bytes(H.F16, B, Hh, S, D, D) == 2 * B * Hh * -(-S // 64) * 64 * D * 2


def test_operators_are_public():
    for n in ("gated_delta_rule", "gated_delta_rule_step"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n)) and "not implemented" in getattr(kfunca, n).__doc__
