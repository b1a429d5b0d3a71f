"""CPU-only: the four state entries of linear attention (kf_linear_attn_state_fwd, kf_linear_attn_state_bwd and its workspace query,
kf_linear_attn_step) are exported and typed as the header declares them, and every refusal comes back with its status and the entry's
name before any device call (host buffers stand in for device pointers; no GPU is needed)."""
import ctypes as C

import pytest

from kfunca_amd import hip_abi as H

BUF = (C.c_float * 4096)()
P = C.addressof(BUF) + (-C.addressof(BUF)) % 16
GOOD = dict(dtype=H.BF16, B=1, H=1, S=8, Dk=64, Dv=64, scale=0.125, q=P, k=P, v=P, g=P, d_o=P, o=P, dq=P, dk=P, dv=P, dg=P, ws=P, wsb=1 << 20,
            h0=P, hT=P, d_hT=P, d_h0=P, state=P)
ENTRIES = ("kf_linear_attn_state_fwd", "kf_linear_attn_state_bwd", "kf_linear_attn_state_bwd_workspace_bytes", "kf_linear_attn_step")
REFUSALS = [   # S is T for the step entry
    (dict(q=None), H.KF_ERR_INVALID), (dict(g=None), H.KF_ERR_INVALID), (dict(S=0), H.KF_ERR_INVALID), (dict(S=-3), H.KF_ERR_INVALID),
    (dict(B=-1), H.KF_ERR_INVALID), (dict(scale=0.0), H.KF_ERR_INVALID), (dict(scale=float("nan")), H.KF_ERR_INVALID),
    (dict(k=P + 2), H.KF_ERR_INVALID), (dict(dtype=H.F32), H.KF_ERR_UNSUPPORTED), (dict(dtype=H.F64), H.KF_ERR_UNSUPPORTED),
    (dict(Dv=128), H.KF_ERR_UNSUPPORTED), (dict(Dk=32, Dv=32), H.KF_ERR_UNSUPPORTED), (dict(Dk=256, Dv=256), H.KF_ERR_UNSUPPORTED),
]
STATE_REFUSALS = [   # a misaligned state, d_h0 without h0, a null state where one is needed
    ("kf_linear_attn_state_fwd", dict(h0=P + 4)), ("kf_linear_attn_state_fwd", dict(hT=P + 8)), ("kf_linear_attn_state_bwd", dict(h0=P + 4)),
    ("kf_linear_attn_state_bwd", dict(d_hT=P + 4)), ("kf_linear_attn_state_bwd", dict(d_h0=P + 4)), ("kf_linear_attn_state_bwd", dict(h0=None)),
    ("kf_linear_attn_step", dict(state=None)), ("kf_linear_attn_step", dict(state=P + 4)),
]


def call(entry, a):
    head = (a["dtype"], a["B"], a["H"], a["S"], a["Dk"], a["Dv"])
    if entry == "kf_linear_attn_state_fwd":
        return H.lib().kf_linear_attn_state_fwd(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["h0"], a["o"], a["hT"], None)
    if entry == "kf_linear_attn_state_bwd":
        return H.lib().kf_linear_attn_state_bwd(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["h0"], a["d_o"], a["d_hT"], a["dq"], a["dk"],
                                                a["dv"], a["dg"], a["d_h0"], a["ws"], a["wsb"], None)
    if entry == "kf_linear_attn_step":
        return H.lib().kf_linear_attn_step(*head, a["scale"], a["q"], a["k"], a["v"], a["g"], a["state"], a["o"], None)
    return H.lib().kf_linear_attn_state_bwd_workspace_bytes(*head, C.byref(C.c_size_t(0)))


# (the workspace query takes neither pointers nor a scale)
@pytest.mark.parametrize("entry,change,status", [(e, c, s) for e in ENTRIES for c, s in REFUSALS
                                                 if not (e.endswith("bytes") and set(c) & {"q", "g", "k", "scale"})]
                         + [(e, c, H.KF_ERR_INVALID) for e, c in STATE_REFUSALS])
def test_refusals(entry, change, status):
    assert call(entry, {**GOOD, **change}) == status and entry in H.lib().kf_last_error().decode()


@pytest.mark.parametrize("change", [dict(ws=None), dict(wsb=15), dict(wsb=2 * 8 * 4)])   # the last: the stateless size, one float short
def test_workspace_refusals(change):
    assert call("kf_linear_attn_state_bwd", {**GOOD, **change}) == H.KF_ERR_WORKSPACE and "kf_linear_attn_state_bwd" in H.lib().kf_last_error().decode()
    assert H.lib().kf_linear_attn_state_bwd_workspace_bytes(H.BF16, 1, 1, 8, 64, 64, None) == H.KF_ERR_INVALID


def test_exported_typed_and_sized():
    for n in ENTRIES:
        fn, (restype, argtypes) = getattr(H.lib(), n), H.HEADER.prototypes[n]
        assert n in H.EXPORTS and fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and callable(getattr(H, n[3:]))
    for shape in [(1, 1, 1, 64, 64), (2, 3, 65, 128, 128), (8, 32, 4096, 128, 128)]:
        n, plain = H.linear_attn_state_bwd_workspace_bytes(H.F16, *shape), H.linear_attn_bwd_workspace_bytes(H.F16, *shape)
        assert n % 16 == 0 and n >= plain + shape[0] * shape[1] * 4 - 15
