"""CPU-only: the fused AdamW entries of the C ABI (kf_adamw_workspace_bytes, kf_adamw_step) are declared and exported, the ctypes mirror
of kf_adamw_tensor has the C layout, the workspace query follows its documented formula, every invalid argument is refused with
KF_ERR_INVALID and a message before any device call, and a valid call without a device reports an error instead of falling back."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import pytest

from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("kf_adamw_workspace_bytes", "kf_adamw_step")


def test_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)
    for n in ENTRIES:
        assert re.search(rf"\bint {n}\s*\(", text), f"{n} not declared"
        assert hasattr(H.lib(), n) and n in H.EXPORTS
    assert re.search(r"}\s*kf_adamw_tensor;", text)


def test_struct_layout_matches_c():
    want = {"sizeof(kf_adamw_tensor)": C.sizeof(H.AdamwTensor)}
    for name, _ in H.AdamwTensor._fields_:
        want[f"offsetof(kf_adamw_tensor, {name})"] = getattr(H.AdamwTensor, name).offset
    src = "#include <stddef.h>\n#include \"kfunca_hip.h\"\n" + "".join(f'_Static_assert({e} == {v}, "{e} != {v}");\n' for e, v in want.items())
    res = subprocess.run(["gcc", "-x", "c", "-fsyntax-only", f"-I{ROOT / 'include'}", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_workspace_follows_the_formula():
    # max_grad_norm > 0: 256 bytes (the clip coefficient) + 2048 f32 partial sums per launch of 48 tensors; no clipping: nothing
    for n in (0, 1, 47, 48, 49, 200, 300, 1000):
        assert H.adamw_workspace_bytes(n, 1.0) == 256 + 8192 * math.ceil(n / 48), n
        assert H.adamw_workspace_bytes(n, math.inf) == 256 + 8192 * math.ceil(n / 48), n
        assert H.adamw_workspace_bytes(n, 0.0) == 0
        assert H.adamw_workspace_bytes(n, -1.0) == 0
    lib, b = H.lib(), C.c_size_t(7)
    assert lib.kf_adamw_workspace_bytes(4, 1.0, None) == H.KF_ERR_INVALID
    assert lib.kf_adamw_workspace_bytes(-1, 1.0, C.byref(b)) == H.KF_ERR_INVALID and "count" in last_error()
    assert lib.kf_adamw_workspace_bytes(4, math.nan, C.byref(b)) == H.KF_ERR_INVALID and "NaN" in last_error()


def last_error():
    return H.lib().kf_last_error().decode()


class Bufs:
    """Host memory standing in for device pointers: validation must refuse before it dereferences or launches anything."""

    def __init__(self, n=64):
        self.p = (C.c_float * n)()
        self.g = (C.c_float * n)()
        self.ms = (C.c_float * n)()
        self.m = (C.c_float * n)()
        self.v = (C.c_float * n)()
        self.s = (C.c_float * 1)()
        self.lr = (C.c_float * 1)(1e-3)
        self.norm = (C.c_float * 1)()
        self.ws = (C.c_char * 65536)()

    def tensor(self, **kw):
        t = dict(numel=64, param_dtype=H.F32, grad_dtype=H.F32, param=C.addressof(self.p), grad=C.addressof(self.g), master=None,
                 exp_avg=C.addressof(self.m), exp_avg_sq=C.addressof(self.v), step=C.addressof(self.s), weight_decay=0.01)
        t.update(kw)
        return H.AdamwTensor(**t)


def step(b, tensors=None, n=None, b1=0.9, b2=0.999, eps=1e-8, lr="lr", gs=1.0, max_norm=1.0, norm="norm", ws="ws", ws_bytes=65536):
    tensors = [b.tensor()] if tensors is None else tensors
    arr = H.adamw_tensors(tensors)
    p = lambda x: C.addressof(getattr(b, x)) if x else None  # noqa: E731
    return H.lib().kf_adamw_step(arr if tensors else None, len(tensors) if n is None else n, b1, b2, eps, p(lr), gs, max_norm, p(norm), p(ws),
                                 ws_bytes, None)


@pytest.mark.parametrize("kw,what", [
    (dict(n=-1), "count"), (dict(tensors=[], n=3), "null tensors"), (dict(b1=1.0), "beta1"), (dict(b1=-0.1), "beta1"), (dict(b1=math.nan), "beta1"),
    (dict(b2=1.0), "beta2"), (dict(b2=-1e-3), "beta2"), (dict(eps=-1e-8), "eps"), (dict(eps=math.nan), "eps"), (dict(lr=None), "null lr"),
    (dict(gs=math.inf), "grad_scale"), (dict(gs=math.nan), "grad_scale"), (dict(max_norm=math.nan), "NaN"),
    (dict(max_norm=0.0), "grad_norm needs"), (dict(ws=None), "workspace"), (dict(ws_bytes=256 + 8191), "workspace"),
])
def test_step_refuses_invalid_arguments(kw, what):
    rc = step(Bufs(), **kw)
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error(), last_error()


def _tensor_cases():
    b = Bufs()
    a = lambda x: C.addressof(getattr(b, x))  # noqa: E731
    return b, [
        (dict(param_dtype=H.F64), "param dtype"), (dict(param_dtype=H.I32), "param dtype"),
        (dict(grad_dtype=H.BF16), "grad dtype"), (dict(param_dtype=H.BF16, grad_dtype=H.F16), "grad dtype"),
        (dict(numel=-1), "numel"), (dict(numel=1 << 60), "too large"),
        (dict(master=a("ms")), "master"), (dict(weight_decay=-0.01), "weight_decay"), (dict(weight_decay=math.nan), "weight_decay"),
        (dict(param=None), "null param"), (dict(grad=None), "null param"), (dict(exp_avg=None), "null param"), (dict(exp_avg_sq=None), "null param"),
        (dict(step=None), "null step"), (dict(step=None, numel=0), "null step"),
        (dict(param=a("p") + 2), "aligned"), (dict(grad=a("g") + 1), "aligned"), (dict(exp_avg=a("m") + 2), "aligned"),
        (dict(param_dtype=H.BF16, grad_dtype=H.F32, param=a("p") + 1), "aligned"), (dict(param_dtype=H.BF16, master=a("ms") + 2), "aligned"),
        (dict(step=a("s") + 2), "aligned"),
    ]


@pytest.mark.parametrize("case", range(len(_tensor_cases()[1])))
def test_step_refuses_invalid_tensors(case):
    b, cases = _tensor_cases()
    kw, what = cases[case]
    # the bad tensor sits second in the list: the first (valid) one must not have been launched before the check
    rc = step(b, tensors=[b.tensor(), b.tensor(**kw)])
    assert rc == H.KF_ERR_INVALID, (kw, rc)
    assert what in last_error() and "tensor 1" in last_error(), last_error()


def test_empty_tensors_may_have_null_data():
    if H.device_count() > 0:
        return  # (a valid call would run on the device; tests/test_gpu_adamw.py covers it)
    b = Bufs()
    rc = step(b, tensors=[b.tensor(numel=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None)])
    assert rc != H.KF_ERR_INVALID, last_error()


def test_valid_calls_without_a_device_fail_loudly():
    if H.device_count() > 0:
        return  # the device path is covered by tests/test_gpu_adamw.py
    b = Bufs()
    bf = dict(param_dtype=H.BF16, grad_dtype=H.F32, master=C.addressof(b.ms))
    for kw in (dict(), dict(max_norm=0.0, norm=None, ws=None, ws_bytes=0), dict(max_norm=math.inf)):
        for ts in ([b.tensor()], [b.tensor(), b.tensor(**bf)]):
            rc = step(b, tensors=ts, **kw)
            assert rc not in (H.KF_OK, H.KF_ERR_INVALID) and last_error(), (kw, rc, last_error())
