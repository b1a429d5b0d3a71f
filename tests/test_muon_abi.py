"""CPU-only: kf_gemm_sym, kf_muon_prepare_workspace_bytes, kf_muon_prepare and kf_muon_apply are exported and typed as the header
declares them, and a valid call without a device reports an error instead of falling back (host buffers stand in for device pointers)."""
import ctypes as C

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H

ENTRIES = ("kf_gemm_sym", "kf_muon_prepare_workspace_bytes", "kf_muon_prepare", "kf_muon_apply")


def test_exported_and_typed_as_declared():
    for n in ENTRIES:
        assert n in H.EXPORTS and hasattr(H.lib(), n)
        fn, (restype, argtypes) = getattr(H.lib(), n), H.HEADER.prototypes[n]
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes)
        assert callable(getattr(H, n[3:]))
    assert len(H.HEADER.prototypes["kf_gemm_sym"][1]) == 13 and H.HEADER.prototypes["kf_gemm_sym"][1][3] is C.c_float
    assert H.muon_prepare_workspace_bytes(4096, 14336) == 4096
    for n in ("Muon", "gemm_sym", "newton_schulz"):
        assert n in kfunca.__all__ and callable(getattr(kfunca, n))


def test_valid_calls_without_a_device_fail_loudly():
    if H.device_count() > 0:
        return  # the device path is covered by tests/test_gpu_gemm_sym.py and tests/test_gpu_muon.py
    buf = (C.c_float * 8192)()
    base = C.addressof(buf)
    base += (-base) % 16
    x, c, ws, lr = base, base + 8192, base + 16384, base + 24576
    err = lambda: H.lib().kf_last_error().decode()
    assert H.lib().kf_gemm_sym(H.F32, 16, 16, 1.0, x, 16, 0.0, None, 0, 0.0, c, 16, None) not in (H.KF_OK, H.KF_ERR_INVALID) and err()
    assert H.lib().kf_muon_prepare(H.F32, 16, 16, x, None, 0.0, 0, 1.0, c, 16, 16, 16, ws, 4096, None) not in (H.KF_OK, H.KF_ERR_INVALID) and err()
    assert H.lib().kf_muon_apply(H.F32, 16, 16, x, None, c, 16, lr, 0.0, 1.0, None) not in (H.KF_OK, H.KF_ERR_INVALID) and err()
