"""CPU-only: the C-ABI shared library loads without a GPU and exports every function that
include/kfunca_hip.h declares; the ctypes mirror of the descriptor structs has the C layout."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent


def declared_functions():
    text = (ROOT / "include" / "kfunca_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = H.lib()
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/kfunca_hip.h but not exported"
    assert sorted(H.EXPORTS) == names, "hip_abi.EXPORTS out of sync with the header"
    assert lib.kf_abi_version() == 7


def test_struct_layout_matches_c():
    # the C compiler checks every size / offset against the ctypes mirror at compile time: nothing is written or run
    want = {"sizeof(kf_iter_desc)": C.sizeof(H.IterDesc), "offsetof(kf_iter_desc, dtype)": H.IterDesc.dtype.offset,
            "offsetof(kf_iter_desc, shape)": H.IterDesc.shape.offset, "offsetof(kf_iter_desc, stride_bytes)": H.IterDesc.stride_bytes.offset,
            "offsetof(kf_iter_desc, data)": H.IterDesc.data.offset, "sizeof(kf_device_props)": C.sizeof(H.DeviceProps),
            "offsetof(kf_device_props, total_mem)": H.DeviceProps.total_mem.offset}
    src = "#include <stddef.h>\n#include \"kfunca_hip.h\"\n" + "".join(f'_Static_assert({e} == {v}, "{e} != {v}");\n' for e, v in want.items())
    res = subprocess.run(["gcc", "-x", "c", "-fsyntax-only", f"-I{ROOT / 'include'}", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_no_gpu_calls_fail_loudly_not_silently():
    if H.device_count() > 0:
        return
    # without a device every compute entry point reports an error status; nothing falls back to a CPU path
    a = (C.c_float * 4)()
    v = H.View(C.addressof(a), (4,), (1,), H.F32)
    d = H.make_desc([v], [v, v])
    rc = H.lib().kf_elementwise(H.EW_ADD, C.byref(d), H.F32, 0.0, None)
    assert rc != H.KF_OK and H.lib().kf_last_error()


def test_descriptor_builder_matches_reference_rules():
    # make_desc mirrors tensor_iterator.cpp: reversed dims, byte strides, broadcast -> 0, coalescing
    a = H.View(0x1000, (5, 7, 11), (77, 11, 1), H.F32)
    b = H.View(0x2000, (5, 1, 11), (11, 11, 1), H.F32)
    d = H.make_desc([a], [a, b])
    assert d.ndim == 3 and list(d.shape[:3]) == [11, 7, 5]
    assert list(d.stride_bytes[2][:3]) == [4, 0, 44]
    c = H.View(0x3000, (12, 11, 331), (3641, 331, 1), H.F32)
    d = H.make_desc([c], [c, c])
    assert d.ndim == 1 and d.shape[0] == 12 * 11 * 331  # fully coalesced
    out = H.View(0x4000, (1024, 1), (1, 1), H.F32)
    inp = H.View(0x5000, (1024, 1024), (1024, 1), H.F32)
    r = H.make_reduce_desc(out, inp, 1)  # C1 sum(1): dims [1024 (reduced, out stride 0), 1024]  
    assert r.ndim == 2 and list(r.shape[:2]) == [1024, 1024]
    assert list(r.stride_bytes[0][:2]) == [0, 4] and list(r.stride_bytes[1][:2]) == [4, 4096]
