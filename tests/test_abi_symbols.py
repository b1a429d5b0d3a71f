"""CPU-only: the C-ABI shared library loads without a GPU and exports every function that
include/kfunca_hip.h declares, each typed as the header declares it; the structs and constants hip_abi derives from the header have the
C compiler's layout and values."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from kfunca_amd import hip_abi as H

ROOT = Path(__file__).resolve().parent.parent


def header_text():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "kfunca_hip.h").read_text(), flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(kf_[a-z0-9_]+)\s*\(", header_text())))


def declared_param_counts():
    """{function: number of parameters}, counted on the header text without the reader."""
    return {n: 0 if p.strip() == "void" else p.count(",") + 1 for n, p in re.findall(r"\b(kf_[a-z0-9_]+)\s*\(([^()]*)\)", header_text())}


def static_assert(exprs):
    """The C compiler checks every expression against the real header at compile time: nothing is written or run."""
    src = "#include <stddef.h>\n#include \"kfunca_hip.h\"\n" + "".join(f'_Static_assert({e}, "{e}");\n' for e in exprs)
    res = subprocess.run(["gcc", "-x", "c", "-std=c11", "-fsyntax-only", f"-I{ROOT / 'include'}", "-"], input=src, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_library_exports_every_declared_symbol():
    lib = H.lib()
    names = declared_functions()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/kfunca_hip.h but not exported"
    assert set(H.HEADER.prototypes) == set(names), "the header reader and the header disagree on the declared functions"
    assert H.EXPORTS == names, "hip_abi.EXPORTS out of sync with the header"
    assert lib.kf_abi_version() == 7 == H.HEADER.constants["KF_ABI_VERSION"]


def test_every_exported_symbol_is_typed_as_the_header_declares():
    # no entry is left at ctypes' defaults (every argument a C int): a 64-bit handle passed to such an entry would be truncated
    lib, counts = H.lib(), declared_param_counts()
    assert sorted(counts) == declared_functions()
    restypes = {"kf_last_error": C.c_char_p, "kf_build_source_sha": C.c_char_p, "kf_index_add_workspace_bytes": C.c_size_t,
                "kf_sort_workspace_bytes": C.c_size_t}
    for n, count in counts.items():
        fn = getattr(lib, n)
        assert fn.argtypes is not None and len(fn.argtypes) == count, (n, fn.argtypes, count)
        assert fn.restype is restypes.get(n, C.c_int), (n, fn.restype)
    assert lib.kf_allreduce_sum_multi.argtypes == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


STRUCTS = {"kf_iter_desc": H.IterDesc, "kf_adamw_tensor": H.AdamwTensor, "kf_gemm_epilogue": H.GemmEpilogue, "kf_gemm_problem": H.GemmProblem,
           "kf_attn_layout": H.AttnLayout, "kf_attn_mask": H.AttnMask, "kf_device_props": H.DeviceProps}
C_SCALAR = {C.c_int: "int", C.c_int64: "int64_t", C.c_uint64: "uint64_t", C.c_float: "float", C.c_char: "char"}


def test_struct_layout_matches_c():
    # size of every struct; offset, size and scalar type of every field; the element count of every array dimension
    assert set(STRUCTS) == set(H.HEADER.structs)
    exprs = []
    for name, cls in STRUCTS.items():
        exprs.append(f"sizeof({name}) == {C.sizeof(cls)}")
        for field, ct in cls._fields_:
            lv = f"(({name} *)0)->{field}"
            exprs += [f"offsetof({name}, {field}) == {getattr(cls, field).offset}", f"sizeof({lv}) == {C.sizeof(ct)}"]
            while issubclass(ct, C.Array):
                exprs.append(f"sizeof({lv}) / sizeof({lv}[0]) == {ct._length_}")
                lv, ct = lv + "[0]", ct._type_
            if ct is C.c_void_p:
                exprs.append(f"sizeof({lv}) == sizeof(void *) && _Generic({lv}, int64_t: 0, uint64_t: 0, double: 0, default: 1)")
            else:
                exprs.append(f"_Generic({lv}, {C_SCALAR[ct]}: 1, default: 0)")
    # what this test asserted before the structs were derived from the header stays asserted, from the classes themselves
    for e in ("sizeof(kf_iter_desc) == 976", "offsetof(kf_iter_desc, dtype) == 16", "offsetof(kf_iter_desc, shape) == 48",
              "offsetof(kf_iter_desc, stride_bytes) == 144", "offsetof(kf_iter_desc, data) == 912", "sizeof(kf_device_props) == 376",
              "offsetof(kf_device_props, total_mem) == 360"):
        assert e in exprs, e
    static_assert(exprs)


def test_constants_match_c():
    # the reader's table against a real compiler, then the names hip_abi publishes against the table
    consts = H.HEADER.constants
    assert {"KF_OK", "KF_F64", "KF_MAX_DIMS", "KF_COMM_ID_BYTES", "KF_MOE_SCORE_SIGMOID", "KF_ABI_VERSION"} <= set(consts)
    assert set(re.findall(r"\bKF_[A-Z0-9_]+\b(?=\s*=)|(?<=#define )KF_[A-Z0-9_]+(?= +\d)", header_text())) == set(consts)
    static_assert(f"{n} == {v}" for n, v in consts.items())
    for n in H.CONSTANTS:
        assert getattr(H, n) == consts[n if n.startswith(("KF_OK", "KF_ERR_")) else "KF_" + n], n
    assert (H.BOOL, H.F64, H.EW_DIV_SCALAR, H.CE_MEAN, H.ACT_GELU_ERF, H.LOG_SOFTMAX, H.ATTN_MASK_DOC, H.KF_ERR_OOM) == (0, 9, 9, 2, 2, 1, 3, 7)
    assert (H.MAX_DIMS, H.MAX_TENSORS, H.COMM_ID_BYTES) == (12, 8, 128)


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
