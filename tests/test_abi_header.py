"""CPU-only: kfunca_amd/_abi_header.py reads include/kfunca_hip.h completely, maps every C type as hip_abi documents, refuses what it
cannot read, and turns a changed parameter type into changed argtypes."""
import ctypes as C
from pathlib import Path

import pytest

from kfunca_amd import _abi_header as A
from kfunca_amd import hip_abi as H

TEXT = (Path(__file__).resolve().parent.parent / "include" / "kfunca_hip.h").read_text()

SMALL = """
#ifndef SMALL_H_
#define SMALL_H_
#define KF_N 3 /* a bound */
enum { KF_A = 0, KF_B = 0x10 };
typedef struct kf_s {
    int32_t a, b;
    const float *p, *q;
    char name[16];
    int64_t m[2][KF_N];
    void *data[KF_N];
    uint64_t big;
} kf_s;
const char *kf_text(void);
size_t kf_bytes(int a, int32_t b, int64_t c, size_t d, uint64_t e, float f, double g);
int kf_ptrs(const kf_s *s, kf_s *t, void *v, void **vv, void *const *vc, const float *f, int64_t *i, const int32_t *j, size_t *z, int *n,
            double *d /* [1] */, const char *text, char *out, char name[64], const char id[KF_N]);
#endif
"""


def test_every_c_type_maps_as_documented():
    h = A.read(SMALL)
    assert h.constants == {"KF_N": 3, "KF_A": 0, "KF_B": 16} and h.exports == ["kf_bytes", "kf_ptrs", "kf_text"]
    S = h.structs["kf_s"]
    assert S._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("p", C.c_void_p), ("q", C.c_void_p), ("name", C.c_char * 16),
                          ("m", (C.c_int64 * 3) * 2), ("data", C.c_void_p * 3), ("big", C.c_uint64)]
    vp = C.c_void_p
    assert h.prototypes == {"kf_text": (C.c_char_p, []),
                            "kf_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int64, C.c_size_t, C.c_uint64, C.c_float, C.c_double]),
                            "kf_ptrs": (C.c_int, [C.POINTER(S), C.POINTER(S), vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_char_p, C.c_char_p,
                                                  C.c_char_p])}


def test_the_real_header_resolves_completely():
    h = H.HEADER
    assert len(h.prototypes) > 100 and len(h.structs) == 7
    allowed = {C.c_int, C.c_int64, C.c_size_t, C.c_uint64, C.c_float, C.c_double, C.c_char_p, C.c_void_p} | {C.POINTER(s) for s in h.structs.values()}
    for name, (restype, argtypes) in h.prototypes.items():
        assert restype in (C.c_int, C.c_size_t, C.c_char_p), name
        assert all(t in allowed for t in argtypes), (name, argtypes)
    assert h.prototypes["kf_gemm_grouped"][1] == [C.c_int, C.c_int, C.POINTER(h.structs["kf_gemm_problem"]), C.c_void_p]
    assert h.prototypes["kf_profile_get"][1] == [C.c_int, C.c_char_p, C.c_void_p, C.c_void_p]


@pytest.mark.parametrize("text, offending", [
    ("int kf_foo(int a, kf_foo_t *x);", "kf_foo_t"),                                     # an unknown type in a prototype
    ("typedef struct kf_s { int32_t a[KF_NOPE]; } kf_s;", "KF_NOPE"),                    # an array bound that is no literal and no #define
    ("int kf_cb(void (*fn)(int), void *stream);", "(*fn)"),                              # a function-pointer parameter
    ("unsigned int kf_u(void);", "unsigned"),
    ("int kf_u(unsigned long n);", "unsigned long n"),
    ("void kf_v(int a);", "void"),                                                       # no entry returns void
    ("typedef struct kf_s { int a; } kf_s;\nint kf_by_value(kf_s s);", "kf_s s"),
    ("typedef struct kf_s { long a; } kf_s;", "long a"),
    ("typedef struct kf_s { struct kf_t *next; } kf_s;", "struct kf_t *next"),
    ("typedef struct kf_s { int a; } kf_t;", "kf_t"),
    ("enum { KF_A, KF_B = 1 };", "KF_A"),                                                # an enumerator without an explicit value
    ("enum kf_e { KF_A = 0 };", "enum kf_e"),
    ("#define KF_N (1 << 4)\n", "(1 << 4)"),
    ("int kf_k();", "kf_k()"),
    ("static inline int kf_i(int a) { return a; }", "return a"),
])
def test_the_reader_refuses_what_it_cannot_read(text, offending):
    with pytest.raises(A.HeaderError) as e:
        A.read(text)
    assert offending in str(e.value), str(e.value)


def test_a_changed_parameter_type_changes_the_argtypes_there_and_only_there():
    was = "int kf_norm_fwd(int kind, int dtype, int64_t rows,"
    assert TEXT.count(was) == 1
    got = A.read(TEXT.replace(was, "int kf_norm_fwd(int kind, int dtype, float rows,")).prototypes
    want = H.HEADER.prototypes
    differ = [(n, i) for n in want for i, (a, b) in enumerate(zip(want[n][1], got[n][1])) if a.__name__ != b.__name__]
    assert differ == [("kf_norm_fwd", 2)] and got["kf_norm_fwd"][1][2] is C.c_float and want["kf_norm_fwd"][1][2] is C.c_int64
    assert got.keys() == want.keys() and all(len(got[n][1]) == len(want[n][1]) and got[n][0] is want[n][0] for n in want)


def test_bind_types_what_a_library_exports_and_nothing_else():
    class Entry:
        pass

    class Subset:   # a variant library: two of the header's entries and one of its own
        kf_attn_fwd, kf_malloc, kfmut_select = Entry(), Entry(), Entry()

    lib = H.bind(Subset())
    assert lib.kf_attn_fwd.argtypes == [C.c_int] + [C.c_int64] * 5 + [C.c_void_p] * 6 and lib.kf_attn_fwd.restype is C.c_int
    assert lib.kf_malloc.argtypes == [C.c_void_p, C.c_size_t]
    assert not hasattr(lib.kfmut_select, "argtypes") and not hasattr(lib, "kf_free")
