"""ctypes binding of the device C ABI (include/kfunca_hip.h -> kfunca_amd/libkfunca_hip.so).

This is the thinnest possible host over the drop-in boundary: the parity tests and bench.py call
the hand-written HIP kernels through it with plain device pointers, exactly as a foreign host
(cgo, JNI, ctypes …) would. There is no fallback of any kind: if the library is missing or a call
fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import os

from . import _abi_header, _build

PKG = Path(__file__).resolve().parent
# KF_HIP_LIB: load another build of the same library (A/B runs of two kernel variants on one box, tools/ only)
LIB_PATH = Path(os.environ["KF_HIP_LIB"]) if os.environ.get("KF_HIP_LIB") else PKG / "libkfunca_hip.so"

HEADER = _abi_header.read((_build.INCLUDE / "kfunca_hip.h").read_text())   # include/kfunca_hip.h is the one statement of the ABI

# The header's enumerators and integer defines under their names here: KF_ dropped, except from the status codes (KF_OK, KF_ERR_*).
# A name the header lacks fails the import. dtype codes == reference ScalarType order (src/core/include/scalar_type.h:9-27)
CONSTANTS = (
    "BOOL", "U8", "I8", "I16", "I32", "I64", "F16", "BF16", "F32", "F64",
    "EW_ADD", "EW_SUB", "EW_MUL", "EW_DIV", "EW_COPY", "EW_FILL", "EW_ADD_SCALAR", "EW_SUB_SCALAR", "EW_MUL_SCALAR", "EW_DIV_SCALAR",
    "RED_SUM", "RED_MEAN",
    "MOM_VAR", "MOM_STD", "MOM_INVSTD",
    "EPI_NONE", "EPI_BIAS_ROW",
    "NORM_RMS", "NORM_LAYER",
    "CE_NONE", "CE_SUM", "CE_MEAN",
    "ACT_SILU", "ACT_GELU_TANH", "ACT_GELU_ERF",
    "SOFTMAX", "LOG_SOFTMAX",
    "ATTN_MASK_FULL", "ATTN_MASK_PREFIX", "ATTN_MASK_WINDOW", "ATTN_MASK_DOC",
    "MOE_SCORE_SOFTMAX", "MOE_SCORE_SIGMOID",
    "FP8_E4M3", "FP8_E5M2",
    "MAX_DIMS", "MAX_TENSORS", "COMM_ID_BYTES",
    "KF_OK", "KF_ERR_HIP", "KF_ERR_INVALID", "KF_ERR_UNSUPPORTED", "KF_ERR_INDEX_RANGE", "KF_ERR_WORKSPACE", "KF_ERR_COMM", "KF_ERR_OOM",
)
for _n in CONSTANTS:
    globals()[_n] = HEADER.constants[_n if _n.startswith(("KF_OK", "KF_ERR_")) else "KF_" + _n]
EXPORTS = HEADER.exports

DTYPE_SIZE = {BOOL: 1, U8: 1, I8: 1, I16: 2, I32: 4, I64: 8, F16: 2, BF16: 2, F32: 4, F64: 8}
NP2CODE = {np.dtype(np.bool_): BOOL, np.dtype(np.uint8): U8, np.dtype(np.int8): I8, np.dtype(np.int16): I16,
           np.dtype(np.int32): I32, np.dtype(np.int64): I64, np.dtype(np.float16): F16,
           np.dtype(np.float32): F32, np.dtype(np.float64): F64}
CODE2NP = {BOOL: np.bool_, U8: np.uint8, I8: np.int8, I16: np.int16, I32: np.int32, I64: np.int64,
           F16: np.float16, BF16: np.uint16, F32: np.float32, F64: np.float64}


class KfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"kfunca_hip status {code}: {msg}")
        self.code = code


class IterDesc(HEADER.structs["kf_iter_desc"]):
    """kf_iter_desc: post-build() TensorIterator state as a POD."""


class AdamwTensor(HEADER.structs["kf_adamw_tensor"]):
    """kf_adamw_tensor: one tensor of a fused AdamW step (param, grad, optional f32 master, f32 exp_avg / exp_avg_sq, f32 step on the device)."""


class GemmEpilogue(HEADER.structs["kf_gemm_epilogue"]):
    """kf_gemm_epilogue: C = (alpha AB + beta C + bias) o mul + add, aux = the value in brackets."""


class GemmProblem(HEADER.structs["kf_gemm_problem"]):
    """kf_gemm_problem: one product of a kf_gemm_grouped call."""


class AttnLayout(HEADER.structs["kf_attn_layout"]):
    """kf_attn_layout: element strides of the batch, head and row dims of one attention operand."""


class AttnMask(HEADER.structs["kf_attn_mask"]):
    """kf_attn_mask: the mask of kf_attn_ext_*. kind is ATTN_MASK_*; a field of another kind keeps its neutral value (None, -1, 0)."""


def attn_mask(kind=ATTN_MASK_FULL, kv_len=None, prefix_len=None, window_left=-1, window_right=-1, doc_start=None, doc_end=None, causal=0) -> AttnMask:
    """An AttnMask with every field the kind does not use at its neutral value (pointers are device addresses or None)."""
    return AttnMask(kind, kv_len, prefix_len, window_left, window_right, doc_start, doc_end, int(causal))


class DeviceProps(HEADER.structs["kf_device_props"]):
    """kf_device_props: what kf_device_props_get reports."""


_lib = None


def build_source_sha() -> str:
    """The device-source hash linked into the loaded library (kf_build_source_sha): compare with kfunca_amd._build.device_src_sha()."""
    l = lib()
    return l.kf_build_source_sha().decode() if hasattr(l, "kf_build_source_sha") else "unstamped"


def bind(cdll):
    """Give every entry of include/kfunca_hip.h that `cdll` exports the restype and argtypes the header declares, and return cdll.
    libkfunca_hip.so exports all of them; a variant build of some device sources (the mutation library of the tests) exports a subset."""
    for name, (restype, argtypes) in HEADER.prototypes.items():
        if hasattr(cdll, name):
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
    return cdll


def lib():
    """Load libkfunca_hip.so; raises if it has not been built (python -m kfunca_amd._build)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m kfunca_amd._build` "
                              "(there is no CPU fallback)")
        loaded = bind(C.CDLL(str(LIB_PATH)))
        # a library that was NOT built from the sources beside it must not pass for them (a failed rebuild leaves the old .so behind):
        # refuse it unless told otherwise (KF_ALLOW_STALE_LIB=1). (A diagnostic variant library under KF_HIP_LIB is linked without the stamp.)
        if hasattr(loaded, "kf_build_source_sha") and (_build.CSRC / "device").exists() and not os.environ.get("KF_ALLOW_STALE_LIB"):
            built, tree = loaded.kf_build_source_sha().decode(), _build.device_src_sha()
            if built != tree:
                raise ImportError(f"{LIB_PATH} was built from device sources {built}, the tree is {tree}: rebuild it (python -m kfunca_amd._build); "
                                  "KF_ALLOW_STALE_LIB=1 loads it anyway")
        _lib = loaded
    return _lib


def check(rc):
    if rc != KF_OK:
        raise KfError(rc, lib().kf_last_error().decode(errors="replace"))


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().kf_device_count(C.byref(n))
    return n.value if rc == KF_OK else 0


def set_device(i: int):
    check(lib().kf_set_device(int(i)))


def device_props(i: int = 0) -> DeviceProps:
    p = DeviceProps()
    check(lib().kf_device_props_get(int(i), C.byref(p)))
    return p


class Stream:
    def __init__(self):
        h = C.c_void_p()
        check(lib().kf_stream_create(C.byref(h)))
        self.handle = h.value

    def sync(self):
        check(lib().kf_stream_sync(self.handle))

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.kf_stream_destroy(self.handle)
            self.handle = None


class Graph:
    """A captured sequence of library calls on one stream (kf_graph_*): `with Graph.capture(stream) as g: ...` then g.launch()."""

    def __init__(self, stream: Stream):
        self.stream, self.handle = stream, None

    @classmethod
    def capture(cls, stream: Stream):
        return cls(stream)

    def __enter__(self):
        check(lib().kf_graph_begin_capture(self.stream.handle))
        return self

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        rc = lib().kf_graph_end_capture(self.stream.handle, C.byref(h))
        if et is None:
            check(rc)
            self.handle = h.value
        return False

    def launch(self, stream: Stream = None):
        check(lib().kf_graph_launch(self.handle, (stream or self.stream).handle))

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.kf_graph_destroy(self.handle)
            self.handle = None


class Event:
    def __init__(self):
        h = C.c_void_p()
        check(lib().kf_event_create(C.byref(h)))
        self.handle = h.value

    def record(self, stream=None):
        check(lib().kf_event_record(self.handle, stream))

    def sync(self):
        check(lib().kf_event_sync(self.handle))

    def elapsed_ms(self, later: "Event") -> float:
        ms = C.c_float(0)
        check(lib().kf_event_elapsed_ms(self.handle, later.handle, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "handle", None) and _lib is not None:
            _lib.kf_event_destroy(self.handle)
            self.handle = None


class DevBuf:
    """A raw device allocation (kf_malloc / kf_free)."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().kf_malloc(C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, arr: np.ndarray) -> "DevBuf":
        arr = np.ascontiguousarray(arr)
        b = cls(arr.nbytes)
        if arr.nbytes:
            check(lib().kf_memcpy_h2d(b.ptr, arr.ctypes.data, arr.nbytes, None))
        return b

    def to_numpy(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        if out.nbytes:
            check(lib().kf_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, None))
        return out

    def zero(self, stream=None):
        check(lib().kf_memset_zero(self.ptr, self.nbytes, stream))

    def free(self):
        if getattr(self, "ptr", None) and _lib is not None:
            _lib.kf_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


class View:
    """A strided typed view of device memory (what the host core's Tensor carries)."""

    def __init__(self, ptr: int, shape, strides_elems, code: int):
        self.ptr, self.shape, self.strides, self.code = int(ptr), tuple(shape), tuple(strides_elems), int(code)

    @classmethod
    def of(cls, buf: DevBuf, arr: np.ndarray, code=None, byte_offset=0):
        """View with the geometry of `arr` (possibly a non-contiguous numpy view of the uploaded base)."""
        code = NP2CODE[arr.dtype] if code is None else code
        return cls(buf.ptr + byte_offset, arr.shape, [s // arr.itemsize for s in arr.strides], code)


def make_desc(outputs, inputs, shape=None, coalesce=True) -> IterDesc:
    """Build a kf_iter_desc the way the reference's TensorIterator::build() leaves it for plain
    loops (tensor_iterator.cpp:486-515), restricted to what a test needs: same-ndim broadcast,
    byte strides, dims reversed to fastest-first, adjacent dims coalesced."""
    ops = list(outputs) + list(inputs)
    nd = len(ops[0].shape)
    if shape is None:
        shape = [max(o.shape[i] for o in ops) for i in range(nd)]
    dims = []
    for i in reversed(range(nd)):
        st = []
        for o in ops:
            es = DTYPE_SIZE[o.code]
            st.append(0 if (o.shape[i] == 1 and shape[i] != 1) else o.strides[i] * es)
        dims.append([shape[i], st])
    if coalesce and len(dims) > 1:
        merged = [dims[0]]
        for sz, st in dims[1:]:
            psz, pst = merged[-1]
            if psz == 1:
                merged[-1] = [sz, st]
            elif sz == 1:
                pass
            elif all(psz * a == b for a, b in zip(pst, st)):
                merged[-1][0] = psz * sz
            else:
                merged.append([sz, st])
        dims = merged
    if not dims:
        dims = [[1, [DTYPE_SIZE[o.code] for o in ops]]]
    d = IterDesc()
    d.ndim, d.ntensors, d.noutputs = len(dims), len(ops), len(outputs)
    for t, o in enumerate(ops):
        d.dtype[t] = o.code
        d.data[t] = o.ptr
    for i, (sz, st) in enumerate(dims):
        d.shape[i] = sz
        for t in range(len(ops)):
            d.stride_bytes[t][i] = st[t]
    return d


def make_reduce_desc(out: View, inp: View, dim: int) -> IterDesc:
    """Descriptor as build_for_reduce leaves it (tensor_iterator.cpp:181-244,523-528): the reduced
    dim gets output stride 0 and moves to the front, the rest are ordered by input stride."""
    nd = len(inp.shape)
    es = DTYPE_SIZE[inp.code]
    dims = []
    for i in range(nd):
        o_st = 0 if i == dim and inp.shape[i] != 1 else out.strides[i] * DTYPE_SIZE[out.code]
        dims.append((inp.shape[i], o_st, inp.strides[i] * es, i == dim and inp.shape[i] != 1))
    red = [x for x in dims if x[3]]
    rest = sorted([x for x in dims if not x[3]], key=lambda x: x[2])
    order = red + rest
    merged = []
    for sz, o_st, i_st, r in order:
        if merged and not r and not merged[-1][3]:
            psz, po, pi, _ = merged[-1]
            if psz * po == o_st and psz * pi == i_st:
                merged[-1] = (psz * sz, po, pi, False)
                continue
            if psz == 1:
                merged[-1] = (sz, o_st, i_st, False)
                continue
            if sz == 1:
                continue
        merged.append((sz, o_st, i_st, r))
    d = IterDesc()
    d.ndim, d.ntensors, d.noutputs = len(merged), 2, 1
    d.dtype[0], d.dtype[1] = out.code, inp.code
    d.data[0], d.data[1] = out.ptr, inp.ptr
    for i, (sz, o_st, i_st, _) in enumerate(merged):
        d.shape[i] = sz
        d.stride_bytes[0][i] = o_st
        d.stride_bytes[1][i] = i_st
    return d


def make_moments_desc(out0: View, out1: View, inp: View, dim: int) -> IterDesc:
    """Two-output form of make_reduce_desc (reduce_ops.cpp:24-25: outputs var, mean, then the input)."""
    d1 = make_reduce_desc(out0, inp, dim)
    d2 = make_reduce_desc(out1, inp, dim)
    d = IterDesc()
    d.ndim, d.ntensors, d.noutputs = d1.ndim, 3, 2
    d.dtype[0], d.dtype[1], d.dtype[2] = out0.code, out1.code, inp.code
    d.data[0], d.data[1], d.data[2] = out0.ptr, out1.ptr, inp.ptr
    for i in range(d1.ndim):
        d.shape[i] = d1.shape[i]
        d.stride_bytes[0][i] = d1.stride_bytes[0][i]
        d.stride_bytes[1][i] = d2.stride_bytes[0][i]
        d.stride_bytes[2][i] = d1.stride_bytes[1][i]
    return d


def reduce_moments(mode, desc: IterDesc, correction=1.0, eps=0.0, stream=None):
    need = C.c_size_t(0)
    check(lib().kf_reduce_moments_workspace_bytes(C.byref(desc), C.byref(need)))
    ws = DevBuf(need.value) if need.value else None
    check(lib().kf_reduce_moments(int(mode), C.byref(desc), float(correction), float(eps), ws.ptr if ws else None, need.value, stream))
    return ws  # keep alive until the stream is synchronised


def elementwise(op, desc: IterDesc, compute_dtype=0, scalar=0.0, stream=None):
    check(lib().kf_elementwise(int(op), C.byref(desc), int(compute_dtype), float(scalar), stream))


def reduce(op, desc: IterDesc, stream=None):
    need = C.c_size_t(0)
    check(lib().kf_reduce_workspace_bytes(C.byref(desc), C.byref(need)))
    ws = DevBuf(need.value) if need.value else None
    check(lib().kf_reduce(int(op), C.byref(desc), ws.ptr if ws else None, need.value, stream))
    return ws  # keep alive until the stream is synchronised


def norm_fwd(kind, dtype, rows, cols, x, weight, bias, eps, y, mean=None, rstd=None, ld=None, stream=None):
    check(lib().kf_norm_fwd(kind, dtype, rows, cols, cols if ld is None else ld, x, weight, bias, float(eps), y, mean, rstd, stream))


def norm_bwd(kind, dtype, rows, cols, x, weight, mean, rstd, dy, dx, dweight, dbias, ld=None, stream=None):
    ld = cols if ld is None else ld
    need = C.c_size_t(0)
    check(lib().kf_norm_bwd_workspace_bytes(kind, dtype, rows, cols, ld, C.byref(need)))
    ws = DevBuf(need.value) if need.value else None
    check(lib().kf_norm_bwd(kind, dtype, rows, cols, ld, x, weight, mean, rstd, dy, dx, dweight, dbias, ws.ptr if ws else None, need.value, stream))
    return ws  # keep alive until the stream is synchronised


def ce_workspace_bytes(dtype, rows, V, reduction):
    need = C.c_size_t(0)
    check(lib().kf_cross_entropy_workspace_bytes(dtype, rows, V, reduction, C.byref(need)))
    return need.value


def ce_fwd(dtype, rows, V, logits, target, loss, lse=None, count=None, ignore_index=-100, label_smoothing=0.0, reduction=CE_MEAN, ld=None,
           stream=None):
    """Softmax cross-entropy forward (kf_cross_entropy_fwd) with scratch of its own; returns the scratch (keep it until the stream is synchronised)."""
    need = ce_workspace_bytes(dtype, rows, V, reduction)
    ws = DevBuf(need) if need else None
    check(lib().kf_cross_entropy_fwd(dtype, rows, V, V if ld is None else ld, logits, target, ignore_index, float(label_smoothing), reduction, loss,
                                     lse, count, ws.ptr if ws else None, need, stream))
    return ws


def ce_bwd(dtype, rows, V, logits, target, lse, count, grad, dlogits, ignore_index=-100, label_smoothing=0.0, reduction=CE_MEAN, ld=None,
           ldd=None, stream=None):
    ld = V if ld is None else ld
    check(lib().kf_cross_entropy_bwd(dtype, rows, V, ld, logits, target, ignore_index, float(label_smoothing), reduction, lse, count, grad,
                                     dlogits, ld if ldd is None else ldd, stream))


def ce_fused_rows_workspace_bytes(rows, V):
    need = C.c_size_t(0)
    check(lib().kf_ce_fused_rows_workspace_bytes(rows, V, C.byref(need)))
    return need.value


def ce_fused_rows(in_dtype, out_dtype, rows, V, logits, target, rowloss, lse=None, dlogits=None, ignore_index=-100, label_smoothing=0.0,
                  z_loss=0.0, ld=None, ldd=None, stream=None):
    """Loss and UNSCALED gradient of a block of logits in one call (kf_ce_fused_rows) with scratch of its own; dlogits None: the loss only.
    Returns the scratch (keep it until the stream is synchronised)."""
    need = ce_fused_rows_workspace_bytes(rows, V)
    ws = DevBuf(need) if need else None
    check(lib().kf_ce_fused_rows(in_dtype, out_dtype, rows, V, V if ld is None else ld, logits, target, ignore_index, float(label_smoothing),
                                 float(z_loss), rowloss, lse, dlogits, V if ldd is None else ldd, ws.ptr if ws else None, need, stream))
    return ws


def ce_fused_reduce(rowloss, target, rows, loss, count=None, ignore_index=-100, mean=True, stream=None):
    """The sum (mean: over the rows not ignored) of a chunked loss's row losses, and the count of those rows (kf_ce_fused_reduce)."""
    check(lib().kf_ce_fused_reduce(rowloss, target, rows, ignore_index, int(bool(mean)), loss, count, stream))


def scale_cast(in_dtype, out_dtype, n, src, dst, g, count=None, stream=None):
    """dst[i] = (out_dtype)(src[i] * g[0] / count[0]) with device scalars g and count (kf_scale_cast); count None: no divisor."""
    check(lib().kf_scale_cast(in_dtype, out_dtype, n, src, dst, g, count, stream))


def adamw_workspace_bytes(n, max_grad_norm=0.0):
    need = C.c_size_t(0)
    check(lib().kf_adamw_workspace_bytes(n, float(max_grad_norm), C.byref(need)))
    return need.value


def adamw_tensors(tensors):
    """A kf_adamw_tensor array from AdamwTensor structs or dicts of its fields."""
    arr = (AdamwTensor * max(len(tensors), 1))()
    for i, t in enumerate(tensors):
        arr[i] = t if isinstance(t, AdamwTensor) else AdamwTensor(**t)
    return arr


def adamw_step(tensors, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, max_grad_norm=0.0, grad_norm=None, workspace=None,
               workspace_bytes=None, stream=None):
    """One fused AdamW step (kf_adamw_step) over `tensors` (AdamwTensor structs or dicts); lr: a device f32 [1]. Without a workspace, one of
    the queried size is made here and returned (keep it until the stream is synchronised)."""
    arr = adamw_tensors(tensors)
    ws = None
    if workspace is None:
        need = adamw_workspace_bytes(len(tensors), max_grad_norm)
        ws = DevBuf(need) if need else None
        workspace, workspace_bytes = (ws.ptr if ws else None), need
    check(lib().kf_adamw_step(arr, len(tensors), beta1, beta2, eps, lr, grad_scale, max_grad_norm, grad_norm, workspace,
                              workspace_bytes or 0, stream))
    return ws


def index_put(desc: IterDesc, sizes, strides_bytes, stream=None):
    n = len(sizes)
    a = (C.c_int64 * n)(*sizes)
    b = (C.c_int64 * n)(*strides_bytes)
    check(lib().kf_index_put(C.byref(desc), n, a, b, stream))


def index_get(table, nrows, row_bytes, idx, n, out, stream=None):
    check(lib().kf_index_get(table, nrows, row_bytes, idx, n, out, stream))


def index_add(dtype, idx, n, src, cols, nrows, dst, stream=None):
    need = lib().kf_index_add_workspace_bytes(n)
    ws = DevBuf(need) if need else None
    check(lib().kf_index_add(dtype, idx, n, src, cols, nrows, dst, ws.ptr if ws else None, need, stream))
    return ws  # keep alive until the stream is synchronised


def sort_segments(keys: np.ndarray, descending=False, code=None, stream=None):
    """keys [nseg, n] (host) -> (sorted keys, int64 positions) through kf_sort; code overrides the dtype (BF16 as uint16)."""
    keys = np.ascontiguousarray(keys)
    nseg, n = keys.shape
    code = NP2CODE[keys.dtype] if code is None else code
    if keys.size == 0:
        check(lib().kf_sort(code, None, None, None, nseg, n, int(descending), None, 0, stream))
        return keys.copy(), np.zeros(keys.shape, np.int64)
    src = DevBuf.from_numpy(keys)
    dst, pos = DevBuf(keys.nbytes), DevBuf(keys.size * 8)
    need = lib().kf_sort_workspace_bytes(code, nseg, n)
    ws = DevBuf(need) if need else None
    check(lib().kf_sort(code, src.ptr, dst.ptr, pos.ptr, nseg, n, int(descending), ws.ptr if ws else None, need, stream))
    device_sync()
    return dst.to_numpy(keys.shape, keys.dtype), pos.to_numpy(keys.shape, np.int64)


def gemm_workspace_bytes(dtype, trans_a, trans_b, M, N, K) -> int:
    need = C.c_size_t(0)
    check(lib().kf_gemm_workspace_bytes(dtype, int(trans_a), int(trans_b), M, N, K, C.byref(need)))
    return need.value


def gemm(dtype, trans_a, trans_b, M, N, K, alpha, A, lda, B, ldb, beta, Cptr, ldc, epilogue=EPI_NONE, bias=None,
         workspace=None, workspace_bytes=0, stream=None):
    check(lib().kf_gemm(dtype, int(trans_a), int(trans_b), M, N, K, alpha, A, lda, B, ldb, beta, Cptr, ldc,
                        epilogue, bias, workspace, workspace_bytes, stream))


def gemm_ex(dtype, trans_a, trans_b, M, N, K, alpha, A, lda, B, ldb, beta, Cptr, ldc, bias=None, mul=None, ldmul=0, add=None, ldadd=0,
            aux=None, ldaux=0, stream=None, c_f32=False):
    e = GemmEpilogue(bias, mul, ldmul, add, ldadd, aux, ldaux, int(c_f32))
    check(lib().kf_gemm_ex(dtype, int(trans_a), int(trans_b), M, N, K, alpha, A, lda, B, ldb, beta, Cptr, ldc, C.byref(e), stream))


def gemm_grouped(dtype, problems, stream=None):
    """problems: tuples (trans_a, trans_b, M, N, K, alpha, beta, A, lda, B, ldb, C, ldc[, c_f32])."""
    arr = (GemmProblem * len(problems))(*[GemmProblem(*p) for p in problems])
    check(lib().kf_gemm_grouped(dtype, len(problems), arr, stream))


def attn_fwd(dtype, B, H, Sq, Skv, D, q, k, v, o, lse=None, stream=None):
    check(lib().kf_attn_fwd(dtype, B, H, Sq, Skv, D, q, k, v, o, lse, stream))


def attn_bwd_workspace_bytes(dtype, B, H, Sq, Skv, D) -> int:
    need = C.c_size_t(0)
    check(lib().kf_attn_bwd_workspace_bytes(dtype, B, H, Sq, Skv, D, C.byref(need)))
    return need.value


def attn_bwd(dtype, B, H, Sq, Skv, D, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, stream=None):
    check(lib().kf_attn_bwd(dtype, B, H, Sq, Skv, D, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes,
                            stream))


def attn_fwd_strided(dtype, B, H, Sq, Skv, D, scale, q, lq, k, lk, v, lv, o, lo, lse=None, stream=None):
    """lq.. are (batch, head, row) element-stride triples."""
    L = [AttnLayout(*t) for t in (lq, lk, lv, lo)]
    check(lib().kf_attn_fwd_strided(dtype, B, H, Sq, Skv, D, scale, q, C.byref(L[0]), k, C.byref(L[1]), v, C.byref(L[2]), o, C.byref(L[3]), lse, stream))


def attn_bwd_strided(dtype, B, H, Sq, Skv, D, scale, q, lq, k, lk, v, lv, o, lo, lse, d_o, ldo, dq, ldq, dk, ldk, dv, ldv, workspace,
                     workspace_bytes, stream=None):
    L = [AttnLayout(*t) for t in (lq, lk, lv, lo, ldo, ldq, ldk, ldv)]
    check(lib().kf_attn_bwd_strided(dtype, B, H, Sq, Skv, D, scale, q, C.byref(L[0]), k, C.byref(L[1]), v, C.byref(L[2]), o, C.byref(L[3]), lse,
                                    d_o, C.byref(L[4]), dq, C.byref(L[5]), dk, C.byref(L[6]), dv, C.byref(L[7]), workspace, workspace_bytes, stream))


def _gqa_layouts(lays, n):
    """None, or n (batch, head, row) element-stride triples -> n kf_attn_layout pointers (NULL for None, for every operand)"""
    if lays is None:
        return [None] * n
    return [None if t is None else C.byref(AttnLayout(*t)) for t in lays]


def attn_fwd_gqa(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse=None, layouts=None, stream=None):
    """Grouped-query attention forward (kf_attn_fwd_gqa). layouts: None (contiguous tensors) or (lq, lk, lv, lo) stride triples."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_fwd_gqa(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, L[0], k, L[1], v, L[2], o, L[3], lse, stream))


def attn_bwd_gqa_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D):
    """(recommended, minimum) bytes of the GQA backward's workspace."""
    rec, mn = C.c_size_t(0), C.c_size_t(0)
    check(lib().kf_attn_bwd_gqa_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D, C.byref(rec), C.byref(mn)))
    return rec.value, mn.value


def attn_bwd_gqa(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, layouts=None, stream=None):
    """Grouped-query attention backward (kf_attn_bwd_gqa). layouts: None or (lq, lk, lv, lo, ldo, ldq, ldk, ldv) stride triples."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_bwd_gqa(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, L[0], k, L[1], v, L[2], o, L[3], lse, d_o, L[4], dq, L[5], dk, L[6],
                                dv, L[7], workspace, workspace_bytes, stream))


def attn_full_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse=None, kv_len=None, layouts=None, stream=None):
    """Full (non-causal) attention forward (kf_attn_full_fwd). kv_len: device pointer to int64 [B] key lengths, or None (every key);
    layouts: None (contiguous tensors) or (lq, lk, lv, lo) stride triples."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_full_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, q, L[0], k, L[1], v, L[2], o, L[3], lse, stream))


def attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D) -> int:
    need = C.c_size_t(0)
    check(lib().kf_attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D, C.byref(need)))
    return need.value


def attn_full_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, kv_len=None, layouts=None,
                  stream=None):
    """Full attention backward (kf_attn_full_bwd). layouts: None or (lq, lk, lv, lo, ldo, ldq, ldk, ldv) stride triples."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_full_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, q, L[0], k, L[1], v, L[2], o, L[3], lse, d_o, L[4], dq, L[5],
                                 dk, L[6], dv, L[7], workspace, workspace_bytes, stream))


def attn_prefix_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse=None, kv_len=None, prefix_len=None, layouts=None, stream=None):
    """Prefix-LM attention forward (kf_attn_prefix_fwd): query m sees key n iff n < kv_len[b] and (n < prefix_len[b] or n <= m).
    kv_len, prefix_len: device pointers to int64 [B], or None (every key / no prefix: causal); layouts as attn_full_fwd."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_prefix_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, prefix_len, q, L[0], k, L[1], v, L[2], o, L[3], lse, stream))


def attn_prefix_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, kv_len=None, prefix_len=None,
                    layouts=None, stream=None):
    """Prefix-LM attention backward (kf_attn_prefix_bwd). The workspace is attn_full_bwd_workspace_bytes'; layouts as attn_full_bwd."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_prefix_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, prefix_len, q, L[0], k, L[1], v, L[2], o, L[3], lse, d_o, L[4], dq,
                                   L[5], dk, L[6], dv, L[7], workspace, workspace_bytes, stream))


def attn_window_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse=None, kv_len=None, window_left=-1, window_right=-1, layouts=None,
                    stream=None):
    """Sliding-window attention forward (kf_attn_window_fwd): query m sees key n iff n < kv_len[b], n >= m - window_left and
    n <= m + window_right; a side of -1 is unbounded. kv_len: device pointer to int64 [B], or None; layouts as attn_full_fwd."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_window_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, window_left, window_right, q, L[0], k, L[1], v, L[2], o, L[3], lse,
                                   stream))


def attn_window_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, kv_len=None, window_left=-1,
                    window_right=-1, layouts=None, stream=None):
    """Sliding-window attention backward (kf_attn_window_bwd). The workspace is attn_full_bwd_workspace_bytes'; layouts as attn_full_bwd."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_window_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, kv_len, window_left, window_right, q, L[0], k, L[1], v, L[2], o, L[3], lse,
                                   d_o, L[4], dq, L[5], dk, L[6], dv, L[7], workspace, workspace_bytes, stream))


def attn_doc_table(B, S, n_docs, cu_doclens, kv_len, doc_start, doc_end, stream=None):
    """The per-token tables of document-masked attention (kf_attn_doc_table). cu_doclens: device pointer to int64 [B, n_docs + 1], the
    cumulative document lengths of each row; written: kv_len int64 [B], doc_start and doc_end int32 [B, S] (device pointers)."""
    check(lib().kf_attn_doc_table(B, S, n_docs, cu_doclens, kv_len, doc_start, doc_end, stream))


def attn_doc_fwd(dtype, B, Hq, Hkv, S, D, scale, q, k, v, o, lse=None, kv_len=None, doc_start=None, doc_end=None, causal=False, layouts=None,
                 stream=None):
    """Document-masked attention forward (kf_attn_doc_fwd) of a packed row, Sq = Skv = S: query m sees key n iff n < kv_len[b],
    doc_start[b, m] <= n < doc_end[b, m] and (not causal or n <= m). doc_start, doc_end: device pointers to int32 [B, S]
    (attn_doc_table writes them; required); kv_len: device pointer to int64 [B], or None; layouts as attn_full_fwd."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_doc_fwd(dtype, B, Hq, Hkv, S, D, scale, int(causal), kv_len, doc_start, doc_end, q, L[0], k, L[1], v, L[2], o, L[3], lse,
                                stream))


def attn_doc_bwd(dtype, B, Hq, Hkv, S, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, kv_len=None, doc_start=None,
                 doc_end=None, causal=False, layouts=None, stream=None):
    """Document-masked attention backward (kf_attn_doc_bwd). The workspace is attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, S, S, D);
    layouts as attn_full_bwd."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_doc_bwd(dtype, B, Hq, Hkv, S, D, scale, int(causal), kv_len, doc_start, doc_end, q, L[0], k, L[1], v, L[2], o, L[3], lse,
                                d_o, L[4], dq, L[5], dk, L[6], dv, L[7], workspace, workspace_bytes, stream))


def attn_ext_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse=None, mask=None, softcap=0.0, sink=None, layouts=None, stream=None):
    """Masked attention with score modifiers, forward (kf_attn_ext_fwd): s = softcap tanh(scale q.k / softcap) when softcap > 0, and
    exp(sink[h]) joins the softmax denominator when sink (device pointer to f32 [Hq]) is given. mask: an AttnMask (attn_mask(...));
    None passes NULL, which the entry refuses. layouts as attn_full_fwd."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_ext_fwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, None if mask is None else C.byref(mask), softcap, sink, q, L[0], k, L[1], v,
                                L[2], o, L[3], lse, stream))


def attn_ext_bwd_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D) -> int:
    need = C.c_size_t(0)
    check(lib().kf_attn_ext_bwd_workspace_bytes(dtype, B, Hq, Hkv, Sq, Skv, D, C.byref(need)))
    return need.value


def attn_ext_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, mask=None, softcap=0.0,
                 sink=None, dsink=None, layouts=None, stream=None):
    """Masked attention with score modifiers, backward (kf_attn_ext_bwd). dsink: device pointer to f32 [Hq], required exactly when sink
    is given. The workspace is attn_ext_bwd_workspace_bytes'; layouts as attn_full_bwd."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_ext_bwd(dtype, B, Hq, Hkv, Sq, Skv, D, scale, None if mask is None else C.byref(mask), softcap, sink, q, L[0], k, L[1], v,
                                L[2], o, L[3], lse, d_o, L[4], dq, L[5], dk, L[6], dv, L[7], dsink, workspace, workspace_bytes, stream))


def attn_span_table(B, S, n_docs, cu_doclens, kv_len, key_lo, key_hi, query_lo, query_hi, doc_prefix=None, causal=False, window_left=-1,
                    window_right=-1, stream=None):
    """The per-token tables of a document mask with a causal rule, per-document prefixes and a window (kf_attn_span_table). cu_doclens:
    device pointer to int64 [B, n_docs + 1]; doc_prefix: device pointer to int64 [B, n_docs] or None (requires causal); a window side of
    -1 is unbounded. Written: kv_len int64 [B]; key_lo, key_hi (the keys a query sees) and query_lo, query_hi (the queries that see a
    key), int32 [B, S] (device pointers)."""
    check(lib().kf_attn_span_table(B, S, n_docs, cu_doclens, doc_prefix, int(causal), window_left, window_right, kv_len, key_lo, key_hi, query_lo,
                                   query_hi, stream))


def attn_span_fwd(dtype, B, Hq, Hkv, S, D, scale, q, k, v, o, lse=None, kv_len=None, key_lo=None, key_hi=None, softcap=0.0, sink=None, layouts=None,
                  stream=None):
    """Attention forward under the tables of attn_span_table (kf_attn_span_fwd), Sq = Skv = S: query m sees key n iff n < kv_len[b] and
    key_lo[b, m] <= n < key_hi[b, m]. key_lo, key_hi: device pointers to int32 [B, S] (required); softcap and sink as attn_ext_fwd;
    layouts as attn_full_fwd."""
    L = _gqa_layouts(layouts, 4)
    check(lib().kf_attn_span_fwd(dtype, B, Hq, Hkv, S, D, scale, kv_len, key_lo, key_hi, softcap, sink, q, L[0], k, L[1], v, L[2], o, L[3], lse, stream))


def attn_span_bwd(dtype, B, Hq, Hkv, S, D, scale, q, k, v, o, lse, d_o, dq, dk, dv, workspace, workspace_bytes, kv_len=None, key_lo=None, key_hi=None,
                  query_lo=None, query_hi=None, softcap=0.0, sink=None, dsink=None, layouts=None, stream=None):
    """Attention backward under the tables of attn_span_table (kf_attn_span_bwd): dQ reads (key_lo, key_hi), dK/dV read (query_lo,
    query_hi). The workspace is attn_full_bwd_workspace_bytes(dtype, B, Hq, Hkv, S, S, D); dsink as attn_ext_bwd; layouts as attn_full_bwd."""
    L = _gqa_layouts(layouts, 8)
    check(lib().kf_attn_span_bwd(dtype, B, Hq, Hkv, S, D, scale, kv_len, key_lo, key_hi, query_lo, query_hi, softcap, sink, q, L[0], k, L[1], v, L[2],
                                 o, L[3], lse, d_o, L[4], dq, L[5], dk, L[6], dv, L[7], dsink, workspace, workspace_bytes, stream))


def rope(dtype, B, H, S, D, x, lx, y=None, ly=None, cos=None, sin=None, table_rows=None, rotary_dim=None, h_rot=None, positions=None,
         interleaved=False, inverse=False, stream=None):
    """Rotary position embeddings (kf_rope). lx / ly are (batch, head, row) element-stride triples; y = None: in place (y = x, ly = lx).
    rotary_dim defaults to D, h_rot to H; cos / sin are f32 [table_rows, rotary_dim / 2] device tables."""
    R = D if rotary_dim is None else rotary_dim
    if y is None:
        y, ly = x, lx
    Lx, Ly = AttnLayout(*lx), AttnLayout(*(lx if ly is None else ly))
    check(lib().kf_rope(dtype, B, H, S, D, H if h_rot is None else h_rot, R, int(interleaved), int(inverse), cos, sin, table_rows, positions, x,
                        C.byref(Lx), y, C.byref(Ly), stream))


def rope_table(base, rotary_dim, rows, cos, sin, stream=None):
    """kf_rope_table: cos / sin = f32 [rows, rotary_dim / 2] device buffers, cos(p base^(-2i/R)) from f64."""
    check(lib().kf_rope_table(float(base), rotary_dim, rows, cos, sin, stream))


def glu_fwd(act, dtype, rows, F, gate, ldg, up, ldu, h, ldh, stream=None):
    """Gated activation forward (kf_glu_fwd): h = act(gate) * up on [rows, F] operands with leading dimensions in elements; up = None is
    the ungated act(gate). The packed [rows, 2F] projection: gate = x, up = x + F * itemsize, ldg = ldu = 2F."""
    check(lib().kf_glu_fwd(act, dtype, rows, F, gate, ldg, up, ldu, h, ldh, stream))


def glu_bwd(act, dtype, rows, F, gate, ldg, up, ldu, dh, lddh, dgate, lddg, dup=None, lddu=0, stream=None):
    """Gated activation backward (kf_glu_bwd): dup = dh act(gate), dgate = dh up act'(gate), recomputed from gate and up (up = dup = None:
    dgate = dh act'(gate)). dgate may be gate and dup may be up (same leading dimension): the projection is overwritten with its gradient."""
    check(lib().kf_glu_bwd(act, dtype, rows, F, gate, ldg, up, ldu, dh, lddh, dgate, lddg, dup, lddu, stream))


def softmax_fwd(kind, dtype, rows, V, scale, x, ldx, y, ldy, stream=None):
    """Row softmax (kind = SOFTMAX) or log_softmax (LOG_SOFTMAX) of scale * x over the last dimension (kf_softmax_fwd) on [rows, V] operands
    with leading dimensions in elements. y may be x (same leading dimension): in place."""
    check(lib().kf_softmax_fwd(kind, dtype, rows, V, scale, x, ldx, y, ldy, stream))


def softmax_bwd(kind, dtype, rows, V, scale, y, ldy, dy, lddy, dx, lddx, stream=None):
    """The backward of softmax_fwd from its OUTPUT y and dy (kf_softmax_bwd). dx may be dy (same leading dimension)."""
    check(lib().kf_softmax_bwd(kind, dtype, rows, V, scale, y, ldy, dy, lddy, dx, lddx, stream))


def qk_norm_rope_fwd(dtype, B, S, Hq, Hk, Hv, D, x, ldx, y=None, ldy=None, wq=None, wk=None, cos=None, sin=None, table_rows=0, rotary_dim=0,
                     positions=None, interleaved=False, eps=1e-6, stream=None):
    """Per-head RMS norm of the q and k heads of the packed [B*S, (Hq + Hk + Hv) D] projection fused with the rotary embedding
    (kf_qk_norm_rope_fwd): n = x rstd w per head, then kf_rope's rotation over the leading rotary_dim dims, in f32 with one rounding.
    Leading dimensions in elements; y = None: in place (y = x, ldy = ldx). wq / wk = None: weight 1. rotary_dim = 0: the norm alone
    (cos, sin, positions are ignored); otherwise cos / sin are f32 [table_rows, rotary_dim / 2] device tables as for rope."""
    if y is None:
        y, ldy = x, ldx
    check(lib().kf_qk_norm_rope_fwd(dtype, B, S, Hq, Hk, Hv, D, rotary_dim, int(interleaved), float(eps), wq, wk, cos, sin, table_rows, positions,
                                    x, ldx, y, ldx if ldy is None else ldy, stream))


def qk_norm_rope_bwd_workspace_bytes(dtype, B, S, Hq, Hk, Hv, D) -> int:
    """Bytes of f32 scratch kf_qk_norm_rope_bwd needs for dwq / dwk (none is needed without them); it needs no initialisation."""
    need = C.c_size_t(0)
    check(lib().kf_qk_norm_rope_bwd_workspace_bytes(dtype, B, S, Hq, Hk, Hv, D, C.byref(need)))
    return need.value


def qk_norm_rope_bwd(dtype, B, S, Hq, Hk, Hv, D, x, ldx, dy, lddy, dx=None, lddx=None, dwq=None, dwk=None, wq=None, wk=None, cos=None, sin=None,
                     table_rows=0, rotary_dim=0, positions=None, interleaved=False, eps=1e-6, workspace=None, workspace_bytes=None, stream=None):
    """The backward of qk_norm_rope_fwd from its INPUT x and dy (kf_qk_norm_rope_bwd): rstd and xhat are recomputed, nothing else is kept.
    dx = None: dx = dy in place (v heads untouched). dwq / dwk = None: not computed. When one is wanted and no workspace is given, one of
    qk_norm_rope_bwd_workspace_bytes is allocated for the call and returned (keep it until the stream is synchronised)."""
    if dx is None:
        dx, lddx = dy, lddy
    own = None
    if (dwq or dwk) and workspace is None:
        own = DevBuf(max(qk_norm_rope_bwd_workspace_bytes(dtype, B, S, Hq, Hk, Hv, D), 4))
        workspace, workspace_bytes = own.ptr, own.nbytes
    check(lib().kf_qk_norm_rope_bwd(dtype, B, S, Hq, Hk, Hv, D, rotary_dim, int(interleaved), float(eps), wq, wk, cos, sin, table_rows, positions,
                                    x, ldx, dy, lddy, dx, lddy if lddx is None else lddx, dwq, dwk, workspace, workspace_bytes or 0, stream))
    return own  # keep alive until the stream is synchronised


def segment_offsets(sorted_ids, n, E, offsets, stream=None):
    """kf_segment_offsets: offsets[e] = the number of the n ascending int64 ids that are < e, for e = 0 .. E (device pointers)."""
    check(lib().kf_segment_offsets(sorted_ids, n, E, offsets, stream))


def gemm_segmented_workspace_bytes(dtype, T, E) -> int:
    """Bytes of scratch kf_gemm_segmented and kf_gemm_segmented_wgrad need (the sanitised offsets and the row-tile table); 16-byte
    aligned, no initialisation."""
    need = C.c_size_t(0)
    check(lib().kf_gemm_segmented_workspace_bytes(dtype, T, E, C.byref(need)))
    return need.value


def gemm_segmented(dtype, trans_b, T, N, K, E, offsets, alpha, A, lda, W, ldw, w_stride, beta, Cp, ldc, workspace, workspace_bytes, stream=None):
    """kf_gemm_segmented: C[r, :] = alpha A[r, :] op(W_e) + beta C[r, :] for offsets[e] <= r < offsets[e + 1]; W_e = W + e w_stride is
    [K, N] (trans_b = 0) or [N, K] (trans_b = 1). offsets is a device pointer; rows no segment covers get beta C."""
    check(lib().kf_gemm_segmented(dtype, int(trans_b), T, N, K, E, offsets, alpha, A, lda, W, ldw, w_stride, beta, Cp, ldc, workspace, workspace_bytes,
                                  stream))


def gemm_segmented_wgrad(dtype, T, M, N, E, offsets, alpha, A, lda, B, ldb, beta, dW, lddw, dw_stride, workspace, workspace_bytes, stream=None):
    """kf_gemm_segmented_wgrad: dW_e = alpha A[seg_e, :]^T B[seg_e, :] + beta dW_e with A [T, M], B [T, N], dW_e = dW + e dw_stride."""
    check(lib().kf_gemm_segmented_wgrad(dtype, T, M, N, E, offsets, alpha, A, lda, B, ldb, beta, dW, lddw, dw_stride, workspace, workspace_bytes,
                                        stream))


def fp8_amax(dtype, rows, cols, ld, x, amax, stream=None):
    """kf_fp8_amax: *amax (device f32) = max |x| over the row-pitched [rows, cols] matrix; a NaN in x gives NaN; 0 for an empty matrix."""
    check(lib().kf_fp8_amax(dtype, rows, cols, ld, x, amax, stream))


def fp8_quantize(dtype, fmt, rows, cols, ld, x, amax, q, ldq, scale_inv, qt=None, ldqt=0, stream=None):
    """kf_fp8_quantize: q [rows, cols] (and qt [cols, ceil16(rows)], zero-padded, when given) = the FP8 codes of x * 2^e, e the largest
    integer with *amax * 2^e <= the format's maximum; *scale_inv = 2^-e. amax and scale_inv are device pointers."""
    check(lib().kf_fp8_quantize(dtype, fmt, rows, cols, ld, x, amax, q, ldq, qt, ldqt, scale_inv, stream))


def gemm_fp8(fmt_a, fmt_b, out_dtype, M, N, K, A, lda, B, ldb, scale_inv_a, scale_inv_b, Cp, ldc, stream=None):
    """kf_gemm_fp8: C [M, N] (out_dtype) = *scale_inv_a * *scale_inv_b * A [M, K] B [N, K]^T over FP8 bytes, both K-contiguous."""
    check(lib().kf_gemm_fp8(fmt_a, fmt_b, out_dtype, M, N, K, A, lda, B, ldb, scale_inv_a, scale_inv_b, Cp, ldc, stream))


def moe_plan_workspace_bytes(T, k, E) -> int:
    """Bytes of scratch kf_moe_plan needs (the keys, the sorted keys, the positions and the sort's own scratch); 16-byte alignment is
    the caller's."""
    need = C.c_size_t(0)
    check(lib().kf_moe_plan_workspace_bytes(T, k, E, C.byref(need)))
    return need.value


def moe_plan(ids, T, k, E, offsets, row_pair, pair_row, workspace, workspace_bytes, stream=None):
    """kf_moe_plan: the stable sort of the T k (token, choice) pairs by expert id (int64 ids on the device; ids outside [0, E) are dropped
    to the tail): row_pair int32 [T k], its inverse pair_row int32 [T k] and offsets int64 [E + 1] (device pointers)."""
    check(lib().kf_moe_plan(ids, T, k, E, offsets, row_pair, pair_row, workspace, workspace_bytes, stream))


def moe_gate_fwd(dtype, T, k, E, ids, p, ldp, normalize, gate, ldg, stream=None):
    """kf_moe_gate_fwd: gate[t, j] = p[t, ids[t, j]] (0 for a dropped pair), divided by their sum over j when normalize."""
    check(lib().kf_moe_gate_fwd(dtype, T, k, E, ids, p, ldp, int(normalize), gate, ldg, stream))


def moe_gate_bwd(dtype, T, k, E, ids, p, ldp, normalize, gate, ldg, dgate, lddg, dp, lddp, stream=None):
    """kf_moe_gate_bwd: dp [T, E] = zeros with dp[t, ids[t, j]] += ds_j in the order j; every element of dp is written."""
    check(lib().kf_moe_gate_bwd(dtype, T, k, E, ids, p, ldp, int(normalize), gate, ldg, dgate, lddg, dp, lddp, stream))


def moe_dispatch(dtype, T, k, cols, row_pair, x, ldx, xs, ldxs, stream=None):
    """kf_moe_dispatch: xs[r, :] = x[row_pair[r] / k, :] for the T k sorted rows, bit for bit."""
    check(lib().kf_moe_dispatch(dtype, T, k, cols, row_pair, x, ldx, xs, ldxs, stream))


def moe_combine(dtype, T, k, cols, pair_row, n_valid, gate, ldg, ys, ldys, y, ldy, stream=None):
    """kf_moe_combine: y[t, :] = sum_j gate[t, j] ys[pair_row[t, j], :] in f32 in the order j; gate None means 1, n_valid (a device pointer
    to one int64, offsets + E) None means T k."""
    check(lib().kf_moe_combine(dtype, T, k, cols, pair_row, n_valid, gate, ldg, ys, ldys, y, ldy, stream))


def moe_combine_bwd(dtype, T, k, cols, pair_row, n_valid, gate, ldg, ys, ldys, dy, lddy, dys, lddys, dgate=None, lddg=0, stream=None):
    """kf_moe_combine_bwd: dys[pair_row[t, j], :] = gate[t, j] dy[t, :] (+0 for a dropped pair) and dgate[t, j] = dy[t, :] . ys[row, :], in
    one pass; dgate None skips the dot products (ys may then be None)."""
    check(lib().kf_moe_combine_bwd(dtype, T, k, cols, pair_row, n_valid, gate, ldg, ys, ldys, dy, lddy, dys, lddys, dgate, lddg, stream))


def moe_router_fwd(dtype, T, E, k, score, normalize, logits, ldl, ids, gate, ldg, stream=None):
    """kf_moe_router_fwd: ids [T, k] (int64) = the first k positions of the stable descending order of each row of logits [T, E] in the
    sort's key order, gate [T, k] = softmax(logits)[ids] (score MOE_SCORE_SOFTMAX) or sigmoid(logits[ids]), over their sum when normalize."""
    check(lib().kf_moe_router_fwd(dtype, T, E, k, int(score), int(normalize), logits, ldl, ids, gate, ldg, stream))


def moe_router_bwd(dtype, T, E, k, score, normalize, logits, ldl, ids, dgate, lddg, dlogits, lddl, stream=None):
    """kf_moe_router_bwd: dlogits [T, E], every element written, from logits, ids and dgate (the row is recomputed)."""
    check(lib().kf_moe_router_bwd(dtype, T, E, k, int(score), int(normalize), logits, ldl, ids, dgate, lddg, dlogits, lddl, stream))


def moe_aux_loss_workspace_bytes(T, E) -> int:
    """Bytes of scratch kf_moe_aux_loss_fwd needs (one f32 partial row of E + 1 sums per block); 16-byte alignment, no initialisation."""
    need = C.c_size_t(0)
    check(lib().kf_moe_aux_loss_workspace_bytes(T, E, C.byref(need)))
    return need.value


def moe_aux_loss_fwd(dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, loss, parts, workspace, workspace_bytes, stream=None):
    """kf_moe_aux_loss_fwd: loss[0] = balance_coef L_bal + z_coef L_z of softmax(logits) and the plan's offsets; parts (or None) = (L_bal, L_z)."""
    check(lib().kf_moe_aux_loss_fwd(dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, loss, parts, workspace, workspace_bytes, stream))


def moe_aux_loss_bwd(dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, dloss, dlogits, lddl, stream=None):
    """kf_moe_aux_loss_bwd: dlogits [T, E], every element written, in one pass; dloss is one f32 on the device."""
    check(lib().kf_moe_aux_loss_bwd(dtype, T, E, k, logits, ldl, offsets, balance_coef, z_coef, dloss, dlogits, lddl, stream))


def device_sync():
    check(lib().kf_device_sync())


def stream_wait_event(stream, event: "Event"):
    check(lib().kf_stream_wait_event(stream, event.handle))


def knobs_reload():
    """Re-read the KF_* A/B switches from the environment (they are cached per process)."""
    check(lib().kf_knobs_reload())


class knobs:
    """`with knobs(KF_ATTN_NO_XCD="1"): ...` — set A/B switches for the calls inside the block, restore them after."""

    def __init__(self, **env):
        self.env, self.old = env, {}

    def __enter__(self):
        import os
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        knobs_reload()
        return self

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        knobs_reload()
        return False


def profile_enable(on: bool):
    check(lib().kf_profile_enable(int(bool(on))))


def profile_reset():
    check(lib().kf_profile_reset())


def profile_samples() -> dict:
    """{kernel name: float32 array of its launches' durations in ms, in launch order} (synchronises)."""
    n = C.c_int(0)
    check(lib().kf_profile_count(C.byref(n)))
    out = {}
    for i in range(n.value):
        name = C.create_string_buffer(64)
        ms, cnt = C.c_double(0), C.c_int64(0)
        check(lib().kf_profile_get(i, name, C.byref(ms), C.byref(cnt)))
        buf = np.empty(min(cnt.value, 65536), dtype=np.float32)
        w = C.c_int(0)
        check(lib().kf_profile_samples(i, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, C.byref(w)))
        out[name.value.decode()] = buf[:w.value]
    return out


def profile_results() -> dict:
    """{kernel name: (summed ms, launches)} for launches made while profiling was enabled (synchronises)."""
    n = C.c_int(0)
    check(lib().kf_profile_count(C.byref(n)))
    out = {}
    for i in range(n.value):
        name = C.create_string_buffer(64)
        ms, cnt = C.c_double(0), C.c_int64(0)
        check(lib().kf_profile_get(i, name, C.byref(ms), C.byref(cnt)))
        out[name.value.decode()] = (ms.value, cnt.value)
    return out
