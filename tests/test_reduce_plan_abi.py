"""CPU-only: a Python mirror of the reduction planner (make_plan and the kernel choice of run_reduce in reduce.hip), pinned against the
library's own workspace queries, plus the case table tests/test_gpu_reduce_paths.py runs on the GPU.

kf_reduce_workspace_bytes / kf_reduce_moments_workspace_bytes need no device: they return nsplit * nout * acc_bytes (0 when nsplit is
1), so equality pins the mirror's split count. At the edges below it also pins tx * vec (through max_split = R / (tx * vec * 8)), the
vector width of the outer path (through gx = ceil(C / (64 * vec))) and the tall / split choice. Two choices leave the workspace alone:
the four-packs-per-lane rule (it only fires at >= 1024 blocks, where nothing splits) and the few-rows / few-columns kernels (they run
unsplit). The mirror states them; a fingerprint of the mirrored source text makes any edit of the planner fail here until the mirror
has been checked against it again.

Descriptors carry fake, suitably aligned pointers, as tests/test_norm_abi.py does; nothing here touches a device."""
import ctypes as C
import hashlib
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

from kfunca_amd import hip_abi as H

REDUCE_HIP = Path(__file__).resolve().parent.parent / "kfunca_amd" / "csrc" / "device" / "reduce.hip"

KB = 256             # kRB: threads per block
WAVE = 64            # kWave
TARGET_BLOCKS = 1024
TALL_BYTES = 16 << 20
FAKE_IN, FAKE_OUT0, FAKE_OUT1 = 1 << 40, 1 << 41, 1 << 42  # 16-byte (and 4 KiB) aligned

FLOATS = (H.F32, H.F64, H.BF16, H.F16)
NAME = {H.BOOL: "bool", H.U8: "u8", H.I8: "i8", H.I16: "i16", H.I32: "i32", H.I64: "i64", H.F16: "f16", H.BF16: "bf16", H.F32: "f32",
        H.F64: "f64"}


def _pow2_floor(v):
    p = 1
    while p * 2 <= v:
        p *= 2
    return p


def plan_of(d, moments=False):
    """The plan run_reduce executes for descriptor `d`: {kernel, vec, tx, nsplit, tall, R, C, nout, nouter, rtot, ws}. kernel is one of
    inner, inner_few, outer, outer_few, outer_tall, generic, with '+fold' when the reduced extent is split over blocks."""
    inp = 2 if moments else 1
    code = d.dtype[inp]
    es, eso = H.DTYPE_SIZE[code], H.DTYPE_SIZE[d.dtype[0]]
    st = [[d.stride_bytes[t][i] for i in range(d.ndim)] for t in range(d.ntensors)]
    shape = [d.shape[i] for i in range(d.ndim)]
    red, nout, rtot = [], 1, 1
    for i in range(d.ndim):
        if st[0][i] == 0 and shape[i] > 1:
            red.append(i)
            rtot *= shape[i]
        else:
            nout *= shape[i]
    acc = (4 if code in (H.F32, H.F16, H.BF16) else 8) * (3 if moments else 1)
    p = dict(kernel="generic", vec=1, tx=1, nsplit=1, tall=False, R=1, C=1, nout=nout, nouter=1, rtot=rtot)
    in_s0 = st[inp][0]
    if red == [0] and in_s0 == es:
        R = shape[0]
        V = 16 // es
        vec = V if R % V == 0 and d.data[inp] % es == 0 else 1
        per = -(-R // vec)
        tx = KB if per >= KB else _pow2_floor(max(per, 1))
        if tx < per and tx < KB:
            tx *= 2
        if 4 <= tx < KB and (nout * (tx // 4) + KB - 1) // KB >= TARGET_BLOCKS:
            tx //= 4
        gx = -(-nout // (KB // tx))
        ns = 1
        if gx < TARGET_BLOCKS // 2:
            ns = max(1, min(TARGET_BLOCKS // gx, R // (tx * vec * 8), 256))
        few = not moments and vec > 1 and R <= 2 * vec and ns == 1 and nout >= 65536
        p.update(kernel="inner_few" if few else "inner", vec=vec, tx=tx, nsplit=ns, R=R)
    elif red == [0] and d.ndim >= 2 and st[inp][1] == es and st[0][1] == eso and (not moments or st[1][1] == eso):
        R, Cx = shape[0], shape[1]
        nouter = nout // Cx
        V = 16 // es
        ok = Cx % V == 0 and d.data[inp] % 16 == 0 and in_s0 % 16 == 0 and all(st[inp][i] % 16 == 0 for i in range(2, d.ndim))
        vec = V if ok else 1
        gx = -(-Cx // (WAVE * vec))
        gz = min(nouter, 1024)
        ns = 1
        if gx * gz < TARGET_BLOCKS // 2:
            ns = max(1, min(TARGET_BLOCKS // (gx * gz), R // 16, 256))
        tall = ns > 1 and R * Cx * nouter * es <= TALL_BYTES and (Cx + 15) // 16 * nouter >= 32
        if tall:
            ns = 1
        kernel = "outer_tall" if tall else ("outer_few" if not moments and R <= 8 and ns == 1 else "outer")
        p.update(kernel=kernel, vec=vec, nsplit=ns, tall=tall, R=R, C=Cx, nouter=nouter)
    if p["nsplit"] > 1:
        p["kernel"] += "+fold"
    p["ws"] = p["nsplit"] * nout * acc if p["nsplit"] > 1 else 0
    return p


def packed(p):
    """Whether the kernel that runs loads 16-byte packs (the tall and generic kernels have one form only: None)."""
    k = p["kernel"].split("+")[0]
    return None if k in ("outer_tall", "generic") else p["vec"] > 1


# ---- descriptors ---------------------------------------------------------------------------------------------------------------
def contiguous_strides(shape, pad=0):
    """Row-major element strides with `pad` spare elements after each innermost row (row stride = shape[-1] + pad)."""
    st, acc = [], 1
    for i, n in enumerate(reversed(shape)):
        st.append(acc)
        acc *= n + (pad if i == 0 else 0)
    return tuple(reversed(st))


def multi_reduce_desc(out, inp, dims, moments_out1=None):
    """make_reduce_desc for any set of reduced dims (what a caller of the C ABI may pass; the operator API reduces one dim): reduced dims
    first with output stride 0, the rest ordered by input stride and merged where they walk memory as one."""
    dims = [i for i in dims if inp.shape[i] != 1]
    nd = len(inp.shape)
    es = H.DTYPE_SIZE[inp.code]
    outs = [out] + ([moments_out1] if moments_out1 is not None else [])
    rows = []
    for i in range(nd):
        o_st = tuple(0 if i in dims else v.strides[i] * H.DTYPE_SIZE[v.code] for v in outs)
        rows.append((inp.shape[i], o_st, inp.strides[i] * es, i in dims))
    order = [x for x in rows if x[3]] + sorted([x for x in rows if not x[3]], key=lambda x: x[2])
    merged = []
    for sz, o_st, i_st, r in order:
        if merged and not r and not merged[-1][3]:
            psz, po, pi, _ = merged[-1]
            if all(psz * a == b for a, b in zip(po, o_st)) and psz * pi == i_st:
                merged[-1] = (psz * sz, po, pi, False)
                continue
            if psz == 1:
                merged[-1] = (sz, o_st, i_st, False)
                continue
            if sz == 1:
                continue
        merged.append((sz, o_st, i_st, r))
    d = H.IterDesc()
    no = len(outs)
    d.ndim, d.ntensors, d.noutputs = len(merged), no + 1, no
    for t, v in enumerate(outs + [inp]):
        d.dtype[t], d.data[t] = v.code, v.ptr
    for i, (sz, o_st, i_st, _) in enumerate(merged):
        d.shape[i] = sz
        for t in range(no):
            d.stride_bytes[t][i] = o_st[t]
        d.stride_bytes[no][i] = i_st
    return d


# ---- the case table tests/test_gpu_reduce_paths.py runs -------------------------------------------------------------------------
class Case:
    """One reduction the GPU tests run. The input is `shape` with element `strides` (default: row-major, `pad` spare elements after
    each innermost row) starting `offset` elements into its buffer; `dims` are reduced. `op` is 'sum' (sum and mean) or 'mom'
    (the moments, with outputs of `out_code`, default the input's dtype). `kernel` / `packed` is what the planner must choose."""

    def __init__(self, op, code, shape, dims, kernel, packed, pad=0, offset=0, strides=None, out_code=None, note=""):
        self.op, self.code, self.shape = op, code, tuple(shape)
        self.dims = (dims,) if isinstance(dims, int) else tuple(dims)
        self.kernel, self.packed = kernel, packed
        self.strides = tuple(strides) if strides is not None else contiguous_strides(self.shape, pad)
        self.offset = offset
        self.out_code = code if out_code is None else out_code
        self.note = note

    @property
    def id(self):
        oc = "" if self.out_code == self.code else f"->{NAME[self.out_code]}"
        extra = (f"-st{'x'.join(map(str, self.strides))}" if self.strides != contiguous_strides(self.shape) else "") + \
                (f"-off{self.offset}" if self.offset else "")
        return f"{self.op}-{NAME[self.code]}{oc}-{'x'.join(map(str, self.shape))}-d{''.join(map(str, self.dims))}{extra}-{self.kernel}"

    @property
    def nelem_base(self):
        """Elements of the buffer the input lives in."""
        return self.offset + 1 + sum((n - 1) * s for n, s in zip(self.shape, self.strides))

    @property
    def out_shape(self):
        return tuple(1 if i in self.dims else n for i, n in enumerate(self.shape))

    def views(self, in_ptr, out_ptrs):
        """(input view, output views) over the given base pointers; outputs are contiguous keepdim tensors."""
        es = H.DTYPE_SIZE[self.code]
        inp = H.View(in_ptr + self.offset * es, self.shape, self.strides, self.code)
        outs = [H.View(p, self.out_shape, contiguous_strides(self.out_shape), self.out_code) for p in out_ptrs]
        return inp, outs

    def desc(self, in_ptr, out_ptrs):
        inp, outs = self.views(in_ptr, out_ptrs)
        if self.op == "mom":
            return multi_reduce_desc(outs[0], inp, self.dims, moments_out1=outs[1])
        return multi_reduce_desc(outs[0], inp, self.dims)

    def plan(self, in_ptr=FAKE_IN, out_ptrs=(FAKE_OUT0, FAKE_OUT1)):
        return plan_of(self.desc(in_ptr, out_ptrs[:2 if self.op == "mom" else 1]), moments=self.op == "mom")


def _sum_cases(c):
    """Every sum kernel the planner can produce for dtype `c`, packed and scalar, plus the geometry edges of the issue."""
    V = 16 // H.DTYPE_SIZE[c]
    return [
        Case("sum", c, (300, 24 * V), 1, "inner", True),
        Case("sum", c, (300, 24 * V + 1), 1, "inner", False),
        Case("sum", c, (301, 24 * V), 1, "inner", True, pad=1, note="row stride R + 1: rows start off a 16-byte boundary"),
        Case("sum", c, (3, 32 * 256 * V), 1, "inner+fold", True),
        Case("sum", c, (3, 32 * 256 * V + 3), 1, "inner+fold", False),
        Case("sum", c, (2, 32 * 256 * V), 1, "inner+fold", True, offset=1, note="base one element off: packs at element alignment"),
        Case("sum", c, (65536, V), 1, "inner_few", True),
        Case("sum", c, (65536 + 300, 2 * V), 1, "inner_few", True),
        Case("sum", c, (65535, 2 * V), 1, "inner", True, note="one row short of the few-packs kernel"),
        Case("sum", c, (65536, 3 * V), 1, "inner", True, note="three packs: past the few-packs kernel"),
        Case("sum", c, (20, 64 * V * 4), 0, "outer", True),
        Case("sum", c, (1100, 12, 64 * V), 1, "outer", True, note="nouter > 1024: the blockIdx.z loop runs twice"),
        Case("sum", c, (20, 64 * V * 4 - 1), 0, "outer", False, note="C % vec != 0"),
        Case("sum", c, (20, 64 * V * 4), 0, "outer", False, offset=1, note="base one element off 16 bytes"),
        Case("sum", c, (20, 64 * V * 4), 0, "outer", False, pad=1, note="row stride not a multiple of 16 bytes"),
        Case("sum", c, (4, 12, 64 * V), 1, "outer", False, strides=(12 * 64 * V + 1, 64 * V, 1), note="dim-2 stride off 16 bytes"),
        Case("sum", c, (4096, 256), 0, "outer+fold", True),
        Case("sum", c, (4096, 255), 0, "outer+fold", False),
        Case("sum", c, (3, 4096, 96), 1, "outer+fold", True, note="outer-layout fold over three outer outputs: o = z * C + c"),
        Case("sum", c, (8, 64 * V * 4), 0, "outer_few", True),
        Case("sum", c, (2, 64 * V * 4), 0, "outer_few", True),
        Case("sum", c, (5, 64 * V * 4 - 1), 0, "outer_few", False),
        Case("sum", c, (1100, 8, 64 * V), 1, "outer_few", True, note="nouter > 1024"),
        Case("sum", c, (9, 64 * V * 4), 0, "outer", True, note="one row past the few-rows kernel"),
        Case("sum", c, (1000, 1024), 0, "outer_tall", None, note="64 blocks: the XCD remap"),
        Case("sum", c, (1000, 1000), 0, "outer_tall", None, note="63 blocks: no remap"),
        Case("sum", c, (2, 700, 250), 1, "outer_tall", None, note="nouter 2, 16 blocks"),
        Case("sum", c, (20, 24, 36), (0, 2), "generic", None, note="two reduced dims"),
        Case("sum", c, (36, 20, 24), 1, "generic", None, strides=(1, 36 * 24, 36), note="permuted: reduced dim neither contiguous nor dim 0"),
    ]


def _mom_cases(c, oc=None):
    V = 16 // H.DTYPE_SIZE[c]
    return [
        Case("mom", c, (300, 24 * V), 1, "inner", True, out_code=oc),
        Case("mom", c, (300, 24 * V + 1), 1, "inner", False, out_code=oc),
        Case("mom", c, (3, 32 * 256 * V), 1, "inner+fold", True, out_code=oc),
        Case("mom", c, (3, 32 * 256 * V + 3), 1, "inner+fold", False, out_code=oc),
        Case("mom", c, (20, 64 * V * 4), 0, "outer", True, out_code=oc),
        Case("mom", c, (5, 64 * V * 4), 0, "outer", True, out_code=oc, note="few rows: the moments keep the four-row-group kernel"),
        Case("mom", c, (20, 64 * V * 4 - 1), 0, "outer", False, out_code=oc),
        Case("mom", c, (4096, 256), 0, "outer+fold", True, out_code=oc),
        Case("mom", c, (4096, 255), 0, "outer+fold", False, out_code=oc),
        Case("mom", c, (3, 4096, 96), 1, "outer+fold", True, out_code=oc),
        Case("mom", c, (1000, 1024), 0, "outer_tall", None, out_code=oc),
        Case("mom", c, (1000, 1000), 0, "outer_tall", None, out_code=oc),
        Case("mom", c, (20, 24, 36), (0, 2), "generic", None, out_code=oc),
    ]


def _int_cases(c):
    """Other integer widths and bool: the few-row / few-column kernels, the tall kernel and both folds."""
    V = 16 // H.DTYPE_SIZE[c]
    return [
        Case("sum", c, (65536, 2 * V), 1, "inner_few", True),
        Case("sum", c, (7, 64 * V * 4), 0, "outer_few", True),
        Case("sum", c, (7, 64 * V * 4 - 1), 0, "outer_few", False),
        Case("sum", c, (1000, 1024), 0, "outer_tall", None),
        Case("sum", c, (3, 32 * 256 * V), 1, "inner+fold", True),
        Case("sum", c, (4096, 256), 0, "outer+fold", True),
    ]


SUM_CASES = [k for c in FLOATS + (H.I32,) for k in _sum_cases(c)] + [k for c in (H.BOOL, H.U8, H.I8, H.I16, H.I64) for k in _int_cases(c)]
MOM_CASES = [k for c in FLOATS for k in _mom_cases(c)] + [k for c in (H.BF16, H.F16) for k in _mom_cases(c, H.F32)]
CASES = SUM_CASES + MOM_CASES

SUM_KERNELS = {("inner", True), ("inner", False), ("inner+fold", True), ("inner+fold", False), ("inner_few", True), ("outer", True),
               ("outer", False), ("outer+fold", True), ("outer+fold", False), ("outer_few", True), ("outer_few", False),
               ("outer_tall", None), ("generic", None)}
MOM_KERNELS = {("inner", True), ("inner", False), ("inner+fold", True), ("inner+fold", False), ("outer", True), ("outer", False),
               ("outer+fold", True), ("outer+fold", False), ("outer_tall", None), ("generic", None)}


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def ws_query(d, moments=False):
    need = C.c_size_t(0)
    fn = H.lib().kf_reduce_moments_workspace_bytes if moments else H.lib().kf_reduce_workspace_bytes
    H.check(fn(C.byref(d), C.byref(need)))
    return need.value


def raw_desc(code, shape, in_strides, out_strides, in_ptr=FAKE_IN, moments=False, out_code=None):
    """A descriptor as the iterator leaves it, written out by hand: byte strides, dim 0 first."""
    oc = code if out_code is None else out_code
    d = H.IterDesc()
    nt = 3 if moments else 2
    d.ndim, d.ntensors, d.noutputs = len(shape), nt, nt - 1
    for t in range(nt - 1):
        d.dtype[t], d.data[t] = oc, (FAKE_OUT0, FAKE_OUT1)[t]
    d.dtype[nt - 1], d.data[nt - 1] = code, in_ptr
    for i, n in enumerate(shape):
        d.shape[i] = n
        for t in range(nt - 1):
            d.stride_bytes[t][i] = out_strides[i] * H.DTYPE_SIZE[oc]
        d.stride_bytes[nt - 1][i] = in_strides[i] * H.DTYPE_SIZE[code]
    return d


def rows_desc(code, nout, R, **kw):
    """Inner layout: nout rows of R contiguous elements, reduced along the row."""
    return raw_desc(code, (R, nout), (1, R), (0, 1), **kw)


def cols_desc(code, R, Cx, nouter=1, **kw):
    """Outer layout: [nouter, R, C] row-major, reduced along R."""
    if nouter == 1:
        return raw_desc(code, (R, Cx), (Cx, 1), (0, 1), **kw)
    return raw_desc(code, (R, Cx, nouter), (Cx, 1, R * Cx), (0, 1, Cx), **kw)


def pinned(d, moments=False):
    """The mirror's plan for `d`, after checking its workspace against the library's."""
    p = plan_of(d, moments)
    assert ws_query(d, moments) == p["ws"], p
    return p


def _mirrored_source():
    text = REDUCE_HIP.read_text()
    plan = re.search(r"static int make_plan\(.*?\n}\n", text, re.S).group(0)
    run = re.search(r"    if \(p\.path == PATH_INNER\) \{\n.*?\n    return KF_OK;\n}\n", text, re.S).group(0)
    consts = re.search(r"constexpr int kRB = \d+;", text).group(0)
    return consts + plan + run


# sha256 of make_plan, run_reduce's kernel choice and kRB (whitespace-normalised). A change there fails this test: check the mirror
# above against the new text, then update the hash.
MIRRORED_SHA = "bdf53047229c1b7a2747b5c987e3af5efbd6a200123961670547a3c79f9f693b"


def test_the_mirrored_source_is_the_one_the_mirror_was_checked_against():
    got = hashlib.sha256(" ".join(_mirrored_source().split()).encode()).hexdigest()
    assert got == MIRRORED_SHA, f"make_plan / run_reduce changed (sha {got}): re-check plan_of against reduce.hip, then update MIRRORED_SHA"


SUM_AND_MOMENTS = [(c, False) for c in FLOATS + (H.I32, H.I8, H.BOOL)] + [(c, True) for c in FLOATS]
SM_IDS = [f"{NAME[c]}-{'moments' if m else 'sum'}" for c, m in SUM_AND_MOMENTS]


@pytest.mark.parametrize("code,moments", SUM_AND_MOMENTS, ids=SM_IDS)
def test_inner_edges(code, moments):
    V = 16 // H.DTYPE_SIZE[code]
    kw = dict(moments=moments)
    # target_blocks / 2: gx = nout rows (one row per block at tx = 256) below and at 512
    assert pinned(rows_desc(code, 511, 4096 * V, **kw), moments)["nsplit"] == 2
    assert pinned(rows_desc(code, 512, 4096 * V, **kw), moments)["nsplit"] == 1
    # the 256 cap: 1024 / gx = 341, 256, 204 with max_split far above
    assert [pinned(rows_desc(code, n, 512 * 256 * V * 8, **kw), moments)["nsplit"] for n in (3, 4, 5)] == [256, 256, 204]
    # max_split = R / (tx * vec * 8): one row, R one pack either side of k * tx * vec * 8 - pins tx * vec = 256 * V
    for k in (2, 7, 100):
        assert pinned(rows_desc(code, 1, k * 256 * V * 8, **kw), moments)["nsplit"] == k
        assert pinned(rows_desc(code, 1, k * 256 * V * 8 - V, **kw), moments)["nsplit"] == k - 1
    # scalar rows (R % vec != 0): tx * vec = 256
    if V > 1:
        assert pinned(rows_desc(code, 1, 9 * 256 * 8 + 1, **kw), moments)["nsplit"] == 9
    # element alignment: a pointer one byte off turns packs off (vec 1: max_split = R / (256 * 8)); one element off keeps them
    if H.DTYPE_SIZE[code] > 1:
        d = rows_desc(code, 1, 4 * 256 * V * 8, in_ptr=FAKE_IN + 1, **kw)
        assert pinned(d, moments)["vec"] == 1 and pinned(d, moments)["nsplit"] == min(4 * V, 256)
        d = rows_desc(code, 1, 4 * 256 * V * 8, in_ptr=FAKE_IN + H.DTYPE_SIZE[code], **kw)
        assert pinned(d, moments)["vec"] == V and pinned(d, moments)["nsplit"] == 4


def test_four_packs_per_lane_rule():
    """(nout * tx/4 + 255) / 256 >= 1024 quarters tx; it fires only where gx >= 1024, so the workspace is 0 on both sides and the
    mirror's tx is what is asserted (the source fingerprint holds it to the text)."""
    for code in FLOATS:
        V = 16 // H.DTYPE_SIZE[code]
        for tx in (4, 8, 64, 128):
            edge = -(-((TARGET_BLOCKS - 1) * KB + 1) // (tx // 4))  # the fewest rows with (nout * tx/4 + 255) / 256 >= 1024
            lo, hi = plan_of(rows_desc(code, edge - 1, tx * V)), plan_of(rows_desc(code, edge, tx * V))
            assert (lo["tx"], hi["tx"]) == (tx, tx // 4), (code, tx, edge)
            assert pinned(rows_desc(code, edge - 1, tx * V))["nsplit"] == pinned(rows_desc(code, edge, tx * V))["nsplit"] == 1


@pytest.mark.parametrize("code,moments", SUM_AND_MOMENTS, ids=SM_IDS)
def test_outer_edges(code, moments):
    es = H.DTYPE_SIZE[code]
    V = 16 // es
    kw = dict(moments=moments)
    # target_blocks / 2 on gx * gz, above the tall limit (64 * 1024 * 511 bytes > 16 MiB): C = one block of packs, nouter 511 / 512
    assert pinned(cols_desc(code, 64, 64 * V, 511, **kw), moments)["nsplit"] == 2
    assert pinned(cols_desc(code, 64, 64 * V, 512, **kw), moments)["nsplit"] == 1
    # nouter > 1024 never splits (gz = 1024, so gx * gz >= 512): no tall or fold kernel runs there
    assert pinned(cols_desc(code, 64, 64 * V, 1100, **kw), moments)["nsplit"] == 1
    # max_split = R / 16 and the 256 cap, 256 columns (one or two column blocks; (C + 15) / 16 = 16 keeps the tall kernel off)
    for R, want in ((1600, 100), (1599, 99), (4096, 256), (4112, 256), (31, 1), (32, 2)):
        assert pinned(cols_desc(code, R, 256, **kw), moments)["nsplit"] == want, R
    # tall: the 16 MiB input limit, exactly and one row past
    Cx = 1024
    R = TALL_BYTES // (Cx * es)
    assert pinned(cols_desc(code, R, Cx, **kw), moments)["kernel"] == "outer_tall"
    p = pinned(cols_desc(code, R + 1, Cx, **kw), moments)
    assert p["kernel"] == "outer+fold" and p["nsplit"] > 1
    # tall: (C + 15) / 16 * nouter >= 32, at nouter 2: C = 240 -> 30, C = 241 -> 32 (the rounding), C = 256 -> 32
    assert pinned(cols_desc(code, 1024, 240, 2, **kw), moments)["kernel"] == "outer+fold"
    assert pinned(cols_desc(code, 1024, 241, 2, **kw), moments)["kernel"] == "outer_tall"
    assert pinned(cols_desc(code, 1024, 496, 1, **kw), moments)["kernel"] == "outer+fold"
    assert pinned(cols_desc(code, 1024, 497, 1, **kw), moments)["kernel"] == "outer_tall"
    # the vector width through gx = ceil(C / (64 * vec)): nouter 64 above the tall limit; ns = 1024 / (gx * 64) = 16 packed, 4 scalar
    # (272 rows x 64 packs x 64 outer = 17 MiB: above the tall limit)
    R, nouter, Cx = 272, 64, 64 * V

    def want(gx):
        return max(1, min(1024 // (gx * nouter), R // 16, 256)) if gx * nouter < 512 else 1

    shape, out_strides, good = (R, Cx, nouter), (0, 1, Cx), (Cx, 1, R * Cx)
    assert pinned(raw_desc(code, shape, good, out_strides, **kw), moments)["nsplit"] == want(1) == 16
    assert want(V) != want(1)
    for in_ptr, strides in ((FAKE_IN + es, good),                       # data off 16 bytes
                            (FAKE_IN, (Cx + 1, 1, R * (Cx + 1))),        # in_s0 off 16 bytes
                            (FAKE_IN, (Cx, 1, R * Cx + 1))):             # a dim >= 2 stride off 16 bytes
        p = pinned(raw_desc(code, shape, strides, out_strides, in_ptr=in_ptr, **kw), moments)
        assert p["vec"] == 1 and p["nsplit"] == want(V), (in_ptr, strides)
    p = pinned(cols_desc(code, R, Cx - 1, nouter, **kw), moments)       # C % vec
    assert p["vec"] == 1 and p["nsplit"] == want(V)
    # few rows: R <= 8 never splits; the few-rows kernel is the sums' only
    for R in (2, 8, 9):
        p = pinned(cols_desc(code, R, 64 * V * 4, **kw), moments)
        assert p["nsplit"] == 1
        assert p["kernel"] == ("outer_few" if R <= 8 and not moments else "outer")


def test_inner_few_edges():
    for code in FLOATS + (H.I32, H.BOOL, H.I16):
        V = 16 // H.DTYPE_SIZE[code]
        assert plan_of(rows_desc(code, 65536, V))["kernel"] == "inner_few"
        assert plan_of(rows_desc(code, 65536, 2 * V))["kernel"] == "inner_few"
        assert plan_of(rows_desc(code, 65535, 2 * V))["kernel"] == "inner"            # nout >= 65536
        assert plan_of(rows_desc(code, 65536, 3 * V))["kernel"] == "inner"            # R <= 2 * vec
        assert plan_of(rows_desc(code, 65536, 2 * V, moments=code in FLOATS), moments=code in FLOATS)["kernel"] == (
            "inner" if code in FLOATS else "inner_few")                                 # sums only
        assert plan_of(rows_desc(code, 65536, 2 * V - 1))["kernel"] == "inner"        # R % vec == 0
        if H.DTYPE_SIZE[code] > 1:
            assert plan_of(rows_desc(code, 65536, 2 * V, in_ptr=FAKE_IN + 1))["kernel"] == "inner"  # element alignment
        for R in (V, 2 * V, 3 * V):
            assert ws_query(rows_desc(code, 65536, R)) == 0


def test_moments_with_f32_outputs_behind_16bit_inputs():
    """acc_bytes = 12 for f32 / bf16 / f16 inputs whatever the output dtype, 24 for f64."""
    for code in (H.BF16, H.F16):
        for oc in (code, H.F32):
            d = rows_desc(code, 3, 32 * 256 * 8, moments=True, out_code=oc)
            p = pinned(d, True)
            assert p["nsplit"] == 4 and ws_query(d, True) == 4 * 3 * 12
            d = cols_desc(code, 4096, 256, moments=True, out_code=oc)
            assert pinned(d, True)["ws"] == 256 * 256 * 12
    d = rows_desc(H.F64, 3, 32 * 256 * 2, moments=True)
    assert pinned(d, True)["ws"] == 4 * 3 * 24


def test_random_descriptors_agree_with_the_library():
    """Random shapes, layouts, offsets and dtypes: the mirror's workspace equals the library's for every one."""
    rng = np.random.default_rng(7)
    n = 0
    for _ in range(3000):
        moments = bool(rng.integers(0, 2))
        code = int(rng.choice(FLOATS)) if moments else int(rng.integers(0, 10))
        es = H.DTYPE_SIZE[code]
        nd = int(rng.integers(1, 4))
        shape = tuple(int(v) for v in np.exp(rng.uniform(0, np.log(5000), nd)).astype(int) + 1)
        while int(np.prod(shape)) * es > (1 << 30):
            shape = tuple(max(1, s // 2) for s in shape)
        dims = (int(rng.integers(0, nd)),)
        pad = int(rng.integers(0, 2)) * int(rng.integers(1, 5))
        off = int(rng.integers(0, 2)) * int(rng.integers(1, 4))
        perm = rng.permutation(nd) if rng.integers(0, 4) == 0 else np.arange(nd)
        base = [shape[i] for i in perm]
        bst = contiguous_strides(base, pad)
        strides = [0] * nd
        for k, i in enumerate(perm):
            strides[i] = bst[k]
        oc = H.F32 if moments and code in (H.BF16, H.F16) and rng.integers(0, 2) else None
        case = Case("mom" if moments else "sum", code, shape, dims, "?", None, strides=strides, offset=off, out_code=oc)
        d = case.desc(FAKE_IN, (FAKE_OUT0, FAKE_OUT1)[:2 if moments else 1])
        assert ws_query(d, moments) == plan_of(d, moments)["ws"], case.id
        n += plan_of(d, moments)["nsplit"] > 1
    assert n > 100  # the draw reaches the split paths often enough to pin them


@pytest.mark.parametrize("case", CASES, ids=lambda k: k.id)
def test_each_case_reaches_its_kernel(case):
    p = case.plan()
    assert (p["kernel"], packed(p)) == (case.kernel, case.packed), p
    assert ws_query(case.desc(FAKE_IN, (FAKE_OUT0, FAKE_OUT1)[:2 if case.op == "mom" else 1]), case.op == "mom") == p["ws"]


def _reachable(code, moments):
    """(kernel, packed) pairs the planner produces for `code` over a grid of shapes and layouts."""
    V = 16 // H.DTYPE_SIZE[code]
    seen = set()
    oc = None
    for nout, R, pad, off in itertools.product((1, 3, 300, 65536), (V, 2 * V, 3 * V, 24 * V, 24 * V + 1, 32 * 256 * V + 3, 32 * 256 * V),
                                               (0, 1), (0, 1)):
        if nout * (R + pad) * H.DTYPE_SIZE[code] >= 1 << 31:
            continue
        case = Case("mom" if moments else "sum", code, (nout, R), 1, "?", None, pad=pad, offset=off, out_code=oc)
        p = case.plan()
        seen.add((p["kernel"], packed(p)))
    for nouter, R, Cx, off in itertools.product((1, 3, 1100), (2, 8, 20, 1000, 4096), (100, 255, 256, 1024, 64 * V * 4 - 1), (0, 1)):
        shape = (R, Cx) if nouter == 1 else (nouter, R, Cx)
        case = Case("mom" if moments else "sum", code, shape, 0 if nouter == 1 else 1, "?", None, offset=off)
        seen.add((case.plan()["kernel"], packed(case.plan())))
    seen.add((Case("sum", code, (20, 24, 36), (0, 2), "?", None).plan()["kernel"], None))
    return seen


@pytest.mark.parametrize("code", FLOATS + (H.I32,), ids=lambda c: NAME[c])
def test_the_case_table_covers_every_kernel_the_planner_produces(code):
    for moments, want in ((False, SUM_KERNELS), (True, MOM_KERNELS)):
        if moments and code not in FLOATS:
            continue
        assert _reachable(code, moments) == want, (NAME[code], moments)  # the list below is exactly the planner's
        ocs = (code, H.F32) if moments and code in (H.BF16, H.F16) else (code,)
        for oc in ocs:
            have = {(k.kernel, k.packed) for k in CASES if k.code == code and k.out_code == oc and (k.op == "mom") == moments}
            assert have == want, (NAME[code], NAME[oc], moments, want - have)
