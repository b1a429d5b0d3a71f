"""-m gpu: every GEMM kernel on operands that are windows of wider buffers (lda, ldb, ldc above the packed value, bases that are not the
start of an allocation), through the C ABI only.

include/kfunca_hip.h promises any leading dimension at or above the extent; this file pins the `row * ld` arithmetic of every kernel
family, of the pad / unpad copies, of the split-K fold and of both legs of the 16-bit eight-column accesses. tests/gemm_views.py builds
the buffers (NaN-poisoned gaps and guards on inputs, 0xA5 on outputs) and operands whose expected outputs are exact, so:
  (a) the set of recorded kernel labels is exactly the one the dispatch code prescribes (restated in gemm_views.expected_labels and
      written out per table row below),
  (b) C's window equals the expected value bit for bit, with alpha = 1, beta = 0 and with alpha = 0.5, beta = 2 + row bias,
  (c) every byte of C's and aux's buffers outside the window is still 0xA5,
  (d) A's and B's buffers come back unchanged,
  (e) for U(-1, 1) operands the window is bit-identical to the same call on packed copies (same kernel, same accumulation order),
  (f) the backward pair as one grid is bit-identical to the two separate products on the same views.
tests/test_gemm_views_ref.py shows on the CPU that these checks reject a product evaluated with any of the classic pitch mistakes.
No tolerance occurs anywhere in this file.
"""
import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from tests import gemm_views as V

pytestmark = pytest.mark.gpu

CODE = {"f32": H.F32, "f64": H.F64, "bf16": H.BF16, "f16": H.F16}
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
EPILOGUES = [(1.0, 0.0, False), (0.5, 2.0, True)]  # (alpha, beta, row bias)
NAMES = ("a", "b", "c", "bias", "mul", "add", "aux")


class Live:
    """A case's views on the device."""

    def __init__(self, case):
        self.case = case
        self.views = {n: getattr(case, n) for n in NAMES if getattr(case, n) is not None}
        self.bufs = {n: H.DevBuf.from_numpy(v.buf) for n, v in self.views.items()}
        assert all(b.ptr % 16 == 0 for b in self.bufs.values())

    def ptr(self, n):
        return self.bufs[n].ptr + self.views[n].off * V.ES[self.views[n].dt] if n in self.views else None

    def ld(self, n):
        return self.views[n].ld if n in self.views else 0

    def base16(self, n):
        return self.ptr(n) % 16 == 0

    def after(self, n):
        return self.bufs[n].to_numpy(self.views[n].buf.shape, self.views[n].buf.dtype)


def profiled(fn):
    H.profile_reset()
    H.profile_enable(True)
    try:
        fn()
        H.device_sync()
    finally:
        H.profile_enable(False)
    return set(H.profile_results())


def workspace_for(c):
    need = H.gemm_workspace_bytes(CODE[c.dt], c.ta, c.tb, c.M, c.N, c.K)
    return H.DevBuf(need) if need else None


def call(live, ws=None):
    """The one library call of a case: kf_gemm, or kf_gemm_ex when it has a tail or a float C."""
    c = live.case
    args = (CODE[c.dt], c.ta, c.tb, c.M, c.N, c.K, c.alpha, live.ptr("a"), live.ld("a"), live.ptr("b"), live.ld("b"), c.beta, live.ptr("c"), live.ld("c"))
    if c.tail or c.c_dt != c.dt:
        assert ws is None
        H.gemm_ex(*args, bias=live.ptr("bias"), mul=live.ptr("mul"), ldmul=live.ld("mul"), add=live.ptr("add"), ldadd=live.ld("add"), aux=live.ptr("aux"),
                  ldaux=live.ld("aux"), c_f32=c.c_dt != c.dt)
    else:
        H.gemm(*args, H.EPI_BIAS_ROW if c.bias is not None else H.EPI_NONE, live.ptr("bias"), ws.ptr if ws else None, ws.nbytes if ws else 0)


def derived_labels(live, ws):
    c = live.case
    return V.expected_labels(c.dt, c.ta, c.tb, c.M, c.N, c.K, live.ld("a"), live.ld("b"), live.base16("a"), live.base16("b"), workspace=ws is not None,
                             tail=c.tail, c_f32=c.c_dt != c.dt)


def inputs_unchanged(live):
    for n, v in live.views.items():
        if v.poison == "nan":
            assert np.array_equal(live.after(n).view(np.uint8), v.buf.view(np.uint8)), f"the call changed input {n}'s buffer"


def run_exact(c, labels):
    """(a) - (d) for one exact case."""
    live, ws = Live(c), workspace_for(c)
    assert derived_labels(live, ws) == labels, (derived_labels(live, ws), labels)
    got = profiled(lambda: call(live, ws))
    what = (c.dt, c.ta, c.tb, c.alpha, c.beta)
    assert got == labels, (got, labels, what)                                   # (a)
    V.check_output(c.c, live.after("c"), c.want)                                # (b), (c)
    if c.tail:
        V.check_output(c.aux, live.after("aux"), c.want_aux)
    inputs_unchanged(live)                                                      # (d)


def run_uniform_vs_packed(c, labels):
    """(e): U(-1, 1) operands, the gapped call against the same call on packed copies - bit-identical windows, the same label."""
    outs = []
    for case in (c, c.packed()):
        live, ws = Live(case), workspace_for(case)
        assert profiled(lambda: call(live, ws)) == labels, (case.dt, case.ta, case.tb, case.a.ld)
        outs.append({n: (case, live.after(n)) for n in ("c", "aux") if n in live.views})
    for n, (case, after) in outs[0].items():
        v, (pcase, pafter) = getattr(case, n), outs[1][n]
        assert v.outside_intact(after), f"{n}: bytes outside the window changed"
        got, ref = v.window(after), getattr(pcase, n).window(pafter)
        assert not np.isnan(V.decode(got, v.dt)).any()
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), f"{n} differs from the packed call"


def seed_of(dt, M, N, K, ta, tb, e):
    return (((M * 3 + N) * 5 + K) * 4 + 2 * ta + tb) * 8 + 4 * e + ("f32", "f64", "bf16", "f16").index(dt) % 4


def run_row(dt, M, N, K, gaps, labels, tail=False, c_f32=False, per_epilogue=None):
    labels = {s.replace("*", dt) for s in labels}
    c_dt = "f32" if c_f32 else None
    for ta, tb in LAYOUTS:
        for e, (alpha, beta, bias) in enumerate(EPILOGUES):
            g = dict(gaps, **(per_epilogue[e] if per_epilogue else {}))
            run_exact(V.Case(dt, ta, tb, M, N, K, g, alpha, beta, bias, tail, c_dt, seed_of(dt, M, N, K, ta, tb, e)), labels)
        # (e): one draw per row; small rows can afford one per layout
        if M * N <= 1 << 20 or (ta, tb) == LAYOUTS[(M + N + K + len(dt)) % 4]:
            run_uniform_vs_packed(V.Case(dt, ta, tb, M, N, K, gaps, 0.5, 2.0, True, tail, c_dt, seed_of(dt, M, N, K, ta, tb, 2), draw="uniform"), labels)


G = V.operand_gaps
# the narrow (element-wise) leg of the 16-bit eight-column accesses: aux's rows (a store) in the first epilogue, mul's rows (a load) in the second
TAIL_NARROW = [{"aux": (24, 4)}, {"mul": (8, 4)}]
RAGGED = {"a": (3, 3), "b": (3, 5), "c": (3, 1)}  # odd column offsets and pitches: the pad / unpad copies read and write through ld_src / ld_dst element-wise
# id, dtype, M, N, K, gaps, labels ('*': the dtype), keywords
ROWS = [
    *[(f"generic-{dt}", dt, 100, 130, 70, G(3, 5), {"gemm_generic"}, {}) for dt in ("f32", "f64", "bf16", "f16")],
    ("f32_mfma_t64", "f32", 128, 192, 48, G(4, 12), {"gemm_f32_mfma_t64"}, {}),
    ("f32_mfma", "f32", 2048, 1536, 32, G(4, 12), {"gemm_f32_mfma"}, {}),                                      # 192 tiles of 128
    ("f64_mfma", "f64", 128, 192, 80, G(2, 6), {"gemm_f64_mfma"}, {}),
    *[(f"mfma_128-{dt}", dt, 256, 384, 128, G(8, 24), {"gemm_*_mfma_128"}, {}) for dt in ("bf16", "f16")],
    *[(f"mfma_128_splitk-{dt}", dt, 128, 256, 1024, G(8, 24), {"gemm_*_mfma_128_splitk"}, {}) for dt in ("bf16", "f16")],  # + the fold, unlabelled
    *[(f"mfma_256-{dt}", dt, 2560, 2560, 128, G(8, 24), {"gemm_*_mfma"}, {}) for dt in ("bf16", "f16")],       # 100 tiles of 256
    *[(f"mfma_256_tail-{dt}", dt, 2560, 2560, 128, G(8, 24), {"gemm_*_mfma"}, dict(tail=True, per_epilogue=TAIL_NARROW)) for dt in ("bf16", "f16")],
    *[(f"pad-{dt}", dt, 300, 520, 700, RAGGED, {"gemm_pad", "gemm_*_mfma_128"}, {}) for dt in ("bf16", "f16")],
    ("pad-f32", "f32", 192, 128, 1001, RAGGED, {"gemm_pad", "gemm_f32_mfma_t64"}, {}),
    # B is whole tiles: with ldb % 8 == 0 on a 16-byte base it is read where it lies, with an odd pitch it is copied; A (ragged M) is always copied
    ("pad_b_in_place-bf16", "bf16", 250, 384, 1024, {"a": (8, 24), "b": (8, 8), "c": (24, 8)}, {"gemm_pad", "gemm_bf16_mfma_128_splitk"}, {}),
    ("pad_b_copied-bf16", "bf16", 250, 384, 1024, {"a": (8, 24), "b": (3, 3), "c": (24, 8)}, {"gemm_pad", "gemm_bf16_mfma_128_splitk"}, {}),
    *[(f"c_f32_128-{dt}", dt, 256, 384, 128, dict(G(8, 24), c=(4, 6)), {"gemm_*_mfma_128"}, dict(c_f32=True)) for dt in ("bf16", "f16")],
    *[(f"c_f32_256-{dt}", dt, 2560, 2560, 128, dict(G(8, 24), c=(4, 6)), {"gemm_*_mfma"}, dict(c_f32=True)) for dt in ("bf16", "f16")],
]


@pytest.mark.parametrize("dt,M,N,K,gaps,labels,kw", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_row(dt, M, N, K, gaps, labels, kw):
    if "splitk" in "".join(labels) and "gemm_pad" not in labels:
        assert H.gemm_workspace_bytes(CODE[dt], 0, 0, M, N, K) == V.splitk_slices(dt, M, N, K) * M * N * 4 > M * N * 4
    run_row(dt, M, N, K, gaps, labels, **kw)


# ---- the backward pair of a linear layer as ONE grid ------------------------------------------------------------------------------
def pair_cases(dt, alpha, beta, draw="int"):
    """dA[2048, 3328] = dC[2048, 2048] W^T (W stored [3328, 2048]) and dW[3328, 2048] = A^T dC (A stored [2048, 3328]): 104 tiles each."""
    return (V.Case(dt, 0, 1, 2048, 3328, 2048, G(8, 24), alpha, beta, seed=41 + (draw != "int"), draw=draw),
            V.Case(dt, 1, 0, 3328, 2048, 2048, G(24, 8), alpha, beta, seed=43 + (draw != "int"), draw=draw))


def problems(lives):
    return [(L.case.ta, L.case.tb, L.case.M, L.case.N, L.case.K, L.case.alpha, L.case.beta, L.ptr("a"), L.ld("a"), L.ptr("b"), L.ld("b"), L.ptr("c"), L.ld("c"))
            for L in lives]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_row_mfma_pair(dt):
    label = {f"gemm_{dt}_mfma_pair"}
    for alpha, beta in ((1.0, 0.0), (0.5, 2.0)):
        cases = pair_cases(dt, alpha, beta)
        # three pitches per product, and no operand shares its pitch with its counterpart in the other product (a mixed-up g0 / g1 shows)
        assert all(len({c.a.ld, c.b.ld, c.c.ld}) == 3 for c in cases) and all(getattr(cases[0], n).ld != getattr(cases[1], n).ld for n in "abc")
        lives = [Live(c) for c in cases]
        assert V.pair_is_one_grid(dt, [dict(ta=c.ta, tb=c.tb, M=c.M, N=c.N, K=c.K, lda=c.a.ld, ldb=c.b.ld, ldc=c.c.ld, a_base16=L.base16("a"),
                                            b_base16=L.base16("b")) for c, L in zip(cases, lives)])
        got = profiled(lambda: H.gemm_grouped(CODE[dt], problems(lives)))
        assert got == label and H.profile_results()[f"gemm_{dt}_mfma_pair"][1] == 1, H.profile_results()   # (a): one launch
        afters = [L.after("c") for L in lives]
        for c, L, after in zip(cases, lives, afters):
            V.check_output(c.c, after, c.want)                                                            # (b), (c)
            inputs_unchanged(L)                                                                           # (d)
        # (f): the two separate products on the same views
        for c, L, after in zip(cases, lives, afters):
            H.check(H.lib().kf_memcpy_h2d(L.bufs["c"].ptr, c.c.buf.ctypes.data, c.c.buf.nbytes, None))
            assert profiled(lambda: call(L)) == {f"gemm_{dt}_mfma"}
            assert np.array_equal(L.after("c").view(np.uint8), after.view(np.uint8)), "the pair differs from the separate product"
        del lives
    # (e), (f) on U(-1, 1) operands: one grid on views == one grid on packed copies == the separate products on the views
    cases = pair_cases(dt, 0.5, 2.0, draw="uniform")
    lives, packed = [Live(c) for c in cases], [Live(c.packed()) for c in cases]
    assert profiled(lambda: H.gemm_grouped(CODE[dt], problems(lives))) == label
    assert profiled(lambda: H.gemm_grouped(CODE[dt], problems(packed))) == label
    for c, L, P in zip(cases, lives, packed):
        after = L.after("c")
        assert c.c.outside_intact(after)
        win = np.ascontiguousarray(c.c.window(after))
        assert not np.isnan(V.decode(win, dt)).any()
        assert np.array_equal(win, np.ascontiguousarray(P.case.c.window(P.after("c")))), "views differ from packed copies"
        H.check(H.lib().kf_memcpy_h2d(L.bufs["c"].ptr, c.c.buf.ctypes.data, c.c.buf.nbytes, None))
        call(L)
        H.device_sync()
        assert np.array_equal(L.after("c").view(np.uint8), after.view(np.uint8)), "the pair differs from the separate product"


# ---- predicate edges: the label follows from gemm_impl's predicates on the pitch and the base address ------------------------------
EDGES = [
    # 16-bit whole tiles, lda = extent + 4: rows are 8-byte aligned only -> no 16-byte DMA rows -> the scalar kernel (too small to pad)
    ("h128_lda_plus_4", "bf16", 128, 128, 64, dict(G(8, 24), a=(0, 4)), {"gemm_generic"}),
    # the same with lda % 8 == 0 but A's base 8 bytes past a 16-byte boundary
    ("h128_a_base_8_bytes_off", "bf16", 128, 128, 64, dict(G(8, 24), a=(4, 4)), {"gemm_generic"}),
    ("f32_lda_mod_4_is_2", "f32", 128, 192, 48, dict(G(4, 12), a=(4, 2)), {"gemm_generic"}),
    ("f64_lda_odd", "f64", 128, 192, 80, dict(G(2, 6), a=(2, 1)), {"gemm_generic"}),
    # C's alignment routes nothing: the 256-tile kernel stays, its epilogue takes the element-wise leg
    ("h256_ldc_mod_8_is_4", "bf16", 2560, 2560, 128, dict(G(8, 24), c=(8, 4)), {"gemm_bf16_mfma"}),
    ("h256_c_base_8_bytes_off", "f16", 2560, 2560, 128, dict(G(8, 24), c=(4, 4)), {"gemm_f16_mfma"}),
]


@pytest.mark.parametrize("dt,M,N,K,gaps,labels", [e[1:] for e in EDGES], ids=[e[0] for e in EDGES])
def test_predicate_edge(dt, M, N, K, gaps, labels):
    for ta, tb in LAYOUTS:
        c = V.Case(dt, ta, tb, M, N, K, gaps, 0.5, 2.0, True, seed=seed_of(dt, M, N, K, ta, tb, 3))
        run_exact(c, labels)


# ---- one large-pitch case per family: the last row of the operand starts beyond byte 2^32 of the view --------------------------------
LARGE = [("generic", "f32", 16, 20, 12, 1, {"gemm_generic"}), ("f32_mfma_t64", "f32", 64, 64, 16, 4, {"gemm_f32_mfma_t64"}),
         ("f64_mfma", "f64", 64, 64, 16, 2, {"gemm_f64_mfma"}), ("mfma_128", "bf16", 128, 128, 64, 8, {"gemm_bf16_mfma_128"}),
         ("mfma_256", "bf16", 2560, 2560, 64, 8, {"gemm_bf16_mfma"})]


@pytest.mark.slow
@pytest.mark.parametrize("dt,M,N,K,q,labels", [r[1:] for r in LARGE], ids=[r[0] for r in LARGE])
def test_large_pitch(dt, M, N, K, q, labels):
    """One operand with a pitch such that its last row starts beyond byte 2^32: A stored [M, K] (rows of M), then B stored [K, N] and A stored
    [K, M] (the transposed-read layouts: K rows, the K loop steps by 64 such rows). The gaps are neither poisoned nor initialised (gigabytes);
    rows are uploaded one by one. Integer-exact expected values; the other operand and C are ordinary views behind their guards."""
    es = V.ES[dt]
    for big, ta, tb in (("a", 0, 1), ("b", 0, 0), ("a", 1, 0)):
        c = V.Case(dt, ta, tb, M, N, K, dict(G(*{"f64": (2, 6), "f32": (4, 12)}.get(dt, (8, 24))), **{big: (0, 0)}), seed=M + N + K + 2 * ta + tb)
        rows, cols = getattr(c, big).rows, getattr(c, big).cols
        ld = -(-((1 << 32) // ((rows - 1) * es) + 1) // q) * q  # the smallest pitch (a multiple of q) that puts the last row beyond byte 2^32
        ld += 1 if q == 1 and ld % 2 == 0 else 0                # the scalar kernel: an odd one
        assert (rows - 1) * ld * es > 1 << 32 and rows * ld * es < 5 << 30 and ld % q == 0 and ld >= cols
        small = {n: getattr(c, n) for n in ("a", "b", "c") if n != big}
        bufs = {n: H.DevBuf.from_numpy(v.buf) for n, v in small.items()}
        ptr = {n: bufs[n].ptr + v.off * V.ES[v.dt] for n, v in small.items()}
        lds = {n: v.ld for n, v in small.items()}
        wide = H.DevBuf(((rows - 1) * ld + cols) * es)
        try:
            stored = np.ascontiguousarray(getattr(c, big).window())
            for r in range(rows):
                H.check(H.lib().kf_memcpy_h2d(wide.ptr + r * ld * es, stored[r].ctypes.data, cols * es, None))
            ptr[big], lds[big] = wide.ptr, ld
            assert V.expected_labels(dt, ta, tb, M, N, K, lds["a"], lds["b"], ptr["a"] % 16 == 0, ptr["b"] % 16 == 0) == labels
            got = profiled(lambda: H.gemm(CODE[dt], ta, tb, M, N, K, 1.0, ptr["a"], lds["a"], ptr["b"], lds["b"], 0.0, ptr["c"], lds["c"]))
            assert got == labels, (got, big, ta, tb)
            V.check_output(c.c, bufs["c"].to_numpy(c.c.buf.shape, c.c.buf.dtype), c.want)
            last = np.empty(cols, dtype=stored.dtype)
            H.check(H.lib().kf_memcpy_d2h(last.ctypes.data, wide.ptr + (rows - 1) * ld * es, cols * es, None))
            assert np.array_equal(last, stored[rows - 1]), "the operand's last row changed"
        finally:
            wide.free()
