"""-m gpu: every scratch-taking entry of the C ABI on POISONED workspaces and outputs (tests/poison.py).

include/kfunca_hip.h promises, for almost every entry family, that caller scratch needs no initialisation, that beta == 0 makes C an
output only, and that any workspace above the minimum gives the same bits. Each case here runs one call three times - every new device
allocation filled with 0x00 (the baseline), 0xFF (NaN / -1) and 0x7F (3.4e38 in f32 and bf16) - and asserts
  (a) every output is BIT-identical across the three runs (the entries document bitwise reproducibility: a condition, not a tolerance),
  (b) the baseline run meets the bound its family's own test file uses, against the f64 / oracle reference (imported from that file where
      it is a function; quoted with its source where it is an inline expression there), so three identical wrong runs fail too,
  (c) where the case allocates its own outputs: the guard band behind them, and the pad columns of a wide leading dimension, still hold
      the pattern,
  (d) the kernel labels (H.profile_results): the path is pinned, not the shape.
Reductions and moments are covered by tests/test_gpu_reduce_paths.py::test_workspace_contract and have no case here.

label -> case
  gemm_{bf16,f16}_mfma_128_splitk           test_gemm_split_k (every layout, alpha / beta / bias, a larger workspace)
  gemm_pad + gemm_f16_mfma_128 / gemm_f32_mfma_t64   test_gemm_pad_route[f16-384x250x512] (N only), [f32-33x2000x1025] (M, N and K)
  gemm_pad + gemm_bf16_mfma_128_splitk      test_gemm_pad_route[bf16-129x257x4100] (M, N and K), [bf16-256x384x1000] (K only, C in place),
                                            [bf16-250x384x1024] (M only): the pad plan's inner split-K, scratch inside the scratch
  gemm_generic, gemm_f32_mfma_t64, gemm_f32_mfma, gemm_f64_mfma, gemm_{bf16,f16}_mfma_128, gemm_{bf16,f16}_mfma (plain, tail kernel,
    narrow-store epilogue, float output)    test_gemm_beta_zero_never_reads_c
  gemm_{bf16,f16}_mfma_pair                 test_gemm_grouped_pair_beta_zero
  sort_radix                                test_sort_global_radix; sort_radix_lds / sort_bitonic_wave: test_sort_paths_without_scratch
  index_wrap, index_add_sorted (+ sort_*)   test_index_add, test_index_add_misaligned_rows_take_the_element_kernel
  norm_bwd, norm_bwd_fold                   test_norm_backward
  ce_fwd_rows, ce_fwd_block, ce_fwd_split, ce_combine, ce_reduce, ce_bwd     test_cross_entropy
  adamw_norm, adamw_fold, adamw_update      test_adamw_clipping
  attn_fwd_mfma*, attn_bwd_delta, attn_bwd_dkv_mfma*, attn_bwd_dq_mfma*      test_attn_bwd_generated_streams, test_attn_bwd_ds_forms,
                                            test_attn_bwd_hand_kernels_fewer_keys
  attn_bwd_dq_mfma_split*                   test_attn_bwd_recomputing_dq
  attn_bwd_dkv_f32_mfma, attn_bwd_dq_f32_mfma, attn_bwd_generic              test_attn_bwd_f32_mfma_and_generic
  attn_bwd_dkv_group_sum                    test_attn_bwd_gqa
  attn_full_*_mfma_d*, attn_full_bwd_delta, attn_full_*_generic              test_attn_full_outputs
"""
import math

import numpy as np
import pytest

from kfunca_amd import hip_abi as H
from oracle import checks as K
from oracle import oracle as O
from tests import test_gpu_adamw as TA
from tests import test_gpu_attention as TAT
from tests import test_gpu_attention_gqa as TG
from tests import test_gpu_attn_full as TF
from tests import test_gpu_cross_entropy as TC
from tests import test_gpu_norm_walk as TN
from tests import test_gpu_sort as TS
from tests.helpers import assert_close
from tests.poison import GUARD, PATTERNS, guard_intact, guarded, poisoned_allocations
from tests.test_norm_abi import PLANS, bwd_plan, pack, plan_cols

pytestmark = pytest.mark.gpu

EPS = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 2.0 ** -20}
NAME = {H.BF16: "bf16", H.F16: "f16", H.F32: "f32", H.F64: "f64"}


# ---- the three runs --------------------------------------------------------------------------------------------------------------

def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def under_patterns(monkeypatch, call, need=(), equal=None, forbid=()):
    """call(p) -> {name: array} under each pattern (p: tests.poison.Poison). Asserts the labels of every run (`need` a subset, `equal` the
    whole set, no label containing a string of `forbid`) and that the 0xFF and 0x7F runs give the baseline's bits; returns
    (baseline outputs, labels with launch counts of the baseline run)."""
    runs, counts = {}, {}
    for byte in PATTERNS:
        p = poisoned_allocations(monkeypatch, byte)
        H.profile_reset()
        H.profile_enable(True)
        try:
            runs[byte] = call(p)
        finally:
            H.profile_enable(False)
        assert p.allocations > 0, "nothing was allocated under the patch"
        res = H.profile_results()
        counts[byte] = {k: v[1] for k, v in res.items()}
        labels = set(res)
        assert set(need) <= labels, (hex(byte), sorted(need), sorted(labels))
        if equal is not None:
            assert labels == set(equal), (hex(byte), sorted(equal), sorted(labels))
        assert not [n for n in labels for s in forbid if s in n], (hex(byte), forbid, sorted(labels))
    base, changed = runs[0x00], []
    for byte in PATTERNS[1:]:
        assert counts[byte] == counts[0x00], (hex(byte), counts[byte], counts[0x00])
        assert runs[byte].keys() == base.keys()
        for name, want in base.items():
            got = runs[byte][name]
            if not same_bits(got, want):
                diff = np.flatnonzero(np.frombuffer(got.tobytes(), np.uint8) != np.frombuffer(want.tobytes(), np.uint8))
                changed.append(f"{name}: a fill of {byte:#04x} changes {diff.size} of {want.nbytes} bytes (first at {diff[0]})")
    assert not changed, "the result depends on what scratch / outputs held before the call - " + "; ".join(changed)
    return base, counts[0x00]


def mk(rng, shape, code):
    x = rng.uniform(-1, 1, shape)
    return x if code == H.F64 else O.from_float(x.astype(np.float32), code)


def f64(x, code):
    return np.asarray(x, np.float64) if code == H.F64 else O.to_float(x, code).astype(np.float64)


def put_rows(buf, arr, ld_bytes):
    """Host [rows, cols] -> the rows of a device matrix with a pitch of ld_bytes (what lies between the rows stays as it is)."""
    TN.h2d_rows(buf, arr, 0, ld_bytes)


# ---- GEMM ------------------------------------------------------------------------------------------------------------------------

def gemm_call(p, code, a, b, ta=False, tb=False, alpha=1.0, beta=0.0, c=None, bias=None, mul=None, add=None, aux=False, c_f32=False,
              ldc=None, ws_extra=0, ex=False, with_ws=True):
    """One product on buffers this test owns: C (and aux) come from H.DevBuf - filled with the pattern - with a guard band, and are
    written with c only when beta != 0. a, b are the stored arrays. Returns {"c": [M, N], "aux": [M, N]} in storage dtypes."""
    M, Kk = (a.shape[1], a.shape[0]) if ta else a.shape
    N = b.shape[0] if tb else b.shape[1]
    ldc = N if ldc is None else ldc
    cdt = np.dtype(np.float32) if c_f32 else a.dtype
    da, db = H.DevBuf.from_numpy(a), H.DevBuf.from_numpy(b)
    cbytes = M * ldc * cdt.itemsize
    dc = guarded(cbytes)
    if beta != 0.0:
        put_rows(dc, c, ldc * cdt.itemsize)
    dbias = H.DevBuf.from_numpy(bias) if bias is not None else None
    dmul = H.DevBuf.from_numpy(mul) if mul is not None else None
    dadd = H.DevBuf.from_numpy(add) if add is not None else None
    daux = guarded(M * N * a.itemsize) if aux else None
    if ex or mul is not None or add is not None or aux or c_f32:
        H.gemm_ex(code, ta, tb, M, N, Kk, alpha, da.ptr, a.shape[1], db.ptr, b.shape[1], beta, dc.ptr, ldc, bias=dbias.ptr if dbias else None,
                  mul=dmul.ptr if dmul else None, ldmul=mul.shape[1] if mul is not None else 0, add=dadd.ptr if dadd else None,
                  ldadd=add.shape[1] if add is not None else 0, aux=daux.ptr if daux else None, ldaux=N if aux else 0, c_f32=c_f32)
    else:
        need = H.gemm_workspace_bytes(code, ta, tb, M, N, Kk) if with_ws else 0
        ws = guarded(need + ws_extra) if need else None
        H.gemm(code, ta, tb, M, N, Kk, alpha, da.ptr, a.shape[1], db.ptr, b.shape[1], beta, dc.ptr, ldc,
               H.EPI_BIAS_ROW if bias is not None else H.EPI_NONE, dbias.ptr if dbias else None, ws.ptr if ws else None, need + ws_extra if ws else 0)
        H.device_sync()
        assert ws is None or guard_intact(ws, need + ws_extra, p.byte), "the GEMM wrote behind its workspace"
    H.device_sync()
    assert guard_intact(dc, cbytes, p.byte), "the GEMM wrote behind C"
    full = dc.to_numpy((M, ldc), cdt)
    if ldc > N:
        assert (full[:, N:].view(np.uint8) == p.byte).all(), "the pad columns of C were written"
    out = {"c": np.ascontiguousarray(full[:, :N])}
    if aux:
        assert guard_intact(daux, M * N * a.itemsize, p.byte), "the GEMM wrote behind aux"
        out["aux"] = daux.to_numpy((M, N), a.dtype)
    return out


def operands(rng, code, M, N, Kk):
    a, b = mk(rng, (M, Kk), code), mk(rng, (Kk, N), code)
    af, bf = f64(a, code), f64(b, code)
    return a, b, af @ bf, np.abs(af) @ np.abs(bf)


def stored(x, t):
    return np.ascontiguousarray(x.T) if t else x


def nan_free(x, code):
    assert np.isfinite(f64(x, code)).all(), "non-finite values in the result"


@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_gemm_split_k(monkeypatch, code):
    """256 x 384 x 4096: 8 K slices whose f32 partial tiles the fold sums straight out of scratch. Every layout (bound: K.gemm_ok),
    alpha / beta / bias through the fold (bound of test_gpu_gemm.test_split_k_skinny_products: 2 eps |c| + 2e-6 sum |a||b| + 2 eps), a
    workspace 4096 bytes larger than needed (the same bits), and beta == 0 on a C full of the pattern. kf_gemm_ex takes no workspace,
    so the mul / add tail cannot reach the split kernels: that call is the unsplit ..._128 kernel's (test_gemm_beta_zero_never_reads_c)."""
    rng = np.random.default_rng(99 + code)
    M, N, Kk = 256, 384, 4096
    a, b, want, mag = operands(rng, code, M, N, Kk)
    label = f"gemm_{NAME[code]}_mfma_128_splitk"
    assert H.gemm_workspace_bytes(code, False, False, M, N, Kk) == 8 * M * N * 4
    nn = None
    for ta in (False, True):
        for tb in (False, True):
            sa, sb = stored(a, ta), stored(b, tb)
            base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, sa, sb, ta, tb), equal={label})
            nan_free(base["c"], code)
            ok, frac = K.gemm_ok(base["c"], a, b, code)
            assert ok, f"{ta} {tb}: at {frac:.2f} of the bound"
            nn = base["c"] if not (ta or tb) else nn
    bigger, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, ws_extra=4096), equal={label})
    assert same_bits(bigger["c"], nn), "a workspace 4096 bytes larger changes the result"
    bias, c = mk(rng, (N,), code), mk(rng, (M, N), code)
    base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, alpha=0.5, beta=2.0, c=c, bias=bias), equal={label})
    want_e = 0.5 * want + 2.0 * f64(c, code) + f64(bias, code)[None, :]
    assert (np.abs(f64(base["c"], code) - want_e) <= 2 * EPS[code] * np.abs(want_e) + 2e-6 * mag + 2 * EPS[code]).all()


# (dtype, M, N, K, the padded product's kernel): 129 x 257 x 4100 pads to 256 x 384 x 4160 (6 tiles, 65 K tiles: 8 slices), 256 x 384 x 1000
# and 250 x 384 x 1024 to 256 x 384 x 1024 (16 K tiles: 2 slices) - split-K inside the pad plan; 384 x 250 x 512 (8 K tiles) runs unsplit
PAD_CASES = [(H.BF16, 129, 257, 4100, "gemm_bf16_mfma_128_splitk"), (H.F32, 33, 2000, 1025, "gemm_f32_mfma_t64"),
             (H.BF16, 256, 384, 1000, "gemm_bf16_mfma_128_splitk"), (H.BF16, 250, 384, 1024, "gemm_bf16_mfma_128_splitk"),
             (H.F16, 384, 250, 512, "gemm_f16_mfma_128")]


@pytest.mark.parametrize("code,M,N,Kk,inner", PAD_CASES, ids=[f"{NAME[c]}-{m}x{n}x{k}" for c, m, n, k, _ in PAD_CASES])
def test_gemm_pad_route(monkeypatch, code, M, N, Kk, inner):
    """Ragged extents on zero-padded images in caller scratch: the borders come from gemm_pad_copy_kernel, the padded C image is left
    unwritten when beta == 0 and the unpad copies out of it; K-only ragged writes C in place; 129 x 257 x 4100 pads to 256 x 384 x 4160,
    whose product is split-K in scratch inside the scratch. beta = 0, and alpha = 0.5 / beta = 2 / bias; bounds of
    test_gpu_gemm.test_ragged_extents_run_on_the_matrix_kernels: 2 eps |c| + 2 eps sum |a||b| (+ 4 in the sum with the epilogue)."""
    rng = np.random.default_rng(M + 3 * N + 7 * Kk + code)
    eps = EPS[code]
    a, b, want, mag = operands(rng, code, M, N, Kk)
    bias, c = mk(rng, (N,), code), mk(rng, (M, N), code)
    assert H.gemm_workspace_bytes(code, False, False, M, N, Kk) > 0
    for tb in (False, True):
        sb = stored(b, tb)
        base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, sb, tb=tb, ldc=N + 3), equal={"gemm_pad", inner})
        nan_free(base["c"], code)
        assert (np.abs(f64(base["c"], code) - want) <= 2 * eps * np.abs(want) + 2 * eps * mag + 1e-30).all(), tb
    base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, alpha=0.5, beta=2.0, c=c, bias=bias), equal={"gemm_pad", inner})
    want_e = 0.5 * want + 2.0 * f64(c, code) + f64(bias, code)[None, :]
    assert (np.abs(f64(base["c"], code) - want_e) <= 2 * eps * np.abs(want_e) + 2 * eps * (mag + 4) + 1e-30).all()


TAIL_EPS = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 1e-6, H.F64: 1e-13}   # test_gpu_gemm.test_fused_elementwise_tail
BETA0_CASES = [  # (label, dtype, M, N, K, modes): the shapes of test_gpu_gemm.test_fused_elementwise_tail, one per kernel family
    ("gemm_generic", H.BF16, 100, 130, 70, ("plain", "tail", "c_f32")), ("gemm_generic", H.F32, 33, 65, 17, ("plain", "tail")),
    ("gemm_f32_mfma_t64", H.F32, 256, 384, 64, ("plain", "tail")), ("gemm_f32_mfma", H.F32, 2048, 2048, 32, ("plain", "tail")),
    ("gemm_f64_mfma", H.F64, 128, 192, 48, ("plain", "tail")),
    ("gemm_bf16_mfma_128", H.BF16, 256, 384, 128, ("plain", "tail", "c_f32")), ("gemm_f16_mfma_128", H.F16, 256, 384, 128, ("plain", "tail", "c_f32")),
    ("gemm_bf16_mfma_128", H.BF16, 256, 384, 4096, ("tail",)),   # the split-K shape through kf_gemm_ex (no workspace there: unsplit)
    ("gemm_bf16_mfma", H.BF16, 2560, 4096, 128, ("plain", "tail", "ldc", "c_f32")), ("gemm_f16_mfma", H.F16, 2560, 4096, 128, ("plain", "tail", "ldc", "c_f32")),
]


@pytest.mark.parametrize("label,code,M,N,Kk,modes", BETA0_CASES, ids=[f"{c[0]}-{NAME[c[1]]}-{c[2]}x{c[3]}x{c[4]}" for c in BETA0_CASES])
def test_gemm_beta_zero_never_reads_c(monkeypatch, label, code, M, N, Kk, modes):
    """beta == 0: C is an output only. C, aux and the float C of c_f32 hold the pattern when the call starts (NaN, -1, 3.4e38); the
    result equals the zero-C run bit for bit and is NaN-free, on every kernel family (label asserted as the only one).
    plain: kf_gemm (16-bit: K.gemm_ok; f32 / f64: the aux bound of test_fused_elementwise_tail). tail: kf_gemm_ex with bias, mul (wide),
    add and aux - that test's bounds with the beta C term gone. ldc: C rows of N + 4 elements (the narrow-store epilogue), pad columns
    keep the pattern. c_f32: float C behind 16-bit operands (test_float_output_behind_16bit_operands: 2e-6 sum |a||b| + 1e-6)."""
    rng = np.random.default_rng(M + N + Kk + code)
    eps = TAIL_EPS[code]
    a, b, want, mag0 = operands(rng, code, M, N, Kk)
    bias, mul_w, add = mk(rng, (N,), code), mk(rng, (M, N + 8), code), mk(rng, (M, N), code)
    acc = 1.0 if code != H.F64 else 1e-7
    for mode in modes:
        if mode in ("plain", "ldc"):
            base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, ldc=N + 4 if mode == "ldc" else None, with_ws=False), equal={label})
            nan_free(base["c"], code)
            if code in (H.BF16, H.F16):
                ok, frac = K.gemm_ok(base["c"], a, b, code)
                assert ok, f"{mode}: at {frac:.2f} of the bound"
            else:
                assert (np.abs(f64(base["c"], code) - want) <= 2 * eps * np.abs(want) + 2e-6 * (mag0 + 1.0) * acc + 2 * eps).all(), mode
        elif mode == "tail":
            base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, alpha=0.5, bias=bias, mul=mul_w, add=add, aux=True), equal={label})
            nan_free(base["c"], code), nan_free(base["aux"], code)
            raw, mag = 0.5 * want + f64(bias, code)[None, :], mag0 + 1.0
            assert (np.abs(f64(base["aux"], code) - raw) <= 2 * eps * np.abs(raw) + 2e-6 * mag * acc + 2 * eps).all(), "aux"
            full = raw * f64(mul_w, code)[:, :N] + f64(add, code)
            assert (np.abs(f64(base["c"], code) - full) <= 4 * eps * (np.abs(full) + np.abs(raw)) + 2e-6 * mag * acc + 4 * eps).all(), "C"
        else:
            base, _ = under_patterns(monkeypatch, lambda p: gemm_call(p, code, a, b, c_f32=True), equal={label})
            assert base["c"].dtype == np.float32 and np.isfinite(base["c"]).all()
            assert (np.abs(base["c"].astype(np.float64) - want) <= 2e-6 * mag0 + 1e-6).all(), "float C"


@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_gemm_grouped_pair_beta_zero(monkeypatch, code):
    """kf_gemm_grouped on the backward pair dA = dC W^T, dW = A^T dC at 4096 x 4096 with K' = 1792 (112 tiles per product: the smallest
    pair grid), beta = 0, both outputs full of the pattern, dW a float output. One launch (label ..._pair); sampled rows against
    K.gemm_ok (dA) and the float-output bound (dW), as test_headline_backward_pair_vs_oracle_at_4096 samples them."""
    rng = np.random.default_rng(123 + code)
    M, N, Kp = 4096, 4096, 1792
    a, w, g = mk(rng, (M, Kp), code), mk(rng, (Kp, N), code), mk(rng, (M, N), code)
    da, dw, dg = H.DevBuf.from_numpy(a), H.DevBuf.from_numpy(w), H.DevBuf.from_numpy(g)
    rows = [0, 1, 127, 128, 255, 256, 1000, 1790, 1791]
    label = f"gemm_{NAME[code]}_mfma_pair"

    def call(p):
        o0, o1 = guarded(M * Kp * 2), guarded(Kp * N * 4)
        H.gemm_grouped(code, [(0, 1, M, Kp, N, 1.0, 0.0, dg.ptr, N, dw.ptr, N, o0.ptr, Kp), (1, 0, Kp, N, M, 1.0, 0.0, da.ptr, Kp, dg.ptr, N, o1.ptr, N, 1)])
        H.device_sync()
        assert guard_intact(o0, M * Kp * 2, p.byte) and guard_intact(o1, Kp * N * 4, p.byte)
        return {"dA": o0.to_numpy((M, Kp), a.dtype), "dW": o1.to_numpy((Kp, N), np.float32)}

    base, counts = under_patterns(monkeypatch, call, equal={label})
    assert counts[label] == 1
    nan_free(base["dA"], code)
    assert np.isfinite(base["dW"]).all()
    ok, frac = K.gemm_ok(base["dA"][rows], g[rows], w, code, trans_b=True)
    assert ok, f"dA at {frac:.2f} of the bound"
    a_cols = f64(np.ascontiguousarray(a[:, rows]), code)
    want_dw, mag_dw = a_cols.T @ f64(g, code), np.abs(a_cols).T @ np.abs(f64(g, code))
    assert (np.abs(base["dW"][rows].astype(np.float64) - want_dw) <= 2e-6 * mag_dw + 1e-6).all()


# ---- sort ------------------------------------------------------------------------------------------------------------------------

def sort_call(keys, code, desc):
    k, pos = H.sort_segments(keys, desc, code=code)   # dst, positions and scratch are DevBufs made inside
    return {"keys": k, "pos": pos}


@pytest.mark.parametrize("nseg,n", [(1, 8193), (3, 20000), (2, 70001)])
@pytest.mark.parametrize("code", [H.F32, H.I64, H.U8, H.BF16], ids=["f32", "i64", "u8", "bf16"])
def test_sort_global_radix(monkeypatch, code, nseg, n):
    """n > 8192: histograms, scans and the ping-pong key / position arrays live in scratch. Bit-exact against the oracle, as
    tests/test_gpu_sort.py::check does, in both directions."""
    keys = TS.draw(np.random.default_rng(n + code), (nseg, n), code)
    assert H.lib().kf_sort_workspace_bytes(code, nseg, n) > 0
    for desc in (False, True):
        base, _ = under_patterns(monkeypatch, lambda p: sort_call(keys, code, desc), equal={"sort_radix"})
        want_k, want_p = O.sort_stable(keys, 1, desc, code=code)
        assert np.array_equal(base["pos"], want_p), desc
        assert np.array_equal(base["keys"].view(np.uint8), want_k.view(np.uint8)), desc


@pytest.mark.parametrize("n,label", [(8192, "sort_radix_lds"), (512, "sort_bitonic_wave")])
def test_sort_paths_without_scratch(monkeypatch, n, label):
    """The LDS and register paths ask for no scratch: asserted, so that a future dependency on scratch shows up here; outputs poisoned."""
    keys = TS.draw(np.random.default_rng(n), (3, n), H.F32)
    assert H.lib().kf_sort_workspace_bytes(H.F32, 3, n) == 0
    base, _ = under_patterns(monkeypatch, lambda p: sort_call(keys, H.F32, True), equal={label})
    want_k, want_p = O.sort_stable(keys, 1, True, code=H.F32)
    assert np.array_equal(base["pos"], want_p) and np.array_equal(base["keys"].view(np.uint8), want_k.view(np.uint8))


# ---- kf_index_add ----------------------------------------------------------------------------------------------------------------

SENTINEL, GUARD_ROWS = 5.0, 8


def index_add_want(idx, srcf, nrows, have):
    """The exact result: per named row the f32 sum of its gradient rows IN INPUT ORDER (what tests/test_gpu_norm.py's loops compute, by
    rank within each row's group so that it stays quick at 20000 indices); rows nobody names keep the sentinel."""
    want = np.full((have + GUARD_ROWS, srcf.shape[1]), SENTINEL, dtype=np.float32)
    ok = (idx >= -nrows) & (idx < nrows)
    js = np.flatnonzero(ok)
    wrapped = np.where(idx < 0, idx + nrows, idx)[js]
    order = np.argsort(wrapped, kind="stable")
    js, wrapped = js[order], wrapped[order]
    if js.size == 0:
        return want
    first = np.r_[True, wrapped[1:] != wrapped[:-1]]
    gid = np.cumsum(first) - 1
    start = np.flatnonzero(first)
    rank = np.arange(js.size) - start[gid]
    acc = np.zeros((start.size, srcf.shape[1]), dtype=np.float32)
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        acc[gid[sel]] = acc[gid[sel]] + srcf[js[sel]]
    want[wrapped[start]] = acc
    return want


def index_add_case(rng, code, n, cols, nrows, have):
    idx = rng.integers(-have, have, size=(n,)).astype(np.int64) if have == nrows else rng.integers(0, have, size=(n,)).astype(np.int64)
    idx[idx % have == 11] = 12                                   # row 11 is named by nobody
    bad = rng.choice(n, size=n // 10, replace=False)            # one tenth out of range: dropped
    idx[bad] = rng.choice(np.array([nrows, nrows + 5, -nrows - 1, 2 ** 40, -2 ** 40, 2 ** 62], dtype=np.int64), size=bad.size)
    return idx, O.from_float(rng.uniform(-1, 1, (n, cols)).astype(np.float32), code)


def index_add_call(code, idx, src, cols, nrows, have, offset=0):
    """dst = have + GUARD_ROWS sentinel rows (have = nrows, or the first rows of a 2^31-row table); offset: bytes by which src and dst
    are moved off their 16-byte-aligned bases."""
    n = idx.size
    sent = O.from_float(np.full((have + GUARD_ROWS, cols), SENTINEL, dtype=np.float32), code)
    bi = H.DevBuf.from_numpy(idx)
    bs, dst = H.DevBuf(src.nbytes + 16), H.DevBuf(sent.nbytes + 16)
    H.check(H.lib().kf_memcpy_h2d(bs.ptr + offset, src.ctypes.data, src.nbytes, None))
    H.check(H.lib().kf_memcpy_h2d(dst.ptr + offset, sent.ctypes.data, sent.nbytes, None))
    ws = H.index_add(code, bi.ptr, n, bs.ptr + offset, cols, nrows, dst.ptr + offset)   # the scratch: a DevBuf made inside
    H.device_sync()
    del ws
    out = np.empty_like(sent)
    H.check(H.lib().kf_memcpy_d2h(out.ctypes.data, dst.ptr + offset, out.nbytes, None))
    return {"dst": out}


def index_add_check(code, base, idx, src, nrows, have):
    want = index_add_want(idx, O.to_float(src, code).astype(np.float32), nrows, have)
    got = O.to_float(base["dst"], code)
    assert np.array_equal(got, O.to_float(O.from_float(want, code), code))
    assert (got[11 % have] == SENTINEL).all() or have <= 11
    assert (got[have:] == SENTINEL).all(), "rows behind the table were written"


@pytest.mark.parametrize("nrows", [300, 65535, 65536, 70000, 1 << 31])
@pytest.mark.parametrize("cols", [64, 100])   # 16-byte packs, element-wise rows
@pytest.mark.parametrize("code", [H.F32, H.BF16], ids=["f32", "bf16"])
def test_index_add(monkeypatch, code, cols, nrows):
    """wrapped indices | sorted keys | positions | the sort's own scratch, all in one poisoned block: n in {1, 64, 65, 600, 20000}
    (20000: the global radix sort, with skipped passes) into tables whose sentinel key nrows needs 9, 16, 17 and 17 bits (65535 | 65536:
    one radix pass more), and 2^31 rows (int64 keys; the first 16 rows exist). The exact input-order f32 sums; unnamed rows, and the
    rows behind the table, keep the sentinel."""
    rng = np.random.default_rng(nrows % 1000 + cols + code)
    have = nrows if nrows < (1 << 31) else 16
    for n in ((1, 64, 65, 600, 20000) if nrows < (1 << 31) else (600,)):
        idx, src = index_add_case(rng, code, n, cols, nrows, have)
        need = {"index_wrap", "index_add_sorted"} | ({"sort_radix"} if n > 8192 else set())
        base, _ = under_patterns(monkeypatch, lambda p: index_add_call(code, idx, src, cols, nrows, have), need=need)
        index_add_check(code, base, idx, src, nrows, have)


@pytest.mark.parametrize("code", [H.F32, H.BF16], ids=["f32", "bf16"])
def test_index_add_misaligned_rows_take_the_element_kernel(monkeypatch, code):
    """cols = 64 gives rows of whole 16-byte packs, but src and dst sit 4 bytes past a 16-byte boundary: the element kernel on rows the
    pack kernel would otherwise take. Bit-identical to the aligned call, under every pattern."""
    rng = np.random.default_rng(404 + code)
    n, cols, nrows = 600, 64, 300
    idx, src = index_add_case(rng, code, n, cols, nrows, nrows)
    need = {"index_wrap", "index_add_sorted"}
    aligned, _ = under_patterns(monkeypatch, lambda p: index_add_call(code, idx, src, cols, nrows, nrows), need=need)
    moved, _ = under_patterns(monkeypatch, lambda p: index_add_call(code, idx, src, cols, nrows, nrows, offset=4), need=need)
    assert same_bits(moved["dst"], aligned["dst"])
    index_add_check(code, moved, idx, src, nrows, nrows)


# ---- norm backward ---------------------------------------------------------------------------------------------------------------

NORM_CASES = [(p, c, k) for p in PLANS for c in (H.F32, H.BF16) for k in (H.NORM_RMS, H.NORM_LAYER)]


@pytest.mark.parametrize("plan,code,kind", NORM_CASES, ids=[f"{t}x{p}-{NAME[c]}-{TN.KNAME[k]}" for (t, p), c, k in NORM_CASES])
def test_norm_backward(monkeypatch, plan, code, kind):
    """Every register-tile plan (lanes per row x packs) of tests/test_gpu_norm_walk.py at its ragged column count, at 1, 5 and 33 row
    groups (the fold's remainder loop alone, and its 8-way loop plus a remainder) with a partial last group: the partial dw / db rows
    go through scratch, dx / dw / db / y / mean / rstd are poisoned outputs. Bounds: reference_check of that file (f64)."""
    R = TN.rpb(plan)
    cols = plan_cols(code, plan)[1]
    assert bwd_plan(code, cols)[:2] == plan
    rng = np.random.default_rng(2000 + 97 * PLANS.index(plan) + 7 * code + kind)
    for nrb in (1, 5, 33):
        rows = (nrb - 1) * R + max(1, R // 2)
        x, dy, w, b = TN.random_case(rng, code, rows, cols, kind, True)

        def call(p):
            y, mean, rstd, dx, dw, db = TN.fwd_bwd(kind, code, x, w, b, dy)
            out = {"y": y, "rstd": rstd, "dx": dx, "dw": dw}
            if kind == H.NORM_LAYER:
                out.update(mean=mean, db=db)
            return out

        o, _ = under_patterns(monkeypatch, call, need={"norm_fwd", "norm_bwd", "norm_bwd_fold"}, forbid=("generic",))
        TN.reference_check(kind, code, x, w, b, dy, o["y"], o.get("mean"), o["rstd"], o["dx"], o["dw"], o.get("db"),
                           what=f"{plan} {NAME[code]} {TN.KNAME[kind]} [{rows}, {cols}]")


@pytest.mark.parametrize("code", [H.F32, H.BF16], ids=["f32", "bf16"])
def test_norm_backward_wide_rows(monkeypatch, code):
    """ld > cols (layer norm, the 64-lane two-pack plan, 33 row groups): same bits as the contiguous call, and the elements between
    dx's rows keep the pattern."""
    kind, plan = H.NORM_LAYER, (64, 2)
    R, cols = TN.rpb(plan), plan_cols(code, plan)[1]
    rows, ld = 32 * R + 1, cols + 3 * pack(code)
    assert bwd_plan(code, cols, ld)[:2] == plan
    rng = np.random.default_rng(3000 + code)
    x, dy, w, _ = TN.random_case(rng, code, rows, cols, kind, True)
    xf = TN.as64(x, code)   # the statistics a forward would hand over, from f64 (reference_check holds them to 256 u / 128 u)
    mean = xf.mean(1).astype(np.float32)
    rstd = (1.0 / np.sqrt(((xf - mean[:, None].astype(np.float64)) ** 2).mean(1) + TN.EPS)).astype(np.float32)
    el = x.itemsize

    def call(p, pitch):
        def up(arr):
            big = np.zeros((rows, pitch), arr.dtype)
            big[:, :cols] = arr
            return H.DevBuf.from_numpy(big)
        bx, bdy, bw, bm, br = up(x), up(dy), H.DevBuf.from_numpy(w), H.DevBuf.from_numpy(mean), H.DevBuf.from_numpy(rstd)
        bdx, bdw, bdb = guarded(rows * pitch * el), guarded(cols * el), guarded(cols * el)
        ws = TN.run_bwd(kind, code, rows, cols, bx, bw, bm, br, bdy, bdx, bdw, bdb, ld=pitch)
        H.device_sync()
        del ws
        assert guard_intact(bdx, rows * pitch * el, p.byte) and guard_intact(bdw, cols * el, p.byte) and guard_intact(bdb, cols * el, p.byte)
        dxf = bdx.to_numpy((rows, pitch), x.dtype)
        assert (dxf[:, cols:].view(np.uint8) == p.byte).all(), "elements between dx rows were written"
        return {"dx": np.ascontiguousarray(dxf[:, :cols]), "dw": bdw.to_numpy((cols,), x.dtype), "db": bdb.to_numpy((cols,), x.dtype)}

    need = {"norm_bwd", "norm_bwd_fold"}
    tight, _ = under_patterns(monkeypatch, lambda p: call(p, cols), need=need, forbid=("generic",))
    wide, _ = under_patterns(monkeypatch, lambda p: call(p, ld), need=need, forbid=("generic",))
    for name in ("dx", "dw", "db"):
        assert same_bits(wide[name], tight[name]), name
    TN.reference_check(kind, code, x, w, None, dy, None, mean, rstd, wide["dx"], wide["dw"], wide["db"], what=f"ld {ld} {NAME[code]}")


# ---- cross-entropy ---------------------------------------------------------------------------------------------------------------

# regimes of cross_entropy.hip (ce_plan): V <= 4096 one wave per row; V > 4096 and rows >= 1024 one block per row; V > 4096 and fewer
# rows: each row split into chunks whose (max, sum, sum x) partials go through scratch and ce_combine
CE_CASES = [("ce_fwd_rows", 37, 1000, None), ("ce_fwd_rows", 5, 4096, 4100), ("ce_fwd_block", 1024, 4097, None), ("ce_fwd_split", 3, 20000, None),
            ("ce_fwd_split", 7, 4097, 4101), ("ce_fwd_split", 1023, 4100, None)]


@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("code", [H.F32, H.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("label,rows,V,ld", CE_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in CE_CASES])
def test_cross_entropy(monkeypatch, label, rows, V, ld, code, smoothing):
    """Every forward regime (label asserted; the split one with ce_combine), reductions mean and sum (ce_reduce folds the per-row losses
    out of scratch) and none, ignored rows, label smoothing; loss, lse, count and dlogits all hold the pattern beforehand (dlogits is not
    zeroed as tests/test_gpu_cross_entropy.py::run does), the pad columns of a wide dlogits keep it. Against that file's f64 ref with
    its tolerances (loss, lse: 1e-4 + 1e-5 |ref|; dlogits: one output rounding; sums: rtol 1e-5)."""
    rng = np.random.default_rng(rows * 7 + V + code)
    xs, x = TC.make(rng, code, rows, V, ld)
    pitch = V if ld is None else ld
    t = rng.integers(0, V, rows)
    t[rng.random(rows) < 0.1] = -100
    t[0] = 3 % V          # (at least one row counts)
    rlse, rloss, rd = TC.ref(x, t, eps=smoothing)
    keep = t != -100
    n = int(keep.sum())
    for red, nloss in ((H.CE_NONE, rows), (H.CE_SUM, 1), (H.CE_MEAN, 1)):
        g = rng.uniform(0.5, 2.0, nloss).astype(np.float32)

        def call(p):
            bx, bt, bg = H.DevBuf.from_numpy(xs), H.DevBuf.from_numpy(t.astype(np.int64)), H.DevBuf.from_numpy(g)
            bl, blse, bc, bd = guarded(4 * nloss), guarded(4 * rows), guarded(4), guarded(xs.nbytes)
            ws = H.ce_fwd(code, rows, V, bx.ptr, bt.ptr, bl.ptr, blse.ptr, bc.ptr, -100, smoothing, red, ld=ld)   # scratch: a DevBuf made inside
            H.ce_bwd(code, rows, V, bx.ptr, bt.ptr, blse.ptr, bc.ptr, bg.ptr, bd.ptr, -100, smoothing, red, ld=ld)
            H.device_sync()
            del ws
            for buf, nb in ((bl, 4 * nloss), (blse, 4 * rows), (bc, 4), (bd, xs.nbytes)):
                assert guard_intact(buf, nb, p.byte)
            dxf = bd.to_numpy(xs.shape, TC.NP[code])
            assert (dxf[:, V:].view(np.uint8) == p.byte).all(), "the backward wrote beyond V"
            return {"loss": bl.to_numpy((nloss,), np.float32), "lse": blse.to_numpy((rows,), np.float32), "count": bc.to_numpy((1,), np.float32),
                    "dlogits": np.ascontiguousarray(dxf[:, :V])}

        need = {label, "ce_bwd"} | ({"ce_combine"} if label == "ce_fwd_split" else set()) | ({"ce_reduce"} if red != H.CE_NONE else set())
        o, _ = under_patterns(monkeypatch, call, need=need)
        assert pitch >= V and o["count"][0] == n
        assert_close(o["lse"][keep], rlse[keep], rtol=1e-5, atol=1e-4, what="lse")
        if red == H.CE_NONE:
            assert_close(o["loss"], rloss, rtol=1e-5, atol=1e-4, what="loss")
            g_eff = g[:, None].astype(np.float64)
        else:
            assert_close(o["loss"], [rloss.sum() / (n if red == H.CE_MEAN else 1)], rtol=1e-5, atol=1e-4, what=f"reduction {red}")
            g_eff = np.full((rows, 1), float(g[0]) / (n if red == H.CE_MEAN else 1))
        TC.check_dx(code, o["dlogits"], rd, g_eff, f"dlogits, reduction {red}")


# ---- AdamW -----------------------------------------------------------------------------------------------------------------------

def test_adamw_clipping(monkeypatch):
    """max_grad_norm > 0: adamw_norm writes 2048 partial sums per group of 48 tensors into scratch and adamw_fold reads them back, with the
    clip coefficient, from the same block. 50 tensors (two groups: 4096 partials, four per fold thread) from 1 to 70001 elements, three
    clipped steps; grad_norm, the scratch and the unused master / pad bytes hold the pattern. Params, both moments and the norm against
    CPU torch with the tolerances of tests/test_gpu_adamw.py (f32_close, rtol 1e-5 + atol 4e-6 on the moments, rtol 1e-5 on the norm)."""
    rng = np.random.default_rng(42)
    sizes = [1, 3, 63, 64, 65, 4097, 70_001] + [int(s) for s in rng.integers(1, 3000, 43)]
    assert len(sizes) > 48
    steps, max_norm, lr, betas, eps, wd = 3, 1.0, 1e-3, (0.9, 0.999), 1e-8, 0.01
    p0s = [rng.uniform(-1, 1, s).astype(np.float32) for s in sizes]
    grads = [[rng.standard_normal(s).astype(np.float32) for s in sizes] for _ in range(steps)]

    def call(p):
        ts = [TA.AbiTensor(q, wd=wd) for q in p0s]
        norms = []
        for gs in grads:
            for t, g in zip(ts, gs):
                t.set_grad(g)
            norms.append(TA.abi_step(ts, lr, beta1=betas[0], beta2=betas[1], eps=eps, max_grad_norm=max_norm))
        reads = [t.read() for t in ts]
        assert all(r[3] == steps for r in reads)
        return {"param": np.concatenate([r[0] for r in reads]), "exp_avg": np.concatenate([r[1] for r in reads]),
                "exp_avg_sq": np.concatenate([r[2] for r in reads]), "norm": np.array(norms, np.float32)}

    o, _ = under_patterns(monkeypatch, call, equal={"adamw_norm", "adamw_fold", "adamw_update"})
    rp, rm, rv, rnorms = TA.torch_run(p0s, grads, lr, betas, eps, wd, max_norm=max_norm)
    assert min(rnorms) > max_norm   # clipped on every step
    assert_close(o["norm"], rnorms, rtol=1e-5, atol=0, what="norm")
    scale = max_norm / min(rnorms)  # the moments see gradients scaled by at most this
    TA.f32_close(o["param"], np.concatenate(rp), "param")
    assert_close(o["exp_avg"], np.concatenate(rm), rtol=1e-5, atol=4e-6 * scale, what="exp_avg")
    assert_close(o["exp_avg_sq"], np.concatenate(rv), rtol=1e-5, atol=4e-6 * scale ** 2, what="exp_avg_sq")


# ---- causal attention backward ---------------------------------------------------------------------------------------------------

def attn_inputs(rng, code, B, Hh, Sq, Skv, D):
    return tuple(O.from_float(rng.uniform(-1, 1, s).astype(np.float32), code) for s in ((B, Hh, Sq, D), (B, Hh, Skv, D), (B, Hh, Skv, D), (B, Hh, Sq, D)))


def attn_min_ws(code, B, Hh, Sq, Skv, D):
    """The statistics alone: the minimum kf_attn_bwd accepts (the GQA query with Hkv = Hq reports it)."""
    return H.attn_bwd_gqa_workspace_bytes(code, B, Hh, Hh, Sq, Skv, D)[1]


def attn_call(p, code, q, k, v, go, ws_bytes=None):
    """kf_attn_fwd + kf_attn_bwd: o, lse, dq, dk, dv and the workspace all come from H.DevBuf (the pattern), each with a guard band."""
    B, Hh, Sq, D = q.shape
    Skv = k.shape[2]
    bq, bk, bv, bgo = (H.DevBuf.from_numpy(x) for x in (q, k, v, go))
    nl = 4 * B * Hh * Sq
    bo, blse = guarded(q.nbytes), guarded(nl)
    H.attn_fwd(code, B, Hh, Sq, Skv, D, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr)
    dq, dk, dv = guarded(q.nbytes), guarded(k.nbytes), guarded(v.nbytes)
    need = H.attn_bwd_workspace_bytes(code, B, Hh, Sq, Skv, D) if ws_bytes is None else ws_bytes
    ws = guarded(need)
    H.attn_bwd(code, B, Hh, Sq, Skv, D, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, dq.ptr, dk.ptr, dv.ptr, ws.ptr, need)
    H.device_sync()
    for name, buf, nb in (("o", bo, q.nbytes), ("lse", blse, nl), ("dq", dq, q.nbytes), ("dk", dk, k.nbytes), ("dv", dv, v.nbytes), ("workspace", ws, need)):
        assert guard_intact(buf, nb, p.byte), f"the bytes behind {name} were written"
    return {"o": bo.to_numpy(q.shape, q.dtype), "lse": blse.to_numpy((B, Hh, Sq), np.float32), "dq": dq.to_numpy(q.shape, q.dtype),
            "dk": dk.to_numpy(k.shape, k.dtype), "dv": dv.to_numpy(v.shape, v.dtype)}


def attn_labels(D, split=False):
    sfx = "_d64" if D == 64 else ""
    return {"attn_fwd_mfma" + sfx, "attn_bwd_delta", "attn_bwd_dkv_mfma" + sfx, ("attn_bwd_dq_mfma_split" if split else "attn_bwd_dq_mfma") + sfx}


def attn_check16(code, q, k, v, go, o, what):
    K.attn_check(q, k, v, code, o=o["o"], lse=o["lse"], d_o=go, dq=o["dq"], dk=o["dk"], dv=o["dv"], what=what)


@pytest.mark.parametrize("Sq,Skv", [(256, 256), (257, 257), (257, 320), (320, 1000)])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_attn_bwd_generated_streams(monkeypatch, code, D, Sq, Skv):
    """The generated streams on whole tiles and on ragged lengths (B H = 3: the rows "beyond the end" of heads 0 and 1 are the next
    head's): the delta kernel's pad rows of the row-constant arrays, partly filled dS squares, dS in the recommended workspace."""
    rng = np.random.default_rng(Sq * 7 + Skv + code + D)
    q, k, v, go = attn_inputs(rng, code, 1, 3, Sq, Skv, D)
    o, _ = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go), equal=attn_labels(D))
    attn_check16(code, q, k, v, go, o, f"{Sq}x{Skv} D{D}")


@pytest.mark.parametrize("Sq,Skv", [(257, 320), (600, 600)])
@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_attn_bwd_ds_forms(monkeypatch, code, D, Sq, Skv):
    """dS as full rows, as the causal half (KF_ATTN_DS_TRI=1) and in two groups of the causal half (a workspace that holds two of the
    three pairs' dS: the second group runs on what the first left in the squares) - each on poisoned memory, and all three the same bits,
    as include/kfunca_hip.h promises. 600 x 600: three query blocks, so the half is smaller than the rows and the squares above the
    diagonal are never written. Launch counts as test_backward_workspace_is_bounded_any_size_above_the_statistics_is_accepted."""
    rng = np.random.default_rng(Sq + Skv + code + D)
    B, Hh = 1, 3
    q, k, v, go = attn_inputs(rng, code, B, Hh, Sq, Skv, D)
    stats = attn_min_ws(code, B, Hh, Sq, Skv, D)
    full = H.attn_bwd_workspace_bytes(code, B, Hh, Sq, Skv, D)
    with H.knobs(KF_ATTN_DS_TRI="1"):
        tri = H.attn_bwd_workspace_bytes(code, B, Hh, Sq, Skv, D)
    one, half = (full - stats) // (B * Hh), (tri - stats) // (B * Hh)
    assert 0 < half <= one and (Sq <= 256 or half < one)
    sfx = "_d64" if D == 64 else ""
    rows, c = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go, full), equal=attn_labels(D))
    assert c["attn_bwd_dkv_mfma" + sfx] == 1 and c["attn_bwd_dq_mfma" + sfx] == 1
    with H.knobs(KF_ATTN_DS_TRI="1"):
        halves, c = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go, tri), equal=attn_labels(D))
    assert c["attn_bwd_dkv_mfma" + sfx] == 1 and c["attn_bwd_dq_mfma" + sfx] == 1
    groups, c = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go, stats + 2 * half + 100), equal=attn_labels(D))
    assert c["attn_bwd_dkv_mfma" + sfx] == 2 and c["attn_bwd_dq_mfma" + sfx] == 2, c
    for name in rows:
        assert same_bits(halves[name], rows[name]), ("causal half", name)
        assert same_bits(groups[name], rows[name]), ("two groups", name)
    attn_check16(code, q, k, v, go, rows, f"dS forms {Sq}x{Skv} D{D}")


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_attn_bwd_recomputing_dq(monkeypatch, code, D):
    """The minimum workspace alone (whole tiles: the only shapes it serves on the matrix cores): no dS, the recomputing dQ kernel."""
    rng = np.random.default_rng(300 + D + code)
    B, Hh, S = 1, 3, 256
    q, k, v, go = attn_inputs(rng, code, B, Hh, S, S, D)
    stats = attn_min_ws(code, B, Hh, S, S, D)
    o, _ = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go, stats), equal=attn_labels(D, split=True))
    attn_check16(code, q, k, v, go, o, f"recomputing dQ D{D}")


@pytest.mark.parametrize("D", [128, 64])
@pytest.mark.parametrize("code", [H.BF16, H.F16], ids=["bf16", "f16"])
def test_attn_bwd_hand_kernels_fewer_keys(monkeypatch, code, D):
    """Skv < Sq (384 x 128): not a shape of the generated streams - the hand-written 128-tile dK/dV kernel stores dS."""
    rng = np.random.default_rng(384 + D + code)
    q, k, v, go = attn_inputs(rng, code, 1, 3, 384, 128, D)
    o, _ = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go), equal=attn_labels(D))
    attn_check16(code, q, k, v, go, o, f"384x128 D{D}")


@pytest.mark.parametrize("code,Sq,Skv,D,labels", [
    (H.F32, 96, 160, 64, {"attn_fwd_f32_mfma", "attn_bwd_delta", "attn_bwd_dkv_f32_mfma", "attn_bwd_dq_f32_mfma"}),
    (H.BF16, 100, 100, 40, {"attn_fwd_generic", "attn_bwd_generic"}), (H.F32, 65, 33, 48, {"attn_fwd_generic", "attn_bwd_generic"})],
    ids=["f32-mfma-96x160", "bf16-generic-100x100", "f32-generic-65x33"])
def test_attn_bwd_f32_mfma_and_generic(monkeypatch, code, Sq, Skv, D, labels):
    """The exact-f32 matrix-core kernels and the generic ones: delta in scratch. f32 against the oracle with the bounds of
    tests/test_gpu_attention.py (forward 2e-5 on U(-1, 1); backward 5e-5 of each gradient's scale), bf16 against K.attn_check."""
    rng = np.random.default_rng(Sq * 3 + Skv + D)
    B, Hh = 2, 3
    if code == H.BF16:
        q, k, v, go = attn_inputs(rng, code, B, Hh, Sq, Skv, D)
    else:
        q, k, v, go = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((B, Hh, Sq, D), (B, Hh, Skv, D), (B, Hh, Skv, D), (B, Hh, Sq, D)))
    o, _ = under_patterns(monkeypatch, lambda p: attn_call(p, code, q, k, v, go), equal=labels)
    if code == H.BF16:
        attn_check16(code, q, k, v, go, o, f"generic {Sq}x{Skv} D{D}")
        return
    o_ref, lse_ref = O.attn_fwd(q, k, v)
    assert_close(o["o"], o_ref, rtol=2e-5, atol=2e-5, what="f32 fwd")
    assert_close(o["lse"], lse_ref, rtol=1e-5, atol=1e-4, what="lse")
    for name, w in zip(("dq", "dk", "dv"), O.attn_bwd(q, k, v, go)):
        scale = np.abs(w).max() + 1e-30
        assert np.isfinite(o[name]).all() and np.abs(o[name] - w).max() <= 5e-5 * scale, (name, float(np.abs(o[name] - w).max() / scale))


# ---- grouped-query attention backward --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Sq,Skv", [(256, 256), (257, 320)])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (4, 1)])
@pytest.mark.parametrize("code,D", [(H.BF16, 128), (H.F16, 64)], ids=["bf16-d128", "f16-d64"])
def test_attn_bwd_gqa(monkeypatch, code, D, Hq, Hkv, Sq, Skv):
    """The dK/dV kernels write one partial per QUERY head into scratch and attn_bwd_dkv_group_sum folds them. Under every pattern: o, lse,
    dq equal MHA-on-repeat and dk, dv its ascending-g group sum, bit for bit (the contract of tests/test_gpu_attention_gqa.py, whose
    helpers allocate under the patch); MHA-on-repeat itself against K.attn_check."""
    rng = np.random.default_rng(1000 * Hq + 10 * Hkv + D + Sq)
    B, G = 1, Hq // Hkv
    q, go = TG.rnd(rng, code, (B, Hq, Sq, D)), TG.rnd(rng, code, (B, Hq, Sq, D))
    k, v = TG.rnd(rng, code, (B, Hkv, Skv, D)), TG.rnd(rng, code, (B, Hkv, Skv, D))
    kr, vr = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
    scale = TG.scale_of(D)
    names = ("o", "lse", "dq", "dk", "dv")
    got, _ = under_patterns(monkeypatch, lambda p: dict(zip(names, TG.gqa(code, q, k, v, go, scale))),
                            equal=attn_labels(D) | {"attn_bwd_dkv_group_sum"})
    rep, _ = under_patterns(monkeypatch, lambda p: dict(zip(names, TG.mha(code, q, kr, vr, go, scale))), equal=attn_labels(D))
    for name in ("o", "lse", "dq"):
        assert TG.same(got[name], rep[name]), f"{name} differs from MHA-on-repeat"
    assert TG.same(got["dk"], TG.group_sum(rep["dk"], G, code)) and TG.same(got["dv"], TG.group_sum(rep["dv"], G, code))
    attn_check16(code, q, kr, vr, go, rep, f"MHA-on-repeat {Hq}/{Hkv} {Sq}x{Skv}")


# ---- full attention --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("code,D,Sq,Skv,lens", [(H.BF16, 128, 130, 200, [200, 0, 1, 65]), (H.F16, 64, 130, 200, [200, 0, 1, 65]), (H.F32, 80, 33, 70, [17, 0, 40, 1])],
                         ids=["bf16-d128", "f16-d64", "f32-generic"])
def test_attn_full_outputs(monkeypatch, code, D, Sq, Skv, lens):
    """tests/test_gpu_attn_full.py::run already fills the workspace with 0xFF; under the patch o, lse, dq, dk, dv hold the pattern too.
    Per-batch key lengths with a batch at 0 keys (the smallest the entry accepts: o, dq zeros and lse -inf must be WRITTEN) and at 1."""
    rng = np.random.default_rng(D + Sq + code)
    q, k, v, go = TF.inputs(rng, code, len(lens), 4, 2, Sq, Skv, D)
    names = ("o", "lse", "dq", "dk", "dv")
    mfma = code != H.F32
    need = {f"{n}_d{D}" for n in TF.MFMA_LABELS} | {"attn_full_bwd_delta"} if mfma else {"attn_full_fwd_generic", "attn_full_bwd_dq_generic", "attn_full_bwd_dkv_generic"}
    o, counts = under_patterns(monkeypatch, lambda p: dict(zip(names, TF.run(code, q, k, v, go, lens))), need=need, forbid=("generic",) if mfma else ("mfma",))
    got = tuple(o[n] for n in names)
    if mfma:
        TF.check16(code, q, k, v, go, got, lens, "poisoned outputs")
    else:
        TF.check_generic(code, q, k, v, go, got, lens, set(counts))
    for b, ln in enumerate(lens):
        assert not TF.bits(o["dk"][b, :, ln:]).any() and not TF.bits(o["dv"][b, :, ln:]).any(), b
    assert not TF.bits(o["o"][1]).any() and not TF.bits(o["dq"][1]).any() and np.isneginf(o["lse"][1]).all()
    assert math.isfinite(float(O.to_float(o["o"], code).astype(np.float64).sum()))
