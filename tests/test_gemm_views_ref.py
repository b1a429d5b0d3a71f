"""CPU: the view helper of the GEMM view suite (tests/gemm_views.py) and proof that the suite's check rejects pitch bugs.

model_product evaluates a product in f64 while walking the buffers with arbitrary pitches. With the true pitches it reproduces the
expected value, and the check the GPU suite applies to a kernel's output accepts it; with each classic pitch mistake the same check
rejects it - through NaN (a gap element entered a product), wrong integers, or a damaged 0xA5 sentinel. So a kernel with one of these
mistakes cannot pass tests/test_gpu_gemm_views.py; no GPU and no mutant kernel is needed to know that.
"""
import numpy as np
import pytest

from tests import gemm_views as V

# the table rows of the GPU suite that are small enough to evaluate by gather on the CPU: (dtype, M, N, K, gaps)
ROWS = [("f32", 100, 130, 70, (3, 5)), ("f64", 100, 130, 70, (3, 5)), ("bf16", 100, 130, 70, (3, 5)), ("f16", 100, 130, 70, (3, 5)),
        ("f32", 128, 192, 48, (4, 12)), ("f64", 128, 192, 80, (2, 6)), ("bf16", 256, 384, 128, (8, 24)), ("f16", 256, 384, 128, (8, 24))]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
IDS = [f"{r[0]}-{r[1]}x{r[2]}x{r[3]}" for r in ROWS]


def make(row, ta, tb, epilogue):
    dt, M, N, K, (g1, g2) = row
    alpha, beta, bias = ((1.0, 0.0, False), (0.5, 2.0, True))[epilogue]
    return V.Case(dt, ta, tb, M, N, K, V.operand_gaps(g1, g2), alpha, beta, bias, seed=M + 3 * N + 7 * K + epilogue)


@pytest.mark.parametrize("dt", ["f32", "f64", "bf16", "f16"])
def test_view_layout_guards_and_poison(dt):
    es = V.ES[dt]
    inp, out = V.View(dt, 7, 10, 3, 5, "nan", reach=1000), V.View(dt, 7, 10, 3, 5, "a5")
    for v in (inp, out):
        assert v.ld == 18 and v.off == v.lo + 3 and v.off > 0 and v.buf.size == v.lo + 7 * 18 + v.hi
        assert v.lo * es >= 1 << 20 and v.hi * es >= 1 << 20 and (v.lo * es) % 16 == 0
    assert np.isnan(V.decode(inp.buf, dt)).all() and (inp.buf.view(np.uint8)[: es] != 0).any()
    assert (out.buf.view(np.uint8) == 0xA5).all() and np.isfinite(V.decode(out.buf, dt)).all()
    vals = np.arange(70, dtype=np.float64).reshape(7, 10) - 30
    inp.put(vals)
    assert np.array_equal(V.decode(inp.window(), dt), vals)
    flat = V.decode(inp.buf, dt)
    assert flat[inp.off] == -30 and flat[inp.off + 18 + 1] == -19 and np.isnan(flat[inp.off - 1]) and np.isnan(flat[inp.off + 10])
    assert int((~np.isnan(flat)).sum()) == 70  # everything that is not the window is poison
    p = inp.packed()
    assert p.ld == 10 and p.off == p.lo > 0 and np.array_equal(V.decode(p.window(), dt), vals)
    after = out.buf.copy()
    out.window(after)[...] = V.encode(vals, dt)
    V.check_output(out, after, vals)
    for spot in (0, out.off - 1, out.off + 10, out.buf.size - 1):  # a guard, the column before the window, the gap behind it
        bad = after.copy()
        bad.view(np.uint8)[spot * es] ^= 1
        with pytest.raises(AssertionError, match="sentinel"):
            V.check_output(out, bad, vals)


def test_codecs_round_to_nearest_even_and_keep_the_draw_exact():
    x = np.array([1.0, -0.5, 123.5, 255.0, 256.0, 1.00390625, 1.01171875, 2047.0, 0.0])
    assert np.array_equal(V.decode(V.encode(x[:5], "bf16"), "bf16"), x[:5])
    assert V.decode(V.encode(x[5:6], "bf16"), "bf16")[0] == 1.0          # 1 + 2^-8: a tie, to the even neighbour
    assert V.decode(V.encode(x[6:7], "bf16"), "bf16")[0] == 1.015625     # 1 + 3 * 2^-8: a tie, to the even neighbour 1 + 2^-6
    assert np.array_equal(V.decode(V.encode(x, "f16"), "f16")[[0, 1, 2, 7]], x[[0, 1, 2, 7]])
    assert V.decode(V.encode(np.array([257.0]), "bf16"), "bf16")[0] != 257.0  # what the exactness assertion of a case guards against
    assert np.isnan(V.decode(V.encode(np.array([np.nan]), "bf16"), "bf16")[0])


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_model_with_true_pitches_is_the_expected_value(row):
    for ta, tb in LAYOUTS:
        for epilogue in (0, 1):
            c = make(row, ta, tb, epilogue)
            assert len({c.a.ld, c.b.ld, c.c.ld}) == 3, "the three pitches of one call must differ"
            assert np.abs(c.want).max() >= 8  # (not a degenerate draw)
            V.check_output(c.c, V.model_product(c), c.want)


def mistakes(c):
    """name -> model_product arguments of one classic pitch mistake."""
    return {
        "lda is the extent": dict(lda=c.a.cols),
        "ldb is the extent": dict(ldb=c.b.cols),
        "lda and ldb swapped": dict(lda=c.b.ld, ldb=c.a.ld),
        "A's pitch on the wrong axis": dict(a_axes_swapped=True),
        "B's pitch on the wrong axis": dict(b_axes_swapped=True),
        "A's column offset dropped": dict(a_off=c.a.off - c.a.c0),
        "B's column offset dropped": dict(b_off=c.b.off - c.b.c0),
        "ldc is N": dict(ldc=c.N),
    }


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_every_pitch_mistake_is_rejected(row):
    for ta, tb in LAYOUTS:
        for epilogue in (0, 1):
            c = make(row, ta, tb, epilogue)
            for name, kw in mistakes(c).items():
                with pytest.raises(AssertionError, match="NaN|differ|sentinel"):
                    V.check_output(c.c, V.model_product(c, **kw), c.want)
                    pytest.fail(f"{name} passed the check: {row} ta={ta} tb={tb} epilogue={epilogue}", pytrace=False)


def test_each_kind_of_rejection_occurs():
    """The three ways the check can fail are all exercised by the mistakes above: NaN, a wrong integer, a damaged sentinel."""
    c = make(ROWS[6], 0, 0, 0)
    kinds = {}
    for name, kw in mistakes(c).items():
        with pytest.raises(AssertionError) as e:
            V.check_output(c.c, V.model_product(c, **kw), c.want)
        kinds[name] = str(e.value)
    assert "NaN" in kinds["lda is the extent"] and "NaN" in kinds["A's column offset dropped"]
    assert "sentinel" in kinds["ldc is N"] or "differ" in kinds["ldc is N"]
    # a wrong pitch on C alone moves correct values: caught by the window and by the sentinel, not by NaN
    after = V.model_product(c, ldc=c.N)
    assert not c.c.outside_intact(after)
    # wrong integers without any NaN: B walked with its pitch on the other axis, on a square packed operand (no gap to run into)
    sq = V.Case("bf16", 0, 0, 128, 128, 128, {"a": (0, 0), "b": (0, 0), "c": (8, 8)}, seed=5)
    with pytest.raises(AssertionError, match="differ"):
        V.check_output(sq.c, V.model_product(sq, b_axes_swapped=True), sq.want)


def test_dispatch_restated_matches_the_labels_the_suite_already_pins():
    """expected_labels against labels that tests/test_gpu_gemm.py asserts on packed operands."""
    L = lambda dt, M, N, K, **kw: V.expected_labels(dt, 0, 0, M, N, K, K, N, True, True, **kw)  # noqa: E731
    assert L("f32", 256, 384, 64) == {"gemm_f32_mfma_t64"} and L("f32", 2048, 2048, 32) == {"gemm_f32_mfma"}
    assert L("f64", 128, 192, 48) == {"gemm_f64_mfma"} and L("bf16", 256, 384, 128) == {"gemm_bf16_mfma_128"}
    assert L("bf16", 2560, 4096, 128) == {"gemm_bf16_mfma"} and L("f16", 2560, 4096, 64, tail=True) == {"gemm_f16_mfma"}
    assert L("bf16", 100, 130, 70) == {"gemm_generic"} and L("f32", 33, 65, 17) == {"gemm_generic"}
    assert V.splitk_slices("bf16", 256, 384, 4096) == 8
    assert L("bf16", 256, 384, 4096, workspace=True) == {"gemm_bf16_mfma_128_splitk"} and L("bf16", 256, 384, 4096) == {"gemm_bf16_mfma_128"}
    assert L("f16", 300, 520, 700, workspace=True) == {"gemm_pad", "gemm_f16_mfma_128"} and L("f16", 300, 520, 700) == {"gemm_generic"}
    assert L("f32", 192, 128, 1001, workspace=True) == {"gemm_pad", "gemm_f32_mfma_t64"}
    assert L("bf16", 250, 384, 1024, workspace=True) == {"gemm_pad", "gemm_bf16_mfma_128_splitk"}
    # the pitch and base predicates
    assert V.expected_labels("bf16", 0, 0, 128, 128, 64, 68, 128, True, True) == {"gemm_generic"}
    assert V.expected_labels("bf16", 0, 0, 128, 128, 64, 72, 128, False, True) == {"gemm_generic"}
    assert V.expected_labels("f32", 0, 0, 128, 192, 48, 50, 192, True, True) == {"gemm_generic"}
    assert V.expected_labels("f64", 0, 0, 128, 192, 80, 81, 192, True, True) == {"gemm_generic"}
