"""CPU-only: the bounds of tests/moe_router_ref.py hold for an honest f32 evaluation and reject wrong formulas, on the very draws
tests/test_gpu_moe_router.py uses (and on U(-30, 30) logits beside them).

The f32 restatement below follows the formulas of the header with every operation rounded to f32. Sums over the k choices and over the
tokens are sequential; sums over the E experts keep 64 sequential partial sums and add them in a tree (lane_sum), the least accurate
order the bounds' c = ceil(E / 64) + 16 admits. Two things are asserted on every case:

  * the restatement, rounded to the dtype as the device stores it, meets every bound;
  * before that last rounding its error, less 2^-18 |ref| (what the rounding of l - m alone costs, see fraction()), is at most HALF
    of the bound's absolute part alone (the part that does not scale with |ref|): the bounds leave room for another summation order and
    for the device's exp2 / log2, and are not met by accident.

Worst fractions measured here (the maximum over all cases, dtypes, draws, scores and both normalize values; `pytest -s` prints them per
case): gate 0.00 of 1e-6, router dlogits 0.01, aux dlogits 0.24 of the absolute part; the losses, whose bound 2^-16 |ref| is purely
relative, 0.20 of it (T = 4099 added sequentially). No constant of the bounds had to be widened.

Mutants, each of which must break at least one bound on these draws: a tie broken to the higher index; -0.0 taken as equal to +0.0; the
normalisation over all E instead of the chosen k; the -sum_u a_u p_u term dropped; HF's factor k on L_bal; lse without the row maximum;
the z gradient without its factor 2."""
import numpy as np
import pytest

from tests import moe_router_ref as R

f32 = np.float32
WORST = {"gate": 0.0, "router_bwd": 0.0, "aux_bwd": 0.0, "loss": 0.0}


def seq_sum(a, axis=-1):
    """The sequential f32 sum along an axis, keepdims."""
    a = np.asarray(a, f32)
    return np.take(np.cumsum(a, axis=axis, dtype=f32), [-1], axis=axis)


def lane_sum(a):
    """The f32 sum over the last axis as 64 sequential partial sums (element e in partial e % 64) and a pairwise tree over them, keepdims:
    the least accurate order the bounds' c = ceil(E / 64) + 16 admits."""
    a = np.asarray(a, f32)
    n = a.shape[-1]
    pad = np.zeros(a.shape[:-1] + ((-n) % 64,), f32)
    part = np.cumsum(np.concatenate([a, pad], axis=-1).reshape(a.shape[:-1] + (-1, 64)), axis=-2, dtype=f32)[..., -1, :]
    while part.shape[-1] > 1:
        part = (part[..., 0::2] + part[..., 1::2]).astype(f32)
    return part


def stored(v, code):
    """An f32 result as the device stores it: one rounding to the dtype, read back exactly."""
    return R.floats(R.bits(v, code), code)


# ---- the f32 restatement ------------------------------------------------------------------------------------------------------------
def select_f32(b, code, k, mutant=None):
    if mutant == "zero_equal":          # the comparison on values: -0.0 == +0.0
        neg0 = R.bits(np.array([-0.0]), code)[0]
        b = np.where(b == neg0, np.zeros_like(b), b)
    key = R.ordered_keys(b, code)
    if mutant == "tie_high":
        E = b.shape[1]
        order = np.argsort((~key)[:, ::-1], axis=-1, kind="stable")
        return (E - 1 - order)[:, :k].astype(np.int64)
    return np.argsort(~key, axis=-1, kind="stable")[:, :k].astype(np.int64)


def state_f32(x):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=-1, keepdims=True)
        e = np.exp((x - m).astype(f32)).astype(f32)
        Z = lane_sum(e)
        return m, e, Z


def score_f32(x, score):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if score == R.SOFTMAX:
            m, e, Z = state_f32(x)
            return (e / Z).astype(f32), None
        one = f32(1.0)
        return (one / (one + np.exp(-x).astype(f32))).astype(f32), (one / (one + np.exp(x).astype(f32))).astype(f32)


def gate_f32(x, ids, score, normalize, mutant=None):
    s, _ = score_f32(x, score)
    sj = np.take_along_axis(s, ids, axis=-1)
    if not normalize:
        return sj
    with np.errstate(invalid="ignore", divide="ignore"):
        return (sj / (lane_sum(s) if mutant == "norm_all_E" else seq_sum(sj))).astype(f32)


def router_bwd_f32(x, ids, dg, score, normalize):
    T, E = x.shape
    s, q = score_f32(x, score)
    sj = np.take_along_axis(s, ids, axis=-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if normalize:
            Sm = seq_sum(sj)
            D = seq_sum(dg * (sj / Sm).astype(f32))
            c = ((dg - D).astype(f32) / Sm).astype(f32)
            sub = f32(0.0)
        else:
            c = dg
            sub = seq_sum(dg * sj) if score == R.SOFTMAX else f32(0.0)
        if score == R.SIGMOID:
            c = ((c * sj).astype(f32) * np.take_along_axis(q, ids, axis=-1)).astype(f32)
        G = np.zeros((T, E), f32)
        for j in range(ids.shape[1]):
            G[np.arange(T), ids[:, j]] += c[:, j]
        return (s * (G - sub).astype(f32)).astype(f32) if score == R.SOFTMAX else G


def aux_f32(x, counts, k, bc, zc, dloss, mutant=None):
    """(loss, L_bal, L_z, dlogits) in f32 with sequential sums over tokens and over experts."""
    T, E = x.shape
    m, e, Z = state_f32(x)
    p = (e / Z).astype(f32)
    logZ = np.log(Z).astype(f32)
    lse = logZ if mutant == "lse_no_max" else (m + logZ).astype(f32)
    col = seq_sum(p, axis=0)[0]
    c = counts.astype(f32)
    l_bal = f32(seq_sum(c * col)[0] * f32(E / (float(T) * T * k)))
    if mutant == "hf_k":
        l_bal = f32(l_bal * f32(k))
    l_z = f32(seq_sum((lse * lse).astype(f32), axis=0)[0, 0] * f32(1.0 / T))
    loss = f32(f32(bc) * l_bal + f32(zc) * l_z)
    a = (f32(float(f32(bc)) * E / (float(T) * T * k)) * c)[None, :]
    zt = (f32(float(f32(zc)) * (1.0 if mutant == "z_no_2" else 2.0) / T) * lse).astype(f32)
    A = f32(0.0) if mutant == "drop_sum" else lane_sum(a * p)
    dl = ((f32(dloss) * p).astype(f32) * ((a - A).astype(f32) + zt).astype(f32)).astype(f32)
    return float(loss), float(l_bal), float(l_z), dl


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
REL = 2.0 ** -18


def fraction(err, absolute, ref):
    """The largest (err - REL |ref|) / absolute. REL |ref| is what the rounding of l - m alone costs: the difference of two stored logits is
    not always an f32 (22 - 1.9e-4 in bf16 is not), its rounding is |l - m| 2^-24 of the exponential and so of the result, and |l - m| < 64
    on these draws. It is a quarter of the f32 R and 2^-10 of the bf16 R. 2^-150 is the restatement's own rounding where an f32 is subnormal."""
    if not np.size(err):
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(absolute > 0, np.maximum(err - REL * np.abs(ref) - 2.0 ** -150, 0.0) / absolute, 0.0)))


def router_case(code, T, E, k, draw):
    rng = np.random.default_rng(R.seed_of(T, E, k, code, draw))
    b = R.draw_logits(rng, draw, code, T, E)
    dgb = R.draw_dgate(rng, code, T, k)
    return b, R.floats(b, code), R.floats(dgb, code)


@pytest.mark.parametrize("code", R.CODES, ids=[R.CODE_NAME[c] for c in R.CODES])
@pytest.mark.parametrize("T,E,k", R.ROUTER_SHAPES)
def test_the_restated_router_meets_the_bounds(code, T, E, k):
    for draw in R.DRAWS + ("uniform",):
        b, x, dg = router_case(code, T, E, k, draw)
        ids = R.select(b, code, k)
        assert np.array_equal(select_f32(b, code, k), ids)
        if draw == "equal":
            assert np.array_equal(ids, np.tile(np.arange(k), (T, 1)))
        fin = R.finite_rows(b, code)
        x32, dg32 = x.astype(f32), dg.astype(f32)
        for score in R.SCORES:
            for normalize in (False, True):
                ref = R.gate(x, ids, score, normalize)
                got = gate_f32(x32, ids, score, normalize).astype(np.float64)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (draw, score, normalize)
                err = np.abs(got - ref)[fin]
                WORST["gate"] = max(WORST["gate"], fraction(err, np.full_like(err, 1e-6), ref[fin]))
                assert fraction(err, np.full_like(err, 1e-6), ref[fin]) <= 0.5
                assert (np.abs(stored(got, code) - ref)[fin] <= R.gate_bound(code, ref)[fin]).all(), (draw, score, normalize)

                ref = R.router_backward(x, ids, dg, score, normalize)
                got = router_bwd_f32(x32, ids, dg32, score, normalize).astype(np.float64)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), (draw, score, normalize)
                absolute = R.router_backward_bound(code, E, k, dg, np.zeros_like(ref))
                err = np.abs(got - ref)[fin]
                WORST["router_bwd"] = max(WORST["router_bwd"], fraction(err, absolute[fin], ref[fin]))
                assert fraction(err, absolute[fin], ref[fin]) <= 0.5, (draw, score, normalize)
                assert (np.abs(stored(got, code) - ref)[fin] <= R.router_backward_bound(code, E, k, dg, ref)[fin]).all(), (draw, score, normalize)


def aux_case(code, T, E, k, plan, draw):
    rng = np.random.default_rng(R.seed_of(T, E, k, code, plan, draw))
    b = R.draw_logits(rng, draw, code, T, E)
    ids = R.draw_plan_ids(rng, T, E, k, plan)
    return b, R.floats(b, code), ids, R.counts_of(ids, E)


@pytest.mark.parametrize("code", R.CODES, ids=[R.CODE_NAME[c] for c in R.CODES])
@pytest.mark.parametrize("T,E,k,plan", R.AUX_SHAPES)
def test_the_restated_aux_loss_meets_the_bounds(code, T, E, k, plan):
    for draw in ("normal", "ties", "uniform"):
        b, x, ids, counts = aux_case(code, T, E, k, plan, draw)
        if plan == "empty" and E > 1:
            assert (counts == 0).any()
        if plan == "dropped":
            assert counts.sum() < T * k
        for bc, zc in R.AUX_COEFS:
            want = R.aux_forward(x, counts, k, bc, zc)
            loss, l_bal, l_z, dl = aux_f32(x.astype(f32), counts, k, bc, zc, R.AUX_DLOSS)
            for got, ref in zip((loss, l_bal, l_z), want):
                assert abs(got - ref) <= R.loss_bound(ref), (draw, bc, zc, got, ref)
                if ref:
                    WORST["loss"] = max(WORST["loss"], abs(got - ref) / R.loss_bound(ref))
            ref = R.aux_backward(x, counts, k, bc, zc, R.AUX_DLOSS)
            absolute = R.aux_backward_bound(code, x, counts, k, bc, zc, R.AUX_DLOSS, np.zeros_like(ref))
            err = np.abs(dl.astype(np.float64) - ref)
            WORST["aux_bwd"] = max(WORST["aux_bwd"], fraction(err, absolute, ref))
            assert fraction(err, absolute, ref) <= 0.5, (draw, bc, zc)
            assert (np.abs(stored(dl, code) - ref) <= R.aux_backward_bound(code, x, counts, k, bc, zc, R.AUX_DLOSS, ref)).all(), (draw, bc, zc)
    print("worst fractions so far:", {n: round(v, 3) for n, v in WORST.items()})


# ---- the mutants --------------------------------------------------------------------------------------------------------------------
def test_selection_mutants_are_rejected():
    code = R.BF16
    b, _, _ = router_case(code, 257, 128, 8, "ties")
    assert not np.array_equal(select_f32(b, code, 8, "tie_high"), R.select(b, code, 8))
    b, _, _ = router_case(code, 257, 8, 8, "special")
    assert not np.array_equal(select_f32(b, code, 8, "zero_equal"), R.select(b, code, 8))


@pytest.mark.parametrize("code", R.CODES, ids=[R.CODE_NAME[c] for c in R.CODES])
def test_normalising_over_all_experts_is_rejected(code):
    T, E, k = 257, 128, 8
    b, x, _ = router_case(code, T, E, k, "normal")
    ids = R.select(b, code, k)
    for score in R.SCORES:
        ref = R.gate(x, ids, score, True)
        got = stored(gate_f32(x.astype(f32), ids, score, True, "norm_all_E"), code)
        assert (np.abs(got - ref) > R.gate_bound(code, ref)).any(), score


@pytest.mark.parametrize("code", R.CODES, ids=[R.CODE_NAME[c] for c in R.CODES])
@pytest.mark.parametrize("mutant,coefs,what", [("drop_sum", (1e-2, 0.0), "dl"), ("hf_k", (1e-2, 0.0), "loss"), ("lse_no_max", (0.0, 1e-3), "loss"),
                                               ("z_no_2", (0.0, 1e-3), "dl")])
def test_aux_mutants_are_rejected(code, mutant, coefs, what):
    T, E, k, plan = 1027, 8, 2, "dropped"
    b, x, ids, counts = aux_case(code, T, E, k, plan, "normal")
    bc, zc = coefs
    loss, l_bal, l_z, dl = aux_f32(x.astype(f32), counts, k, bc, zc, R.AUX_DLOSS, mutant)
    want = R.aux_forward(x, counts, k, bc, zc)
    if what == "loss":
        assert abs(loss - want[0]) > R.loss_bound(want[0])
    else:
        ref = R.aux_backward(x, counts, k, bc, zc, R.AUX_DLOSS)
        assert (np.abs(stored(dl, code) - ref) > R.aux_backward_bound(code, x, counts, k, bc, zc, R.AUX_DLOSS, ref)).any()
