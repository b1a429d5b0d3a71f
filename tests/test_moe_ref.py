"""CPU-only: tests/moe_ref.py checked against itself and against torch. The plan on a grid of (T, k, E) with k = 1, E = 1, every pair to
one expert, empty experts and ids outside [0, E): row_pair is a permutation, pair_row its inverse, keys ascend along the rows with equal
keys in pair order, dropped pairs sit at the tail, offsets are tests/gemm_seg_ref.segment_offsets of the sorted keys. The four backward
formulas (gate, dispatch, combine in ys and in gate) equal torch-CPU autograd in f64 on the same layer written with torch indexing,
with normalize on and off, a token with two equal ids and a token with every pair dropped."""
import numpy as np
import pytest
import torch

from tests import gemm_seg_ref as R
from tests import moe_ref as M

GRID = [(1, 1, 1), (7, 1, 1), (5, 3, 1), (9, 1, 4), (16, 2, 8), (33, 3, 5), (12, 8, 8), (64, 2, 128), (40, 4, 3)]


def draw_ids(rng, T, k, E, mode):
    if mode == "uniform":
        return rng.integers(0, E, (T, k)).astype(np.int64)
    if mode == "one expert":
        return np.full((T, k), E - 1, dtype=np.int64)
    if mode == "empty experts":
        return (rng.integers(0, max(E // 2, 1), (T, k)) * 2 % E).astype(np.int64)
    ids = rng.integers(0, E, (T, k)).astype(np.int64)   # "bad": every fourth pair outside [0, E)
    flat = ids.reshape(-1)
    bad = [E if b is None else b for b in M.BAD_IDS]
    for i in range(0, flat.size, 4):
        flat[i] = bad[(i // 4) % len(bad)]
    return ids


@pytest.mark.parametrize("mode", ["uniform", "one expert", "empty experts", "bad"])
@pytest.mark.parametrize("T,k,E", GRID)
def test_plan(T, k, E, mode):
    rng = np.random.default_rng(T * 131 + k * 17 + E)
    ids = draw_ids(rng, T, k, E, mode)
    n = T * k
    offsets, row_pair, pair_row = M.plan(ids, E)
    assert row_pair.dtype == np.int32 and pair_row.dtype == np.int32 and offsets.dtype == np.int64
    assert np.array_equal(np.sort(row_pair), np.arange(n))
    assert np.array_equal(pair_row[row_pair], np.arange(n)) and np.array_equal(row_pair[pair_row], np.arange(n))
    keys = M.keys_of(ids, E)
    sk = keys[row_pair]
    assert (np.diff(sk) >= 0).all()
    same = np.diff(sk) == 0
    assert (np.diff(row_pair)[same] > 0).all()          # equal keys keep pair order
    n_valid = int((keys < E).sum())
    assert (sk[:n_valid] < E).all() and (sk[n_valid:] == E).all()
    assert np.array_equal(row_pair[n_valid:], np.flatnonzero(keys == E))   # the dropped pairs, in pair order
    assert np.array_equal(offsets, R.segment_offsets(sk, E))
    assert offsets[0] == 0 and offsets[E] == n_valid
    if mode == "bad":
        assert n_valid < n


def test_plan_of_nothing():
    offsets, row_pair, pair_row = M.plan(np.zeros((0, 2), np.int64), 3)
    assert np.array_equal(offsets, np.zeros(4, np.int64)) and row_pair.size == 0 and pair_row.size == 0


def layer_inputs(seed, T=6, k=3, E=5, d=4):
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, E, (T, k)).astype(np.int64)
    ids[1] = [2, 2, 4]                      # two equal ids in one token
    ids[3] = [-1, E, 1 << 40]               # every pair dropped
    ids[4, 1] = M.INT64_MIN                 # one pair dropped
    p = rng.uniform(0.05, 1.0, (T, E))
    return ids, p, rng.normal(size=(T, d)), rng.normal(size=(T * k, d)), rng.normal(size=(T, k)), rng.normal(size=(T, d)), rng


def torch_gate(p, ids, E, normalize):
    ok = (ids >= 0) & (ids < E)
    s = torch.where(ok, p.gather(1, torch.where(ok, ids, torch.zeros_like(ids))), torch.zeros((), dtype=p.dtype))
    return s / s.sum(1, keepdim=True) if normalize else s


@pytest.mark.parametrize("normalize", [False, True])
def test_gate_backward_is_autograd(normalize):
    ids, p, *_, dgate, _, _ = layer_inputs(3)
    T, k = ids.shape
    E = p.shape[1]
    tp = torch.tensor(p, requires_grad=True)
    g = torch_gate(tp, torch.tensor(ids), E, normalize)
    ref = M.gate_fwd(p, ids, E, normalize, "f32", exact=True)
    live = ~np.isnan(ref)
    assert np.allclose(g.detach().numpy()[live], ref[live], rtol=1e-14, atol=0)
    assert normalize == bool(np.isnan(ref[3]).all())      # the token with every pair dropped: 0 / 0 when normalised
    tg = torch.tensor(dgate)
    g.backward(tg)
    dp = M.gate_bwd(p, ids, E, normalize, np.nan_to_num(ref), dgate, "f32", exact=True)
    want = tp.grad.numpy()
    assert not dp[3].any() and not np.isnan(dp[[0, 1, 2, 4, 5]]).any()
    rows = [0, 1, 2, 4, 5]
    assert np.allclose(dp[rows], want[rows], rtol=1e-12, atol=1e-14)
    assert not np.nan_to_num(want[3]).any()
    off = np.ones_like(dp, dtype=bool)
    for t in range(T):
        for j in range(k):
            if 0 <= ids[t, j] < E:
                off[t, ids[t, j]] = False
    assert not dp[off].any()


def test_dispatch_and_combine_backwards_are_autograd():
    ids, p, x, ys, gate, dy, rng = layer_inputs(11)
    T, k = ids.shape
    E, n = p.shape[1], T * k
    offsets, row_pair, pair_row = M.plan(ids, E)
    n_valid = int(offsets[E])
    trp, tpr = torch.tensor(row_pair.astype(np.int64)), torch.tensor(pair_row.astype(np.int64)).reshape(T, k)

    # dispatch: xs = x[row_pair // k]; its backward is the combine without a gate over ALL rows
    tx = torch.tensor(x, requires_grad=True)
    txs = tx[trp // k]
    assert np.array_equal(txs.detach().numpy(), M.dispatch(x, row_pair, k))
    dxs = rng.normal(size=(n, x.shape[1]))
    txs.backward(torch.tensor(dxs))
    dx, _ = M.combine(dxs, pair_row, None, None, T, k, "f32", exact=True)
    assert np.allclose(dx, tx.grad.numpy(), rtol=1e-13, atol=1e-15)

    # combine: y[t] = sum over the live pairs of gate ys[pair_row]
    for with_gate in (True, False):
        tys = torch.tensor(ys, requires_grad=True)
        tg = torch.tensor(gate, requires_grad=True)
        live = (tpr < n_valid).to(torch.float64)
        w = (tg if with_gate else torch.ones_like(tg)) * live
        ty = (w[:, :, None] * tys[tpr]).sum(1)
        y, _ = M.combine(ys, pair_row, n_valid, gate if with_gate else None, T, k, "f32", exact=True)
        assert np.allclose(y, ty.detach().numpy(), rtol=1e-13, atol=1e-15)
        assert not y[3].any()                                  # the token with no live pair
        ty.backward(torch.tensor(dy))
        dys, dgate, _ = M.combine_bwd(ys, pair_row, n_valid, gate if with_gate else None, dy, T, k, "f32", want_dgate=with_gate, exact=True)
        assert not np.isnan(dys).any()                         # a permutation names every row
        assert np.allclose(dys, tys.grad.numpy(), rtol=1e-13, atol=1e-15)
        assert not dys[n_valid:].any()
        if with_gate:
            assert np.allclose(dgate, tg.grad.numpy(), rtol=1e-12, atol=1e-14)
            assert not dgate[3].any() and dgate[4, 1] == 0


def test_rounding_and_malformed_tables():
    """The rounded evaluation: bf16 products are exact in f32, so y is the f32 sum in the order j rounded once; table entries outside
    [0, n) name no row (dys keeps its fill, y skips them, dispatch writes +0)."""
    rng = np.random.default_rng(5)
    T, k, d = 4, 2, 3
    ys, gate, dy = M.rnd(rng.normal(size=(T * k, d)), "bf16"), M.rnd(rng.normal(size=(T, k)), "bf16"), M.rnd(rng.normal(size=(T, d)), "bf16")
    pr = np.arange(T * k, dtype=np.int32)
    pr[2], pr[5] = T * k + 3, -5
    y, _ = M.combine(ys, pr, None, gate, T, k, "bf16")
    want = np.zeros((T, d), dtype=np.float32)
    for t in range(T):
        for j in range(k):
            if 0 <= pr[t * k + j] < T * k:
                want[t] = want[t] + np.float32(gate[t, j]) * ys[pr[t * k + j]].astype(np.float32)
    assert np.array_equal(y, M.rnd(want, "bf16"))
    dys, dgate, _ = M.combine_bwd(ys, pr, None, gate, dy, T, k, "bf16")
    assert np.isnan(dys[[2, 5]]).all() and not np.isnan(np.delete(dys, [2, 5], axis=0)).any()
    assert dgate[1, 0] == 0 and dgate[2, 1] == 0
    xs = M.dispatch(dy, pr, k)
    assert not xs[[2, 5]].any() and np.array_equal(xs[3], dy[1])
