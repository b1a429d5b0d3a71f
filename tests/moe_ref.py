"""numpy reference of the mixture-of-experts routing entries (kf_moe_plan, kf_moe_gate_fwd / _bwd, kf_moe_dispatch, kf_moe_combine,
kf_moe_combine_bwd), restating include/kfunca_hip.h. n = T k, pair p = t k + j is token t's j-th choice.

Values travel as float64 arrays that hold numbers representable in the storage type dt ("f32", "bf16", "f16"). With exact=False a
function does what the kernels do: f32 arithmetic in the stated order, one rounding to dt at the store. With exact=True it evaluates the
same formula in f64 without any rounding, for the tests' error bounds. Nothing here touches a GPU."""
import numpy as np

from tests import gemm_views as V

INT64_MIN = -(1 << 63)
BAD_IDS = (-1, None, 1 << 40, INT64_MIN)   # None stands for E itself
H = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -23}   # half an ulp of the store (f32: one ulp of slack, as tests/test_gpu_gemm_seg.py)


def rnd(x, dt):
    """Round to the storage type (nearest even), back as float64."""
    return V.decode(V.encode(np.asarray(x, dtype=np.float64), dt), dt)


def keys_of(ids, E):
    """key_p = ids[p] if 0 <= ids[p] < E else E: a pair with the key E is dropped."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return np.where((ids >= 0) & (ids < E), ids, E).astype(np.int64)


def plan(ids, E):
    """(offsets int64 [E + 1], row_pair int32 [n], pair_row int32 [n]): the stable ascending sort of the pairs by key."""
    keys = keys_of(ids, E)
    n = keys.size
    row_pair = np.argsort(keys, kind="stable").astype(np.int32)
    pair_row = np.empty(n, dtype=np.int32)
    pair_row[row_pair] = np.arange(n, dtype=np.int32)
    offsets = np.array([(keys < e).sum() for e in range(E + 1)], dtype=np.int64)
    return offsets, row_pair, pair_row


def _chosen(p, ids, E, ft):
    """s[t, j] = p[t, ids[t, j]], 0 for a dropped pair; ok[t, j]: the pair is not dropped."""
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < E)
    s = np.where(ok, np.take_along_axis(np.asarray(p, dtype=ft), np.where(ok, ids, 0), axis=1), ft(0))
    return s.astype(ft), ok


def _seq_sum(terms, ft):
    """sum over the last axis from +0 in index order, in ft."""
    acc = np.zeros(terms.shape[:-1], dtype=ft)
    for j in range(terms.shape[-1]):
        acc = (acc + terms[..., j]).astype(ft)
    return acc


def gate_fwd(p, ids, E, normalize, dt, exact=False):
    ft = np.float64 if exact else np.float32
    s, _ = _chosen(p, ids, E, ft)
    if normalize:
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (s / _seq_sum(s, ft)[:, None]).astype(ft)
    return s.astype(np.float64) if exact else rnd(s, dt)


def gate_bwd(p, ids, E, normalize, gate, dgate, dt, exact=False):
    """dp [T, E]: zeros, then dp[t, ids[t, j]] += ds_j in the order j; ds_j = dgate_j or (dgate_j - sum_i dgate_i gate_i) / S, the sum
    over the pairs that are not dropped."""
    ft = np.float64 if exact else np.float32
    ids = np.asarray(ids, dtype=np.int64)
    T, k = ids.shape
    s, ok = _chosen(p, ids, E, ft)
    dg, g = np.asarray(dgate, dtype=ft), np.asarray(gate, dtype=ft)
    if normalize:
        S = _seq_sum(s, ft)
        dot = _seq_sum(np.where(ok, (dg * g).astype(ft), ft(0)), ft)
        with np.errstate(divide="ignore", invalid="ignore"):
            ds = ((dg - dot[:, None]).astype(ft) / S[:, None]).astype(ft)
    else:
        ds = dg
    dp = np.zeros((T, E), dtype=ft)
    rows = np.arange(T)
    for j in range(k):
        m = ok[:, j]
        dp[rows[m], ids[m, j]] = (dp[rows[m], ids[m, j]] + ds[m, j]).astype(ft)
    return dp.astype(np.float64) if exact else rnd(dp, dt)


def dispatch(x, row_pair, k):
    """xs[r] = x[row_pair[r] // k]; an entry outside [0, n) gives a row of +0."""
    x = np.asarray(x, dtype=np.float64)
    rp = np.asarray(row_pair, dtype=np.int64)
    ok = (rp >= 0) & (rp < rp.size)
    xs = np.zeros((rp.size, x.shape[1]))
    xs[ok] = x[rp[ok] // k]
    return xs


def _live(n_valid, n):
    return n if n_valid is None else min(max(int(n_valid), 0), n)


def combine(ys, pair_row, n_valid, gate, T, k, dt, exact=False):
    """(y, bound): y[t] = sum_j gate[t, j] ys[pair_row[t, j]] from +0 in the order j over the pairs with 0 <= pair_row < n_valid;
    bound[t] = sum_j |gate ys| over the same pairs (the scale of the f32 error bound)."""
    ft = np.float64 if exact else np.float32
    ys = np.asarray(ys, dtype=ft)
    pr = np.asarray(pair_row, dtype=np.int64).reshape(T, k)
    live = _live(n_valid, T * k)
    acc, mag = np.zeros((T, ys.shape[1]), dtype=ft), np.zeros((T, ys.shape[1]))
    for j in range(k):
        m = (pr[:, j] >= 0) & (pr[:, j] < live)
        g = np.ones(T, dtype=ft) if gate is None else np.asarray(gate, dtype=ft)[:, j]
        term = (g[m, None] * ys[pr[m, j]]).astype(ft)
        acc[m] = (acc[m] + term).astype(ft)
        mag[m] += np.abs(term.astype(np.float64))
    return (acc.astype(np.float64) if exact else rnd(acc, dt)), mag


def combine_bwd(ys, pair_row, n_valid, gate, dy, T, k, dt, want_dgate=True, fill=np.nan, exact=False):
    """(dys, dgate, bound). dys starts as `fill`: a row that no table entry names keeps it. For pair (t, j) with r = pair_row in [0, n):
    dys[r] = gate dy[t] (live), dy[t] (no gate), +0 (r >= n_valid). dgate[t, j] = sum_c dy[t, c] ys[r, c] for a live pair, else +0,
    here in f64 (the kernel's order of that sum is its own: the tests bound it); bound = sum_c |dy ys|."""
    ft = np.float64 if exact else np.float32
    dy = np.asarray(dy, dtype=ft)
    pr = np.asarray(pair_row, dtype=np.int64).reshape(T, k)
    n, live = T * k, _live(n_valid, T * k)
    dys = np.full((n, dy.shape[1]), fill, dtype=np.float64)
    dgate, mag = np.zeros((T, k)), np.zeros((T, k))
    for t in range(T):
        for j in range(k):
            r = pr[t, j]
            if r < 0 or r >= n:
                continue
            if r >= live:
                dys[r] = 0.0
                continue
            if gate is None:
                dys[r] = dy[t]
            else:
                out = (ft(np.asarray(gate)[t, j]) * dy[t]).astype(ft)
                dys[r] = out if exact else rnd(out, dt)
            if want_dgate:
                prod = dy[t].astype(np.float64) * np.asarray(ys, dtype=np.float64)[r]
                dgate[t, j], mag[t, j] = prod.sum(), np.abs(prod).sum()
    return dys, (dgate if want_dgate else None), mag
