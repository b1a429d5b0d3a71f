"""The f64 numpy reference of the fused mixture-of-experts router (kf_moe_router_fwd / kf_moe_router_bwd) and of the auxiliary losses
(kf_moe_aux_loss_fwd / kf_moe_aux_loss_bwd), the bounds the device results are held to, and the draws of tests/test_gpu_moe_router.py
(shared with tests/test_moe_router_ref.py, which checks on the CPU that an f32 restatement meets the bounds on those very draws and that
wrong formulas do not).

The reference takes the STORED logits (16-bit values widened exactly). With l a row of logits:

    selection   ids = the first k positions of the stable descending order of the row in the sort's key order: the stored bits mapped to
                unsigned keys (the sign bit of a non-negative flipped, every bit of a negative), so -0.0 < +0.0 and NaNs sort by bit
                pattern; equal keys by lower index first. No arithmetic: exact.
    gate        softmax: s_j = exp(l_(ids_j) - m) / Z; sigmoid: s_j = 1 / (1 + exp(-l_(ids_j))); gate_j = s_j or s_j / sum_i s_i
    dlogits     the exact derivative of that gate contracted with dgate; an id outside [0, E) is in no sum
    aux         p = softmax(l), L_bal = E / (T k) sum_e c_e mean_t p[t, e], L_z = mean_t lse_t^2, loss = bc L_bal + zc L_z
                dlogits[t, e] = dloss p_e (a_e - sum_u a_u p_u + z_t), a_e = bc E c_e / (T^2 k), z_t = zc 2 lse_t / T

Bounds, with R = softmax_ref.OUT_R (one output rounding, 2^-16 for f32), H = softmax_ref.OUT_HALF_SPACING and c = ceil(E / 64) + 16 (the
first-order bound of a summation that keeps at least 64 partial sums and then a tree):

    gate             |err| <= R |ref| + 1e-6                                                          (softmax_ref's forward bound)
    router dlogits   |err| <= R |ref| + 4 (c + k) 2^-24 sum_j |dgate_j| + H          (every entry of the gate's Jacobian is <= 1 in magnitude)
    L_bal, L_z, loss |err| <= 2^-16 |ref|                                                             (sums of non-negative terms)
    aux dlogits      |err| <= R |ref| + |dloss| p_e (2^-22 (|a_e| + zeta_t) + c 2^-24 (sum_u |a_u p_u| + zeta_t)) + H,
                     zeta_t = |zc| (2 / T) (|m_t| + |lse_t| + 1)
"""
import math

import numpy as np

from tests import softmax_ref as S

SOFTMAX, SIGMOID = 0, 1
SCORES = (SOFTMAX, SIGMOID)
SCORE_NAME = {SOFTMAX: "softmax", SIGMOID: "sigmoid"}
F16, BF16, F32 = S.F16, S.BF16, S.F32
CODES = S.CODES
CODE_NAME = S.CODE_NAME
ES, UINT = S.ES, S.UINT
bits, floats = S.bits, S.floats
MAX_E, MAX_K = 1024, 64


# ---- selection ----------------------------------------------------------------------------------------------------------------------
def ordered_keys(b, code):
    """The sort's unsigned key of stored bits: ascending keys are ascending values, -0.0 below +0.0, NaNs by bit pattern."""
    b = np.asarray(b)
    w = 8 * b.dtype.itemsize
    wide = b.astype(np.uint64)
    sign, every = np.uint64(1 << (w - 1)), np.uint64((1 << w) - 1)
    return np.where(wide & sign != 0, wide ^ every, wide ^ sign)


def select(b, code, k):
    """ids [T, k]: the first k positions of the stable descending order (the ascending stable order of the complemented key)."""
    key = ordered_keys(b, code)
    every = np.uint64((1 << (8 * np.asarray(b).dtype.itemsize)) - 1)
    return np.argsort(key ^ every, axis=-1, kind="stable")[:, :k].astype(np.int64)


# ---- the router ---------------------------------------------------------------------------------------------------------------------
def softmax_state(x):
    """(m, Z, lse, p) of the rows of x in f64; a row with a NaN, a +inf or only -inf is NaN throughout."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = x.max(axis=-1, keepdims=True)
        e = np.exp(x - m)
        Z = e.sum(axis=-1, keepdims=True)
        return m, Z, m + np.log(Z), e / Z


def scores(x, score):
    """s [T, E] and, for the sigmoid, 1 - s without cancellation."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if score == SOFTMAX:
            return softmax_state(x)[3], None
        return 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))


def _chosen(s, ids):
    """(s at the ids [T, k] with 0 for an id outside [0, E), the mask of the ids inside)."""
    E = s.shape[-1]
    ok = (ids >= 0) & (ids < E)
    return np.where(ok, np.take_along_axis(s, np.where(ok, ids, 0), axis=-1), 0.0), ok


def gate(x, ids, score, normalize):
    s, _ = scores(x, score)
    sj, _ = _chosen(s, ids)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sj / sj.sum(axis=-1, keepdims=True) if normalize else sj


def router_backward(x, ids, dgate, score, normalize):
    """dlogits [T, E] in f64: d gate / d s contracted with dgate, scattered to the chosen columns, then through d s / d logits."""
    x, dgate = np.asarray(x, np.float64), np.asarray(dgate, np.float64)
    T, E = x.shape
    s, q = scores(x, score)
    sj, ok = _chosen(s, ids)
    dg = np.where(ok, dgate, 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if normalize:
            Sm = sj.sum(axis=-1, keepdims=True)
            ds = (dg - (dg * (sj / Sm)).sum(axis=-1, keepdims=True)) / Sm
        else:
            ds = dg
        if score == SIGMOID:   # d s_e / d l_e = s_e (1 - s_e), and nothing off the chosen columns: a NaN there stays out
            ds = ds * sj * _chosen(q, ids)[0]
        dsE = np.zeros((T, E))
        for j in range(ids.shape[1]):
            rows = np.nonzero(ok[:, j])[0]
            np.add.at(dsE, (rows, ids[rows, j]), ds[rows, j])
        if score == SOFTMAX:
            return s * (dsE - (dsE * s).sum(axis=-1, keepdims=True))
        return dsE


# ---- the auxiliary losses -----------------------------------------------------------------------------------------------------------
def aux_forward(x, counts, k, balance_coef, z_coef):
    """(loss, L_bal, L_z) in f64; counts [E] = the live pairs per expert; the coefficients as the f32 the entry receives."""
    T, E = np.asarray(x).shape
    _, _, lse, p = softmax_state(x)
    l_bal = E / (T * k) * float((np.asarray(counts, np.float64) * p.mean(axis=0)).sum())
    l_z = float((lse ** 2).mean())
    return float(np.float32(balance_coef)) * l_bal + float(np.float32(z_coef)) * l_z, l_bal, l_z


def aux_terms(x, counts, k, balance_coef, z_coef):
    T, E = np.asarray(x).shape
    m, _, lse, p = softmax_state(x)
    a = float(np.float32(balance_coef)) * E * np.asarray(counts, np.float64) / (T * T * k)
    z = float(np.float32(z_coef)) * 2.0 * lse / T
    return m, lse, p, a[None, :], z


def aux_backward(x, counts, k, balance_coef, z_coef, dloss):
    _, _, p, a, z = aux_terms(x, counts, k, balance_coef, z_coef)
    return float(dloss) * p * (a - (a * p).sum(axis=-1, keepdims=True) + z)


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
def csum(E):
    return math.ceil(E / 64) + 16


def gate_bound(code, ref):
    return S.OUT_R[code] * np.abs(ref) + 1e-6


def router_backward_bound(code, E, k, dgate, ref):
    A = np.abs(np.asarray(dgate, np.float64)).sum(axis=-1, keepdims=True)
    return S.OUT_R[code] * np.abs(ref) + 4 * (csum(E) + k) * 2.0 ** -24 * A + S.OUT_HALF_SPACING[code]


def loss_bound(ref):
    return 2.0 ** -16 * abs(ref)


def aux_backward_bound(code, x, counts, k, balance_coef, z_coef, dloss, ref):
    T, E = np.asarray(x).shape
    m, lse, p, a, _ = aux_terms(x, counts, k, balance_coef, z_coef)
    zeta = abs(float(np.float32(z_coef))) * (2.0 / T) * (np.abs(m) + np.abs(lse) + 1.0)
    A = np.abs(a * p).sum(axis=-1, keepdims=True)
    return (S.OUT_R[code] * np.abs(ref) + abs(float(dloss)) * p * (2.0 ** -22 * (np.abs(a) + zeta) + csum(E) * 2.0 ** -24 * (A + zeta))
            + S.OUT_HALF_SPACING[code])


# ---- the draws ----------------------------------------------------------------------------------------------------------------------
DRAWS = ("normal", "ties", "equal", "special")    # the GPU tests'; "uniform" U(-30, 30) joins them in the CPU check of the bounds
TIE_VALUES = (-1.5, 0.0, 0.25, 3.0)               # exact in every dtype: ties across lanes and inside one lane's values
_NAN = {BF16: (0x7FC0, 0xFFC0, 0x7F81, 0xFFFF), F16: (0x7E00, 0xFE00, 0x7C01, 0xFFFF), F32: (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF)}


def special_bits(code):
    """+0, -0, +inf, -inf and NaNs of both signs (quiet, signalling, all ones) as stored bits."""
    z = bits(np.array([0.0, -0.0, np.inf, -np.inf]), code)
    return np.concatenate([z, np.array(_NAN[code], dtype=UINT[code])])


def draw_logits(rng, which, code, T, E):
    """Stored bits [T, E]. 'special': N(0, 2^2) rows, every row seeded with +-0 and every second row with +-inf or NaNs as well."""
    if which == "normal":
        return bits(rng.normal(0.0, 2.0, (T, E)), code)
    if which == "uniform":
        return bits(rng.uniform(-30.0, 30.0, (T, E)), code)
    if which == "ties":
        return bits(rng.choice(TIE_VALUES, (T, E)), code)
    if which == "equal":
        return bits(np.full((T, E), 0.75), code)
    assert which == "special"
    b = bits(rng.normal(0.0, 2.0, (T, E)), code)
    sp = special_bits(code)
    for t in range(T):
        pool = sp if t % 2 else sp[:2]
        n = min(E, int(rng.integers(1, 2 * len(pool) + 1)))
        b[t, rng.choice(E, n, replace=False)] = rng.choice(pool, n)
    return b


def finite_rows(b, code):
    return np.isfinite(floats(b, code)).all(axis=-1)


def draw_dgate(rng, code, T, k):
    return bits(rng.normal(0.0, 1.0, (T, k)), code)


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------
# (T, E, k): a partial last block (T not a multiple of 4) and more than one block; E under, at and over a wave's 64 lanes and over a
# span per lane, whole packs and ragged tails; k = 1, E (E <= 64) and 64
ROUTER_SHAPES = [(1, 1, 1), (3, 2, 2), (4, 7, 7), (5, 8, 2), (257, 8, 8), (3, 63, 63), (5, 64, 64), (4, 65, 6), (257, 128, 8), (5, 160, 64), (3, 257, 1),
                 (4, 512, 8), (5, 1000, 6), (257, 1024, 64), (1, 1024, 2), (5, 128, 1)]
# (T, E, k, plan): 'full' ids from the selection's range, 'empty' the upper half of the experts gets no pair, 'dropped' every third pair
# carries an id outside [0, E)
AUX_SHAPES = [(1, 8, 2, "full"), (5, 128, 8, "empty"), (1027, 8, 2, "dropped"), (1027, 1000, 6, "full"), (4099, 128, 8, "dropped"), (4099, 8, 1, "empty"),
              (5, 1000, 64, "full"), (1, 128, 1, "full")]
AUX_COEFS = ((1e-2, 0.0), (0.0, 1e-3), (1e-2, 1e-3))     # the balance term alone, the z term alone, both
AUX_DLOSS = 0.75


def seed_of(*parts):
    h = 0
    for p in parts:
        h = (h * 1000003 + (sum(map(ord, p)) if isinstance(p, str) else int(p))) % (2 ** 31)
    return h


def draw_plan_ids(rng, T, E, k, plan):
    """ids [T, k] the plan is built from (the aux loss takes only the plan's offsets)."""
    hi = max(1, E // 2) if plan == "empty" else E
    ids = rng.integers(0, hi, (T, k)).astype(np.int64)
    if plan == "dropped":
        flat = ids.reshape(-1)
        flat[::3] = np.where(np.arange(flat[::3].size) % 2 == 0, E, -1)
    return ids


def counts_of(ids, E):
    flat = ids.reshape(-1)
    return np.bincount(flat[(flat >= 0) & (flat < E)], minlength=E).astype(np.int64)
