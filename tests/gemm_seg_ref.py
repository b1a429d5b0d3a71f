"""The segmented (expert) GEMM restated in numpy: the offset sanitising, the three products in f64, and a mirror of the row-tile map of
kfunca_amd/csrc/device/gemm_seg.hip (seg_plan_kernel). numpy only; shared by the CPU and the GPU tests."""
import numpy as np

TILE = 128
UNCOVERED = -2


def sanitize(offsets, T):
    """o'_0 = clamp(o_0, 0, T), o'_e = clamp(max(o_e, o'_(e-1)), 0, T)."""
    out, prev = [], None
    for o in [int(v) for v in offsets]:
        v = o if prev is None else max(o, prev)
        v = min(max(v, 0), T)
        out.append(v)
        prev = v
    return np.array(out, dtype=np.int64)


def segment_offsets(sorted_ids, E):
    """offsets[e] = the number of ids < e for e = 0 .. E (a lower bound over ascending ids)."""
    ids = np.asarray(sorted_ids, dtype=np.int64)
    return np.searchsorted(ids, np.arange(E + 1, dtype=np.int64), side="left").astype(np.int64)


def row_expert(offsets, T):
    """The expert of every row after sanitising, -1 for a row no segment covers."""
    so = sanitize(offsets, T)
    owner = np.full(T, -1, dtype=np.int64)
    for e in range(len(so) - 1):
        owner[so[e]:so[e + 1]] = e
    return owner


def forward(a, w, offsets, alpha=1.0, beta=0.0, c0=None, trans_b=False):
    """C[r] = alpha a[r] op(w[e]) + beta c0[r] for the rows of segment e, beta c0[r] (+0 when beta == 0) elsewhere. f64.
    a [T, K]; w [E, K, N], or [E, N, K] with trans_b."""
    a, w = np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64)
    T, N = a.shape[0], (w.shape[1] if trans_b else w.shape[2])
    so = sanitize(offsets, T)
    out = np.zeros((T, N)) if beta == 0.0 else beta * np.asarray(c0, dtype=np.float64)
    for e in range(len(so) - 1):
        lo, hi = so[e], so[e + 1]
        if hi > lo:
            out[lo:hi] += alpha * (a[lo:hi] @ (w[e].T if trans_b else w[e]))
    return out


def wgrad(a, b, offsets, alpha=1.0, beta=0.0, dw0=None):
    """dW_e = alpha a[seg_e]^T b[seg_e] + beta dw0_e; rows outside the segment never enter (not even times zero). f64. [E, M, N]."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    so = sanitize(offsets, a.shape[0])
    E = len(so) - 1
    out = np.zeros((E, a.shape[1], b.shape[1])) if beta == 0.0 else beta * np.asarray(dw0, dtype=np.float64)
    for e in range(E):
        lo, hi = so[e], so[e + 1]
        if hi > lo:
            out[e] += alpha * (a[lo:hi].T @ b[lo:hi])
    return out


def abs_forward(a, w, offsets, trans_b=False):
    """sum_k |a_k w_k| per output element (the accumulation term of the error bound); 0 for uncovered rows."""
    return forward(np.abs(a), np.abs(w), offsets, trans_b=trans_b)


def abs_wgrad(a, b, offsets):
    return wgrad(np.abs(a), np.abs(b), offsets)


def tile_map(offsets, T):
    """The row tiles in table order: (row0, rend, seg) with seg = the expert, or UNCOVERED for the head [0, o'_0) and the tail
    [o'_E, T). Segment e owns ceil(len_e / 128) tiles starting at o'_e; no tile straddles a segment."""
    so = sanitize(offsets, T)
    bounds = [0] + [int(v) for v in so] + [T]
    segs = [UNCOVERED] + list(range(len(so) - 1)) + [UNCOVERED]
    tiles = []
    for s, seg in enumerate(segs):
        lo, hi = bounds[s], bounds[s + 1]
        for r0 in range(lo, hi, TILE):
            tiles.append((r0, min(r0 + TILE, hi), seg))
    return tiles


def tile_bound(T, E):
    return T // TILE + E + 2
