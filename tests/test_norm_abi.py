"""CPU-only: a Python mirror of the norm backward's register-tile plan (norm_plan(..., bwd=true) in norm.hip), pinned against the
library's own workspace query. kf_norm_bwd_workspace_bytes needs no device: it returns min(nrb, 1024) * 2 * cols * 4 bytes for a
register-tile plan, where nrb = ceil(rows / RPB) is the number of row groups, and 0 for the generic kernel. Equality at every edge
below therefore pins the mirror's rows per block and its generic cut-offs exactly. tests/test_gpu_norm_walk.py picks its shapes
from this mirror, so a plan change in norm.hip fails here first, on any machine."""
import ctypes as C

import pytest

from kfunca_amd import hip_abi as H

MAX_BLOCKS = 1024  # kNormMaxBlocks: partial rows the backward's scratch is sized for

# every reachable backward plan: (threads per row, packs per lane)
PLANS = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (256, 1), (512, 1), (1024, 1), (1024, 2))
DTYPES = (H.F32, H.BF16, H.F16)


def pack(dtype):
    """Elements per 16-byte pack."""
    return 4 if dtype == H.F32 else 8


def bwd_plan(dtype, cols, ld=None):
    """(TPR, PACKS, RPB) of the backward's register-tile plan, or None for the generic kernel (16-byte-aligned pointers assumed)."""
    ld = cols if ld is None else ld
    V = pack(dtype)
    if cols % V or ld % V:
        return None
    npk = cols // V
    for t in (8, 16, 32):
        if npk <= t:
            return (t, 1, 256 // t)
    for p in (1, 2):
        if npk <= 64 * p:
            return (64, p, 4)
    for p in (1, 2):
        for t in (256, 512, 1024):
            if npk <= t * p:
                return (t, p, 1)
    return None


def plan_packs(plan):
    """(smallest, largest) pack count a row of this plan has: the plans are tried in the order of bwd_plan."""
    i = PLANS.index(plan)
    order = [PLANS[j][0] * PLANS[j][1] for j in range(len(PLANS))]
    # (1024, 2) follows (1024, 1); every other plan's lower edge is one past the previous plan's capacity
    lo = order[i - 1] + 1 if i else 1
    return lo, order[i]


def plan_cols(dtype, plan):
    """Column counts for a plan: the smallest, a ragged one (npk not a multiple of TPR: some lanes hold dead columns), the largest."""
    lo, hi = plan_packs(plan)
    V = pack(dtype)
    ragged = lo + 1 if lo + 1 < hi and (lo + 1) % plan[0] else lo
    return lo * V, ragged * V, hi * V


def ws_bytes(kind, dtype, rows, cols, ld=None):
    need = C.c_size_t(0)
    H.check(H.lib().kf_norm_bwd_workspace_bytes(kind, dtype, rows, cols, cols if ld is None else ld, C.byref(need)))
    return need.value


def expected_ws(dtype, rows, cols, ld=None):
    pl = bwd_plan(dtype, cols, ld)
    if pl is None or rows == 0:
        return 0
    nrb = -(-rows // pl[2])
    return min(nrb, MAX_BLOCKS) * 2 * cols * 4


def test_mirror_covers_every_plan_once_in_order():
    for dtype in DTYPES:
        V = pack(dtype)
        seen = [bwd_plan(dtype, npk * V)[:2] for npk in range(1, 2049)]
        assert sorted(set(seen), key=PLANS.index) == list(PLANS)
        assert [p for i, p in enumerate(seen) if i == 0 or seen[i - 1] != p] == list(PLANS)  # each plan one contiguous range
        assert bwd_plan(dtype, 2049 * V) is None


@pytest.mark.parametrize("plan", PLANS, ids=[f"{t}x{p}" for t, p in PLANS])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_workspace_pins_the_plan(dtype, plan):
    """Each plan at its smallest, ragged and largest column count; rows giving nrb just below, at and above 1024 (and 1 row), with
    the last row group full and partial. Both kinds: the plan does not depend on the kind."""
    rpb = 256 // plan[0] if plan[0] < 256 else 1
    for cols in plan_cols(dtype, plan):
        assert bwd_plan(dtype, cols)[:2] == plan
        for nrb in (1, 2, 1023, 1024, 1025, 3073):
            for rows in {(nrb - 1) * rpb + 1, nrb * rpb}:
                want = min(nrb, MAX_BLOCKS) * 2 * cols * 4
                for kind in (H.NORM_RMS, H.NORM_LAYER):
                    assert ws_bytes(kind, dtype, rows, cols) == want, (kind, rows, cols)
        # rows per block, exactly: one more row past a full group adds a partial row while nrb < 1024
        assert ws_bytes(H.NORM_RMS, dtype, 5 * rpb, cols) == 5 * 2 * cols * 4
        assert ws_bytes(H.NORM_RMS, dtype, 5 * rpb + 1, cols) == 6 * 2 * cols * 4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_generic_cut_offs(dtype):
    """The generic kernel (workspace 0): cols % V != 0, ld % V != 0, more than 2048 packs. ld > cols with ld % V == 0 keeps the plan."""
    V = pack(dtype)
    for cols in (V + 1, 3, 1000 * V + V // 2, 2048 * V + 1):
        assert expected_ws(dtype, 64, cols) == 0 and ws_bytes(H.NORM_LAYER, dtype, 64, cols) == 0, cols
    assert ws_bytes(H.NORM_RMS, dtype, 64, 128 * V, 128 * V + 1) == 0  # ld not a multiple of the pack
    assert ws_bytes(H.NORM_RMS, dtype, 64, 2049 * V) == 0  # one pack beyond 1024 threads x 2 packs
    assert ws_bytes(H.NORM_RMS, dtype, 64, 2048 * V) == 64 * 2 * 2048 * V * 4
    for cols in (V, 100 * V, 2048 * V):
        ld = cols + V
        assert bwd_plan(dtype, cols, ld) == bwd_plan(dtype, cols)
        assert ws_bytes(H.NORM_LAYER, dtype, 3000, cols, ld) == expected_ws(dtype, 3000, cols, ld) > 0
    assert ws_bytes(H.NORM_RMS, dtype, 0, 64 * V) == 0


def test_bad_extents_are_refused_without_a_device():
    with pytest.raises(H.KfError) as e:
        ws_bytes(H.NORM_RMS, H.F32, 4, 16, 8)  # ld < cols
    assert e.value.code == H.KF_ERR_INVALID
    with pytest.raises(H.KfError) as e:
        ws_bytes(H.NORM_RMS, H.F32, 1 << 31, 16)  # rows beyond one launch
    assert e.value.code == H.KF_ERR_INDEX_RANGE
