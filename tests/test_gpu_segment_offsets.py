"""-m gpu: kf_segment_offsets / kfunca.segment_offsets - exact integers: offsets[e] is the number of ascending ids below e."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import gemm_seg_ref as R

pytestmark = pytest.mark.gpu


def run_abi(ids, E):
    ids = np.asarray(ids, dtype=np.int64)
    d_ids = H.DevBuf.from_numpy(ids) if ids.size else None
    guard = np.full(E + 1 + 16, -77, dtype=np.int64)   # eight sentinel entries on either side of the result
    out = H.DevBuf.from_numpy(guard)
    H.segment_offsets(d_ids.ptr if d_ids else None, ids.size, E, out.ptr + 64, None)
    H.device_sync()
    got = out.to_numpy(guard.shape, np.int64)
    assert (got[:8] == -77).all() and (got[-8:] == -77).all(), "entries outside offsets[0 .. E] were written"
    return got[8:-8]


CASES = [
    ([0, 0, 2, 2, 2, 5], 6),                       # repeated values, absent experts 1, 3, 4
    ([-4, -1, 0, 1, 1, 3, 7, 9], 3),               # ids below 0 and at least E fall outside [offsets[0], offsets[E])
    ([], 4),                                       # n = 0: all zeros
    ([0, 0, 0], 1), ([], 1), ([5, 5], 1),          # E = 1
    ([3] * 1000, 8),                               # one expert takes everything
    (sorted(np.random.default_rng(3).integers(-2, 70, 5000).tolist()), 64),
    (sorted(np.random.default_rng(4).integers(0, 300, 777).tolist()), 300),   # more than one block of entries
]


@pytest.mark.parametrize("ids,E", CASES)
def test_exact_offsets(ids, E):
    want = R.segment_offsets(ids, E)
    assert np.array_equal(run_abi(ids, E), want)
    ids = np.asarray(ids, dtype=np.int64)
    assert want[0] == (ids < 0).sum() and want[E] == (ids < E).sum()
    if ids.size:   # the operator returns the same integers
        got = kfunca.segment_offsets(kfunca.from_numpy(ids, 0), E)
        assert got.sizes() == [E + 1] and np.array_equal(got.numpy(), want)


def test_operator_refuses():
    ids = kfunca.from_numpy(np.zeros(4, np.int64), 0)
    with pytest.raises(RuntimeError):
        kfunca.segment_offsets(ids, 0)
    with pytest.raises(RuntimeError):
        kfunca.segment_offsets(kfunca.from_numpy(np.zeros(4, np.int32), 0), 2)
