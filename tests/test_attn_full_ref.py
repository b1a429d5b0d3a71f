"""not gpu: the full-attention reference helper (tests/attn_full_ref.py) is pinned to the oracle, and the project's scale-aware bounds
(oracle/checks.py), fed by it, CAN FAIL on the defects a non-causal kernel with key lengths and grouped heads can have: a dropped
64-key tile, a key length that is not applied, a group member missing from dk, an all-zero gradient."""
import numpy as np
import pytest

from tests.attn_full_ref import attn_ref64_vis, format_floor_vis, key_len_vis
from oracle import checks as K
from oracle import oracle as O


def draw(rng, shape, code):
    return O.from_float(rng.uniform(-1, 1, shape).astype(np.float32), code)


@pytest.mark.parametrize("Sq,Skv", [(70, 70), (50, 90)])
def test_tril_visibility_equals_the_oracle(Sq, Skv):
    rng = np.random.default_rng(Sq * 1000 + Skv)
    code, B, H, D = O.BF16, 2, 2, 64
    q, go = (draw(rng, (B, H, Sq, D), code) for _ in range(2))
    k, v = (draw(rng, (B, H, Skv, D), code) for _ in range(2))
    want = O.attn_ref64(q, k, v, go, code=code)
    vis = np.broadcast_to(np.arange(Skv)[None, :] <= np.arange(Sq)[:, None], (B, Sq, Skv))
    got = attn_ref64_vis(q, k, v, go, vis, code)
    assert set(got) == set(want)
    for n in want:
        scale_ = np.abs(want[n]).max()
        assert np.abs(got[n] - want[n]).max() <= 1e-12 * scale_, n
    # the floors: the same sums as oracle.checks.format_floor takes over causal prefixes and suffixes
    fw, fg = K.format_floor(q, k, v, go, code), format_floor_vis(q, k, v, go, vis, code)
    for n in fw:
        assert np.allclose(fg[n], fw[n], rtol=1e-12, atol=0.0), n


Sq, Skv, D, Hq, Hkv = 256, 320, 64, 2, 1
LEN = 300


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(320)
    code = O.BF16
    q, go = (draw(rng, (1, Hq, Sq, D), code) for _ in range(2))
    k, v = (draw(rng, (1, Hkv, Skv, D), code) for _ in range(2))
    vis = key_len_vis([LEN], Sq, Skv)
    ref = attn_ref64_vis(q, k, v, go, vis, code)
    return dict(code=code, q=q, k=k, v=v, go=go, vis=vis, ref=ref)


def to16(x, code):
    return O.from_float(np.asarray(x, dtype=np.float32), code)


def reject(c, name, bad):
    with pytest.raises(AssertionError, match="scale-aware bound"):
        K.check_one(name, to16(bad, c["code"]), c["ref"], c["code"], what="defect")


def test_accepts_the_reference_rounded_once(case):
    c = case
    for name in K.NAMES:
        m = K.check_one(name, to16(c["ref"][name], c["code"]), c["ref"], c["code"], what="reference")
        assert m["row"] < 0.3, (name, m)


def test_rejects_a_dropped_key_tile(case):
    c = case
    for t0 in (0, 128, 256):
        vis = c["vis"].copy()
        vis[:, :, t0:t0 + 64] = False
        bad = attn_ref64_vis(c["q"], c["k"], c["v"], c["go"], vis, c["code"])
        for name in ("o", "dq"):
            reject(c, name, bad[name])


def test_rejects_a_key_length_that_is_not_applied(case):
    c = case
    bad = attn_ref64_vis(c["q"], c["k"], c["v"], c["go"], key_len_vis(None, Sq, Skv, 1), c["code"])  # keys >= LEN are included
    for name in K.NAMES:
        reject(c, name, bad[name])


def test_rejects_a_missing_group_member_and_zeros(case):
    c = case
    one = attn_ref64_vis(c["q"][:, :1], c["k"], c["v"], c["go"][:, :1], c["vis"], c["code"])  # query head 1 never reaches dk, dv
    reject(c, "dk", one["dk"])
    reject(c, "dv", one["dv"])
    for name in K.NAMES:
        reject(c, name, np.zeros_like(c["ref"][name]))
