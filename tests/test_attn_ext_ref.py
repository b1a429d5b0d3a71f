"""CPU: the float64 reference of the score modifiers (tests/attn_ext_ref.py) is what it claims to be, and the GPU tests' modifiers bite.

 * modifiers off: attn_ref64_ext EQUALS attn_ref64_vis, key by key;
 * with modifiers it matches torch's float64 autograd to 1e-10 - soft-cap as a tanh on the scores, the sink as a logit column that is
   concatenated before the softmax and dropped after it - under all four masks, with grouped heads, a row that sees no key and a batch
   with len_b = 0;
 * discrimination: for every softcap and every sink vector tests/test_gpu_attn_ext.py uses (CAPS, sinks_for), the reference WITHOUT
   that modifier fails oracle.checks.check_one against the reference with it, on that file's own inputs, and so does a backward that
   drops the factor 1 - t^2. A kernel that ignored a modifier would therefore fail the GPU tests. BIG_CAP is the opposite case: a cap
   that bends nothing agrees with the uncapped reference within the bounds."""
import numpy as np
import pytest
import torch

from oracle import checks as K
from oracle import oracle as O
from tests.attn_doc_ref import cu_of, doc_vis
from tests.attn_ext_ref import BIG_CAP, CAPS, attn_ref64_ext, sinks_for
from tests.attn_full_ref import attn_ref64_vis, format_floor_vis, key_len_vis
from tests.attn_window_ref import window_vis
from tests.test_gpu_attn_full import inputs


def prefix_vis(kv_len, prefix_len, Sq, Skv):
    ln, pre = np.clip(np.asarray(kv_len), 0, Skv), np.clip(np.asarray(prefix_len), 0, Skv)
    n, m = np.arange(Skv)[None, None, :], np.arange(Sq)[None, :, None]
    return (n < ln[:, None, None]) & ((n < pre[:, None, None]) | (n <= m))


def masks(B, Sq, Skv):
    """the four kinds, each with a batch of length 0; the window one with rows that see no key inside a live batch"""
    lens = [Skv, 0, max(1, Skv - 5)][:B]
    out = {"full": key_len_vis(lens, Sq, Skv, B), "prefix": prefix_vis(lens, [3, 0, 2][:B], Sq, Skv),
           "window": window_vis([Skv // 2, 0, Skv][:B], 2, 0, Sq, Skv, B)}
    if Sq == Skv:
        out["doc"] = doc_vis(cu_of([[Sq // 2, Sq - Sq // 2 - 3], [], [Sq]][:B], 2), Sq, True)
    return out


def test_modifiers_off_is_the_plain_reference():
    rng = np.random.default_rng(0)
    q, k, v, go = inputs(rng, O.BF16, 3, 4, 2, 19, 19, 16)
    for name, vis in masks(3, 19, 19).items():
        a, b = attn_ref64_vis(q, k, v, go, vis, O.BF16), attn_ref64_ext(q, k, v, go, vis, O.BF16)
        assert set(a) == set(b), name
        for key in a:
            assert np.array_equal(a[key], b[key], equal_nan=True), (name, key)
        c = attn_ref64_ext(q, k, v, go, vis, O.BF16, softcap=0, sink=None)
        assert all(np.array_equal(a[key], c[key], equal_nan=True) for key in a), name


def torch_ext(q, k, v, go, vis, softcap, sink):
    """float64 autograd: tanh on the scores, the sink as an extra logit column dropped after the softmax; a row without a key keeps only
    its sink column (or, without a sink, is given zero weights by hand)"""
    G = q.shape[1] // k.shape[1]
    tq, tk, tv = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (q, k, v))
    ts = None if sink is None else torch.tensor(np.asarray(sink, np.float64), requires_grad=True)
    x = tq @ tk.repeat_interleave(G, dim=1).transpose(-1, -2) / np.sqrt(q.shape[-1])
    if softcap:
        x = softcap * torch.tanh(x / softcap)
    m = torch.tensor(vis)[:, None]
    x = x.masked_fill(~m, -np.inf)
    if ts is not None:
        x = torch.cat([x, ts[None, :, None, None].expand(x.shape[0], -1, x.shape[2], 1)], dim=-1)
    live = torch.isfinite(x).any(dim=-1, keepdim=True)
    lse = torch.logsumexp(torch.where(live, x, torch.zeros_like(x)), dim=-1)
    p = torch.where(live, torch.exp(x - lse[..., None]), torch.zeros_like(x))
    lse = torch.where(live[..., 0], lse, torch.full_like(lse, -np.inf))
    o = p[..., :vis.shape[2]] @ tv.repeat_interleave(G, dim=1)
    o.backward(torch.tensor(go, dtype=torch.float64))
    out = {"o": o, "lse": lse, "dq": tq.grad, "dk": tk.grad, "dv": tv.grad}
    if ts is not None:
        out["dsink"] = ts.grad
    return {n: t.detach().numpy() for n, t in out.items()}


@pytest.mark.parametrize("softcap,with_sink", [(0.7, False), (None, True), (0.7, True), (30.0, True)])
@pytest.mark.parametrize("Sq,Skv", [(13, 13), (9, 17)])
def test_matches_torch_float64_autograd(Sq, Skv, softcap, with_sink):
    rng = np.random.default_rng(Sq + Skv)
    B, Hq, Hkv, D = 3, 4, 2, 8
    q, k, v, go = inputs(rng, O.BF16, B, Hq, Hkv, Sq, Skv, D)
    f = lambda a: K.to_f64(a, O.BF16)  # noqa: E731
    sink = np.array([0.5, -1.0, 3.0, -np.inf]) if with_sink else None
    for name, vis in masks(B, Sq, Skv).items():
        assert (~vis.any(axis=2)).any(), "the case must hold a row that sees no key"
        ref = attn_ref64_ext(q, k, v, go, vis, O.BF16, softcap=softcap, sink=sink)
        want = torch_ext(f(q), f(k), f(v), f(go), vis, softcap, sink)
        for key, w in want.items():
            assert np.allclose(ref[key], w, rtol=1e-10, atol=1e-10, equal_nan=True), (name, key, np.abs(ref[key] - w).max())
        dead = ~vis.any(axis=2)
        for b in range(B):
            assert not ref["o"][b][:, dead[b]].any() and not ref["dq"][b][:, dead[b]].any()
            for h in range(Hq):
                want_lse = -np.inf if sink is None else sink[h]
                assert (ref["lse"][b, h][dead[b]] == want_lse).all(), (name, b, h)
        if sink is not None:
            assert (ref["dsink_bound"] > 0)[:3].all() and ref["dsink"][3] == 0 and ref["dsink_bound"][3] == 0     # sink = -inf: no sink


# ---- discrimination: the shapes, inputs and modifiers of tests/test_gpu_attn_ext.py ----
def fails(name, got, ref, code, fl):
    try:
        K.check_one(name, O.from_float(got.astype(np.float32), code), ref, code, floor=fl.get(name))
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(200)
    code, B, Hq, Hkv, S, D = O.BF16, 2, 4, 2, 200, 64
    q, k, v, go = inputs(rng, code, B, Hq, Hkv, S, S, D)
    vis = window_vis([S, S - 37], 70, 0, S, S, B)
    return code, q, k, v, go, vis, attn_ref64_vis(q, k, v, go, vis, code), format_floor_vis(q, k, v, go, vis, code)


@pytest.mark.parametrize("cap", CAPS)
def test_every_cap_of_the_gpu_tests_bends_the_result(case, cap):
    code, q, k, v, go, vis, plain, fl = case
    ref = attn_ref64_ext(q, k, v, go, vis, code, softcap=cap)
    for name in ("o", "dq", "dk", "dv"):
        assert fails(name, plain[name], ref, code, fl), f"cap {cap}: the uncapped {name} passes for the capped one"
    wrong = attn_ref64_ext(q, k, v, go, vis, code, softcap=cap, drop_dtanh=True)
    assert np.array_equal(wrong["o"], ref["o"])
    for name in ("dq", "dk"):
        assert fails(name, wrong[name], ref, code, fl), f"cap {cap}: {name} without the factor 1 - t^2 passes"
    # (lse too, in the typical row: a row whose scores are all tiny is bent by less than any bound)
    assert np.median(np.abs(plain["lse"] - ref["lse"])[np.isfinite(ref["lse"])]) > 100 * (2e-6 * (1 + np.abs(ref["lse"]).max()) + cap * 2.0 ** -20)


def test_a_large_cap_bends_nothing(case):
    code, q, k, v, go, vis, plain, fl = case
    ref = attn_ref64_ext(q, k, v, go, vis, code, softcap=BIG_CAP)
    for name in ("o", "dq", "dk", "dv"):
        assert not fails(name, plain[name], ref, code, fl), name


@pytest.mark.parametrize("Hq", [2, 4])
def test_every_sink_vector_of_the_gpu_tests_carries_mass(case, Hq):
    code, q, k, v, go, vis, plain, fl = case
    q, go = q[:, :Hq], go[:, :Hq]
    k, v = k[:, :Hq // 2], v[:, :Hq // 2]
    plain = attn_ref64_vis(q, k, v, go, vis, code)
    fl = format_floor_vis(q, k, v, go, vis, code)
    sink = sinks_for(Hq)
    assert sink.dtype == np.float32 and sink.shape == (Hq,) and (sink >= -1).all() and (sink <= 3).all()
    ref = attn_ref64_ext(q, k, v, go, vis, code, sink=sink)
    for name in ("o", "dq", "dk", "dv"):
        assert fails(name, plain[name], ref, code, fl), f"{name} without the sink passes for the one with it"
    live = np.isfinite(plain["lse"])
    assert (np.abs(plain["lse"] - ref["lse"])[live] > 1e-3).all()
    # (dsink_bound is a worst case over B Sq rows and of dsink's own size here; what holds dsink to a relative error is the operator
    # test's comparison with torch, tests/test_gpu_attn_ext_operator.py)
    assert (ref["dsink"] != 0).all() and (ref["dsink_bound"] > 0).all()
