"""-m gpu: kfunca.linear_fp8, fp8_quantize and gemm_fp8 through the operator API.

Tight check: y, dX and dW against the reference pipeline of tests/fp8_ref.py - its quantisation of the same inputs (e4m3 for x and
weight, e5m2 for dy), the f64 product of the decoded codes and the kf_gemm_fp8 bound. End-to-end check: against the f64 product of the
UNQUANTISED operands within the formats' worst case, sum_k (|a| db + |b| da + da db) with d = max(u |v|, sub / (2 scale)) per element,
plus the GEMM bound. Then: what the backward holds (allocator statistics), a row-pitched x, forward + backward replayed from a graph
after the inputs were rewritten, and accumulation into an existing gradient."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import fp8_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [((1,), 16, 16), ((37,), 48, 80), ((200,), 256, 144), ((2, 130), 128, 256)]
DTYPES = ["bf16", "f16", "f32"]


def to_t(stored, dt, requires_grad=False):
    t = kfunca.from_numpy_bf16(np.ascontiguousarray(stored), 0) if dt == "bf16" else kfunca.from_numpy(np.ascontiguousarray(stored), 0)
    t.set_requires_grad(requires_grad)
    return t


def stored_of(t, dt):
    a = np.ascontiguousarray(t.numpy())
    return a.view(np.uint16) if dt == "bf16" else a


def values(t, dt):
    return R.to_f32(stored_of(t, dt), dt).astype(np.float64)


def draw(lead, K, N, dt, seed):
    rng = np.random.default_rng(seed)
    x = R.round_to(rng.standard_normal(lead + (K,)), dt)
    w = R.round_to(rng.standard_normal((N, K)) * 0.05, dt)
    dy = R.round_to(rng.standard_normal(lead + (N,)) * 1e-3, dt)
    return x, w, dy


def reference(x, w, dy, dt):
    """{name: (c, mag, end-to-end reference, end-to-end quantisation bound)} for y, dx, dw."""
    K, N = x.shape[-1], w.shape[0]
    x32, w32, g32 = R.to_f32(x, dt).reshape(-1, K), R.to_f32(w, dt), R.to_f32(dy, dt).reshape(-1, N)
    T = x32.shape[0]
    xq, xt, sx, _ = R.quantize(x32, R.E4M3)
    wq, wt, sw, _ = R.quantize(w32, R.E4M3)
    gq, gt, sg, _ = R.quantize(g32, R.E5M2)
    assert wt.shape == (K, N) and xt.shape[1] == gt.shape[1] == (T + 15) // 16 * 16
    x64, w64, g64 = x32.astype(np.float64), w32.astype(np.float64), g32.astype(np.float64)
    scx, scw, scg = 1.0 / float(sx), 1.0 / float(sw), 1.0 / float(sg)
    return {
        "y": R.product(xq, R.E4M3, wq, R.E4M3, sx, sw) + (x64 @ w64.T, R.end_to_end_bound(x64, w64, scx, R.E4M3, scw, R.E4M3)),
        "dx": R.product(gq, R.E5M2, wt, R.E4M3, sg, sw) + (g64 @ w64, R.end_to_end_bound(g64, w64.T, scg, R.E5M2, scw, R.E4M3)),
        "dw": R.product(gt, R.E5M2, xt, R.E4M3, sg, sx) + (g64.T @ x64, R.end_to_end_bound(g64.T, x64.T, scg, R.E5M2, scx, R.E4M3)),
    }


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("lead,K,N", SHAPES)
def test_output_and_gradients(lead, K, N, dt):
    x, w, dy = draw(lead, K, N, dt, K + N + len(lead))
    tx, tw = to_t(x, dt, True), to_t(w, dt, True)
    y = kfunca.linear_fp8(tx, tw)
    assert y.sizes() == list(lead) + [N]
    y.backward(to_t(dy, dt))
    assert tx.grad().sizes() == list(x.shape) and tw.grad().sizes() == [N, K]
    ref = reference(x, w, dy, dt)
    got = {"y": values(y, dt).reshape(-1, N), "dx": values(tx.grad(), dt).reshape(-1, K), "dw": values(tw.grad(), dt)}
    for name in ("y", "dx", "dw"):
        c, mag, full, qbound = ref[name]
        assert np.abs(full).max() > 0, name
        frac = R.gemm_frac(got[name], c, mag, dt)
        e2e = float((np.abs(got[name] - full) / (qbound + R.gemm_bound(c, mag, dt))).max())
        print(f"linear_fp8 {lead} K {K} N {N} {dt} {name}: {frac:.3f} of the GEMM bound, {e2e:.3f} of the end-to-end bound")
        assert frac <= 1.0, (name, frac)
        assert e2e <= 1.0, (name, e2e)


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_operator_quantize_and_gemm_match_the_reference(fmt):
    code = R.E4M3 if fmt == "e4m3" else R.E5M2
    rng = np.random.default_rng(3)
    a, b = R.round_to(rng.standard_normal((37, 48)), "bf16"), R.round_to(rng.standard_normal((80, 48)) * 7, "bf16")
    qa, qat, sa = kfunca.fp8_quantize(to_t(a, "bf16"), fmt, True)
    qb, none, sb = kfunca.fp8_quantize(to_t(b, "bf16"), fmt)
    assert none is None and qat.sizes() == [48, 48] and sa.sizes() == [1]
    ra, rb = R.quantize(R.to_f32(a, "bf16"), code), R.quantize(R.to_f32(b, "bf16"), code)
    assert np.array_equal(qa.numpy(), ra[0]) and np.array_equal(qat.numpy(), ra[1]) and np.array_equal(qb.numpy(), rb[0])
    assert sa.numpy()[0] == ra[2] and sb.numpy()[0] == rb[2]
    out = kfunca.gemm_fp8(qa, qb, sa, sb, fmt, fmt, kfunca.dtype.float)
    c, mag = R.product(ra[0], code, rb[0], code, ra[2], rb[2])
    assert out.sizes() == [37, 80] and R.gemm_frac(out.numpy(), c, mag, "f32") <= 1.0
    with pytest.raises(Exception, match="e4m3 or e5m2"):
        kfunca.fp8_quantize(to_t(a, "bf16"), "e3m4")


def test_the_backward_holds_fp8_copies_only():
    lead, K, N, dt = (200,), 256, 144, "bf16"
    x, w, dy = draw(lead, K, N, dt, 9)

    tx, tw = to_t(x, dt, True), to_t(w, dt, True)
    kfunca.synchronize(0)
    kfunca.release_cached(0)        # an empty cache: every allocation below is a fresh block of its own (rounded) size, not a larger cached one
    before = kfunca.memstat_dict(0)
    y = kfunca.linear_fp8(tx, tw)
    kfunca.synchronize(0)
    after = kfunca.memstat_dict(0)
    T16 = 208
    want = 200 * N * 2 + K * T16 + K * N                       # y, x_t [K, ceil16(T)], w_t [K, N]
    held = after["active_bytes"] - before["active_bytes"]
    print(f"linear_fp8 holds {held} bytes in {after['active_blocks'] - before['active_blocks']} blocks; y + x_t + w_t = {want}")
    assert after["active_blocks"] - before["active_blocks"] == 5   # ... and the two scales; x_q, w_q and the amax scratch are gone
    assert want <= held <= want + 5 * 4096                         # nothing of x's size in x's dtype (102400 bytes) is kept


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_a_row_pitched_x_gives_the_bits_of_its_contiguous_copy(dt):
    lead, K, N = (37,), 48, 80
    x, w, dy = draw(lead, K, N, dt, 4)
    wide = np.concatenate([x, R.round_to(np.full((37, 16), np.nan), dt)], axis=1)   # [37, 64]: NaN behind every row
    outs = []
    for pitched in (False, True):
        tx = to_t(wide, dt)[:, :K] if pitched else to_t(x, dt)
        if pitched:
            assert tx.strides() == [64, 1]
        tx.set_requires_grad(True)
        tw = to_t(w, dt, True)
        y = kfunca.linear_fp8(tx, tw)
        y.backward(to_t(dy, dt))
        outs.append([stored_of(t, dt).copy() for t in (y, tw.grad())])
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_forward_and_backward_replay_from_one_graph():
    lead, K, N, dt = (2, 130), 128, 256, "bf16"
    x, w, dy = draw(lead, K, N, dt, 1)
    x2, w2, dy2 = draw(lead, K, N, dt, 2)

    def step(tx, tw, tg):
        y = kfunca.linear_fp8(tx, tw)
        y.backward(tg)
        return y

    def eager(x, w, dy):
        tx, tw = to_t(x, dt, True), to_t(w, dt, True)
        y = step(tx, tw, to_t(dy, dt))
        kfunca.synchronize(0)
        return [stored_of(t, dt).copy() for t in (y, tx.grad(), tw.grad())]

    want1 = eager(x, w, dy)        # also warms the allocator
    want2 = eager(x2, w2, dy2)
    assert not np.array_equal(want1[0], want2[0])
    tx, tw, tg = to_t(x, dt, True), to_t(w, dt, True), to_t(dy, dt)
    kfunca.synchronize(0)
    kfunca.graph_begin(0)
    y = step(tx, tw, tg)           # recorded, not run: the leaves' first gradients are written, not added, by every replay
    graph = kfunca.graph_end(0)
    for want, (nx, nw, ng) in ((want1, (x, w, dy)), (want2, (x2, w2, dy2)), (want1, (x, w, dy))):
        for t, new in ((tx, nx), (tw, nw), (tg, ng)):
            new = np.ascontiguousarray(new)
            H.check(H.lib().kf_memcpy_h2d(t.data_ptr(), new.ctypes.data, new.nbytes, None))
        H.device_sync()
        kfunca.graph_launch(graph, 0)
        kfunca.synchronize(0)
        got = [stored_of(t, dt) for t in (y, tx.grad(), tw.grad())]
        for g, v in zip(got, want):
            assert np.array_equal(g, v)
    kfunca.graph_destroy(graph)


def test_gradients_accumulate_into_an_existing_grad():
    lead, K, N, dt = (37,), 48, 80, "f32"
    x, w, dy = draw(lead, K, N, dt, 6)
    tx, tw, tg = to_t(x, dt, True), to_t(w, dt, True), to_t(dy, dt)
    kfunca.linear_fp8(tx, tw).backward(tg)
    once = [t.grad().numpy().copy() for t in (tx, tw)]
    kfunca.linear_fp8(tx, tw).backward(tg)
    twice = [t.grad().numpy().copy() for t in (tx, tw)]
    for a, b in zip(once, twice):
        assert np.abs(a).max() > 0 and np.array_equal(b, a + a)
