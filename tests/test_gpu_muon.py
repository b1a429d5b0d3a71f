"""-m gpu: the Muon optimizer - kf_muon_prepare / kf_muon_apply through the C ABI against their f64 formulas, kfunca.newton_schulz against
the f64 iteration started from the same bf16 X0 (and against the same iteration composed from kf_gemm calls with bf16 roundings at A,
B and X), and kfunca.Muon: one step against a numpy restatement, a captured second step against an eager one, no pool growth, refusals.

Tolerances: the momentum buffer, f32 params and masters within 2 ulp of f32 of the f64 formula; a bf16 param without a master within
half a bf16 ulp (its one rounding) plus those 2 ulp of f32; X within one bf16 ulp. Newton-Schulz:
e = |Y - Y64|_F / |Y64|_F at most 1.5 times the composed iteration's e (the two differ in summation order inside f32 accumulators and in
the rounding of B's diagonal) and at most 0.03 (a CPU emulation of the bf16 roundings gives 0.011 - 0.013); singular values in [0.6, 1.2]
(the f64 iteration: [0.68, 1.14]). Muon.step(): |p - p_ref|_F <= lr scale 0.03 |O64|_F plus 2 ulp per element - the Newton-Schulz cap
carried through the linear update p (1 - lr wd) - lr scale O."""
import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from tests import gemm_views as V

pytestmark = pytest.mark.gpu

COEFFS = (3.4445, -4.7750, 2.0315)
F32 = lambda v: np.float64(np.float32(v))


def bf16(x):
    return V.decode(V.encode(x, "bf16"), "bf16")


def within_ulp_f32(got, want, n):
    return np.all(np.abs(got.astype(np.float64) - want) <= n * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))


def ns64(X, steps=5):
    a, b, c = COEFFS
    for _ in range(steps):
        A = X @ X.T
        X = a * X + (b * A + c * A @ A) @ X
    return X


@pytest.mark.parametrize("pdt,master", [("f32", False), ("bf16", True), ("bf16", False)])
@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(128, 256), (256, 128), (200, 72), (72, 200)])
def test_prepare_and_apply(rows, cols, gdt, nesterov, pdt, master):
    rng = np.random.default_rng(rows * 7 + cols)
    mu, gs, lr, wd, scale = F32(0.95), F32(0.5), F32(0.02), F32(0.1), F32(1.5)
    g = V.decode(V.encode(rng.standard_normal((rows, cols)), gdt), gdt)
    b0 = rng.standard_normal((rows, cols)).astype(np.float32)
    buf64 = mu * b0.astype(np.float64) + g * gs
    u = g * gs + mu * buf64 if nesterov else buf64
    X64 = u / (np.linalg.norm(u) + 1e-7)
    X64 = X64.T if rows > cols else X64
    m, n = X64.shape
    xm, xn, ldx = m + 8, n + 8, n + 16                 # a zero border of 8 inside a pitch gap of 8 that keeps its 0xA5 bytes
    gb = H.DevBuf.from_numpy(np.ascontiguousarray(V.encode(g, gdt)))
    runs = []
    for _ in range(2):
        bb, xb = H.DevBuf.from_numpy(b0), H.DevBuf.from_numpy(np.full(xm * ldx, 0xA5A5, np.uint16))
        H.muon_prepare({"f32": H.F32, "bf16": H.BF16}[gdt], rows, cols, gb.ptr, bb.ptr, mu, nesterov, xb.ptr, xm, xn, ldx, grad_scale=gs)
        runs.append((bb.to_numpy((rows, cols), np.float32), xb.to_numpy((xm, ldx), np.uint16), xb))
    (buf, X, xb), (buf2, X2, _) = runs
    assert np.array_equal(buf.view(np.uint32), buf2.view(np.uint32)) and np.array_equal(X, X2)
    assert within_ulp_f32(buf, buf64, 2)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(X64), 1e-30))) - 7)
    assert np.all(np.abs(V.decode(X[:m, :n], "bf16") - X64) <= ulp)
    assert not X[m:, :xn].any() and not X[:, n:xn].any() and np.all(X[:, xn:] == 0xA5A5)

    p0 = V.decode(V.encode(rng.standard_normal((rows, cols)), pdt), pdt)
    m0 = p0.astype(np.float32) + (rng.standard_normal((rows, cols)) * 1e-4).astype(np.float32) if master else None
    pb, mb, lrb = H.DevBuf.from_numpy(np.ascontiguousarray(V.encode(p0, pdt))), (H.DevBuf.from_numpy(m0) if master else None), H.DevBuf.from_numpy(np.float32([lr]))
    H.muon_apply({"f32": H.F32, "bf16": H.BF16}[pdt], rows, cols, pb.ptr, mb.ptr if master else None, xb.ptr, ldx, lrb.ptr, weight_decay=wd, scale=scale)
    O = V.decode(X[:m, :n], "bf16")
    want = (m0 if master else p0).astype(np.float64) * (1 - lr * wd) - lr * scale * (O.T if rows > cols else O)
    if master:
        got = mb.to_numpy((rows, cols), np.float32)
        assert np.array_equal(pb.to_numpy((rows, cols), np.uint16), V.encode(got, "bf16"))
    elif pdt == "bf16":
        got = V.decode(pb.to_numpy((rows, cols), np.uint16), "bf16")
        half = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 8)
        assert np.all(np.abs(got - want) <= half + 2 * np.spacing(np.abs(want).astype(np.float32)))
        return
    else:
        got = pb.to_numpy((rows, cols), np.float32)
    assert within_ulp_f32(got, want, 2)


def composed_ns(X0):
    """The iteration from kf_gemm calls alone: A = X X^T, B = c A A + b A (C preloaded with A), X = B X + a X (C preloaded with X). Through
    the C ABI, not kfunca.gemm: the operator allocates its own output, so its beta has no preloaded C to act on; it runs the same kf_gemm,
    and the host round trips between the products move bf16 values unchanged, so the roundings fall at the same three points."""
    a, b, c = COEFFS
    m, n = X0.shape
    up = lambda v: H.DevBuf.from_numpy(np.ascontiguousarray(V.encode(v, "bf16")))
    X = X0
    for _ in range(5):
        xb, ab = up(X), H.DevBuf(m * m * 2)
        H.gemm(H.BF16, 0, 1, m, m, n, 1.0, xb.ptr, n, xb.ptr, n, 0.0, ab.ptr, m)
        A = V.decode(ab.to_numpy((m, m), np.uint16), "bf16")
        bb = up(A)
        H.gemm(H.BF16, 0, 0, m, m, m, c, ab.ptr, m, ab.ptr, m, b, bb.ptr, m)
        x2 = up(X)
        H.gemm(H.BF16, 0, 0, m, n, m, 1.0, bb.ptr, m, xb.ptr, n, a, x2.ptr, n)
        X = V.decode(x2.to_numpy((m, n), np.uint16), "bf16")
    return X


@pytest.mark.parametrize("rows,cols", [(128, 256), (256, 128), (384, 1024), (200, 72)])
def test_newton_schulz(rows, cols):
    x = np.random.default_rng(rows + cols).standard_normal((rows, cols)).astype(np.float32)
    xt = kfunca.from_numpy(x, 0)
    wide = lambda t: (lambda v: v.T if rows > cols else v)(t.float().numpy().astype(np.float64))
    X0 = wide(kfunca.newton_schulz(xt, steps=0))
    assert np.all(np.abs(X0 - bf16((x.T if rows > cols else x) / (np.linalg.norm(x.astype(np.float64)) + 1e-7))) <= 2.0 ** -7 * np.abs(X0))
    y = kfunca.newton_schulz(xt)
    assert y.shape(0) == rows and y.shape(1) == cols
    Y, Y64 = wide(y), ns64(X0)
    e_new = np.linalg.norm(Y - Y64) / np.linalg.norm(Y64)
    e_comp = np.linalg.norm(composed_ns(X0) - Y64) / np.linalg.norm(Y64)
    sv = np.linalg.svd(Y, compute_uv=False)
    print(f"newton_schulz {rows}x{cols}: e_new {e_new:.5f} e_composed {e_comp:.5f} singular values [{sv.min():.3f}, {sv.max():.3f}]")
    assert e_new <= 1.5 * e_comp and e_new <= 0.03
    assert 0.6 <= sv.min() and sv.max() <= 1.2


SHAPES = [((128, 256), "f32"), ((256, 128), "bf16"), ((200, 72), "bf16")]
HYPER = dict(lr=0.02, momentum=0.95, weight_decay=0.01)


def make_muon(seed=3):
    rng = np.random.default_rng(seed)
    arrs = [bf16(rng.standard_normal(s)) for s, _ in SHAPES]
    grads = [bf16(rng.standard_normal(s)) for s, _ in SHAPES]
    ps = [kfunca.from_numpy(a.astype(np.float32), 0) for a in arrs]
    ps = [p.bfloat16() if dt == "bf16" else p for p, (_, dt) in zip(ps, SHAPES)]
    for p, g in zip(ps, grads):
        p.set_requires_grad(True)
        gt, ones = kfunca.from_numpy(g.astype(np.float32), 0), kfunca.from_numpy(np.ones(g.shape, np.float32), 0)
        if p.dtype() != gt.dtype():
            gt, ones = gt.bfloat16(), ones.bfloat16()
        (p * ones).backward(gt)                     # p.grad() = g exactly
    return arrs, grads, ps, kfunca.Muon(ps, **HYPER)


def test_muon_step_against_numpy():
    arrs, grads, ps, opt = make_muon()
    assert len(opt) == 3 and opt.lr == pytest.approx(0.02)
    before = kfunca.memstat_dict()
    opt.step()
    kfunca.synchronize()
    assert kfunca.memstat_dict() == before
    lr, mu, wd = F32(0.02), F32(0.95), F32(0.01)
    for a, g, p, (shape, dt) in zip(arrs, grads, ps, SHAPES):
        rows, cols = shape
        u = g + mu * g                                # buf = g after the first step; Nesterov
        X0 = bf16(u / (np.linalg.norm(u) + 1e-7))
        O = ns64(X0.T if rows > cols else X0)
        O = O.T if rows > cols else O
        scale = F32(np.sqrt(max(1.0, rows / cols)))
        want = a * (1 - lr * wd) - lr * scale * O
        buf, master = opt.state(p)
        assert within_ulp_f32(buf.numpy(), g, 2)
        got = (master if dt == "bf16" else p).numpy()
        assert np.linalg.norm(got - want) <= lr * scale * 0.03 * np.linalg.norm(O) + 2 * np.linalg.norm(np.spacing(np.abs(want).astype(np.float32)))
        if dt == "bf16":
            assert np.array_equal(V.encode(p.float().numpy(), "bf16"), V.encode(got, "bf16"))


def test_muon_captured_step_matches_eager():
    (_, _, ps_e, opt_e), (_, _, ps_g, opt_g) = make_muon(), make_muon()
    opt_e.step()
    opt_g.step()
    kfunca.synchronize()
    kfunca.graph_begin()
    opt_g.step()
    graph = kfunca.graph_end()
    try:
        kfunca.graph_launch(graph)
        opt_e.step()
        kfunca.synchronize()
        for a, b in zip(ps_e, ps_g):
            assert np.array_equal(a.float().numpy().view(np.uint32), b.float().numpy().view(np.uint32))
            for x, y in zip(opt_e.state(a), opt_g.state(b)):
                assert (x is None and y is None) or np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    finally:
        kfunca.graph_destroy(graph)


@pytest.mark.parametrize("what,match", [("1d", "AdamW"), ("3d", "AdamW"), ("nonleaf", "non-leaf"), ("momentum", "momentum"), ("ns_steps", "ns_steps"),
                                        ("adjust", "adjust")])
def test_muon_refusals(what, match):
    mk = lambda *s: kfunca.from_numpy(np.ones(s, np.float32), 0)
    p = {"1d": mk(8), "3d": mk(2, 4, 4)}.get(what, mk(4, 8))
    p.set_requires_grad(True)
    if what == "nonleaf":
        p = p * mk(4, 8)
    kw = {"momentum": dict(momentum=1.0), "ns_steps": dict(ns_steps=-1), "adjust": dict(adjust="sqrt")}.get(what, {})
    with pytest.raises(Exception, match=match):
        kfunca.Muon([p], lr=0.02, **kw)
