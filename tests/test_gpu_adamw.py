"""-m gpu: the fused AdamW step (kf_adamw_step and kfunca.AdamW) against CPU torch.optim.AdamW(foreach=False) and
torch.nn.utils.clip_grad_norm_, and against an f64 numpy restatement of the kernel's f32 arithmetic.

Tolerances (stated):
  f32 params vs torch   |got - ref| <= STEPS * 2^-22 (|ref| + 1): torch and the kernel round the same f32 operations, but in places
                        differently (torch's lerp for exp_avg, fused multiply-adds here), a few units of 2^-24 of |p| or of the update per
                        step, and the differences add up over the steps. Every mutation listed in the PR (bias correction with s - 1, eps
                        under the square root, coupled weight decay, beta1 <-> beta2) moves the params by 1e-4 or more.
  exp_avg / exp_avg_sq  rtol 1e-5 + atol 4e-6 (gradient scale 1): a few f32 roundings of terms up to |g| ~ 5 per step
  the clipping norm     rtol 1e-5 (f32 squares summed in a different order; the fold runs in double)
  16-bit params         1 unit in the last place of the 16-bit param against the f64 restatement, checked after every step from the
                        kernel's previous state (f32 and f64 can land on different sides of a 16-bit tie); within one step the f32
                        states to rtol 1e-6 (+ 2e-6 for exp_avg, whose terms cancel) and the master to 2^-21 (|p| + 1)
Bitwise: one call over many tensors == one call per tensor; clipping below the threshold == no clipping; grad_scale c == grads
premultiplied by c; repeated runs; graph replays == eager steps.
"""
import math

import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

STEPS = 20
NP16 = {H.BF16: np.uint16, H.F16: np.float16}
ESIZE = {H.F32: 4, H.BF16: 2, H.F16: 2}


def to16(x, code):
    return O.f32_to_bf16(np.asarray(x, np.float32)) if code == H.BF16 else np.asarray(x, np.float32).astype(np.float16)


def from16(x, code):
    return O.bf16_to_f32(x) if code == H.BF16 else x.astype(np.float32)


def ulp16(x, code):
    """The spacing of the 16-bit grid at |x|."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - (7 if code == H.BF16 else 10))


class AbiTensor:
    """One tensor of a kf_adamw_step call in its own device buffers; `off` = element offsets of (param, grad, master, exp_avg, exp_avg_sq)
    from a 16-byte boundary."""

    def __init__(self, p0, pdt=H.F32, gdt=H.F32, master=False, wd=0.0, off=(0, 0, 0, 0, 0)):
        self.n, self.pdt, self.gdt, self.wd, self.off = p0.size, pdt, gdt, wd, off
        pad = 16
        self.bp, self.bg = H.DevBuf((self.n + pad) * ESIZE[pdt]), H.DevBuf((self.n + pad) * ESIZE[gdt])
        self.bm, self.bv = H.DevBuf((self.n + pad) * 4), H.DevBuf((self.n + pad) * 4)
        self.bms = H.DevBuf((self.n + pad) * 4) if master else None
        self.bs = H.DevBuf(4)
        self.bm.zero(), self.bv.zero(), self.bs.zero()
        self.put(self.bp, off[0], p0 if pdt == H.F32 else to16(p0, pdt))
        if master:
            self.put(self.bms, off[2], from16(to16(p0, pdt), pdt))

    @staticmethod
    def put(buf, off, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            H.check(H.lib().kf_memcpy_h2d(buf.ptr + off * arr.itemsize, arr.ctypes.data, arr.nbytes, None))

    @staticmethod
    def get(buf, off, n, dtype):
        out = np.empty(n, dtype)
        if out.nbytes:
            H.check(H.lib().kf_memcpy_d2h(out.ctypes.data, buf.ptr + off * out.itemsize, out.nbytes, None))
        return out

    def set_grad(self, g):
        self.put(self.bg, self.off[1], g.astype(np.float32) if self.gdt == H.F32 else to16(g, self.gdt))

    def desc(self):
        o = self.off
        return dict(numel=self.n, param_dtype=self.pdt, grad_dtype=self.gdt, param=self.bp.ptr + o[0] * ESIZE[self.pdt],
                    grad=self.bg.ptr + o[1] * ESIZE[self.gdt], master=self.bms.ptr + o[2] * 4 if self.bms else None,
                    exp_avg=self.bm.ptr + o[3] * 4, exp_avg_sq=self.bv.ptr + o[4] * 4, step=self.bs.ptr, weight_decay=self.wd)

    def read(self):
        """(param as f32, exp_avg, exp_avg_sq, step, master or None, raw param)"""
        raw = self.get(self.bp, self.off[0], self.n, np.float32 if self.pdt == H.F32 else NP16[self.pdt])
        p = raw if self.pdt == H.F32 else from16(raw, self.pdt)
        ms = self.get(self.bms, self.off[2], self.n, np.float32) if self.bms else None
        return (p, self.get(self.bm, self.off[3], self.n, np.float32), self.get(self.bv, self.off[4], self.n, np.float32),
                float(self.get(self.bs, 0, 1, np.float32)[0]), ms, raw)


def abi_step(tensors, lr, **kw):
    blr = H.DevBuf.from_numpy(np.array([lr], np.float32))
    need = H.adamw_workspace_bytes(len(tensors), kw.get("max_grad_norm", 0.0))
    ws = H.DevBuf(need) if need else None
    norm = H.DevBuf(4) if need else None
    H.adamw_step([t.desc() for t in tensors], blr.ptr, grad_norm=norm.ptr if norm else None, workspace=ws.ptr if ws else None,
                 workspace_bytes=need, **kw)
    H.device_sync()
    return float(norm.to_numpy((1,), np.float32)[0]) if norm else None


class RefTensor:
    """f64 restatement of the kernel's arithmetic; state rounded to f32 (and the param to 16 bits) where the kernel stores it."""

    def __init__(self, p0, pdt=H.F32, master=False, wd=0.0):
        self.pdt, self.master, self.wd = pdt, master, wd
        self.p = p0.astype(np.float32).astype(np.float64) if pdt == H.F32 else from16(to16(p0, pdt), pdt).astype(np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.s = 0

    def step(self, g, lr, b1, b2, eps, gmul=1.0):
        f32 = lambda x: np.float32(x).astype(np.float64) if np.isscalar(x) else x.astype(np.float32).astype(np.float64)  # noqa: E731
        self.s += 1
        lr = float(np.float32(lr))
        decay, bc2s, nss = f32(1 - lr * float(np.float32(self.wd))), f32(math.sqrt(1 - b2 ** self.s)), f32(-lr / (1 - b1 ** self.s))
        g = f32(g.astype(np.float64) * gmul)
        self.m = f32(f32(b1) * self.m + f32(1 - b1) * g)
        self.v = f32(f32(b2) * self.v + f32(1 - b2) * g * g)
        p = f32(self.p * decay + nss * self.m / (np.sqrt(self.v) / bc2s + f32(eps)))
        self.p = p if (self.pdt == H.F32 or self.master) else from16(to16(p, self.pdt), self.pdt).astype(np.float64)

    def param16(self):
        return self.p if self.pdt == H.F32 else from16(to16(self.p, self.pdt), self.pdt)


def torch_run(p0s, grads, lr, betas, eps, wd, max_norm=None):
    """CPU torch: (params, exp_avg, exp_avg_sq, norms) after len(grads) steps of AdamW(foreach=False), clip_grad_norm_ first when max_norm."""
    import torch
    ps = [torch.tensor(p, dtype=torch.float32, requires_grad=True) for p in p0s]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    norms = []
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.tensor(g, dtype=torch.float32)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)))
        opt.step()
    st = [opt.state[p] if p in opt.state else None for p in ps]
    return ([p.detach().numpy() for p in ps], [s["exp_avg"].numpy() if s else None for s in st],
            [s["exp_avg_sq"].numpy() if s else None for s in st], norms)


def f32_close(got, want, what):
    assert_close(got, want, rtol=STEPS * 2.0 ** -22, atol=STEPS * 2.0 ** -22, what=what)


SIZES = (0, 1, 3, 63, 64, 65, 1_000_007)
HYPER = [  # lr, betas, eps, weight_decay, gradient scale
    (1e-3, (0.9, 0.999), 1e-8, 1e-2, 1.0),
    (3e-3, (0.9, 0.95), 1e-8, 0.1, 1.0),
    (1e-2, (0.8, 0.99), 1e-2, 0.0, 1e-2),   # eps comparable to sqrt(v): under or beside the square root differs
    (5e-3, (0.0, 0.5), 1e-6, 0.05, 3.0),
]


@pytest.mark.parametrize("hyper", range(len(HYPER)))
def test_f32_matches_torch(hyper):
    lr, betas, eps, wd, gscale = HYPER[hyper]
    rng = np.random.default_rng(100 + hyper)
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in SIZES]
    grads = [[(rng.standard_normal(n) * gscale).astype(np.float32) for n in SIZES] for _ in range(STEPS)]
    ts = [AbiTensor(p, wd=wd) for p in p0s]
    for gs in grads:
        for t, g in zip(ts, gs):
            t.set_grad(g)
        assert abi_step(ts, lr, beta1=betas[0], beta2=betas[1], eps=eps) is None
    rp, rm, rv, _ = torch_run(p0s, grads, lr, betas, eps, wd)
    for t, n, p, m, v in zip(ts, SIZES, rp, rm, rv):
        gp, gm, gv, s, _, _ = t.read()
        assert s == STEPS
        f32_close(gp, p, f"param n={n}")
        assert_close(gm, m, rtol=1e-5, atol=4e-6 * gscale, what=f"exp_avg n={n}")
        assert_close(gv, v, rtol=1e-5, atol=4e-6 * gscale ** 2, what=f"exp_avg_sq n={n}")


@pytest.mark.parametrize("off", [(1, 1, 0, 1, 1), (3, 1, 0, 2, 0), (2, 2, 0, 2, 2)])
def test_element_offset_pointers(off):
    """f32 streams starting off 16-byte boundaries: all at the same phase (head + packs + tail) or at different ones (element by element)."""
    rng = np.random.default_rng(7)
    sizes = (5, 70, 4096 * 3 + 11)
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in sizes]
    grads = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(STEPS)]
    ts = [AbiTensor(p, wd=0.1, off=off) for p in p0s]
    for gs in grads:
        for t, g in zip(ts, gs):
            t.set_grad(g)
        abi_step(ts, 3e-3, beta1=0.9, beta2=0.95, eps=1e-8)
    rp, _, _, _ = torch_run(p0s, grads, 3e-3, (0.9, 0.95), 1e-8, 0.1)
    for t, p in zip(ts, rp):
        f32_close(t.read()[0], p, f"offsets {off}")


MIXED = [(H.F32, H.F32, False), (H.BF16, H.F32, True), (H.BF16, H.BF16, False), (H.BF16, H.BF16, True), (H.F16, H.F32, True),
         (H.F16, H.F16, False), (H.BF16, H.F32, False), (H.F16, H.F16, True)]


def test_multi_tensor_equals_one_tensor_at_a_time():
    """300 tensors of mixed sizes, dtypes, offsets and weight decays in ONE call == each tensor in a call of its own, bit for bit."""
    rng = np.random.default_rng(300)
    specs = []
    for i in range(300):
        n = int(rng.choice([0, 1, 7, 64, 100, 4095, 4097, 30000])) if i % 50 else 200_003
        pdt, gdt, master = MIXED[i % len(MIXED)]
        o = int(rng.integers(0, 4))
        off = (o, o, o, o, o) if i % 7 else (1, 0, 2, 3, 0)
        specs.append((rng.uniform(-1, 1, n).astype(np.float32), pdt, gdt, master, float(rng.choice([0.0, 0.01, 0.1])), off))
    grads = [[rng.standard_normal(s[0].size).astype(np.float32) for s in specs] for _ in range(3)]
    together = [AbiTensor(p, pdt, gdt, master, wd, off) for p, pdt, gdt, master, wd, off in specs]
    alone = [AbiTensor(p, pdt, gdt, master, wd, off) for p, pdt, gdt, master, wd, off in specs]
    for gs in grads:
        for a, b, g in zip(together, alone, gs):
            a.set_grad(g)
            b.set_grad(g)
        abi_step(together, 2e-3, beta1=0.9, beta2=0.95, eps=1e-8)
        for b in alone:
            abi_step([b], 2e-3, beta1=0.9, beta2=0.95, eps=1e-8)
    for i, (a, b) in enumerate(zip(together, alone)):
        ra, rb = a.read(), b.read()
        assert ra[3] == rb[3] == 3
        for k in (1, 2, 5):
            assert np.array_equal(ra[k].view(np.uint8), rb[k].view(np.uint8)), (i, k)
        if ra[4] is not None:
            assert np.array_equal(ra[4].view(np.uint32), rb[4].view(np.uint32)), i


@pytest.mark.parametrize("pdt", [H.BF16, H.F16])
@pytest.mark.parametrize("gdt16", [False, True])
@pytest.mark.parametrize("master", [False, True])
def test_16bit_params(pdt, gdt16, master):
    """Step by step against the f64 restatement started from the kernel's own state of the step before: a 16-bit param rounded to the
    other neighbour at one step would otherwise stay one unit off at that step's magnitude, many units of a later, smaller value."""
    rng = np.random.default_rng(16 + pdt + 2 * gdt16 + 4 * master)
    gdt = pdt if gdt16 else H.F32
    sizes = (1, 65, 4096 + 9, 100_003)
    p0s = [rng.uniform(-2, 2, n).astype(np.float32) for n in sizes]
    ts = [AbiTensor(p, pdt, gdt, master, wd=0.05, off=(1, 1, 1, 1, 1) if i == 2 else (0, 0, 0, 0, 0)) for i, p in enumerate(p0s)]
    refs = [RefTensor(p, pdt, master, wd=0.05) for p in p0s]
    for k in range(STEPS):
        for t, r in zip(ts, refs):
            g = rng.standard_normal(t.n).astype(np.float32)
            g = g if gdt == H.F32 else from16(to16(g, gdt), gdt)  # the grad the kernel sees
            t.set_grad(g)
            r.step(g, 1e-2, 0.9, 0.99, 1e-8)
        abi_step(ts, 1e-2, beta1=0.9, beta2=0.99, eps=1e-8)
        for t, r in zip(ts, refs):
            p, m, v, s, ms, raw = t.read()
            assert s == k + 1
            want = r.param16()
            err = np.abs(p - want) / ulp16(want, pdt)
            assert err.max() <= 1.0, f"step {k + 1}: {err.max()} ulp at {np.argmax(err)} (n={t.n})"
            assert_close(m, r.m, rtol=1e-6, atol=2e-6, what="exp_avg")
            assert_close(v, r.v, rtol=1e-6, atol=1e-9, what="exp_avg_sq")
            if master:
                assert_close(ms, r.p, rtol=2.0 ** -21, atol=2.0 ** -21, what="master")
                assert np.array_equal(raw, to16(ms, pdt))  # the 16-bit param is the master rounded to nearest even
            r.p, r.m, r.v = (ms if master else p).astype(np.float64), m.astype(np.float64), v.astype(np.float64)


def test_master_accumulates_updates_below_a_bf16_ulp():
    """p = 1 in bf16 has a spacing of 2^-7 below it; ten AdamW updates of ~1e-3 each move it only through the f32 master."""
    p0 = np.ones(1000, np.float32)
    with_m, without = AbiTensor(p0, H.BF16, H.F32, True), AbiTensor(p0, H.BF16, H.F32, False)
    for _ in range(10):
        for t in (with_m, without):
            t.set_grad(np.ones(1000, np.float32))
        abi_step([with_m, without], 1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    p, _, _, _, ms, _ = with_m.read()
    assert np.all(without.read()[0] == 1.0)
    assert_close(ms, np.full(1000, 1 - 10e-3), rtol=0, atol=1e-5, what="master")
    assert np.all(p == O.bf16_to_f32(O.f32_to_bf16(ms)))
    assert np.all(p < 1.0)


def test_clipping_matches_torch():
    rng = np.random.default_rng(42)
    sizes = (3, 64, 4097, 300_001)
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in sizes]
    grads = [[rng.standard_normal(n).astype(np.float32) * (1 + 3 * (k % 4)) for n in sizes] for k in range(STEPS)]
    max_norm = 100.0  # the gradients' norms run from ~550 to ~2200: clipped every step
    ts = [AbiTensor(p, wd=0.01) for p in p0s]
    norms = []
    for gs in grads:
        for t, g in zip(ts, gs):
            t.set_grad(g)
        norms.append(abi_step(ts, 1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=max_norm))
    rp, _, _, rnorms = torch_run(p0s, grads, 1e-3, (0.9, 0.999), 1e-8, 0.01, max_norm=max_norm)
    assert_close(norms, rnorms, rtol=1e-5, atol=0, what="norm")
    for t, p in zip(ts, rp):
        f32_close(t.read()[0], p, "clipped param")


def test_clipping_below_the_threshold_is_bitwise_no_clipping():
    rng = np.random.default_rng(43)
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in (5, 5000, 70_001)]
    a, b = [AbiTensor(p, wd=0.1) for p in p0s], [AbiTensor(p, wd=0.1) for p in p0s]
    for _ in range(5):
        gs = [rng.standard_normal(p.size).astype(np.float32) * 0.1 for p in p0s]
        for x, y, g in zip(a, b, gs):
            x.set_grad(g)
            y.set_grad(g)
        n = abi_step(a, 1e-2, beta1=0.9, beta2=0.95, eps=1e-8, max_grad_norm=1e4)
        assert 0 < n < 1e4
        abi_step(b, 1e-2, beta1=0.9, beta2=0.95, eps=1e-8)
    for x, y in zip(a, b):
        for k in (0, 1, 2):
            assert np.array_equal(x.read()[k].view(np.uint32), y.read()[k].view(np.uint32))


def test_grad_scale_equals_prescaled_grads():
    rng = np.random.default_rng(44)
    c = 0.37
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, 4096, 50_001)]
    for pdt, gdt, master in ((H.F32, H.F32, False), (H.BF16, H.F32, True)):
        a, b = [AbiTensor(p, pdt, gdt, master, 0.1) for p in p0s], [AbiTensor(p, pdt, gdt, master, 0.1) for p in p0s]
        for _ in range(4):
            gs = [rng.standard_normal(p.size).astype(np.float32) * 5 for p in p0s]
            for x, y, g in zip(a, b, gs):
                x.set_grad(g)
                y.set_grad((g * np.float32(c)).astype(np.float32))
            na = abi_step(a, 1e-2, beta1=0.9, beta2=0.95, eps=1e-8, max_grad_norm=10.0, grad_scale=c)
            nb = abi_step(b, 1e-2, beta1=0.9, beta2=0.95, eps=1e-8, max_grad_norm=10.0)
            assert np.float32(na).view(np.uint32) == np.float32(nb).view(np.uint32) and na > 10
        for x, y in zip(a, b):
            for k in (0, 1, 2, 5):
                assert np.array_equal(x.read()[k].view(np.uint8), y.read()[k].view(np.uint8))


def test_nonfinite_norm_makes_params_nan():
    p0s = [np.ones(n, np.float32) for n in (10, 5000)]
    ts = [AbiTensor(p) for p in p0s]
    ts[0].set_grad(np.ones(10, np.float32))
    g = np.ones(5000, np.float32)
    g[17] = np.nan
    ts[1].set_grad(g)
    assert math.isnan(abi_step(ts, 1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=1.0))
    for t in ts:
        assert np.isnan(t.read()[0]).all()


def test_reproducible_bitwise():
    rng = np.random.default_rng(45)
    p0s = [rng.uniform(-1, 1, n).astype(np.float32) for n in (1, 77, 4096 * 5 + 3, 2_000_001)]
    gs = [rng.standard_normal(p.size).astype(np.float32) for p in p0s]
    outs = []
    for _ in range(2):
        ts = [AbiTensor(p, wd=0.01) for p in p0s]
        norms = []
        for _ in range(3):
            for t, g in zip(ts, gs):
                t.set_grad(g)
            norms.append(abi_step(ts, 1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=50.0))
        outs.append((np.array(norms, np.float32), [t.read() for t in ts]))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32))
    for ra, rb in zip(outs[0][1], outs[1][1]):
        for k in (0, 1, 2):
            assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32))


# ---- the operator API -----------------------------------------------------------------------------------------------------------
def set_grad(p, g):
    """p.grad() = g exactly: the backward of p * 1 with output gradient g (same dtype as p)."""
    ones = kfunca.from_numpy(np.ones(p.sizes(), np.float32), 0)
    gt = kfunca.from_numpy(g.astype(np.float32), 0)
    if p.dtype() != ones.dtype():
        conv = "bfloat16" if p.dtype() == kfunca.from_numpy(np.ones(1, np.float32), 0).bfloat16().dtype() else "half"
        ones, gt = getattr(ones, conv)(), getattr(gt, conv)()
    (p * ones).backward(gt)


def test_api_skips_params_without_grad_and_groups():
    rng = np.random.default_rng(50)
    arrs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (10, 300, 7)]
    ps = [kfunca.from_numpy(a, 0) for a in arrs]
    for p in ps:
        p.set_requires_grad(True)
    opt = kfunca.AdamW([{"params": ps[:2], "weight_decay": 0.0}, {"params": [ps[2]]}], lr=1e-2, weight_decay=0.1)
    assert len(opt) == 3 and opt.lr == pytest.approx(1e-2)
    g0 = rng.standard_normal(10).astype(np.float32)
    g2 = rng.standard_normal(7).astype(np.float32)
    set_grad(ps[0], g0)
    set_grad(ps[2], g2)
    assert opt.step() is None
    rp, _, _, _ = torch_run([arrs[0]], [[g0]], 1e-2, (0.9, 0.999), 1e-8, 0.0)
    f32_close(ps[0].numpy(), rp[0], "group 0")
    rp, _, _, _ = torch_run([arrs[2]], [[g2]], 1e-2, (0.9, 0.999), 1e-8, 0.1)
    f32_close(ps[2].numpy(), rp[0], "group 1")
    assert np.array_equal(ps[1].numpy(), arrs[1])
    m, v, s, ms = opt.state(ps[1])
    assert ms is None and s.numpy()[0] == 0 and not m.numpy().any() and not v.numpy().any()
    assert opt.state(ps[0])[2].numpy()[0] == 1 and opt.state(ps[2])[2].numpy()[0] == 1
    opt.zero_grad()
    assert opt.step() is None  # nothing has a grad: nothing moves
    assert opt.state(ps[0])[2].numpy()[0] == 1
    with pytest.raises(ValueError):
        kfunca.AdamW([{"params": ps, "lr": 1e-3}])


def test_api_graph_capture_and_set_lr():
    rng = np.random.default_rng(51)
    arrs = [rng.uniform(-1, 1, n).astype(np.float32) for n in (100, 70_001, 5)]
    grads = [rng.standard_normal(a.size).astype(np.float32) for a in arrs]

    def make():
        ps = [kfunca.from_numpy(a, 0).bfloat16() if i == 1 else kfunca.from_numpy(a, 0) for i, a in enumerate(arrs)]
        for p, g in zip(ps, grads):
            p.set_requires_grad(True)
            set_grad(p, g)
        return ps, kfunca.AdamW(ps, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05, max_grad_norm=5.0)

    ps_e, opt_e = make()
    ps_g, opt_g = make()
    kfunca.synchronize()
    kfunca.graph_begin()
    norm_g = opt_g.step()
    with pytest.raises(RuntimeError):
        opt_g.set_lr(1.0)
    graph = kfunca.graph_end()
    try:
        for k in range(4):
            if k == 2:
                opt_e.set_lr(3e-3)
                opt_g.set_lr(3e-3)
            norm_e = opt_e.step()
            kfunca.graph_launch(graph)
            kfunca.synchronize()
            assert norm_e.numpy().view(np.uint32)[0] == norm_g.numpy().view(np.uint32)[0]
            for a, b in zip(ps_e, ps_g):
                assert np.array_equal(a.numpy(), b.numpy()), k
                for x, y in zip(opt_e.state(a)[:3], opt_g.state(b)[:3]):
                    assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32)), k
        assert opt_g.state(ps_g[0])[2].numpy()[0] == 4
        # the rate changed between replays took effect: the same graph without the change would not match these steps
        ps_c, opt_c = make()
        for _ in range(4):
            opt_c.step()
        assert not np.array_equal(ps_c[1].numpy(), ps_g[1].numpy())
    finally:
        kfunca.graph_destroy(graph)


def lm_data(seed=5, vocab=257, d=64, n=96):
    rng = np.random.default_rng(seed)
    table = rng.uniform(-1, 1, (vocab, d)).astype(np.float32)
    w_norm = rng.uniform(0.5, 1.5, d).astype(np.float32)
    head = rng.uniform(-0.3, 0.3, (d, vocab)).astype(np.float32)
    tokens = rng.integers(0, vocab, n)
    target = np.r_[tokens[1:], -100]
    return table, w_norm, head, tokens, target


def torch_lm_losses(steps, lr, wd):
    import torch
    import torch.nn.functional as F
    table, w_norm, head, tokens, target = lm_data()
    rt, rw, rh = (torch.tensor(a, requires_grad=True) for a in (table, w_norm, head))
    opt = torch.optim.AdamW([rt, rw, rh], lr=lr, weight_decay=wd, foreach=False)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        e = rt[torch.tensor(tokens)]
        hh = e * torch.rsqrt((e * e).mean(-1, keepdim=True) + 1e-5) * rw
        loss = F.cross_entropy(hh @ rh, torch.tensor(target))
        loss.backward()
        opt.step()
        out.append(loss.item())
    return np.array(out)


def kf_lm_losses(steps, lr, wd, bf16=False):
    table, w_norm, head, tokens, target = lm_data()
    ps = [kfunca.from_numpy(a, 0) for a in (table, w_norm, head)]
    if bf16:
        ps = [p.bfloat16() for p in ps]
    for p in ps:
        p.set_requires_grad(True)
    bucket = None
    if bf16:
        bucket = kfunca.GradBucket(ps, 1.0, True)
        bucket.attach()
    opt = kfunca.AdamW(ps, lr=lr, weight_decay=wd)
    tok, tgt, one = kfunca.from_numpy(tokens, 0), kfunca.from_numpy(target, 0), kfunca.from_numpy(np.ones(1, np.float32), 0)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        h = kfunca.rms_norm(kfunca.embedding(ps[0], tok), ps[1], 1e-5)
        loss = kfunca.cross_entropy(kfunca.gemm(h, ps[2], 1.0, 0.0), tgt)
        loss.backward(one)
        if bucket is not None:
            bucket.wait()
            assert all(p.grad().dtype() == one.dtype() for p in ps)  # f32 views of the bucket
        opt.step()
        out.append(float(loss.numpy()[0]))
    return np.array(out), ps, opt


def test_tiny_lm_trains_like_torch():
    """embedding -> rms_norm -> gemm head -> cross_entropy, 30 AdamW steps: the losses track torch-CPU's within 2e-3 relative (f32 models:
    the gradients agree to ~1e-6 relative; an element whose gradient is rounding noise takes a full +-lr Adam step either way, which
    moves the loss by ~1e-4) and the loss falls."""
    steps = 30
    want = torch_lm_losses(steps, 1e-2, 0.01)
    got, _, _ = kf_lm_losses(steps, 1e-2, 0.01)
    assert_close(got, want, rtol=2e-3, atol=1e-4, what="losses")
    assert got[-1] < 0.5 * got[0]


def test_tiny_lm_bf16_with_grad_bucket_and_masters():
    """bf16 params, f32 gradients in a GradBucket(accum_f32=True) (one GPU, no communicator), f32 masters: the loss falls like the f32
    model's (bf16 rounding of the weights and activations: within 5 %), and every param is its master rounded to nearest even."""
    steps = 30
    want = torch_lm_losses(steps, 1e-2, 0.01)
    got, ps, opt = kf_lm_losses(steps, 1e-2, 0.01, bf16=True)
    assert got[-1] < 0.5 * got[0]
    assert_close(got, want, rtol=5e-2, atol=1e-2, what="bf16 losses")
    for p in ps:
        m, v, s, ms = opt.state(p)
        assert s.numpy()[0] == steps and ms is not None
        assert np.array_equal(p.numpy(), O.f32_to_bf16(ms.numpy()))


@pytest.mark.slow
def test_f32_beyond_2_31_elements():
    """One f32 tensor of 2^31 + 1000 elements (4 x 8.6 GB): elements on both sides of 2^31 and the last one against the f64
    restatement, and the norm. Params and grads are a random tile repeated (element i holds tile[i % T])."""
    n, T = (1 << 31) + 1000, 1 << 20
    rng = np.random.default_rng(231)
    tp, tg = rng.uniform(-1, 1, T).astype(np.float32), rng.standard_normal(T).astype(np.float32)
    t = AbiTensor(np.zeros(0, np.float32))
    t.n = n
    t.bp, t.bg, t.bm, t.bv = H.DevBuf(n * 4), H.DevBuf(n * 4), H.DevBuf(n * 4), H.DevBuf(n * 4)
    t.bm.zero(), t.bv.zero()
    for buf, tile in ((t.bp, tp), (t.bg, tg)):
        AbiTensor.put(buf, 0, tile)
        have = T
        while have < n:
            k = min(have, n - have)
            H.check(H.lib().kf_memcpy_d2d(buf.ptr + have * 4, buf.ptr, k * 4, None))
            have += k
    H.device_sync()
    norm = abi_step([t], 1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=math.inf)
    full, rest = divmod(n, T)
    want_norm = math.sqrt(full * float(np.sum(tg.astype(np.float64) ** 2)) + float(np.sum(tg[:rest].astype(np.float64) ** 2)))
    assert abs(norm - want_norm) <= 1e-5 * want_norm
    for i in (0, (1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, n - 1):
        r = RefTensor(tp[i % T:i % T + 1], wd=0.0)
        r.step(tg[i % T:i % T + 1], 1e-3, 0.9, 0.999, 1e-8)
        got = AbiTensor.get(t.bp, i, 1, np.float32)
        assert_close(got, r.p, rtol=2.0 ** -22, atol=2.0 ** -22, what=f"element {i}")
        assert AbiTensor.get(t.bs, 0, 1, np.float32)[0] == 1
