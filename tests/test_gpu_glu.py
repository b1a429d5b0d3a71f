"""-m gpu: gated activations (kf_glu_fwd, kf_glu_bwd, kfunca.swiglu / geglu / silu / gelu) against an f64 reference on the float
values of the stored inputs, against torch-CPU, bit for bit where the ABI promises it, and through a small gated MLP end to end.

The bound per element (the issue's):

    |got - ref| <= r |ref| + k 2^-24 (1 + |g|) M + 2^-126 (1 + |g|) A

r |ref| one output rounding (r = 2^-8 bf16, 2^-11 f16, 0 for f32: folded into k) and never less than half the spacing of the format's
subnormals (2^-25 f16, 2^-134 bf16, 2^-150 f32), which is what one rounding is below the smallest normal (6.1e-5 in f16: dgate near the zero of
act' at g = -1.28 gets there with ordinary inputs, and the correctly rounded f16 of the exact result would miss r |ref| too); M the magnitude of the result with no cancellation (|ref|
for h and dup; |dh u| (|a(g)| + |g b(g)|) for dgate, act' = a + g b); A the product of the other factors (|u|, |dh|, |dh u|).
a, b:  SiLU sigma, sigma (1 - sigma);  GELU-tanh s, s (1 - s) w'(g) with s = sigma(w), w = 2 sqrt(2/pi) (g + 0.044715 g^3);
GELU-erf Phi(g), phi(g).

k: `model()` below is the kernel's f32 sequence in numpy (exp2, rcp and erfc correctly rounded, every other operation rounded as the
hardware rounds it). Over 3.8 M samples (g over [-110, 110], U(-12, 12), N(0, 1) and U(-15, -5), the tails where the two GELU forms
are worst; u in [-4, 4], dh in [-2, 2]; two seeds) its largest error in units of 2^-24 (1 + |g|) M, with no NaN, is
    SiLU       h / dup 3.4,  dgate 4.7     k = 8  (the issue's)
    GELU-tanh  h / dup 14.8, dgate 14.5    k = 16 (next power of two; at g = -8.5 .. -8.9, where w = 92 log 2 and the three roundings
                                                   of w's f32 evaluation, 1.5 ulp, reach the exponent as 92 x 1.5 x 2^-24)
    GELU-erf   h / dup 10.6, dgate 9.8     k = 16 (next power of two; at g = -11.5: erfc's tail turns the one rounding of g / sqrt 2
                                                   into g^2 2^-24, 12 (1 + |g|) 2^-24 where Phi leaves the normal range at g = -13)
(test_model_stays_below_k recomputes them on fewer samples). torch parity: twice the bound (both sides round); for the two GELU forms on g >= -2, where torch's own 1 + tanh / 1 + erf has not
cancelled beyond it (test_against_torch_cpu).
End to end: f32 loss 1e-5 relative, gradients rtol 1e-3 / atol 1e-5; bf16 loss 2e-2 relative, gradients 6 % of each tensor's max
(bf16 rounding of every operand, as in tests/test_gpu_rope.py).
"""
import math

import numpy as np
import pytest

import kfunca_amd as kfunca
from kfunca_amd import hip_abi as H
from oracle import oracle as O
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

SILU, TANH, ERF = H.ACT_SILU, H.ACT_GELU_TANH, H.ACT_GELU_ERF
ACTS = [SILU, TANH, ERF]
CODES = [H.F32, H.BF16, H.F16]
K = {SILU: 8.0, TANH: 16.0, ERF: 16.0}
OUT_R = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 0.0}
OUT_HALF_SPACING = {H.BF16: 2.0 ** -134, H.F16: 2.0 ** -25, H.F32: 2.0 ** -150}   # one rounding below the smallest normal
ES = {H.BF16: 2, H.F16: 2, H.F32: 4}
UINT = {H.BF16: np.uint16, H.F16: np.uint16, H.F32: np.uint32}
GUARD = 64          # elements before and after every buffer: 128 or 256 bytes, so the base stays 16-byte aligned
MODEL_N = 400_000
WORST = {}          # (act, output, dtype) -> the largest fraction of the bound met in this run (printed by the last test)

C1 = 2.0 * math.sqrt(2.0 / math.pi)
C3 = C1 * 0.044715
LOG2E = 1.0 / math.log(2.0)


def erfc64(x):
    import torch
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(x, np.float64))).numpy()


def sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ref(act, g, u=None, dh=None):
    """f64 on the given float values. Returns {name: (value, M, A)} for h and, with dh, dup and dgate (u = None: ungated)."""
    g = np.asarray(g, np.float64)
    one = np.ones_like(g)
    u = one if u is None else np.asarray(u, np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if act == SILU:
            s = sigmoid64(g)
            a, b = s, s * sigmoid64(-g)
            actv = g * s
        elif act == TANH:
            w = C1 * g + C3 * g ** 3
            s = sigmoid64(w)
            sq = s * sigmoid64(-w)
            a, b = s, np.where(sq == 0, 0.0, sq * (C1 + 3 * C3 * np.minimum(g * g, 1e300)))
            actv = g * s
        else:
            a = 0.5 * erfc64(-g / math.sqrt(2.0))
            b = np.exp(-0.5 * np.minimum(g * g, 1e300)) / math.sqrt(2.0 * math.pi)
            actv = np.where(a == 0, 0.0, g * a)
        out = {"h": (actv * u, np.abs(actv * u), np.abs(u))}
        if dh is not None:
            dh = np.asarray(dh, np.float64)
            gb = np.where(b == 0, 0.0, g * b)
            out["dup"] = (dh * actv, np.abs(dh * actv), np.abs(dh))
            out["dgate"] = (dh * u * (a + gb), np.abs(dh * u) * (np.abs(a) + np.abs(gb)), np.abs(dh * u))
    return out


def bound(act, code, g, val, M, A, scale=1.0):
    g1 = 1.0 + np.abs(np.asarray(g, np.float64))
    return scale * (np.maximum(OUT_R[code] * np.abs(val), OUT_HALF_SPACING[code]) + K[act] * 2.0 ** -24 * g1 * M + 2.0 ** -126 * g1 * A)


def check(act, code, g, got, want, what, scale=1.0):
    """got: {name: float values}; want: ref(...). Asserts the bound and records the largest fraction of it."""
    for name, gv in got.items():
        val, M, A = want[name]
        gv = np.asarray(gv, np.float64)
        assert np.isfinite(gv[np.isfinite(val)]).all(), (what, name, "non-finite result for a finite reference")
        err = np.abs(gv - val)
        tol = bound(act, code, g, val, M, A, scale)
        bad = ~(err <= tol)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = np.where(tol > 0, err / tol, 0.0)
        if frac.size:
            WORST[(act, name, code)] = max(WORST.get((act, name, code), 0.0), float(np.nanmax(frac)))
        assert not bad.any(), (what, name, int(bad.sum()), float(np.nanmax(frac)), np.argwhere(bad)[:3].tolist(),
                               np.asarray(g, np.float64)[bad][:3].tolist())


# ---- the kernel's f32 sequence in numpy -------------------------------------------------------------------------------------------
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)   # a b exact in f64; one rounding to f64 below f32's


def _sigmoid_parts(t, nonneg):
    e = np.exp2(-t.astype(np.float64)).astype(f32)
    r = (1.0 / (f32(1) + e).astype(np.float64)).astype(f32)
    er = e * r
    return np.where(nonneg, r, er), np.where(nonneg, er, r), er * r


def model(act, g, u, dh):
    """(h, dup, dgate) as f32, operation by operation as glu.hip writes them."""
    g, u, dh = (np.asarray(x, f32) for x in (g, u, dh))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if act == SILU:
            s, q, _ = _sigmoid_parts(np.abs(g) * f32(LOG2E), g >= 0)
            a = g * s
            d = s * _fma(g, q, np.ones_like(g))
        elif act == TANH:
            g2 = g * g
            s, _, sq = _sigmoid_parts(np.abs(g) * _fma(np.full_like(g, f32(C3 * LOG2E)), g2, np.full_like(g, f32(C1 * LOG2E))), g >= 0)
            a = g * s
            d = _fma(g, sq * _fma(np.full_like(g, f32(3 * C3)), np.minimum(g2, f32(1e30)), np.full_like(g, f32(C1))), s)
        else:
            c = f32(1.0 / math.sqrt(2.0))
            x = _fma(-g, np.full_like(g, c), -g * f32(1.0 / math.sqrt(2.0) - float(c)))
            p = f32(0.5) * erfc64(x.astype(np.float64)).astype(f32)
            a = g * p
            ph = np.exp2((g * g * f32(-0.5 * LOG2E)).astype(np.float64)).astype(f32) * f32(1.0 / math.sqrt(2.0 * math.pi))
            d = _fma(g, ph, p)
        return a * u, dh * a, dh * u * d


def test_model_stays_below_k():
    rng = np.random.default_rng(1)
    n = MODEL_N
    for act in ACTS:
        worst = {"h": 0.0, "dup": 0.0, "dgate": 0.0}
        for g in (rng.uniform(-110, 110, n), rng.uniform(-12, 12, n), rng.normal(0, 1, n), rng.uniform(-15, -5, n)):
            g = g.astype(f32)
            u, dh = rng.uniform(-4, 4, n).astype(f32), rng.uniform(-2, 2, n).astype(f32)
            got = dict(zip(("h", "dup", "dgate"), model(act, g, u, dh)))
            want = ref(act, g, u, dh)
            for name in worst:
                val, M, A = want[name]
                assert np.isfinite(got[name]).all()
                g1 = 1.0 + np.abs(g.astype(np.float64))
                over = np.maximum(np.abs(got[name].astype(np.float64) - val) - 2.0 ** -126 * g1 * A, 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst[name] = max(worst[name], float(np.nanmax(np.where(M > 0, over / (2.0 ** -24 * g1 * M), 0.0))))
        print(f"model act {act}: {worst} (k = {K[act]})")
        assert max(worst.values()) <= K[act], (act, worst)


# ---- device buffers with guards -----------------------------------------------------------------------------------------------------
def bits(x, code):
    return O.from_float(np.asarray(x, np.float32), code).view(UINT[code])


def floats(b, code):
    b = np.ascontiguousarray(b)
    if code == H.BF16:
        return O.bf16_to_f32(b.view(np.uint16)).astype(np.float64)
    return b.view(np.float16 if code == H.F16 else np.float32).astype(np.float64)


class Buf:
    """rows x width elements at leading dimension ld, `off` elements past a 16-byte boundary, random bits everywhere else."""

    def __init__(self, rng, code, rows, width, ld=None, off=0):
        self.code, self.rows, self.width, self.ld = code, rows, width, width if ld is None else ld
        self.base = GUARD + off
        self.host = rng.integers(0, 1 << (8 * ES[code]), self.base + rows * self.ld + GUARD, dtype=np.uint64).astype(UINT[code])
        self.dev = None

    def idx(self, col0, F):
        return self.base + np.arange(self.rows)[:, None] * self.ld + col0 + np.arange(F)[None, :]

    def put(self, b, col0=0):
        self.host[self.idx(col0, b.shape[1])] = b
        return self

    def up(self):
        self.dev = H.DevBuf.from_numpy(self.host)
        return self

    def ptr(self, col0=0):
        return self.dev.ptr + (self.base + col0) * ES[self.code]

    def get(self, col0, F, written=None):
        """The [rows, F] block at col0; everything outside the written blocks (default: this one) must hold its old bits."""
        after = self.dev.to_numpy(self.host.shape, UINT[self.code])
        mask = np.ones(after.shape, bool)
        for c0, f in (written if written is not None else [(col0, F)]):
            mask[self.idx(c0, f)] = False
        assert np.array_equal(after[mask], self.host[mask]), "bytes outside the output were written"
        return after[self.idx(col0, F)]


def run(code, act, g, u=None, dh=None, form="dense", lds=None, offs=None, alias=(), seed=0, stream=None, sync=True):
    """Through the C ABI. g, u, dh: [rows, F] bit patterns (u = None: ungated; dh = None: forward only). form "packed": gate | up in
    one buffer of leading dimension lds['x'] (default 2F), the gradient packed the same way. lds / offs: per-buffer leading dimension and
    base offset in elements (keys x, g, u, dh, h, dx, dg, du). alias: any of 'h=g', 'h=u', 'dg=g', 'du=u'. Returns {name: bits}."""
    rng = np.random.default_rng(seed)
    rows, F = g.shape
    lds, offs = lds or {}, offs or {}
    mk = lambda name, width: Buf(rng, code, rows, width, lds.get(name, width), offs.get(name, 0))  # noqa: E731
    packed = form == "packed"
    if packed:
        X = mk("x", 2 * F).put(g).put(u, F).up()
        G, Uu, gc, uc = X, X, 0, F
    else:
        G, gc = mk("g", F).put(g).up(), 0
        Uu, uc = (mk("u", F).put(u).up(), 0) if u is not None else (None, 0)
    out = {}
    gp, up_ = G.ptr(gc), Uu.ptr(uc) if Uu is not None else None
    ldu = Uu.ld if Uu is not None else 0
    if dh is None or not any(a.startswith("d") for a in alias):   # (an aliased backward overwrites the inputs: forward not run with it)
        if "h=g" in alias:
            Hb, hc = G, gc
        elif "h=u" in alias:
            Hb, hc = Uu, uc
        else:
            Hb, hc = mk("h", F).up(), 0
        H.glu_fwd(act, code, rows, F, gp, G.ld, up_, ldu, Hb.ptr(hc), Hb.ld, stream)
        if sync:
            H.device_sync()
            if Hb is G or Hb is Uu:   # in place: the buffer's other contents (the other half, paddings, guards) stay
                Hb.host[Hb.idx(hc, F)] = out["h"] = Hb.get(hc, F)
                out["_restore"] = True
            else:
                out["h"] = Hb.get(hc, F)
        out["_keep"] = (G, Uu, Hb)
    if dh is not None and "h=g" not in alias and "h=u" not in alias:
        D = mk("dh", F).put(dh).up()
        if packed and not alias:
            DX = mk("dx", 2 * F).up()
            DG, DU, dgc, duc = DX, DX, 0, F
        else:
            DG, dgc = (G, gc) if "dg=g" in alias else (mk("dg", F).up(), 0)
            DU, duc = (None, 0) if u is None else ((Uu, uc) if "du=u" in alias else (mk("du", F).up(), 0))
        H.glu_bwd(act, code, rows, F, gp, G.ld, up_, ldu, D.ptr(), D.ld, DG.ptr(dgc), DG.ld, DU.ptr(duc) if DU is not None else None,
                  DU.ld if DU is not None else 0, stream)
        if sync:
            H.device_sync()
            written = {}
            for b, c in ((DG, dgc),) + (((DU, duc),) if DU is not None else ()):
                written.setdefault(id(b), (b, []))[1].append((c, F))
            out["dgate"] = DG.get(dgc, F, written[id(DG)][1])
            if DU is not None:
                out["dup"] = DU.get(duc, F, written[id(DU)][1])
        out["_keep2"] = (D, DG, DU)
    return out


def draw(rng, code, rows, F, spread=6.0):
    g = bits(rng.normal(0, spread / 3, (rows, F)), code)
    u = bits(rng.uniform(-4, 4, (rows, F)), code)
    dh = bits(rng.uniform(-2, 2, (rows, F)), code)
    return g, u, dh


def verify(code, act, g, u, dh, out, what):
    want = ref(act, floats(g, code), None if u is None else floats(u, code), None if dh is None else floats(dh, code))
    got = {k: floats(v, code) for k, v in out.items() if not k.startswith("_")}
    check(act, code, floats(g, code), got, want, what)


FORMS = {
    "packed": dict(form="packed"),
    "packed, padded rows, base + 1": dict(form="packed", lds={"x": None, "dx": None, "h": None}, offs={"x": 1, "h": 1, "dh": 1, "dx": 1}),
    "dense": dict(),
    "mixed leading dimensions": dict(lds={"g": 3, "u": 17, "h": 8, "dh": 5, "dg": 16, "du": 1}, offs={"u": 1, "dg": 1}),
    "ungated": dict(ungated=True),
    "ungated, base + 1": dict(ungated=True, offs={"g": 1, "h": 1, "dh": 1, "dg": 1}, lds={"g": 7}),
}


def layout(spec, F):
    """lds in FORMS are paddings added to the natural width (None: + 24 elements on a packed row)."""
    spec = dict(spec)
    ungated = spec.pop("ungated", False)
    nat = {"x": 2 * F, "dx": 2 * F}
    if "lds" in spec:
        spec["lds"] = {k: nat.get(k, F) + (24 if v is None else v) for k, v in spec["lds"].items()}
    return spec, ungated


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("form", list(FORMS))
def test_accuracy_forward_and_backward(code, act, form):
    for F in (1, 7, 8, 63, 64, 1000, 4097, 14336):
        rows = 3 if F > 1000 else 9
        rng = np.random.default_rng(F + 31 * act + 7 * code)
        g, u, dh = draw(rng, code, rows, F)
        spec, ungated = layout(FORMS[form], F)
        if ungated:
            u = None
        verify(code, act, g, u, dh, run(code, act, g, u, dh, seed=F, **spec), f"{form}, F {F}")


@pytest.mark.parametrize("code,F,rows", [(H.BF16, 64, 200_000), (H.F32, 64, 100_000), (H.F16, 63, 30_000), (H.BF16, 8, 1), (H.F32, 1, 1),
                                         (H.BF16, 14336, 1)])
def test_rows_from_one_to_several_grid_stride_rounds(code, F, rows):
    """The grid is capped at 2048 blocks of 256 threads (524288 packs or elements per round): 3 rounds on both paths, and single rows."""
    rng = np.random.default_rng(rows + F)
    g, u, dh = draw(rng, code, rows, F)
    if rows > 1:
        assert rows * (F // (16 // ES[code]) if F % (16 // ES[code]) == 0 else F) > 3 * 2048 * 256
    for act in ACTS if rows == 1 else (SILU,):
        verify(code, act, g, u, dh, run(code, act, g, u, dh, form="packed"), f"rows {rows}")


EXTREME_G = [-110.0, -89.0, -88.0, -20.0, -1e-30, 0.0, 1e-30, 20.0, 88.0, 110.0, -10.05, -13.0, -14.1, 5.0, -5.5]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
def test_extreme_inputs_are_finite_and_within_the_bound(code, act):
    big = {H.F32: 3.0e38, H.BF16: float(O.bf16_to_f32(np.array([0x7F7F], np.uint16))[0]), H.F16: 65504.0}[code]
    gs = np.array(EXTREME_G + [big, -big, big / 4, -big / 4], np.float64)
    us = np.array([1.0, -0.75, 0.5, 2.0 ** -20, 0.0])
    us = us[np.abs(us) <= 1.0]   # |u| <= 1: the product with the largest finite g stays in range
    dhs = np.array([1.0, -0.5, 2.0 ** -10])
    G3, U3, D3 = np.meshgrid(gs, us, dhs, indexing="ij")
    F = 8 * ((G3.size + 7) // 8)
    pad = lambda a: np.resize(a.reshape(-1), F).reshape(1, F)  # noqa: E731
    g, u, dh = bits(pad(G3), code), bits(pad(U3), code), bits(pad(D3), code)
    for spec in (dict(form="packed"), dict(offs={"g": 1})):   # both paths
        out = run(code, act, g, u, dh, **spec)
        for k, v in out.items():
            if not k.startswith("_"):
                assert np.isfinite(floats(v, code)).all(), (k, floats(g, code)[~np.isfinite(floats(v, code))][:4])
        verify(code, act, g, u, dh, out, "extremes")
    out = run(code, act, g, None, dh)
    verify(code, act, g, None, dh, out, "extremes, ungated")


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
def test_nan_propagates_and_infinities_are_as_documented(code, act):
    F = 16
    g = np.full((1, F), 0.5)
    u = np.full((1, F), 2.0)
    dh = np.ones((1, F))
    g[0, 1], u[0, 2], dh[0, 3] = np.nan, np.nan, np.nan
    g[0, 4], g[0, 5] = np.inf, -np.inf
    for spec in (dict(form="packed"), dict(offs={"g": 1})):
        out = run(code, act, bits(g, code), bits(u, code), bits(dh, code), **spec)
        h, dg, du = (floats(out[k], code)[0] for k in ("h", "dgate", "dup"))
        assert np.isnan(h[[1, 2]]).all() and np.isnan(dg[[1, 2, 3]]).all() and np.isnan(du[[1, 3]]).all()
        assert h[4] == np.inf and np.isnan(h[5])   # +inf * u; -inf * 0
        clean = [0] + list(range(6, F))
        assert np.isfinite(h[clean]).all() and np.isfinite(dg[clean]).all() and np.isfinite(du[clean]).all()
        assert np.isfinite(h[3]) and np.isfinite(du[2])


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("F,off", [(64, 0), (61, 0), (64, 1)])
def test_every_allowed_alias_equals_the_out_of_place_call(code, act, F, off):
    rng = np.random.default_rng(F + off + act)
    g, u, dh = draw(rng, code, 21, F)
    offs = {k: off for k in ("x", "g", "u", "h", "dh", "dx", "dg", "du")}
    for form in ("packed", "dense"):
        base = run(code, act, g, u, dh, form=form, offs=offs)
        for al in ("h=g", "h=u"):
            assert np.array_equal(run(code, act, g, u, None, form=form, offs=offs, alias=(al,))["h"], base["h"]), (form, al)
        for al in (("dg=g",), ("du=u",), ("dg=g", "du=u")):
            got = run(code, act, g, u, dh, form=form, offs=offs, alias=al)
            assert np.array_equal(got["dgate"], base["dgate"]) and np.array_equal(got["dup"], base["dup"]), (form, al)
    base = run(code, act, g, None, dh, offs=offs)
    assert np.array_equal(run(code, act, g, None, None, offs=offs, alias=("h=g",))["h"], base["h"])
    assert np.array_equal(run(code, act, g, None, dh, offs=offs, alias=("dg=g",))["dgate"], base["dgate"])


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
def test_packed_equals_two_tensors_and_vector_path_equals_scalar_path(code, act):
    rng = np.random.default_rng(3 + act)
    g, u, dh = draw(rng, code, 33, 256, spread=30.0)
    H.profile_reset()
    H.profile_enable(True)
    try:
        packed = run(code, act, g, u, dh, form="packed")
        names_v = set(H.profile_results())
        H.profile_reset()
        shifted = run(code, act, g, u, dh, form="packed", offs={"x": 1, "h": 1, "dh": 1, "dx": 1})   # the same values one element further
        names_s = set(H.profile_results())
    finally:
        H.profile_enable(False)
    assert {"glu_fwd_vec", "glu_bwd_vec"} <= names_v and {"glu_fwd_elem", "glu_bwd_elem"} <= names_s, (names_v, names_s)
    dense = run(code, act, g, u, dh)
    padded = run(code, act, g, u, dh, lds={"g": 264, "u": 512, "h": 272, "dh": 256, "dg": 280, "du": 264})
    odd = run(code, act, g, u, dh, lds={"g": 257, "u": 259})
    for other in (shifted, dense, padded, odd):
        for k in ("h", "dgate", "dup"):
            assert np.array_equal(other[k], packed[k]), k


def test_repeated_runs_and_graph_replay_are_identical():
    rng = np.random.default_rng(9)
    code, rows, F = H.BF16, 257, 1024
    g, u, dh = draw(rng, code, rows, F)
    a, b = run(code, SILU, g, u, dh, form="packed"), run(code, SILU, g, u, dh, form="packed")
    assert all(np.array_equal(a[k], b[k]) for k in ("h", "dgate", "dup"))
    X = Buf(rng, code, rows, 2 * F).put(g).put(u, F).up()
    D = Buf(rng, code, rows, F).put(dh).up()
    Hb, DX = Buf(rng, code, rows, F).up(), Buf(rng, code, rows, 2 * F).up()
    st = H.Stream()
    with H.Graph.capture(st) as graph:
        H.glu_fwd(SILU, code, rows, F, X.ptr(), 2 * F, X.ptr(F), 2 * F, Hb.ptr(), F, st.handle)
        H.glu_bwd(SILU, code, rows, F, X.ptr(), 2 * F, X.ptr(F), 2 * F, D.ptr(), F, DX.ptr(), 2 * F, DX.ptr(F), 2 * F, st.handle)
    for _ in range(2):
        graph.launch()
        st.sync()
        assert np.array_equal(Hb.get(0, F), a["h"])
        assert np.array_equal(DX.get(0, F, [(0, 2 * F)]), a["dgate"]) and np.array_equal(DX.get(F, F, [(0, 2 * F)]), a["dup"])
        Hb.dev.zero()
        DX.dev.zero()
        H.device_sync()
        Hb.host[:] = 0
        DX.host[:] = 0
    # new inputs written in place are followed by the replay
    g2, u2, _ = draw(np.random.default_rng(10), code, rows, F)
    X.put(g2).put(u2, F)
    H.check(H.lib().kf_memcpy_h2d(X.dev.ptr, X.host.ctypes.data, X.host.nbytes, None))
    graph.launch()
    st.sync()
    assert np.array_equal(Hb.get(0, F), run(code, SILU, g2, u2, None, form="packed")["h"])


@pytest.mark.slow
def test_row_offsets_beyond_2_31_elements():
    """bf16 packed, 5 rows at a leading dimension of 2^29 + 8 elements: rows * ld = 2.7e9, the last row starts at element 2^31 + 32.
    Only the rows' own F or 2F elements are touched; every row is checked, both directions."""
    code, rows, F, ld = H.BF16, 5, 4096, (1 << 29) + 8
    assert rows * ld > 1 << 31 and (rows - 1) * ld > 1 << 31
    rng = np.random.default_rng(41)
    g, u, dh = draw(rng, code, rows, F)
    bx, bh, bdx = (H.DevBuf(((rows - 1) * ld + 2 * F) * 2) for _ in range(3))
    bd = H.DevBuf.from_numpy(dh)
    for r in range(rows):
        row = np.concatenate([g[r], u[r]])
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r * ld * 2, row.ctypes.data, row.nbytes, None))
    H.glu_fwd(SILU, code, rows, F, bx.ptr, ld, bx.ptr + 2 * F, ld, bh.ptr, ld)
    H.glu_bwd(SILU, code, rows, F, bx.ptr, ld, bx.ptr + 2 * F, ld, bd.ptr, F, bdx.ptr, ld, bdx.ptr + 2 * F, ld)
    H.device_sync()
    small = run(code, SILU, g, u, dh, form="packed")
    for r in range(rows):
        hrow, dxrow = np.empty(F, np.uint16), np.empty(2 * F, np.uint16)
        H.check(H.lib().kf_memcpy_d2h(hrow.ctypes.data, bh.ptr + r * ld * 2, F * 2, None))
        H.check(H.lib().kf_memcpy_d2h(dxrow.ctypes.data, bdx.ptr + r * ld * 2, 4 * F, None))
        assert np.array_equal(hrow, small["h"][r]) and np.array_equal(dxrow[:F], small["dgate"][r]) and np.array_equal(dxrow[F:], small["dup"][r]), r
    verify(code, SILU, g, u, dh, small, "rows beyond 2^31")


# ---- against torch-CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("act", ACTS)
def test_against_torch_cpu(code, act):
    import torch
    import torch.nn.functional as Fn
    rng = np.random.default_rng(50 + act)
    g, u, dh = draw(rng, code, 40, 512)
    if act != SILU:
        # torch's own two GELU forms compute 0.5 g (1 + tanh z) and 0.5 g (1 + erf(g / sqrt 2)): the bracket cancels for negative g and
        # carries an absolute 2^-24, a relative 2^-24 / (1 + tanh z) of the result - 1.3e-6 at g = -2, inside twice the bound there
        # (5.7e-6), 1.7e-5 at g = -3, outside it. The comparison with torch therefore takes g >= -2; the f64 tests above cover the tail.
        g = bits(np.maximum(floats(g, code), -2.0), code)
    gf, uf, df = (floats(x, code) for x in (g, u, dh))
    tg, tu = (torch.tensor(x, dtype=torch.float32, requires_grad=True) for x in (gf, uf))   # 16-bit inputs: torch in f32 on the stored values
    ta = Fn.silu(tg) if act == SILU else Fn.gelu(tg, approximate="tanh" if act == TANH else "none")
    th = ta * tu
    th.backward(torch.tensor(df, dtype=torch.float32))
    out = run(code, act, g, u, dh, form="packed")
    want = ref(act, gf, uf, df)
    for name, tv in (("h", th.detach()), ("dgate", tg.grad), ("dup", tu.grad)):
        val, M, A = want[name]
        err = np.abs(floats(out[name], code) - tv.numpy().astype(np.float64))
        tol = 2 * bound(act, H.F32, gf, val, M, A) + np.maximum(OUT_R[code] * np.abs(val), OUT_HALF_SPACING[code])   # both sides round in f32; ours once more on the way out
        assert (err <= tol).all(), (name, float((err / np.maximum(tol, 1e-300)).max()))


# ---- the operator API -------------------------------------------------------------------------------------------------------------
def to_t(b, code, requires_grad=False):
    f = floats(b, code).astype(np.float32)
    t = kfunca.from_numpy_bf16(np.ascontiguousarray(b.view(np.uint16)), 0) if code == H.BF16 else kfunca.from_numpy(f.astype(np.float16) if code == H.F16 else f, 0)
    t.set_requires_grad(requires_grad)
    return t


def t_bits(t, code):
    return np.ascontiguousarray(t.numpy()).view(UINT[code])


@pytest.mark.parametrize("code", CODES)
def test_operator_packed_equals_split_halves_and_the_abi(code):
    rng = np.random.default_rng(60)
    B, S, F = 2, 9, 96
    g, u, dh = draw(rng, code, B * S, F)
    abi = run(code, SILU, g, u, dh, form="packed")
    x = to_t(np.concatenate([g, u], 1).reshape(B, S, 2 * F), code, True)
    y = kfunca.swiglu(x)
    assert y.sizes() == [B, S, F] and np.array_equal(t_bits(y, code).reshape(B * S, F), abi["h"])
    y.backward(to_t(dh.reshape(B, S, F), code))
    assert x.grad().sizes() == [B, S, 2 * F]
    dx = t_bits(x.grad(), code).reshape(B * S, 2 * F)
    assert np.array_equal(dx[:, :F], abi["dgate"]) and np.array_equal(dx[:, F:], abi["dup"])
    # the halves Tensor.split returns are read in place through their leading dimension: the same bits, gradients shaped like the inputs
    x2 = to_t(np.concatenate([g, u], 1).reshape(B, S, 2 * F), code, True)
    hg, hu = x2.split([F, F], 2)
    assert hg.strides() == [S * 2 * F, 2 * F, 1] and hu.strides() == [S * 2 * F, 2 * F, 1] and hu.storage_offset() == F
    y2 = kfunca.swiglu(hg, hu)
    assert np.array_equal(t_bits(y2, code), t_bits(y, code))
    y2.backward(to_t(dh.reshape(B, S, F), code))
    assert np.array_equal(t_bits(x2.grad(), code).reshape(B * S, 2 * F), dx)
    # two dense tensors; only up asks for a gradient
    tg, tu = to_t(g, code), to_t(u, code, True)
    y3 = kfunca.swiglu(tg, tu)
    assert np.array_equal(t_bits(y3, code), abi["h"])
    y3.backward(to_t(dh, code))
    assert not tg.grad().defined() and np.array_equal(t_bits(tu.grad(), code), abi["dup"])
    # a strided gradient (a column slice of a wider tensor) is read in place too
    wide = to_t(np.concatenate([dh, dh], 1), code)
    tg2, tu2 = to_t(g, code, True), to_t(u, code, True)
    kfunca.swiglu(tg2, tu2).backward(wide[:, F:])
    assert np.array_equal(t_bits(tg2.grad(), code), abi["dgate"]) and np.array_equal(t_bits(tu2.grad(), code), abi["dup"])
    # a transposed operand has no unit stride: it is made dense first, with the same result
    gt = to_t(np.ascontiguousarray(g.T), code).permute(1, 0)
    assert np.array_equal(t_bits(kfunca.swiglu(gt, to_t(u, code)), code), abi["h"])


@pytest.mark.parametrize("act", ACTS)
def test_operator_variants_match_the_abi(act):
    code = H.F32
    rng = np.random.default_rng(61 + act)
    g, u, dh = draw(rng, code, 12, 40)
    gated, plain = run(code, act, g, u, dh, form="packed"), run(code, act, g, None, dh)
    kw = {} if act == SILU else {"approximate": "tanh" if act == TANH else "none"}
    glu = kfunca.swiglu if act == SILU else kfunca.geglu
    unary = kfunca.silu if act == SILU else kfunca.gelu
    x = to_t(np.concatenate([g, u], 1), code, True)
    y = glu(x, **kw)
    assert np.array_equal(t_bits(y, code), gated["h"])
    y.backward(to_t(dh, code))
    assert np.array_equal(t_bits(x.grad(), code), np.concatenate([gated["dgate"], gated["dup"]], 1))
    assert np.array_equal(t_bits(glu(to_t(g, code), to_t(u, code), **kw), code), gated["h"])
    tg = to_t(g.reshape(3, 4, 40), code, True)
    z = unary(tg, **kw)
    assert z.sizes() == [3, 4, 40] and np.array_equal(t_bits(z, code).reshape(12, 40), plain["h"])
    z.backward(to_t(dh.reshape(3, 4, 40), code))
    assert np.array_equal(t_bits(tg.grad(), code).reshape(12, 40), plain["dgate"])
    if act == ERF:   # the default is the erf form, as torch's
        assert np.array_equal(t_bits(kfunca.gelu(to_t(g, code)), code), plain["h"])
        assert np.array_equal(t_bits(kfunca.geglu(to_t(g, code), to_t(u, code)), code), gated["h"])


def test_operator_refusals():
    f = kfunca.from_numpy(np.zeros((4, 6), np.float32), 0)
    with pytest.raises(RuntimeError, match="must be even"):
        kfunca.swiglu(kfunca.from_numpy(np.zeros((4, 7), np.float32), 0))
    with pytest.raises(RuntimeError, match="one shape, dtype and device"):
        kfunca.swiglu(f, kfunca.from_numpy(np.zeros((4, 5), np.float32), 0))
    with pytest.raises(RuntimeError, match="one shape, dtype and device"):
        kfunca.geglu(f, f.bfloat16())
    with pytest.raises(RuntimeError, match="float, half and bfloat16"):
        kfunca.swiglu(kfunca.from_numpy(np.zeros((4, 6), np.int32), 0))
    with pytest.raises(RuntimeError, match="float, half and bfloat16"):
        kfunca.gelu(kfunca.from_numpy(np.zeros((4, 6), np.float64), 0))
    with pytest.raises(RuntimeError, match="approximate"):
        kfunca.gelu(f, approximate="fast")
    with pytest.raises(RuntimeError, match="approximate"):
        kfunca.geglu(f, approximate="erf")
    assert kfunca.swiglu(kfunca.from_numpy(np.zeros((0, 8), np.float32), 0)).sizes() == [0, 4]


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def mlp_model(bf16, seed=23):
    """x -> gemm(W1 = [Wg | Wu]) -> swiglu -> gemm(W2) -> cross_entropy, through kfunca and through torch-CPU f64 on the same rounded weights."""
    import torch
    import torch.nn.functional as Fn
    rng = np.random.default_rng(seed)
    T, Kd, F, vocab = 96, 64, 160, 50
    w = {"x": rng.uniform(-1, 1, (T, Kd)), "w1": rng.uniform(-1, 1, (Kd, 2 * F)) * (2.0 / np.sqrt(Kd)), "w2": rng.uniform(-1, 1, (F, vocab)) / np.sqrt(F)}
    w = {k: v.astype(np.float32) for k, v in w.items()}
    if bf16:
        w = {k: O.bf16_to_f32(O.f32_to_bf16(v)) for k, v in w.items()}
    target = rng.integers(0, vocab, T)
    ps = {k: kfunca.from_numpy(v, 0) for k, v in w.items()}
    if bf16:
        ps = {k: v.bfloat16() for k, v in ps.items()}
    for p in ps.values():
        p.set_requires_grad(True)
    ttgt = kfunca.from_numpy(target, 0)

    def forward():
        h = kfunca.swiglu(kfunca.gemm(ps["x"], ps["w1"], 1.0, 0.0))
        return kfunca.cross_entropy(kfunca.gemm(h, ps["w2"], 1.0, 0.0), ttgt)

    loss = forward()
    loss.backward(kfunca.from_numpy(np.ones(1, np.float32), 0))
    kgrads = {k: p.grad().float().numpy() if bf16 else p.grad().numpy() for k, p in ps.items()}
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    gu = t["x"] @ t["w1"]
    rl = Fn.cross_entropy((Fn.silu(gu[:, :F]) * gu[:, F:]) @ t["w2"], torch.tensor(target))
    rl.backward()
    return float(loss.float().numpy()[0]) if bf16 else float(loss.numpy()[0]), kgrads, rl.item(), {k: v.grad.numpy() for k, v in t.items()}, ps, forward


@pytest.mark.parametrize("bf16", [False, True])
def test_gated_mlp_end_to_end_and_one_adamw_step(bf16):
    loss, kg, rloss, tg, ps, forward = mlp_model(bf16)
    if not bf16:
        assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)
        for k in kg:
            assert_close(kg[k], tg[k], rtol=1e-3, atol=1e-5, what=f"d {k}")
    else:
        assert abs(loss - rloss) <= 2e-2 * abs(rloss), (loss, rloss)
        for k in kg:
            scale = np.abs(tg[k]).max()
            assert np.abs(kg[k] - tg[k]).max() <= 0.06 * scale, (k, float(np.abs(kg[k] - tg[k]).max()), float(scale))
    opt = kfunca.AdamW([ps["w1"], ps["w2"]], lr=3e-3, weight_decay=0.0)
    opt.step()
    after = forward()
    after = float(after.float().numpy()[0]) if bf16 else float(after.numpy()[0])
    assert after != loss and after < loss, (loss, after)


def test_zz_report_the_largest_fraction_of_the_bound():
    """Not a check: prints what the accuracy tests above met (run with -s), for DESIGN.md section 4.8."""
    names, dt = {SILU: "SiLU", TANH: "GELU-tanh", ERF: "GELU-erf"}, {H.F32: "f32", H.BF16: "bf16", H.F16: "f16"}
    for (act, out, code), v in sorted(WORST.items()):
        print(f"largest fraction of the bound: {names[act]:9s} {out:5s} {dt[code]:4s} {v:.3f}")
