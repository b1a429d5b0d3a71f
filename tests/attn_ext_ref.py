"""Test helper (not a test): tests/attn_full_ref.py's double-precision attention with the two score modifiers of kf_attn_ext_*.

    x = scale q.k        s = softcap tanh(x / softcap) (softcap > 0) or x, for visible n
    Z = sum_n exp s + exp sink[h] (sink given)        o = sum_n exp(s) v / Z        lse = log Z
    dS = P (dP - delta) (1 - t^2),  t = tanh(x / softcap)        dsink[h] = - sum_{b, m} exp(sink[h] - lse) delta

attn_ref64_ext returns attn_ref64_vis's keys - the same formulas term by term, with the factor 1 - t^2 inside ds and inside the worst-case
and statistical scales built from it (mdq qdq bdq mdk qdk) - plus dsink [Hq] and dsink_bound [Hq]:
    eps sum_{b,m} p_sink sum_d |dO| (C_OUT |o| + C_SUM mo)  +  1e-5 sum_{b,m} p_sink |delta|
the error delta inherits from the rounded O (the source of bdq) and f32 summation noise relative to the sum of magnitudes. With softcap
None (or 0) and sink None every operation is attn_ref64_vis's, in its order: the results are equal, not close
(tests/test_attn_ext_ref.py). A row without a visible key has o = 0; its lse is -inf without a sink and sink[h] with one."""
import numpy as np

from oracle import checks as K

# The modifiers of the GPU tests (tests/test_gpu_attn_ext.py), chosen under the condition tests/test_attn_ext_ref.py asserts on that
# file's inputs (U(-1, 1) operands: scores of standard deviation 1/3): each cap of CAPS bends every output beyond its bound, BIG_CAP
# bends none, and the sinks - U(-1, 3) per head - carry visible mass in every row.
CAPS = (0.25, 1.0)
BIG_CAP = 1000.0


def sinks_for(Hq, seed=0):
    return np.random.default_rng(1000 + seed).uniform(-1.0, 3.0, Hq).astype(np.float32)


def attn_ref64_ext(q, k, v, d_o, vis, code, softcap=None, sink=None, scale=None, drop_dtanh=False):
    """drop_dtanh: the WRONG backward that forgets the factor 1 - t^2 (the discrimination test's mutant; never a reference)."""
    qf, kf, vf = (K.to_f64(x, code) for x in (q, k, v))
    gf = None if d_o is None else K.to_f64(d_o, code)
    B, Hq, Sq, D = qf.shape
    Hkv, Skv = kf.shape[1], kf.shape[2]
    G = Hq // Hkv
    assert Hq == Hkv * G and vis.shape == (B, Sq, Skv)
    cap = float(softcap) if softcap else 0.0
    sk = None if sink is None else np.asarray(sink, np.float64)
    assert sk is None or sk.shape == (Hq,)
    scale = 1.0 / np.sqrt(D) if scale is None else scale
    r = {n: np.zeros(qf.shape) for n in ("o", "mo", "qo")}
    r["lse"] = np.zeros((B, Hq, Sq))
    if gf is not None:
        for n in ("dq", "mdq", "qdq", "bdq"):
            r[n] = np.zeros(qf.shape)
        for n in ("dk", "dv", "mdk", "mdv", "qdk", "qdv"):
            r[n] = np.zeros(kf.shape)
        if sk is not None:
            r["dsink"], r["dsink_bound"] = np.zeros(Hq), np.zeros(Hq)
    for b in range(B):
        for h in range(Hq):
            g = h // G
            Q, Kk, V, m = qf[b, h], kf[b, g], vf[b, g], vis[b]
            x = Q @ Kk.T * scale
            dfac = None
            if cap > 0:
                t = np.tanh(x / cap)
                x = cap * t
                dfac = None if drop_dtanh else 1.0 - t * t
            s = np.where(m, x, -np.inf)
            mx = s.max(axis=1, keepdims=True)
            if sk is not None:
                mx = np.maximum(mx, sk[h])
            mx = np.where(np.isfinite(mx), mx, 0.0)
            p = np.exp(s - mx)
            l = p.sum(axis=1, keepdims=True)
            if sk is not None:
                l = l + np.exp(sk[h] - mx)
            with np.errstate(divide="ignore"):
                r["lse"][b, h] = (mx + np.log(l))[:, 0]
            p = p / np.where(l > 0, l, 1.0)
            o = p @ V
            r["o"][b, h], r["mo"][b, h], r["qo"][b, h] = o, p @ np.abs(V), np.sqrt((p * p) @ (V * V))
            if gf is None:
                continue
            Gd = gf[b, h]
            dp = Gd @ V.T
            delta = (p * dp).sum(axis=1, keepdims=True)
            tt = Gd * o
            dabs, da2 = np.abs(tt).sum(axis=1, keepdims=True), np.sqrt((tt * tt).sum(axis=1, keepdims=True))
            ds = p * (dp - delta) * scale
            pk = p                       # the weights a change of delta reaches dS through: P (1 - t^2)
            if dfac is not None:
                ds = ds * dfac
                pk = p * dfac
            c = np.abs(pk @ Kk) * scale
            r["dq"][b, h], r["mdq"][b, h] = ds @ Kk, np.abs(ds) @ np.abs(Kk)
            r["bdq"][b, h] = c * dabs
            r["qdq"][b, h] = np.sqrt((ds * ds) @ (Kk * Kk) + (c * da2) ** 2)
            wk, w2 = np.abs(ds) + pk * dabs * scale, ds * ds + (pk * da2 * scale) ** 2
            r["dk"][b, g] += ds.T @ Q
            r["dv"][b, g] += p.T @ Gd
            r["mdk"][b, g] += wk.T @ np.abs(Q)
            r["mdv"][b, g] += p.T @ np.abs(Gd)
            r["qdk"][b, g] += w2.T @ (Q * Q)       # squares: the root is taken below, over the whole group
            r["qdv"][b, g] += (p * p).T @ (Gd * Gd)
            if sk is not None:
                with np.errstate(invalid="ignore"):
                    ps = np.where(np.isneginf(r["lse"][b, h]), 0.0, np.exp(sk[h] - r["lse"][b, h]))[:, None]
                r["dsink"][h] -= float((ps * delta).sum())
                if code in K.EPS:
                    r["dsink_bound"][h] += K.EPS[code] * float((ps * (np.abs(Gd) * (K.C_OUT * np.abs(o) + K.C_SUM * r["mo"][b, h])).sum(axis=1, keepdims=True)).sum())
                r["dsink_bound"][h] += 1e-5 * float((ps * np.abs(delta)).sum())
    if gf is not None:
        r["qdk"], r["qdv"] = np.sqrt(r["qdk"]), np.sqrt(r["qdv"])
    return r


def check_lse_ext(lse, ref, softcap=None, sink=None, what=""):
    """lse against the reference: |d| <= 2e-6 (1 + |lse|) + softcap 2^-20 - the project's bound (tests/attn_full_ref.check_lse) plus the
    error of the kernels' tanh, 1 - 2 rcp(exp2(2 |x| log2 e) + 1) with 1-ulp exp2 and rcp: absolute error <= about 3 2^-23 = 2^-21.4 (the
    rounding of the argument enters weighted by y 2 e^y / (e^y + 1)^2 <= 0.45), scaled by softcap, doubled. A row without a visible key
    is -inf exactly without a sink; with one it is the f32 sink itself (got == f32(sink[h])), whatever the other rows are."""
    want = ref["lse"]
    got = np.asarray(lse, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    dead = np.isneginf(want)
    assert np.isneginf(got[dead]).all(), f"{what} lse: a row without a visible key or sink is not -inf"
    cap = float(softcap) if softcap else 0.0
    d = np.abs(got[~dead] - want[~dead])
    tol = 2e-6 * (1.0 + np.abs(want[~dead])) + cap * 2.0 ** -20
    assert np.isfinite(got[~dead]).all() and (d <= tol).all(), f"{what} lse: max error {d.max():.3e} ({(d / tol).max():.2f} of the bound)"
