"""Test helper (not a test): the double-precision attention reference of oracle.c's orc_attn_ref64, restated in numpy for an ARBITRARY
boolean visibility vis[B, Sq, Skv] and grouped K/V heads.

attn_ref64_vis returns the dict oracle.attn_ref64 returns - o lse mo qo dq dk dv mdq mdk mdv qdq qdk qdv bdq, the same formulas term by
term - so oracle.checks.check_one consumes it unchanged and the tolerances are the project's own (EPS, C_*, the element / row / head
bounds). With vis = tril it equals the oracle (tests/test_attn_full_ref.py). Grouped heads: q, o, dq have Hq heads, k, v, dk, dv have
Hkv; dk and dv and their worst-case scales are summed over a group's query heads, the statistical scales in quadrature (independent
roundings). A query row without a visible key has o = 0, lse = -inf and contributes nothing to any gradient.
format_floor_vis is oracle.checks.format_floor with the sums taken over all visible partners instead of causal prefixes / suffixes."""
import numpy as np

from oracle import checks as K
from oracle import oracle as O


def key_len_vis(kv_len, Sq, Skv, B=None):
    """vis[B, Sq, Skv] of per-batch key lengths (None: every key), clamped to [0, Skv] as the kernels clamp them."""
    if kv_len is None:
        return np.ones((B, Sq, Skv), bool)
    ln = np.clip(np.asarray(kv_len, np.int64), 0, Skv)
    return np.broadcast_to(np.arange(Skv)[None, None, :] < ln[:, None, None], (len(ln), Sq, Skv)).copy()


def attn_ref64_vis(q, k, v, d_o, vis, code, scale=None):
    qf, kf, vf = (K.to_f64(x, code) for x in (q, k, v))
    gf = None if d_o is None else K.to_f64(d_o, code)
    B, Hq, Sq, D = qf.shape
    Hkv, Skv = kf.shape[1], kf.shape[2]
    G = Hq // Hkv
    assert Hq == Hkv * G and vis.shape == (B, Sq, Skv)
    scale = 1.0 / np.sqrt(D) if scale is None else scale
    r = {n: np.zeros(qf.shape) for n in ("o", "mo", "qo")}
    r["lse"] = np.zeros((B, Hq, Sq))
    if gf is not None:
        for n in ("dq", "mdq", "qdq", "bdq"):
            r[n] = np.zeros(qf.shape)
        for n in ("dk", "dv", "mdk", "mdv", "qdk", "qdv"):
            r[n] = np.zeros(kf.shape)
    for b in range(B):
        for h in range(Hq):
            g = h // G
            Q, Kk, V, m = qf[b, h], kf[b, g], vf[b, g], vis[b]
            s = np.where(m, Q @ Kk.T * scale, -np.inf)
            mx = s.max(axis=1, keepdims=True)
            mx = np.where(np.isfinite(mx), mx, 0.0)
            p = np.exp(s - mx)
            l = p.sum(axis=1, keepdims=True)
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
            t = Gd * o
            dabs, da2 = np.abs(t).sum(axis=1, keepdims=True), np.sqrt((t * t).sum(axis=1, keepdims=True))
            ds = p * (dp - delta) * scale
            c = np.abs(p @ Kk) * scale
            r["dq"][b, h], r["mdq"][b, h] = ds @ Kk, np.abs(ds) @ np.abs(Kk)
            r["bdq"][b, h] = c * dabs
            r["qdq"][b, h] = np.sqrt((ds * ds) @ (Kk * Kk) + (c * da2) ** 2)
            wk, w2 = np.abs(ds) + p * dabs * scale, ds * ds + (p * da2 * scale) ** 2
            r["dk"][b, g] += ds.T @ Q
            r["dv"][b, g] += p.T @ Gd
            r["mdk"][b, g] += wk.T @ np.abs(Q)
            r["mdv"][b, g] += p.T @ np.abs(Gd)
            r["qdk"][b, g] += w2.T @ (Q * Q)       # squares: the root is taken below, over the whole group
            r["qdv"][b, g] += (p * p).T @ (Gd * Gd)
    if gf is not None:
        r["qdk"], r["qdv"] = np.sqrt(r["qdk"]), np.sqrt(r["qdv"])
    return r


def format_floor_vis(q, k, v, d_o, vis, code, scale=None):
    """oracle.checks.format_floor for a visibility: {name: per-element absolute floor} for dq, dk, dv."""
    qa, ka, da = (np.abs(K.to_f64(x, code)) for x in (q, k, d_o))
    B, Hq, Sq, D = qa.shape
    Hkv = ka.shape[1]
    G = Hq // Hkv
    scale = 1.0 / np.sqrt(D) if scale is None else scale
    if code == O.F16:
        u_p, u_ds = 2.0 ** -25 * 2.0 ** -K.P_SHIFT_F16, 2.0 ** -25
    else:
        u_p = u_ds = 2.0 ** -126
    p32 = 2.0 ** -126
    a_i = 2.0 * np.linalg.norm(K.to_f64(d_o, code), axis=-1, keepdims=True)
    vn_j = np.linalg.norm(K.to_f64(v, code), axis=-1, keepdims=True)
    out = {"dv": np.zeros(ka.shape), "dk": np.zeros(ka.shape), "dq": np.zeros(qa.shape)}
    for b in range(B):
        m = vis[b].astype(np.float64)
        for h in range(Hq):
            g = h // G
            out["dv"][b, g] += K.C_FLOOR * u_p * (m.T @ da[b, h])
            out["dk"][b, g] += K.C_FLOOR * scale * (u_ds * (m.T @ qa[b, h]) + p32 * vn_j[b, g] * (m.T @ (a_i[b, h] * qa[b, h])))
            out["dq"][b, h] = K.C_FLOOR * scale * (u_ds * (m @ ka[b, g]) + p32 * a_i[b, h] * (m @ (vn_j[b, g] * ka[b, g])))
    return out


def check_lse(lse, ref, what=""):
    """The project's lse bound 2e-6 (1 + |lse|); a row without a visible key must be -inf exactly."""
    want = ref["lse"]
    dead = np.isneginf(want)
    got = np.asarray(lse, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isneginf(got[dead]).all(), f"{what} lse: a row without a visible key is not -inf"
    d = np.abs(got[~dead] - want[~dead])
    assert np.isfinite(got[~dead]).all() and (d <= 2e-6 * (1.0 + np.abs(want[~dead]))).all(), f"{what} lse: max error {d.max():.3e}"
