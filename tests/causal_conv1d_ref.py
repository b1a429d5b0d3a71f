"""float64 reference of kf_causal_conv1d_* on the inputs as stored, each result beside its absref: the same expression over absolute values.

  pre = bias + sum_j w[j] z[t + j],  z = h0 (K - 1 rows or zeros) then x;  y = act(pre);  hT = the last K - 1 rows of z
  dpre = dy act'(pre);  dz[m] = sum_j w[j] dpre[m - j] + d_hT[m - S];  dx = dz[K - 1:], dh0 = dz[:K - 1];  dw[j] = sum dpre z[t + j]

SiLU in the absrefs: |SiLU'| <= 1.1, so apre bounds what pre's rounding does to y; |SiLU''| <= 1/2, so |dy| apre / 2 joins adpre for what it does
to act'(pre). SILU_TERM is the kernel's exp2 / rcp sigmoid, which cannot be derived: the worst error of act (relative to |act|) and of act'
(relative to s (1 + |p| (1 - s))) against float64 was measured once on an MI355X over 2^20 f32 points of [-12, 12], a superset of the tests'
pre-activations (K = 2, w = (0, 1), no bias: pre is x exactly) - 8.17 2^-23 and 7.30 2^-23 - and the term is twice the worse."""
import numpy as np

from tests import gemm_views as V

U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}
TINY = {"bf16": 0.0, "f16": 2.0 ** -25, "f32": 0.0}   # half the spacing of f16's subnormals: a sum that cancels below 2^-14 is stored on that grid
ROWS = 64                       # rows one wave walks (KF_CONV1D_STEP_MAX); a workgroup covers 4 ROWS
SILU_TERM = 2 * 8.17 * 2.0 ** -23


def stored(a, dt):
    return V.decode(V.encode(a, dt), dt)


def reference(x, w, bias=None, h0=None, silu=False, dy=None, d_hT=None):
    """x [B, S, C], w [K, C], bias [C], h0 / d_hT [B, K - 1, C], dy [B, S, C], float64 -> (ref, absref) dicts."""
    (B, S, C), K = x.shape, w.shape[0]
    z = np.concatenate([np.zeros((B, K - 1, C)) if h0 is None else h0, x], 1)
    b = np.zeros(C) if bias is None else bias
    pre = b + sum(w[j] * z[:, j:j + S] for j in range(K))
    apre = np.abs(b) + sum(np.abs(w[j] * z[:, j:j + S]) for j in range(K))
    s = 1 / (1 + np.exp(-pre))
    y, der, ader = (pre * s, s * (1 + pre * (1 - s)), s * (1 + np.abs(pre) * (1 - s)) + apre / 2) if silu else (pre, 1.0, 1.0)
    ref, absref = dict(y=y, hT=z[:, S:]), dict(y=apre)
    if dy is None:
        return ref, absref
    dpre, adpre = dy * der, np.abs(dy) * ader
    dz, adz = np.zeros_like(z), np.zeros_like(z)
    for j in range(K):
        dz[:, j:j + S] += w[j] * dpre
        adz[:, j:j + S] += np.abs(w[j]) * adpre
    if d_hT is not None:
        dz[:, S:] += d_hT
        adz[:, S:] += np.abs(d_hT)
    ref.update(dx=dz[:, K - 1:], dh0=dz[:, :K - 1], dw=np.stack([(dpre * z[:, j:j + S]).sum((0, 1)) for j in range(K)]), dbias=dpre.sum((0, 1)))
    absref.update(dx=adz[:, K - 1:], dh0=adz[:, :K - 1], dw=np.stack([(adpre * np.abs(z[:, j:j + S])).sum((0, 1)) for j in range(K)]),
                  dbias=adpre.sum((0, 1)))
    return ref, absref


def bound(ref, absref, dt, n, silu):
    """u |ref| (or the half spacing of f16's subnormals) + n 2^-23 (absref + |ref|), and the measured SiLU term on absref + |ref| when the
    activation is on"""
    return np.maximum(U[dt] * np.abs(ref), TINY[dt]) + (n * 2.0 ** -23 + (SILU_TERM if silu else 0.0)) * (absref + np.abs(ref))
