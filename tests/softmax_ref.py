"""The f64 numpy reference of the four row-softmax maps (kf_softmax_fwd / kf_softmax_bwd), the bounds the device results are held to,
and the input draws of tests/test_gpu_softmax.py (shared with tests/test_softmax_ref.py, which checks on the CPU that the bounds
reject wrong formulas on those very draws).

Over the last dimension, with s = scale * x and lse = log sum_v exp(s_v):

    softmax       y_v = exp(s_v - lse)            dx_v = scale * y_v * (dy_v - sum_u dy_u y_u)
    log_softmax   y_v = s_v - lse                 dx_v = scale * (dy_v - exp(y_v) * sum_u dy_u)

The reference takes the STORED inputs (16-bit values widened exactly) and, for the backward, the STORED y: what the device reads.

Bounds (the project's cross-entropy tests' - their gradient is this softmax - plus the summation error of the backward's own row sum):

    softmax forward        |err| <= R |ref| + 1e-6
    log_softmax forward    |err| <= R |ref| + 1e-5 |lse_ref| + 1e-4
    softmax backward       |err| <= R |ref| + scale |y_v| (2^-22 |dy_v| + c 2^-24 A) + H          A = sum_u |dy_u y_u|
    log_softmax backward   |err| <= R |ref| + scale exp(y_v) (2^-22 |dy_v| + c 2^-24 A) + H       A = sum_u |dy_u|

R = OUT_R: one output rounding (2^-8 bf16, 2^-11 f16) or 2^-16 for f32; H = OUT_HALF_SPACING: half the spacing of the format's subnormals,
which is what one rounding is below the smallest normal; c = ceil(V / 64) + 16: the first-order bound of any summation that keeps at least
64 partial sums and then a tree (all three regimes do).
"""
import math
import re
from pathlib import Path

import numpy as np

from oracle import oracle as O

SOFTMAX, LOG_SOFTMAX = 0, 1
KINDS = (SOFTMAX, LOG_SOFTMAX)
KIND_NAME = {SOFTMAX: "softmax", LOG_SOFTMAX: "log_softmax"}
F16, BF16, F32 = O.F16, O.BF16, O.F32
CODES = (F32, BF16, F16)
CODE_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
OUT_R = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 2.0 ** -16}
OUT_HALF_SPACING = {BF16: 2.0 ** -134, F16: 2.0 ** -25, F32: 2.0 ** -150}
ES = {BF16: 2, F16: 2, F32: 4}
UINT = {BF16: np.uint16, F16: np.uint16, F32: np.uint32}


def thresholds():
    """(T1, T2): the largest V of the wave regime and of the block regime, as the device source has them."""
    text = (Path(__file__).resolve().parent.parent / "kfunca_amd" / "csrc" / "device" / "softmax.hip").read_text()
    t1 = re.search(r"constexpr int64_t kSmWaveMax = (\d+);", text)
    t2 = re.search(r"constexpr int64_t kSmBlockMax = (\d+);", text)
    return int(t1.group(1)), int(t2.group(1))


def regime(V):
    t1, t2 = thresholds()
    return "wave" if V <= t1 else "block" if V <= t2 else "stream"


# ---- stored values ------------------------------------------------------------------------------------------------------------------
def bits(x, code):
    """float values -> the bit patterns of dtype `code` (round to nearest even)."""
    with np.errstate(over="ignore"):
        return O.from_float(np.asarray(x, np.float32), code).view(UINT[code])


def floats(b, code):
    """bit patterns -> their exact values in f64."""
    b = np.ascontiguousarray(b)
    if code == BF16:
        return O.bf16_to_f32(b.view(np.uint16)).astype(np.float64)
    return b.view(np.float16 if code == F16 else np.float32).astype(np.float64)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def forward(kind, x, scale):
    """(y, lse) in f64 from the stored logits x [rows, V]. scale is taken as the f32 the entry receives."""
    s = np.asarray(x, np.float64) * float(np.float32(scale))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = s.max(axis=-1, keepdims=True) if s.shape[-1] else np.zeros(s.shape[:-1] + (1,))
        m = np.where(np.isnan(s).any(axis=-1, keepdims=True), np.nan, m)   # (numpy's max propagates a NaN already; said out loud)
        lns = np.log(np.exp(s - m).sum(axis=-1, keepdims=True))
        lse = m + lns
        y = (s - m) - lns   # (not s - lse: at |s| ~ 1e5 the rounding of lse alone is 1e-11)
        return (np.exp(y) if kind == SOFTMAX else y), lse


def backward(kind, y, dy, scale):
    """dx in f64 from the stored result y and the stored gradient dy."""
    y, dy, sc = np.asarray(y, np.float64), np.asarray(dy, np.float64), float(np.float32(scale))
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == SOFTMAX:
            return sc * y * (dy - (dy * y).sum(axis=-1, keepdims=True))
        return sc * (dy - np.exp(y) * dy.sum(axis=-1, keepdims=True))


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
def forward_bound(kind, code, ref, lse):
    if kind == SOFTMAX:
        return OUT_R[code] * np.abs(ref) + 1e-6
    return OUT_R[code] * np.abs(ref) + 1e-5 * np.abs(lse) + 1e-4


def backward_bound(kind, code, y, dy, scale, ref):
    y, dy, sc = np.asarray(y, np.float64), np.asarray(dy, np.float64), float(np.float32(scale))
    c = math.ceil(y.shape[-1] / 64) + 16
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == SOFTMAX:
            w, A = np.abs(y), np.abs(dy * y).sum(axis=-1, keepdims=True)
        else:
            w, A = np.exp(y), np.abs(dy).sum(axis=-1, keepdims=True)
        return OUT_R[code] * np.abs(ref) + sc * w * (2.0 ** -22 * np.abs(dy) + c * 2.0 ** -24 * A) + OUT_HALF_SPACING[code]


# ---- the draws of the GPU tests -----------------------------------------------------------------------------------------------------
LOGITS = ("normal", "wide", "large")     # N(0, 1), N(0, 6^2), 1e4 + N(0, 3^2)
SCALES = (1.0, 0.125, 7.5)
# gradients: "normal" N(0, 1); "huge" the same with one element of 1e4 per row


def draw_logits(rng, which, code, rows, V):
    z = rng.normal(0.0, 1.0, (rows, V))
    return bits({"normal": z, "wide": 6.0 * z, "large": 1e4 + 3.0 * z}[which], code)


def draw_dy(rng, which, code, rows, V):
    z = rng.normal(0.0, 1.0, (rows, V))
    if which == "huge" and V > 0:
        z[np.arange(rows), rng.integers(0, V, rows)] = 1e4
    return bits(z, code)


def value_cases():
    """(logits, scale, dy) of the value-draw test: every logit draw at every scale with the plain gradient, and the huge gradient element
    with every logit draw at scale 1."""
    return [(lg, sc, "normal") for lg in LOGITS for sc in SCALES] + [(lg, 1.0, "huge") for lg in LOGITS]


def value_shapes():
    """(rows, V) of the value-draw test: one shape per regime, just past each threshold, odd."""
    t1, t2 = thresholds()
    return [(3, 65), (3, t1 + 1), (3, t2 + 1)]
