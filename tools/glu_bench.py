#!/usr/bin/env python3
"""Gated activations (kf_glu_fwd, kf_glu_bwd) against the box's own copy rate, through the C ABI.

For each case: the call timed with HIP events (median of --iters after --warmup), interleaved in the same loop with a kf_memcpy_d2d
that moves the same algorithmic bytes (half of them each way). Bytes per element of the [rows, F] result, s = sizeof(T): forward 3 s
(gate, up in; h out), ungated 2 s; backward 5 s (gate, up, dh in; dgate, dup out), in place too (the projection is overwritten with
its gradient: the same traffic, no second [rows, 2F] buffer). TB/s = those bytes / median time; `time_over_copy` is the kernel's time
over the copy's for the same bytes (1.0 = copy speed, higher = slower). torch's GPU `F.silu(g) * u` on the same packed tensor is
timed as context for the packed SiLU forward cases when torch sees a GPU (`torch_ms`; --no-torch skips it). --check compares sampled rows with f64 numpy.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (the kernels are glu_fwd_kernel / glu_bwd_kernel).
Prints one JSON object; --json saves it."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

CODES = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}
ACTS = {"silu": H.ACT_SILU, "gelu_tanh": H.ACT_GELU_TANH, "gelu_erf": H.ACT_GELU_ERF}
ROWS = 8 * 4096
# (label, dtype, rows, F, act, form, mode)   form: packed | dense | ungated   mode: fwd | bwd | bwd_inplace
CASES = [(f"packed bf16 F {F} silu {m}", "bf16", ROWS, F, "silu", "packed", m) for F in (14336, 16384, 11008) for m in ("fwd", "bwd", "bwd_inplace")]
CASES += [(f"packed bf16 F 14336 {a} {m}", "bf16", ROWS, 14336, a, "packed", m) for a in ("gelu_tanh", "gelu_erf") for m in ("fwd", "bwd")]
CASES += [
    ("packed f32 F 14336 silu fwd", "f32", ROWS, 14336, "silu", "packed", "fwd"),
    ("packed f32 F 14336 silu bwd", "f32", ROWS, 14336, "silu", "packed", "bwd"),
    ("ungated bf16 F 14336 silu fwd", "bf16", ROWS, 14336, "silu", "ungated", "fwd"),
    ("ungated bf16 F 14336 gelu_erf bwd", "bf16", ROWS, 14336, "gelu_erf", "ungated", "bwd"),
    ("two dense bf16 F 14336 silu fwd", "bf16", ROWS, 14336, "silu", "dense", "fwd"),
    ("two dense bf16 F 14336 silu bwd", "bf16", ROWS, 14336, "silu", "dense", "bwd"),
    ("packed bf16 F 14335 silu fwd (element path)", "bf16", ROWS, 14335, "silu", "packed", "fwd"),
    ("packed bf16 F 14335 silu bwd (element path)", "bf16", ROWS, 14335, "silu", "packed", "bwd"),
]
TILE = 61


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def torch_ms(case, args):
    """torch's GPU F.silu(g) * u (two kernels and a temporary) on the packed tensor's halves: context only."""
    try:
        import torch
    except ImportError:
        return None
    if args.no_torch or not torch.cuda.is_available():
        return None
    _, name, rows, F, act, form, mode = case
    if act != "silu" or form != "packed" or mode != "fwd":
        return None
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[name]
    x = torch.randn(rows, 2 * F, device="cuda", dtype=dt)

    def step():
        g, u = x.split(F, 1)
        return torch.nn.functional.silu(g) * u

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def fill(buf, tile, rows, row_bytes):
    """The tile's rows repeated down the buffer (row r holds tile[r % TILE])."""
    for r0 in range(0, rows, TILE):
        n = min(TILE, rows - r0)
        H.check(H.lib().kf_memcpy_h2d(buf.ptr + r0 * row_bytes, tile.ctypes.data, n * row_bytes, None))


def reference(act, g, u, dh):
    """f64: (h, dgate, dup) for float arrays."""
    g, u, dh = (np.asarray(x, np.float64) for x in (g, u, dh))
    sig = lambda x: np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))  # noqa: E731
    if act == "silu":
        s = sig(g)
        a, d = g * s, s * (1 + g * (1 - s))
    elif act == "gelu_tanh":
        c1 = 2 * math.sqrt(2 / math.pi)
        w = c1 * (g + 0.044715 * g ** 3)
        s = sig(w)
        a, d = g * s, s + g * s * (1 - s) * c1 * (1 + 3 * 0.044715 * g * g)
    else:
        p = 0.5 * (1 + np.vectorize(math.erf)(g / math.sqrt(2)))
        a, d = g * p, p + g * np.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
    return a * u, dh * u * d, dh * a


def bench_case(case, args):
    label, name, rows, F, act, form, mode = case
    code, es = CODES[name], H.DTYPE_SIZE[CODES[name]]
    gated = form != "ungated"
    width = 2 * F if form == "packed" else F
    rng = np.random.default_rng(rows + F)
    tg = O.from_float(rng.normal(0, 2, (TILE, F)).astype(np.float32), code)
    tu = O.from_float(rng.uniform(-4, 4, (TILE, F)).astype(np.float32), code)
    td = O.from_float(rng.uniform(-2, 2, (TILE, F)).astype(np.float32), code)
    if form == "packed":
        bx = H.DevBuf(rows * width * es)
        fill(bx, np.ascontiguousarray(np.concatenate([tg, tu], 1)), rows, width * es)
        gp, up, ldg, ldu = bx.ptr, bx.ptr + F * es, width, width
    else:
        bg = H.DevBuf(rows * F * es)
        fill(bg, tg, rows, F * es)
        gp, ldg, up, ldu = bg.ptr, F, None, 0
        if gated:
            bu = H.DevBuf(rows * F * es)
            fill(bu, tu, rows, F * es)
            up, ldu = bu.ptr, F
    bwd = mode != "fwd"
    n_out = (2 if gated else 1) if bwd else 1
    n_in = (2 if gated else 1) + (1 if bwd else 0)
    moved = (n_in + n_out) * rows * F * es
    if bwd:
        bd = H.DevBuf(rows * F * es)
        fill(bd, td, rows, F * es)
        if mode == "bwd_inplace":
            dgp, dup_, lddg, lddu = gp, up, ldg, ldu
        elif form == "packed":
            bdx = H.DevBuf(rows * width * es)
            dgp, dup_, lddg, lddu = bdx.ptr, bdx.ptr + F * es, width, width
        else:
            bdg = H.DevBuf(rows * F * es)
            dgp, lddg, dup_, lddu = bdg.ptr, F, None, 0
            if gated:
                bdu = H.DevBuf(rows * F * es)
                dup_, lddu = bdu.ptr, F
    else:
        bh = H.DevBuf(rows * F * es)
    copy_bytes = (moved // 2) // 256 * 256
    csrc, cdst = H.DevBuf(copy_bytes), H.DevBuf(copy_bytes)

    def kernel():
        if bwd:
            H.glu_bwd(ACTS[act], code, rows, F, gp, ldg, up, ldu, bd.ptr, F, dgp, lddg, dup_, lddu)
        else:
            H.glu_fwd(ACTS[act], code, rows, F, gp, ldg, up, ldu, bh.ptr, F)

    def copy():
        H.check(H.lib().kf_memcpy_d2d(cdst.ptr, csrc.ptr, copy_bytes, None))

    check = None
    if args.check and mode != "bwd_inplace":   # (in place overwrites the inputs on every call: the out-of-place case checks the same kernel)
        kernel()
        H.device_sync()
        worst = 0.0
        for r in (0, 1, TILE, rows // 2, rows - 1):
            fg, fu, fd = (O.to_float(t[r % TILE], code) for t in (tg, tu, td))
            h, dg, du = reference(act, fg, fu if gated else np.ones_like(fu), fd)
            outs = []
            if bwd:
                outs.append((dgp + r * lddg * es, dg))
                if gated:
                    outs.append((dup_ + r * lddu * es, du))
            else:
                outs.append((bh.ptr + r * F * es, h))
            for ptr, want in outs:
                row = np.empty(F, H.CODE2NP[code])
                H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, ptr, F * es, None))
                got = O.to_float(row, code).astype(np.float64)
                # one output rounding, plus the f32 evaluation's own error where act' cancels (relative to the factors, not to the result)
                tol = {2: 2.0 ** -8 if name == "bf16" else 2.0 ** -11, 4: 2.0 ** -20}[es] * np.abs(want)
                tol = tol + 2.0 ** -18 * (1 + np.abs(fg)) * np.abs(fd if bwd else 1.0) * np.abs(fu if gated else 1.0) + 1e-30
                worst = max(worst, float((np.abs(got - want) / tol).max()))
        check = {"worst_error_over_tolerance": worst, "ok": worst <= 1.0}
    for _ in range(args.warmup):
        copy(), kernel()
    H.device_sync()
    ms = {"kernel": [], "copy": []}
    for _ in range(args.iters):  # interleaved: drift of the clock or of the neighbours' load hits both sides alike
        ms["copy"].append(event_ms(copy))
        ms["kernel"].append(event_ms(kernel))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"case": label, "dtype": name, "rows": rows, "F": F, "act": act, "form": form, "mode": mode, "bytes": moved, "ms": med["kernel"],
           "TBps": moved / med["kernel"] / 1e9, "copy_ms": med["copy"], "copy_TBps": 2 * copy_bytes / med["copy"] / 1e9,
           "spread_ms": [min(ms["kernel"]), max(ms["kernel"])]}
    res["time_over_copy"] = res["copy_TBps"] / res["TBps"]
    if check is not None:
        res["check"] = check
    t = torch_ms(case, args)
    if t is not None:
        res["torch_ms"] = t
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--check", action="store_true", help="compare sampled rows with f64 numpy before timing")
    ap.add_argument("--only", default="", help="run the cases whose label contains this text")
    ap.add_argument("--json", type=Path)
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("glu_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"cases": [bench_case(c, args) for c in CASES if args.only in c[0]]}
    if args.check and not all(c["check"]["ok"] for c in out["cases"] if "check" in c):
        print(json.dumps(out))
        raise SystemExit("glu_bench --check: a sampled row is outside one output rounding (+ 2^-18 of the factors) of the f64 reference")
    text = json.dumps(out)
    print(text)
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
