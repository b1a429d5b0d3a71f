#!/usr/bin/env python3
"""Row softmax / log_softmax (kf_softmax_fwd, kf_softmax_bwd) against the box's own copy rate, through the C ABI.

For each shape, kind (softmax, log_softmax) and mode (fwd, bwd, fwd_inplace): the call timed with HIP events (median of --iters after
--warmup), interleaved in the same loop with a kf_memcpy_d2d that moves the same algorithmic bytes (half of them each way). Bytes, with
s = sizeof(T): forward rows * V * s * 2 (x in, y out; in place the same traffic in one buffer), backward rows * V * s * 3 (y, dy in; dx
out). TB/s = those bytes / median time; `time_over_copy` is the kernel's time over the copy's for the same bytes (1.0 = copy speed, higher
= slower). The stream regime (V > 16384) reads its input twice: its forward moves 1.5x the algorithmic bytes unless the second read hits in
a cache, and the figure here says which. torch's GPU softmax / log_softmax on a tensor of the same shape is timed as context for the forward
cases when torch sees a GPU (`torch_ms`; --no-torch skips it). --check compares sampled rows with f64 numpy under the bounds of
tests/softmax_ref.py. Shapes: an MoE router (32768 x 64, x 256), attention rows (262144 x 4096, 65536 x 1024), vocabulary rows (8192 x
50257, 32768 x 128256, and the sampling shape 16 x 128256, which one block per row cannot fill the chip with), f32 8192 x 32000.
Prints one JSON object with the box's large-copy rate and the source stamp of softmax.hip; --json saves it."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

CODES = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}
KINDS = {"softmax": H.SOFTMAX, "log_softmax": H.LOG_SOFTMAX}
MODES = ("fwd", "bwd", "fwd_inplace")
SOURCES = ("softmax.hip", "float_pack.h", "common.h", "runtime.hip")
# (label, dtype, rows, V)
SHAPES = [
    ("router 32768 x 64", "bf16", 32768, 64),
    ("router 32768 x 256", "bf16", 32768, 256),
    ("attention rows 65536 x 1024", "bf16", 65536, 1024),
    ("attention rows 262144 x 4096", "bf16", 262144, 4096),
    ("vocabulary 8192 x 50257", "bf16", 8192, 50257),
    ("vocabulary 32768 x 128256", "bf16", 32768, 128256),
    ("sampling 16 x 128256", "bf16", 16, 128256),
    ("f32 8192 x 32000", "f32", 8192, 32000),
]
TILE = 61
OUT_R = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -16}


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def d2d(dst, src, n):
    H.check(H.lib().kf_memcpy_d2d(dst, src, n, None))


def fill(buf, tile, rows, row_bytes):
    """The tile's rows repeated down the buffer (row r holds tile[r % TILE]): one upload, then device copies that double the filled part."""
    n = min(TILE, rows)
    H.check(H.lib().kf_memcpy_h2d(buf.ptr, tile.ctypes.data, n * row_bytes, None))
    done = n
    while done < rows:
        step = min(done // TILE * TILE or done, rows - done)
        d2d(buf.ptr + done * row_bytes, buf.ptr, step * row_bytes)
        done += step


def reference_fwd(kind, x):
    x = np.asarray(x, np.float64)
    m = x.max()
    lns = math.log(np.exp(x - m).sum())
    y = (x - m) - lns
    return (np.exp(y) if kind == "softmax" else y), m + lns


def reference_bwd(kind, y, dy):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    c = math.ceil(y.size / 64) + 16
    if kind == "softmax":
        return y * (dy - (dy * y).sum()), np.abs(y) * (2.0 ** -22 * np.abs(dy) + c * 2.0 ** -24 * np.abs(dy * y).sum())
    return dy - np.exp(y) * dy.sum(), np.exp(y) * (2.0 ** -22 * np.abs(dy) + c * 2.0 ** -24 * np.abs(dy).sum())


def read_row(ptr, V, code):
    row = np.empty(V, H.CODE2NP[code])
    H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, ptr, row.nbytes, None))
    return O.to_float(row, code).astype(np.float64)


def torch_ms(kind, name, rows, V, args):
    """torch's GPU softmax / log_softmax over the last dim of a tensor of the same shape: context only."""
    try:
        import torch
    except ImportError:
        return None
    if args.no_torch or not torch.cuda.is_available():
        return None
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[name]
    x = torch.randn(rows, V, device="cuda", dtype=dt)
    fn = torch.softmax if kind == "softmax" else torch.log_softmax
    for _ in range(args.warmup):
        fn(x, -1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(x, -1)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    del x
    torch.cuda.empty_cache()
    return statistics.median(ms)


def timed(kernel, copy, args):
    for _ in range(args.warmup):
        copy(), kernel()
    H.device_sync()
    ms = {"kernel": [], "copy": []}
    for _ in range(args.iters):   # interleaved: drift of the clock or of the neighbours' load hits both sides alike
        ms["copy"].append(event_ms(copy))
        ms["kernel"].append(event_ms(kernel))
    return {k: statistics.median(v) for k, v in ms.items()}, [min(ms["kernel"]), max(ms["kernel"])]


def bench_shape(shape, args):
    label, name, rows, V = shape
    code, es = CODES[name], H.DTYPE_SIZE[CODES[name]]
    rng = np.random.default_rng(rows + V)
    tx = O.from_float(rng.normal(0, 2, (TILE, V)).astype(np.float32), code)
    td = O.from_float(rng.normal(0, 1, (TILE, V)).astype(np.float32), code)
    n = rows * V * es
    bx, by, bd, bdx = (H.DevBuf(n) for _ in range(4))
    fill(bx, tx, rows, V * es)
    fill(bd, td, rows, V * es)
    copy_n = (3 * n // 2) // 256 * 256
    csrc, cdst = H.DevBuf(copy_n), H.DevBuf(copy_n)
    out = []
    sample = sorted({0, 1, TILE % rows, rows // 2, rows - 1})
    for kind in KINDS:
        if args.kind and kind != args.kind:
            continue
        k = KINDS[kind]
        for mode in MODES:
            moved = n * (3 if mode == "bwd" else 2)
            half = (moved // 2) // 256 * 256
            if mode == "fwd":
                kernel = lambda: H.softmax_fwd(k, code, rows, V, 1.0, bx.ptr, V, by.ptr, V)  # noqa: E731
            elif mode == "bwd":   # (y holds the forward's result of this kind)
                kernel = lambda: H.softmax_bwd(k, code, rows, V, 1.0, by.ptr, V, bd.ptr, V, bdx.ptr, V)  # noqa: E731
            else:                 # in place on the result buffer: the values change from call to call, the traffic does not
                kernel = lambda: H.softmax_fwd(k, code, rows, V, 1.0, by.ptr, V, by.ptr, V)  # noqa: E731
            copy = lambda: d2d(cdst.ptr, csrc.ptr, half)  # noqa: E731
            check = None
            if args.check and mode != "fwd_inplace":   # (the in-place call runs the same kernel on the same addresses' phase)
                kernel()
                H.device_sync()
                worst = 0.0
                for r in sample:
                    if mode == "fwd":
                        want, lse = reference_fwd(kind, O.to_float(tx[r % TILE], code))
                        tol = OUT_R[name] * np.abs(want) + (1e-6 if kind == "softmax" else 1e-5 * abs(lse) + 1e-4)
                        got = read_row(by.ptr + r * V * es, V, code)
                    else:
                        y = read_row(by.ptr + r * V * es, V, code)
                        want, slack = reference_bwd(kind, y, O.to_float(td[r % TILE], code))
                        tol = OUT_R[name] * np.abs(want) + slack + 2.0 ** -134
                        got = read_row(bdx.ptr + r * V * es, V, code)
                    worst = max(worst, float((np.abs(got - want) / tol).max()))
                check = {"worst_error_over_tolerance": worst, "ok": worst <= 1.0}
            med, spread = timed(kernel, copy, args)
            res = {"case": f"{label} {kind} {mode}", "dtype": name, "rows": rows, "V": V, "kind": kind, "mode": mode, "bytes": moved,
                   "ms": med["kernel"], "TBps": moved / med["kernel"] / 1e9, "copy_ms": med["copy"], "copy_TBps": 2 * half / med["copy"] / 1e9,
                   "spread_ms": spread}
            res["time_over_copy"] = res["copy_TBps"] / res["TBps"]
            if check is not None:
                res["check"] = check
            if mode == "fwd":
                t = torch_ms(kind, name, rows, V, args)
                if t is not None:
                    res["torch_ms"] = t
            out.append(res)
    return out


def box_copy_rate(args):
    """The box's own large-copy rate: a 2 GiB kf_memcpy_d2d (read + write bytes over the median time)."""
    n = 2 << 30
    a, b = H.DevBuf(n), H.DevBuf(n)
    copy = lambda: d2d(b.ptr, a.ptr, n)  # noqa: E731
    for _ in range(args.warmup):
        copy()
    H.device_sync()
    return 2 * n / statistics.median(event_ms(copy) for _ in range(args.iters)) / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--check", action="store_true", help="compare sampled rows with f64 numpy before timing")
    ap.add_argument("--only", default="", help="run the shapes whose label contains this text")
    ap.add_argument("--kind", default="", choices=("", *KINDS), help="one kind only")
    ap.add_argument("--json", type=Path)
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("softmax_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = dict(bench.stamp(SOURCES))
    out["memcpy_TBps"] = box_copy_rate(args)
    out["cases"] = [c for s in SHAPES if args.only in s[0] for c in bench_shape(s, args)]
    if args.check and not all(c["check"]["ok"] for c in out["cases"] if "check" in c):
        print(json.dumps(out))
        raise SystemExit("softmax_bench --check: a sampled row is outside the bound of the f64 reference")
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
