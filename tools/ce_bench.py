#!/usr/bin/env python3
"""Softmax cross-entropy (kf_cross_entropy_fwd / _bwd) against the box's own copy rate, through the C ABI.

For each shape: the forward and the backward timed with HIP events (median of --iters after --warmup), interleaved in the same loop with a
kf_memcpy_d2d that moves the same number of bytes - the forward reads rows*V*s bytes (a copy of half the logits moves as many), the backward
reads the logits and writes the gradient, 2*rows*V*s (a copy of the whole logits). TB/s = those algorithmic bytes / median time; `of_copy`
is the kernel's rate over the copy's. torch.nn.functional.cross_entropy on the same GPU is timed as context only (--no-torch skips it).
--check compares seeded sampled rows against an f64 numpy reference. Kernel times: run this under `rocprofv3 --kernel-trace --stats`
in a run of its own (the kernels are named ce_fwd_rows / ce_fwd_block / ce_fwd_split / ce_combine / ce_reduce / ce_bwd_rows / ce_bwd).
The logits are a 61-row random tile repeated down the rows (row r holds tile row r % 61): gigabytes are filled without building them
on the host. Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

SHAPES = [("bf16", 32768, 128256), ("bf16", 8192, 50257), ("bf16", 16, 128256), ("f32", 8192, 32000)]
CODES = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}
TILE = 61


def regime(rows, V):  # mirrors the header's documented partition (for the report only)
    if V <= 4096:
        return "wave per row"
    return "block per row" if rows >= 1024 else "split rows"


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def ref_row(x, t):
    x = x.astype(np.float64)
    m = x.max()
    e = np.exp(x - m)
    lse = m + np.log(e.sum())
    d = e / e.sum()
    d[t] -= 1.0
    return lse - x[t], d


def bench_shape(name, rows, V, args, out):
    code = CODES[name]
    es = H.DTYPE_SIZE[code]
    rng = np.random.default_rng(rows + V)
    tile = O.from_float(rng.uniform(-4, 4, (TILE, V)).astype(np.float32), code)
    t = rng.integers(0, V, rows).astype(np.int64)
    nbytes = rows * V * es
    bx, bt, bd = H.DevBuf(nbytes), H.DevBuf.from_numpy(t), H.DevBuf(nbytes)
    for r0 in range(0, rows, TILE):
        n = min(TILE, rows - r0)
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r0 * V * es, tile.ctypes.data, n * V * es, None))
    bl, blse, bc, bg = H.DevBuf(4 * rows), H.DevBuf(4 * rows), H.DevBuf(4), H.DevBuf.from_numpy(np.ones(1, np.float32))
    need = H.ce_workspace_bytes(code, rows, V, H.CE_MEAN)
    ws = H.DevBuf(max(need, 1))
    half = (nbytes // 2) // 256 * 256

    def fwd():
        H.check(H.lib().kf_cross_entropy_fwd(code, rows, V, V, bx.ptr, bt.ptr, -100, 0.0, H.CE_MEAN, bl.ptr, blse.ptr, bc.ptr, ws.ptr, need, None))

    def bwd():
        H.check(H.lib().kf_cross_entropy_bwd(code, rows, V, V, bx.ptr, bt.ptr, -100, 0.0, H.CE_MEAN, blse.ptr, bc.ptr, bg.ptr, bd.ptr, V, None))

    def copy_fwd():  # moves half the logits: nbytes in all (read + write)
        H.check(H.lib().kf_memcpy_d2d(bd.ptr, bx.ptr, half, None))

    def copy_bwd():
        H.check(H.lib().kf_memcpy_d2d(bd.ptr, bx.ptr, nbytes, None))

    for _ in range(args.warmup):
        copy_fwd(), copy_bwd(), fwd(), bwd()
    H.device_sync()
    ms = {"fwd": [], "bwd": [], "copy_fwd": [], "copy_bwd": []}
    for _ in range(args.iters):  # interleaved: drift of the clock or of the neighbours' load hits both sides alike
        ms["copy_fwd"].append(event_ms(copy_fwd))
        ms["fwd"].append(event_ms(fwd))
        ms["copy_bwd"].append(event_ms(copy_bwd))
        ms["bwd"].append(event_ms(bwd))
    med = {k: statistics.median(v) for k, v in ms.items()}
    fb, bb = nbytes, 2 * nbytes
    res = {"dtype": name, "rows": rows, "V": V, "regime": regime(rows, V), "workspace_bytes": need,
           "fwd_ms": med["fwd"], "bwd_ms": med["bwd"], "fwd_bytes": fb, "bwd_bytes": bb,
           "fwd_TBps": fb / med["fwd"] / 1e9, "bwd_TBps": bb / med["bwd"] / 1e9,
           "copy_fwd_TBps": 2 * half / med["copy_fwd"] / 1e9, "copy_bwd_TBps": 2 * nbytes / med["copy_bwd"] / 1e9,
           "spread_fwd_ms": [min(ms["fwd"]), max(ms["fwd"])], "spread_bwd_ms": [min(ms["bwd"]), max(ms["bwd"])]}
    res["fwd_of_copy"] = res["fwd_TBps"] / res["copy_fwd_TBps"]
    res["bwd_of_copy"] = res["bwd_TBps"] / res["copy_bwd_TBps"]
    if args.check:
        fwd()  # the mean's count for the backward, then the per-row losses of a NONE run
        bwd()
        H.device_sync()
        dl = H.DevBuf(4 * rows)
        keep = H.ce_fwd(code, rows, V, bx.ptr, bt.ptr, dl.ptr, reduction=H.CE_NONE)
        H.device_sync()
        del keep
        loss = dl.to_numpy((rows,), np.float32)
        worst_l = worst_d = 0.0
        r_out = {H.BF16: 2.0 ** -8, H.F16: 2.0 ** -11, H.F32: 2.0 ** -16}[code]
        for r in sorted(set(rng.choice(rows, min(rows, 8), replace=False).tolist()) | {0, rows - 1}):
            x = O.to_float(tile[r % TILE], code)
            rl, rd = ref_row(x, t[r])
            rd /= rows  # mean, nothing ignored
            worst_l = max(worst_l, abs(loss[r] - rl) / (1e-4 + 1e-5 * abs(rl)))
            row = np.empty(V, tile.dtype)
            H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, bd.ptr + r * V * es, V * es, None))
            got = O.to_float(row, code).astype(np.float64)
            worst_d = max(worst_d, float(np.max(np.abs(got - rd) / (r_out * np.abs(rd) + 1e-6 / rows))))
        res["check"] = {"loss_err_over_tol": float(worst_l), "dlogits_err_over_tol": worst_d, "ok": bool(worst_l <= 1 and worst_d <= 1)}
    del ws
    if not args.no_torch:
        try:
            res["torch"] = torch_context(name, rows, V, tile, t, args)
        except RuntimeError as e:  # context only: a torch that sees no GPU leaves the row "not measured"
            res["torch"] = {"not_measured": str(e)}
    out.append(res)
    print(json.dumps(res), file=sys.stderr)


def torch_context(name, rows, V, tile, t, args):
    import torch
    import torch.nn.functional as F
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[name]
    src = torch.from_numpy(O.to_float(tile, CODES[name]).astype(np.float32)).to("cuda").to(dt)
    x = src.repeat((rows + TILE - 1) // TILE, 1)[:rows].contiguous().requires_grad_(True)
    tt = torch.from_numpy(t).to("cuda")
    f_ms, fb_ms = [], []
    for i in range(args.warmup + args.iters):
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        x.grad = None
        a.record()
        loss = F.cross_entropy(x, tt)
        b.record()
        loss.backward()
        c.record()
        c.synchronize()
        if i >= args.warmup:
            f_ms.append(a.elapsed_time(b))
            fb_ms.append(a.elapsed_time(c))
    res = {"fwd_ms": statistics.median(f_ms), "fwd_bwd_ms": statistics.median(fb_ms), "torch": torch.__version__}
    del x, src
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated shape indices into the default list")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("ce_bench needs a GPU: there is no CPU path to time")
    H.set_device(0)
    p = H.device_props(0)
    shapes = [SHAPES[int(i)] for i in args.only.split(",")] if args.only else SHAPES
    out = []
    for name, rows, V in shapes:
        bench_shape(name, rows, V, args, out)
    doc = {"device": p.name.decode(errors="replace"), "arch": p.arch.decode(errors="replace"), "cus": p.compute_units,
           "warmup": args.warmup, "iters": args.iters, "device_lib_sha": H.lib().kf_build_source_sha().decode(), "shapes": out}
    print(json.dumps(doc))
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
