#!/usr/bin/env python3
"""The fused AdamW step (kf_adamw_step) against the box's own copy rate, through the C ABI.

Cases: one large flat f32 tensor (f32 grads), the same with a bf16 param + f32 master, and the ~200 weight tensors of a Llama-style
model of ~1.1B parameters (TinyLlama's shapes: vocab 32000, d 2048, 22 layers, FFN 5632, 4 KV heads of 64; bf16 params, f32 masters,
f32 grads) - each without and with clipping. Every step is timed with HIP events (median of --iters after --warmup), interleaved in the
same loop with a kf_memcpy_d2d that moves the same algorithmic bytes (half of them read, half written). Bytes per element:
  f32 param and grad: 28 (p r+w, g r, m r+w, v r+w), +4 for the norm pass (g read again)
  bf16 param + f32 master, f32 grad: 30 (master r+w, p16 w, g r, m r+w, v r+w), +4 for the norm pass
TB/s = those bytes / median time; `of_copy` = that over the copy's rate. Launches per step: 2 ceil(n / 48) without clipping, one more
with. Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (kernels adamw_norm / adamw_fold /
adamw_advance / adamw_update). Prints one JSON object; --json saves it."""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402


def llama_1b_shapes(vocab=32000, d=2048, layers=22, ffn=5632, kv=256):
    shapes = [(vocab, d)]
    for _ in range(layers):
        shapes += [(d,), (d, d), (kv, d), (kv, d), (d, d), (d,), (ffn, d), (ffn, d), (d, ffn)]
    return shapes + [(d,), (vocab, d)]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def make_tensors(numels, bf16):
    """Device buffers for each tensor (param, grad, master, m, v, step), filled with small values (the step's speed does not depend on
    them). Returns (the kf_adamw_tensor array, the buffers to keep alive)."""
    keep, descs = [], []
    for n in numels:
        p = H.DevBuf(n * (2 if bf16 else 4))
        g, m, v, s = H.DevBuf(n * 4), H.DevBuf(n * 4), H.DevBuf(n * 4), H.DevBuf(4)
        ms = H.DevBuf(n * 4) if bf16 else None
        for b in (p, g, m, v, s) + ((ms,) if ms else ()):
            b.zero()
        keep += [p, g, m, v, s, ms]
        descs.append(dict(numel=n, param_dtype=H.BF16 if bf16 else H.F32, grad_dtype=H.F32, param=p.ptr, grad=g.ptr, master=ms.ptr if ms else None,
                          exp_avg=m.ptr, exp_avg_sq=v.ptr, step=s.ptr, weight_decay=0.01))
    return H.adamw_tensors(descs), keep


def bench_case(name, numels, bf16, args):
    arr, keep = make_tensors(numels, bf16)
    n = len(numels)
    total = sum(numels)
    per = 30 if bf16 else 28
    lr = H.DevBuf.from_numpy(np.array([1e-4], np.float32))
    norm = H.DevBuf(4)
    need = H.adamw_workspace_bytes(n, 1.0)
    ws = H.DevBuf(need)
    res = {"case": name, "tensors": n, "elements": total}
    for clip in (False, True):
        nbytes = total * (per + (4 if clip else 0))
        half = nbytes // 2 // 256 * 256
        src, dst = H.DevBuf(half), H.DevBuf(half)

        def step():
            H.check(H.lib().kf_adamw_step(arr, n, 0.9, 0.95, 1e-8, lr.ptr, 1.0, 1.0 if clip else 0.0, norm.ptr if clip else None,
                                          ws.ptr if clip else None, need if clip else 0, None))

        def copy():
            H.check(H.lib().kf_memcpy_d2d(dst.ptr, src.ptr, half, None))

        for _ in range(args.warmup):
            copy(), step()
        H.device_sync()
        ms = {"step": [], "copy": []}
        for _ in range(args.iters):  # interleaved: drift of the clock or of the neighbours' load hits both sides alike
            ms["copy"].append(event_ms(copy))
            ms["step"].append(event_ms(step))
        med = {k: statistics.median(v) for k, v in ms.items()}
        key = "clip" if clip else "noclip"
        res[key] = {"ms": med["step"], "bytes": nbytes, "TBps": nbytes / med["step"] / 1e9, "copy_TBps": 2 * half / med["copy"] / 1e9,
                    "launches": 2 * math.ceil(n / 48) + (1 if clip else 0), "spread_ms": [min(ms["step"]), max(ms["step"])]}
        res[key]["of_copy"] = res[key]["TBps"] / res[key]["copy_TBps"]
        del src, dst
    del keep
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--flat", type=int, default=1 << 28, help="elements of the flat tensor")
    ap.add_argument("--json", type=Path)
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("adamw_bench.py needs a GPU")
    H.set_device(0)
    shapes = llama_1b_shapes()
    out = {"results": [bench_case("flat f32", [args.flat], False, args), bench_case("flat bf16 + master", [args.flat], True, args),
                       bench_case(f"llama-1.1B list ({len(shapes)} tensors)", [math.prod(s) for s in shapes], True, args)]}
    print(json.dumps(out))
    if args.json:
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
