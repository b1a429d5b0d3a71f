#!/usr/bin/env python3
"""Rotary position embeddings (kf_rope) against the box's own copy rate, through the C ABI.

For each case: the call timed with HIP events (median of --iters after --warmup), interleaved in the same loop with a kf_memcpy_d2d of
the same algorithmic bytes - out of place and backward read and write the whole packed tensor (2 * T * W * s bytes, a copy of all of it);
in place reads and writes only the rotated elements (2 * T * h_rot * R * s: the copied heads and dims are not touched). TB/s = those bytes / median time;
`time_over_copy` is the kernel's time over the copy's for the same bytes (1.0 = copy speed, higher = slower).
torch's GPU HF-style RoPE (split, rotate_half, cat) on the same tensor is timed as context when torch sees a GPU (--no-torch skips it).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (the kernels are rope_packed / rope_elem).
Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

CODES = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}
# (name, dtype, B, S, Hq, Hkv, D, R, positions, mode)
CASES = [
    ("packed bf16 fwd", "bf16", 8, 4096, 32, 32, 128, 128, False, "fwd"),
    ("packed bf16 fwd in place", "bf16", 8, 4096, 32, 32, 128, 128, False, "inplace"),
    ("packed bf16 bwd", "bf16", 8, 4096, 32, 32, 128, 128, False, "bwd"),
    ("packed bf16 fwd, positions", "bf16", 8, 4096, 32, 32, 128, 128, True, "fwd"),
    ("packed bf16 bwd, positions", "bf16", 8, 4096, 32, 32, 128, 128, True, "bwd"),
    ("GQA 32/8 bf16 fwd", "bf16", 8, 4096, 32, 8, 128, 128, False, "fwd"),
    ("D 64 / H 64 bf16 fwd", "bf16", 8, 4096, 64, 64, 64, 64, False, "fwd"),
    ("f32 fwd", "f32", 8, 4096, 32, 32, 128, 128, False, "fwd"),
    ("R = D/2 bf16 fwd", "bf16", 8, 4096, 32, 32, 128, 64, False, "fwd"),
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
    """torch's GPU RoPE as HF writes it, on the same packed shape: context only."""
    try:
        import torch
    except ImportError:
        return None
    if args.no_torch or not torch.cuda.is_available():
        return None
    _, name, B, S, Hq, Hkv, D, R, _, _ = case
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[name]
    qkv = torch.randn(B, S, Hq + 2 * Hkv, D, device="cuda", dtype=dt)
    inv = 1.0 / (10000 ** (torch.arange(0, R, 2, device="cuda", dtype=torch.float32) / R))
    f = torch.outer(torch.arange(S, device="cuda", dtype=torch.float32), inv)
    cos, sin = torch.cat([f, f], -1).cos().to(dt)[None, :, None], torch.cat([f, f], -1).sin().to(dt)[None, :, None]

    def rot(x):
        x1, x2 = x[..., : R // 2], x[..., R // 2: R]
        return torch.cat([x[..., :R] * cos + torch.cat([-x2, x1], -1) * sin, x[..., R:]], -1)

    def step():
        q, k, v = qkv.split([Hq, Hkv, Hkv], 2)
        return torch.cat([rot(q), rot(k), v], 2)

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


def bench_case(case, args):
    label, name, B, S, Hq, Hkv, D, R, use_pos, mode = case
    code = CODES[name]
    es = H.DTYPE_SIZE[code]
    Ht, h_rot = Hq + 2 * Hkv, Hq + Hkv
    W, T = Ht * D, B * S
    nbytes = T * W * es
    rng = np.random.default_rng(T + W)
    tile = O.from_float(rng.uniform(-2, 2, (TILE, W)).astype(np.float32), code)
    bx, by = H.DevBuf(nbytes), H.DevBuf(nbytes)
    for r0 in range(0, T, TILE):
        n = min(TILE, T - r0)
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r0 * W * es, tile.ctypes.data, n * W * es, None))
    P = S
    cos, sin = H.DevBuf(P * R // 2 * 4), H.DevBuf(P * R // 2 * 4)
    H.rope_table(10000.0, R, P, cos.ptr, sin.ptr)
    bp = H.DevBuf.from_numpy(rng.permutation(np.tile(np.arange(S), B)).astype(np.int64)) if use_pos else None
    lay = (S * W, D, W)
    if mode == "inplace":
        moved = 2 * T * h_rot * R * es  # reads and writes the rotated elements only; v heads and dims >= R stay put, unread
    else:
        moved = 2 * nbytes
    copy_bytes = (moved // 2) // 256 * 256

    def kernel():
        if mode == "inplace":
            H.rope(code, B, Ht, S, D, bx.ptr, lay, None, None, cos.ptr, sin.ptr, P, R, h_rot, bp.ptr if bp else None)
        else:
            H.rope(code, B, Ht, S, D, bx.ptr, lay, by.ptr, lay, cos.ptr, sin.ptr, P, R, h_rot, bp.ptr if bp else None, inverse=mode == "bwd")

    def copy():
        H.check(H.lib().kf_memcpy_d2d(by.ptr, bx.ptr, copy_bytes, None))

    for _ in range(args.warmup):
        copy(), kernel()
    H.device_sync()
    ms = {"kernel": [], "copy": []}
    for _ in range(args.iters):  # interleaved: drift of the clock or of the neighbours' load hits both sides alike
        ms["copy"].append(event_ms(copy))
        ms["kernel"].append(event_ms(kernel))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"case": label, "dtype": name, "B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "R": R, "positions": use_pos, "mode": mode,
           "bytes": moved, "ms": med["kernel"], "TBps": moved / med["kernel"] / 1e9, "copy_ms": med["copy"],
           "copy_TBps": 2 * copy_bytes / med["copy"] / 1e9, "spread_ms": [min(ms["kernel"]), max(ms["kernel"])]}
    res["time_over_copy"] = res["copy_TBps"] / res["TBps"]
    t = torch_ms(case, args)
    res["torch_ms"] = t if t is not None else "not measured"
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose label contains this text")
    ap.add_argument("--json", type=Path)
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("rope_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"cases": [bench_case(c, args) for c in CASES if args.only in c[0]]}
    text = json.dumps(out)
    print(text)
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
