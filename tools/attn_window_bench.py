#!/usr/bin/env python3
"""Sliding-window attention (kf_attn_window_fwd / kf_attn_window_bwd) through the C ABI: median HIP-event times of forward and backward
(bf16, D 128 and 64) beside padded-causal attention on the same tensors.

For each case, in one interleaved loop of --iters after --warmup:
  window_fwd / window_bwd   kf_attn_window_fwd / kf_attn_window_bwd (backward = delta + dQ + dK/dV kernels)
  causal_fwd / causal_bwd   kf_attn_prefix_fwd / kf_attn_prefix_bwd without a prefix on the same tensors and key lengths: the same kernels
                            under the causal mask, every tile below the diagonal - what a model without a window kernel would run, and
                            what the window's shorter key loop has to beat
A visited tile is a (128-query block, 64-key tile) pair of one query head that the forward's workgroup walks: under a window the tiles
max(0, q0 - left) / 64 .. ceil(min(len_b, qe + right) / 64) - 1 of the block [q0, qe), under the causal mask 0 .. ceil(min(len_b, qe) / 64) - 1.
Times are reported per visited tile, as the ratio window / causal (time_ratio) beside the ratio of the visited tiles (tile_ratio), and as
their quotient (excess = time_ratio / tile_ratio: 1.0 is "time follows the tiles").
--check samples two K/V heads per case (one at S > 4096) against the float64 reference (tests/attn_full_ref.py under
tests/attn_window_ref.py's visibility) with the project's bounds. Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

MIXED = (1.0, 0.25, 0.6, 0.9, 0.1, 0.75, 0.5, 0.33)
# (name, B, Hq, Hkv, S, (left, right) with None = unbounded, key lengths as fractions of S per batch (cycled) or None); each at D 128 and 64
SHAPES = [
    ("window 512 S4096", 8, 16, 16, 4096, (512, 0), None),
    ("window 1024 S4096", 8, 16, 16, 4096, (1024, 0), None),
    ("window 4096 S8192", 2, 16, 16, 8192, (4096, 0), None),
    ("symmetric 256 S1024", 32, 16, 16, 1024, (256, 256), None),
    ("padded window 512 S4096", 8, 16, 16, 4096, (512, 0), MIXED),
    ("GQA 32/8 window 512 S4096", 4, 32, 8, 4096, (512, 0), None),
]
CASES = [(f"{s[0]} D{D}",) + s[1:5] + (D,) + s[5:] for D in (128, 64) for s in SHAPES]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def visited_tiles(S, lens, window):
    """(128-query block, 64-key tile) pairs per query head the window forward walks, and those the causal forward walks"""
    left, right = window
    win = causal = 0
    for ln in lens:
        for q0 in range(0, S, 128):
            qe = min(S, q0 + 128)
            first = 0 if left is None else max(0, q0 - left) // 64
            last = (min(ln, S if right is None else qe + right) + 63) // 64
            win += max(0, last - first)
            causal += (min(ln, qe) + 63) // 64
    return win, causal


def run_case(case, args):
    name, B, Hq, Hkv, S, D, window, fr = case
    code = H.BF16
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    wl, wr = (-1 if x is None else x for x in window)
    rng = np.random.default_rng(len(name))
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * S * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    q, go = take(0, (B, Hq, S, D)), take(1024, (B, Hq, S, D))
    k, v = take(2048, (B, Hkv, S, D)), take(3072, (B, Hkv, S, D))
    lens = None if fr is None else [max(1, int(S * fr[b % len(fr)])) for b in range(B)]
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    bl = None if lens is None else H.DevBuf.from_numpy(np.asarray(lens, np.int64))
    lp = None if bl is None else bl.ptr
    bo, blse, bdq, bdk, bdv = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    bo2, blse2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S)     # the yardstick's outputs: the window call's stay for --check
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    ws = H.DevBuf(need)
    fwd_args = (code, B, Hq, Hkv, S, S, D, scale, bq.ptr, bk.ptr, bv.ptr)
    wkw = dict(kv_len=lp, window_left=wl, window_right=wr)
    window_fwd = lambda: H.attn_window_fwd(*fwd_args, bo.ptr, blse.ptr, **wkw)  # noqa: E731
    window_bwd = lambda: H.attn_window_bwd(*fwd_args, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, **wkw)  # noqa: E731
    causal_fwd = lambda: H.attn_prefix_fwd(*fwd_args, bo2.ptr, blse2.ptr, kv_len=lp)  # noqa: E731
    causal_bwd = lambda: H.attn_prefix_bwd(*fwd_args, bo2.ptr, blse2.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, kv_len=lp)  # noqa: E731
    timed = {"window_fwd": window_fwd, "causal_fwd": causal_fwd, "window_bwd": window_bwd, "causal_bwd": causal_bwd}
    t = {n: [] for n in timed}
    for it in range(args.warmup + args.iters):
        for n, fn in timed.items():   # each backward follows its own forward: o and lse are its family's
            ms = event_ms(fn)
            if it >= args.warmup:
                t[n].append(ms)
    win, causal = visited_tiles(S, lens or [S] * B, window)
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "window": [wl, wr], "kv_len": lens, "visited_tiles": Hq * win,
           "causal_tiles": Hq * causal, "tile_ratio": round(win / causal, 4)}
    med = {n: statistics.median(x) for n, x in t.items()}
    out.update({f"{n}_ms": round(m, 4) for n, m in med.items()})
    for d in ("fwd", "bwd"):
        out[f"window_{d}_ns_per_tile"] = round(med[f"window_{d}"] * 1e6 / (Hq * win), 2)
        out[f"causal_{d}_ns_per_tile"] = round(med[f"causal_{d}"] * 1e6 / (Hq * causal), 2)
        out[f"{d}_time_ratio"] = round(med[f"window_{d}"] / med[f"causal_{d}"], 3)
        out[f"{d}_excess"] = round(med[f"window_{d}"] / med[f"causal_{d}"] / (win / causal), 3)
    if args.check:
        from oracle import checks as K
        from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis
        from tests.attn_window_ref import window_vis
        window_fwd()
        window_bwd()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), bdq.to_numpy(q.shape, q.dtype)
        dk, dv = bdk.to_numpy(k.shape, k.dtype), bdv.to_numpy(k.shape, k.dtype)
        G = Hq // Hkv
        samples = ((1 % B, 0), (B - 1, Hkv - 1))
        for b, j in samples[:1] if S > 4096 else samples:   # a whole group: its query heads and their K/V head
            hs, js = slice(j * G, (j + 1) * G), slice(j, j + 1)
            sl = lambda x, s: x[b:b + 1, s]  # noqa: E731
            vis = window_vis(None if lens is None else lens[b:b + 1], window[0], window[1], S, S, 1)
            ops = (sl(q, hs), sl(k, js), sl(v, js), sl(go, hs))
            ref, fl = attn_ref64_vis(*ops, vis, code), format_floor_vis(*ops, vis, code)
            for nm, got in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, js)), ("dv", sl(dv, js))):
                K.check_one(nm, got, ref, code, f"{name} b{b} kv-head {j}", floor=fl.get(nm))
            check_lse(sl(lse, hs), ref, name)
        out["check"] = "ok"
    print(f"[attn_window_bench] {name}: fwd {out['fwd_time_ratio']} of causal for {out['tile_ratio']} of its tiles", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--json")
    args = ap.parse_args()
    H.set_device(0)
    cases = [c for c in CASES if not args.cases or c[0] in args.cases.split(",")]
    props = H.device_props(0)
    import bench
    res = {"tool": "attn_window_bench", "device": props.name.decode(), "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_full.hip", "common.h", "runtime.hip")))   # the sources every column of the table comes from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
