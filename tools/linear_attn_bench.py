#!/usr/bin/env python3
"""Chunked linear attention (kf_linear_attn_fwd, kf_linear_attn_bwd) beside causal softmax attention (kf_attn_fwd, kf_attn_bwd) on the
same q, k, v, in bf16 at B 8, S 4096 and 8192, with H 32, D 128 and H 64, D 64.

  time    median event times of four calls interleaved in one process in an order that rotates every round: linear forward, linear
          backward, and attention forward + backward TWICE (attn_a, attn_b): the distance between its two medians is the box's spread.
          TFLOP/s count the products the linear kernels execute (the forward forms P once per 64-column slice of Dv, and so on), and
          the causal half of attention's.
  --check sampled heads (the first and the last) of o, dq, dk, dv, dg against the f64 O(S^2) expression of tests/linear_attn_ref.py on
          the operands read back, within the tests' random-tier bound (c = 2): the shapes no test reaches - 256 and 512 heads of half a
          gigabyte per tensor and 64 to 128 turns of the double buffer.
Prints one JSON object; --json saves it (default profiles/r06_linear_attn_bench.json), stamped with the content hash of linear_attn.hip."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from tests import gemm_views as V  # noqa: E402
from tests.linear_attn_ref import U, reference  # noqa: E402
from tools.gemm_fp8_bench import bf16_seed, event_ms, fill, read, rotate_times  # noqa: E402

SOURCES = ("linear_attn.hip",)
SHAPES = [(8, 32, 4096, 128), (8, 32, 8192, 128), (8, 64, 4096, 64), (8, 64, 8192, 64)]


def linear_flops(B, Hh, S, D):
    """(forward, backward) products as executed, per 64-step chunk: the forward's P, Q S, P V and state update once per Dv slice; the
    ascending walk's dP, dO S^T, M K and state update; the descending walk's P, M, the two carried and the two in-chunk products, dS."""
    per = B * Hh * ((S + 63) // 64) * 2 * 64
    return per * (D // 64) * 64 * (3 * D + 64), per * ((2 * 64 * D + 2 * D * D) + (4 * 64 * D + 3 * D * D))


def check_heads(B, Hh, S, D, scale, bufs):
    """the worst fraction of the random-tier bound over the sampled heads, per output"""
    worst = {}
    for head in (0, B * Hh - 1):
        t16 = lambda n: V.decode(read(bufs[n].ptr + head * S * D * 2, S * D, np.uint16), "bf16").reshape(1, S, D)
        f32 = lambda n: read(bufs[n].ptr + head * S * 4, S, np.float32).astype(np.float64).reshape(1, S)
        ref, absref = reference(t16("q"), t16("k"), t16("v"), f32("g"), t16("do"), scale)
        for n in ("o", "dq", "dk", "dv", "dg"):
            got = f32(n) if n == "dg" else t16(n)
            frac = np.abs(got - ref[n]) / (U * np.abs(ref[n]) + (2 * U + S * 2.0 ** -23) * absref[n] + 1e-300)
            worst[n] = max(worst.get(n, 0.0), float(frac.max()))
    return {"heads": [0, B * Hh - 1], "worst_fraction_of_bound": worst, "ok": bool(max(worst.values()) <= 1.0)}


def bench_shape(shape, args, rng):
    B, Hh, S, D = shape
    n16, scale = B * Hh * S * D * 2, float(np.float32(D ** -0.5))
    bufs = {n: H.DevBuf(n16) for n in ("q", "k", "v", "do", "o", "dq", "dk", "dv", "ao")}
    bufs.update({n: H.DevBuf(B * Hh * S * 4) for n in ("g", "dg", "lse")})
    for n in ("q", "k", "v", "do"):
        fill(bufs[n].ptr, n16, bf16_seed(rng))
    bufs["g"] = H.DevBuf.from_numpy(-rng.uniform(0, 0.05, B * Hh * S).astype(np.float32))
    lws = H.DevBuf(H.linear_attn_bwd_workspace_bytes(H.BF16, B, Hh, S, D, D))
    aws = H.DevBuf(H.attn_bwd_workspace_bytes(H.BF16, B, Hh, S, S, D))
    p = {n: b.ptr for n, b in bufs.items()}

    def lin_fwd():
        H.linear_attn_fwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["o"])

    def lin_bwd():
        H.linear_attn_bwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["do"], p["dq"], p["dk"], p["dv"], p["dg"], workspace=lws.ptr,
                          workspace_bytes=lws.nbytes)

    def attn():
        H.attn_fwd(H.BF16, B, Hh, S, S, D, p["q"], p["k"], p["v"], p["ao"], p["lse"])
        H.attn_bwd(H.BF16, B, Hh, S, S, D, p["q"], p["k"], p["v"], p["ao"], p["lse"], p["do"], p["dq"], p["dk"], p["dv"], aws.ptr, aws.nbytes)

    out = {"B": B, "H": Hh, "S": S, "D": D, "forward_workgroups": B * Hh * D // 64, "backward_workgroups_per_walk": B * Hh}
    t = rotate_times({"linear_fwd": lin_fwd, "linear_bwd": lin_bwd, "attn_a": attn, "attn_b": attn}, args.iters, args.warmup, event_ms)
    if args.check:   # after the timing: the last writer of dq, dk, dv must be the linear backward
        lin_fwd(), lin_bwd()
        H.device_sync()
        out["check"] = check_heads(B, Hh, S, D, scale, bufs)
    ff, fb = linear_flops(B, Hh, S, D)
    a = min(t["attn_a"]["median"], t["attn_b"]["median"])
    lin = t["linear_fwd"]["median"] + t["linear_bwd"]["median"]
    out.update({"time_ms": t, "attn_spread_ms": abs(t["attn_a"]["median"] - t["attn_b"]["median"]),
                "linear_fwd_TFLOPs": ff / t["linear_fwd"]["median"] / 1e9, "linear_bwd_TFLOPs": fb / t["linear_bwd"]["median"] / 1e9,
                "attn_fwd_bwd_TFLOPs_causal_half": 3.5 * 2.0 * B * Hh * S * S * D / a / 1e9, "linear_fwd_bwd_over_attn_fwd_bwd": lin / a})
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="hold sampled heads to the tests' random-tier bound")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_linear_attn_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("linear_attn_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    rng = np.random.default_rng(950)
    out = {"tool": "tools/linear_attn_bench.py", "iters": args.iters, "warmup": args.warmup, "dtype": "bf16"}
    out["shapes"] = [bench_shape(s, args, rng) for s in SHAPES]
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    if args.check and not all(r["check"]["ok"] for r in out["shapes"]):
        raise SystemExit("linear_attn_bench --check: an output is outside its bound")


if __name__ == "__main__":
    main()
