#!/usr/bin/env python3
"""The causal depthwise conv1d (kf_causal_conv1d_fwd, kf_causal_conv1d_bwd) and its decode step at B 8, S 4096 and 8192, K 4 with SiLU:
bf16 at C 12288 with ld 12288 and 16384 (Gated-DeltaNet-like q | k | v), bf16 at C 5376 with ld 10880 (a Mamba-2-like slice), f32 at C 4096.

  time    median event times of forward, backward and a kf_memcpy_d2d of the same algorithmic bytes (forward: read x, write y - one
          copy of x's bytes; backward: read x and dy, write dx - one and a half), interleaved in one process in an order that rotates
          every round, every call TWICE (_a, _b): the distance between the two medians of one call is the box's spread for it.
  step    the forward at T = 1 and T = 4 on the [B, K - 1, C] state in place, STEP_BATCH calls per event pair.
  --check sampled channels (the first and the last 16-byte pack) of y, hT, dx, d_h0, dw, dbias against tests/causal_conv1d_ref.py on
          the operands read back, within the bounds of tests/test_gpu_causal_conv1d.py.
Prints one JSON object; --json saves it (default profiles/r06_causal_conv1d_bench.json), stamped with the content hash of causal_conv1d.hip."""
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
from tests.causal_conv1d_ref import ROWS, bound, reference  # noqa: E402
from tools.gemm_fp8_bench import bf16_seed, event_ms, fill, read, rotate_times  # noqa: E402

SOURCES = ("causal_conv1d.hip",)
SHAPES = [(dt, 8, S, C, ld) for S in (4096, 8192) for dt, C, ld in (("bf16", 12288, 12288), ("bf16", 12288, 16384), ("bf16", 5376, 10880), ("f32", 4096, 4096))]
K, ACT, STEP_BATCH = 4, H.CONV1D_ACT_SILU, 50


def check_channels(dt, B, S, C, ld, p):
    """the worst fraction of the tests' bound over the sampled packs, per output"""
    es, code = (2, np.uint16) if dt == "bf16" else (4, np.float32)
    pack, worst = 16 // es, {}
    cols = (0, C - pack)
    shapes = dict(x=(B * S, ld), dy=(B * S, ld), y=(B * S, C), dx=(B * S, C), w=(K, C), dw=(K, C), bias=(1, C), dbias=(1, C),
                  **{n: (B * (K - 1), C) for n in ("h0", "dhT", "hT", "dh0")})
    got = {}
    for n, (r, w) in shapes.items():   # one read per operand, the sampled packs kept
        full = read(p[n], r * w, code).reshape(r, w)
        got[n] = [V.decode(full[:, c:c + pack].copy(), dt) for c in cols]
    for i in range(len(cols)):
        g = {n: v[i] for n, v in got.items()}
        seq, sta = lambda n: g[n].reshape(B, S, pack), lambda n: g[n].reshape(B, K - 1, pack)
        ref, absref = reference(seq("x"), g["w"], g["bias"][0], sta("h0"), True, seq("dy"), sta("dhT"))
        parts = ROWS + 3 + B * -(-S // (4 * ROWS)) + K + 2
        for n, out, cnt in (("y", seq("y"), K + 1), ("dx", seq("dx"), K + 2), ("dh0", sta("dh0"), K + 2), ("dw", g["dw"], parts), ("dbias", g["dbias"][0], parts)):
            worst[n] = max(worst.get(n, 0.0), float((np.abs(out - ref[n]) / (bound(ref[n], absref[n], dt, cnt, True) + 1e-300)).max()))
        worst["hT_exact"] = worst.get("hT_exact", True) and bool(np.array_equal(sta("hT"), ref["hT"]))
    return {"channels": list(cols), "worst_fraction_of_bound": worst,
            "ok": bool(worst["hT_exact"] and max(v for n, v in worst.items() if n != "hT_exact") <= 1.0)}


def bench_shape(shape, args, rng):
    dt, B, S, C, ld = shape
    es, code = (2, H.BF16) if dt == "bf16" else (4, H.F32)
    wide, dense, state = B * S * ld * es, B * S * C * es, B * (K - 1) * C * es
    bufs = {n: H.DevBuf(wide) for n in ("x", "dy")}
    bufs.update({n: H.DevBuf(dense) for n in ("y", "dx", "src", "dst")}, dst2=H.DevBuf(dense // 2))
    bufs.update({n: H.DevBuf(state) for n in ("h0", "dhT", "hT", "dh0", "st")}, w=H.DevBuf(K * C * es), dw=H.DevBuf(K * C * es), bias=H.DevBuf(C * es),
                dbias=H.DevBuf(C * es))
    for n in ("x", "dy", "h0", "dhT", "w", "bias", "src", "st"):
        fill(bufs[n].ptr, bufs[n].nbytes, bf16_seed(rng))
    ws = H.DevBuf(H.causal_conv1d_bwd_workspace_bytes(code, B, S, C, K))
    p = {n: b.ptr for n, b in bufs.items()}

    def fwd():
        H.causal_conv1d_fwd(code, ACT, B, S, C, K, p["x"], ld, p["w"], p["bias"], p["h0"], p["y"], C, p["hT"])

    def bwd():
        H.causal_conv1d_bwd(code, ACT, B, S, C, K, p["x"], ld, p["w"], p["bias"], p["h0"], p["dy"], ld, p["dhT"], p["dx"], C, p["dw"], p["dbias"], p["dh0"],
                            workspace=ws.ptr, workspace_bytes=ws.nbytes)

    def copy(halves):   # halves x half of the dense bytes read and written
        def run():
            H.check(H.lib().kf_memcpy_d2d(p["dst"], p["src"], dense, None))
            if halves == 3:
                H.check(H.lib().kf_memcpy_d2d(p["dst2"], p["src"], dense // 2, None))
        return run

    def step(T):   # the first T rows of every batch row of x serve as the new tokens
        def run():
            for _ in range(STEP_BATCH):
                H.causal_conv1d_fwd(code, ACT, B, T, C, K, p["x"], ld, p["w"], p["bias"], p["st"], p["y"], C, p["st"])
        return run

    calls = {"fwd": fwd, "bwd": bwd, "copy_fwd_bytes": copy(2), "copy_bwd_bytes": copy(3)}
    t = rotate_times({f"{n}_{x}": f for n, f in calls.items() for x in "ab"}, args.iters, args.warmup, event_ms)
    ts = rotate_times({f"step_T{T}_{x}": step(T) for T in (1, 4) for x in "ab"}, args.iters, args.warmup, event_ms)
    best = lambda r, n: min(r[n + "_a"]["median"], r[n + "_b"]["median"])
    out = {"dtype": dt, "B": B, "S": S, "C": C, "ld": ld, "K": K, "act": "silu", "time_ms": t,
           "spread_ms": {n: abs(t[n + "_a"]["median"] - t[n + "_b"]["median"]) for n in calls},
           "fwd_TBps": 2 * dense / best(t, "fwd") / 1e9, "bwd_TBps": 3 * dense / best(t, "bwd") / 1e9, "copy_TBps": 2 * dense / best(t, "copy_fwd_bytes") / 1e9,
           "fwd_fraction_of_copy_rate": best(t, "copy_fwd_bytes") / best(t, "fwd"), "bwd_fraction_of_copy_rate": best(t, "copy_bwd_bytes") / best(t, "bwd"),
           "halo_over_algorithmic_bytes": (K - 1) / ROWS / 2, "workspace_over_backward_bytes": 2 * ws.nbytes / (3 * dense),
           "step_us_per_call": {f"T{T}": 1e3 * best(ts, f"step_T{T}") / STEP_BATCH for T in (1, 4)}}
    if args.check:
        fwd(), bwd()
        H.device_sync()
        out["check"] = check_channels(dt, B, S, C, ld, p)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="hold sampled channels to the tests' bounds")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_causal_conv1d_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("causal_conv1d_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    rng = np.random.default_rng(960)
    out = {"tool": "tools/causal_conv1d_bench.py", "iters": args.iters, "warmup": args.warmup}
    out["shapes"] = [bench_shape(s, args, rng) for s in SHAPES]
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    if args.check and not all(r["check"]["ok"] for r in out["shapes"]):
        raise SystemExit("causal_conv1d_bench --check: an output is outside its bound")


if __name__ == "__main__":
    main()
