#!/usr/bin/env python3
"""The gated delta rule (kf_delta_rule_fwd: the chunk-parallel prepare kernel and the walk; kf_delta_rule_step) in bf16 at B 8, S 4096 and
8192, with H 32, D 128 and H 64, D 64, with h0 given and hT returned.

  time    median event times of the calls interleaved in one process in an order that rotates every round, every one of them TWICE
          (_a, _b: the distance between the two medians of one call is the box's spread for it): kf_delta_rule_fwd, and beside it
          kf_linear_attn_state_fwd on the same q, k, v, g - context, not a pass mark: the delta rule does the linear kernel's products
          and W S0, T W, T V and K K^T besides, and the inversion. The prepare kernel's share comes from the per-label profile
          (kf_profile_*) of one extra call.
  step    kf_delta_rule_step at T = 1 and T = 4 on the [B, H, D, D] f32 state beside a kf_memcpy_d2d of the state's bytes (one read and
          one write of them, the step's algorithmic traffic), STEP_BATCH calls per event pair, interleaved and rotated the same way.
  --check the first and the last head of o and hT against the float64 recurrence of tests/delta_rule_ref.py on the operands read back,
          within the tests' random-tier bound (C = 5): shapes no test reaches.
k and q are unit-norm rows, v in U(-1, 1), beta in U(0, 1), g in -U(0, 0.05): the recurrence is contractive and stays bounded.
Prints one JSON object; --json saves it (default profiles/r06_delta_rule_bench.json), stamped with the content hashes of its sources."""
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
from tests.delta_rule_ref import C, U, reference, worst  # noqa: E402
from tools.gemm_fp8_bench import bf16_seed, event_ms, fill, read, rotate_times  # noqa: E402

SOURCES = ("delta_rule.hip", "linear_mix.h", "linear_attn.hip")
SHAPES = [(8, 32, 4096, 128), (8, 32, 8192, 128), (8, 64, 4096, 64), (8, 64, 8192, 64)]
STEP_BATCH = 20   # one step call moves tens of megabytes: too short for one event pair


def unit_rows_seed(rng, D):
    """a host block of whole unit-norm bf16 rows: fill() doubles it on the device, and rows stay rows"""
    a = rng.normal(size=(1 << 14, D))
    return V.encode(a / np.linalg.norm(a, axis=1, keepdims=True), "bf16")


def check_heads(B, Hh, S, D, scale, p):
    out = {}
    for head in (0, B * Hh - 1):
        t16 = lambda n: V.decode(read(p[n] + head * S * D * 2, S * D, np.uint16), "bf16").reshape(1, S, D)
        f32 = lambda n: read(p[n] + head * S * 4, S, np.float32).astype(np.float64).reshape(1, S)
        sta = lambda n: read(p[n] + head * D * D * 4, D * D, np.float32).astype(np.float64).reshape(1, D, D)
        ro, rs = reference(t16("q"), t16("k"), t16("v"), f32("g"), f32("beta"), scale, sta("h0"))
        out[head] = {"o_error_over_u_max_ref": worst(t16("o"), ro) / U, "hT_error_over_u_max_ref": worst(sta("hT"), rs) / U}
    return {"heads": out, "bound": C, "ok": bool(max(max(v.values()) for v in out.values()) <= C)}


def bench_shape(shape, args, rng):
    B, Hh, S, D = shape
    n16, nst, scale = B * Hh * S * D * 2, B * Hh * D * D * 4, float(np.float32(D ** -0.5))
    bufs = {n: H.DevBuf(n16) for n in ("q", "k", "v", "o")}
    fill(bufs["q"].ptr, n16, unit_rows_seed(rng, D)), fill(bufs["k"].ptr, n16, unit_rows_seed(rng, D)), fill(bufs["v"].ptr, n16, bf16_seed(rng))
    bufs["g"] = H.DevBuf.from_numpy(-rng.uniform(0, 0.05, B * Hh * S).astype(np.float32))
    bufs["beta"] = H.DevBuf.from_numpy(rng.uniform(0, 1, B * Hh * S).astype(np.float32))
    bufs["h0"] = H.DevBuf.from_numpy(rng.uniform(-0.125, 0.125, B * Hh * D * D).astype(np.float32))
    bufs.update({n: H.DevBuf(nst) for n in ("hT", "st")})
    ws = H.DevBuf(H.delta_rule_fwd_workspace_bytes(H.BF16, B, Hh, S, D, D))
    p = {n: b.ptr for n, b in bufs.items()}
    head = (H.BF16, B, Hh, S, D, D, scale)

    def delta_fwd():
        H.delta_rule_fwd(*head, p["q"], p["k"], p["v"], p["g"], p["beta"], p["h0"], p["o"], p["hT"], workspace=ws.ptr, workspace_bytes=ws.nbytes)

    def linear_fwd():
        H.linear_attn_state_fwd(*head, p["q"], p["k"], p["v"], p["g"], p["h0"], p["o"], p["hT"])

    def step(T):   # the first T D values of every head's q, k, v serve as its [T, D] operands
        def run():
            for _ in range(STEP_BATCH):
                H.delta_rule_step(H.BF16, B, Hh, T, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["beta"], p["st"], p["o"])
        return run

    def copy():
        for _ in range(STEP_BATCH):
            H.check(H.lib().kf_memcpy_d2d(p["hT"], p["st"], nst, None))

    H.check(H.lib().kf_memcpy_d2d(p["st"], p["h0"], nst, None))
    t = rotate_times({f"{n}_{x}": f for n, f in dict(delta_fwd=delta_fwd, linear_state_fwd=linear_fwd).items() for x in "ab"}, args.iters, args.warmup,
                     event_ms)
    ts = rotate_times({f"{n}_{x}": f for n, f in dict(step_T1=step(1), step_T4=step(4), copy=copy).items() for x in "ab"}, args.iters, args.warmup,
                      event_ms)
    best = lambda r, n: min(r[n + "_a"]["median"], r[n + "_b"]["median"])
    cp = best(ts, "copy") / STEP_BATCH
    out = {"B": B, "H": Hh, "S": S, "D": D, "prepare_workgroups": B * Hh * ((S + 63) // 64), "walk_workgroups": B * Hh * D // 64,
           "workspace_bytes": ws.nbytes, "time_ms": t, "spread_ms": {n: abs(t[n + "_a"]["median"] - t[n + "_b"]["median"]) for n in ("delta_fwd", "linear_state_fwd")},
           "delta_fwd_over_linear_state_fwd": best(t, "delta_fwd") / best(t, "linear_state_fwd"),
           "step": {"calls_per_event_pair": STEP_BATCH, "state_bytes": nst, "batch_time_ms": ts, "copy_TBps": 2 * nst / cp / 1e9,
                    **{f"T{T}": {"ms_per_call": best(ts, f"step_T{T}") / STEP_BATCH, "fraction_of_copy_rate": cp / best(ts, f"step_T{T}") * STEP_BATCH}
                       for T in (1, 4)}}}
    H.profile_enable(True)   # the two kernels of one call, by label
    H.profile_reset()
    delta_fwd()
    H.device_sync()
    out["one_call_by_label_ms"] = {k: ms for k, (ms, _) in H.profile_results().items() if k.startswith("delta_rule")}
    H.profile_enable(False)
    if args.check:
        out["check"] = check_heads(B, Hh, S, D, scale, p)
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="hold sampled heads to the tests' random-tier bound")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_delta_rule_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("delta_rule_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    rng = np.random.default_rng(950)
    out = {"tool": "tools/delta_rule_bench.py", "iters": args.iters, "warmup": args.warmup, "dtype": "bf16"}
    out["shapes"] = [bench_shape(s, args, rng) for s in SHAPES]
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    if args.check and not all(r["check"]["ok"] for r in out["shapes"]):
        raise SystemExit("delta_rule_bench --check: an output is outside its bound")


if __name__ == "__main__":
    main()
