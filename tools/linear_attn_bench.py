#!/usr/bin/env python3
"""Chunked linear attention (kf_linear_attn_fwd, kf_linear_attn_bwd), its state variants (kf_linear_attn_state_fwd / _bwd with h0, hT,
d_hT and d_h0 all given) and the token-by-token recurrence (kf_linear_attn_step) beside causal softmax attention (kf_attn_fwd,
kf_attn_bwd) on the same q, k, v, in bf16 at B 8, S 4096 and 8192, with H 32, D 128 and H 64, D 64.

  time    median event times of the calls interleaved in one process in an order that rotates every round: the stateless and the state
          forward and backward, and attention forward + backward, every one of them TWICE (_a, _b): the distance between the two
          medians of one call is the box's spread for it. TFLOP/s count the products the linear kernels execute (the forward forms P
          once per 64-column slice of Dv, and so on), and the causal half of attention's.
  step    kf_linear_attn_step at T = 1 and T = 4 on the [B, H, D, D] f32 state beside a kf_memcpy_d2d of the state's bytes (one read
          and one write of them, the step's algorithmic traffic), STEP_BATCH calls per event pair, interleaved and rotated the same way.
  --check sampled heads (the first and the last) of o, dq, dk, dv, dg, and with the state of hT and d_h0 too, against the f64 O(S^2)
          expressions of tests/linear_attn_state_ref.py on the operands read back, within the tests' random-tier bound (c = 2): the
          shapes no test reaches - 256 and 512 heads of half a gigabyte per tensor and 64 to 128 turns of the double buffer.
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
from tests.linear_attn_state_ref import bound, reference  # noqa: E402
from tools.gemm_fp8_bench import bf16_seed, event_ms, fill, read, rotate_times  # noqa: E402

SOURCES = ("linear_attn.hip",)
SHAPES = [(8, 32, 4096, 128), (8, 32, 8192, 128), (8, 64, 4096, 64), (8, 64, 8192, 64)]
STEP_BATCH = 20   # one step call moves tens of megabytes: too short for one event pair


def linear_flops(B, Hh, S, D):
    """(forward, backward) products as executed, per 64-step chunk: the forward's P, Q S, P V and state update once per Dv slice; the
    ascending walk's dP, dO S^T, M K and state update; the descending walk's P, M, the two carried and the two in-chunk products, dS."""
    per = B * Hh * ((S + 63) // 64) * 2 * 64
    return per * (D // 64) * 64 * (3 * D + 64), per * ((2 * 64 * D + 2 * D * D) + (4 * 64 * D + 3 * D * D))


def check_heads(B, Hh, S, D, scale, bufs, state):
    """the worst fraction of the random-tier bound over the sampled heads, per output (state: h0 and dhT went in, hT and dh0 came out)"""
    worst = {}
    for head in (0, B * Hh - 1):
        t16 = lambda n: V.decode(read(bufs[n].ptr + head * S * D * 2, S * D, np.uint16), "bf16").reshape(1, S, D)
        f32 = lambda n: read(bufs[n].ptr + head * S * 4, S, np.float32).astype(np.float64).reshape(1, S)
        sta = lambda n: read(bufs[n].ptr + head * D * D * 4, D * D, np.float32).astype(np.float64).reshape(1, D, D)
        ref, absref = reference(t16("q"), t16("k"), t16("v"), f32("g"), t16("do"), scale, *((sta("h0"), sta("dhT")) if state else ()))
        for n in ("o", "dq", "dk", "dv", "dg") + (("hT", "dh0") if state else ()):
            got = f32(n) if n == "dg" else sta(n) if n in ("hT", "dh0") else t16(n)
            frac = np.abs(got - ref[n]) / (bound(ref[n], absref[n], S, 2) + 1e-300)
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
    for n in ("h0", "dhT"):
        bufs[n] = H.DevBuf.from_numpy(rng.uniform(-1, 1, B * Hh * D * D).astype(np.float32))
    bufs.update({n: H.DevBuf(B * Hh * D * D * 4) for n in ("hT", "dh0", "st")})
    lws = H.DevBuf(H.linear_attn_state_bwd_workspace_bytes(H.BF16, B, Hh, S, D, D))
    aws = H.DevBuf(H.attn_bwd_workspace_bytes(H.BF16, B, Hh, S, S, D))
    p = {n: b.ptr for n, b in bufs.items()}

    def lin_fwd():
        H.linear_attn_fwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["o"])

    def lin_bwd():
        H.linear_attn_bwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["do"], p["dq"], p["dk"], p["dv"], p["dg"], workspace=lws.ptr,
                          workspace_bytes=lws.nbytes)

    def state_fwd():
        H.linear_attn_state_fwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["h0"], p["o"], p["hT"])

    def state_bwd():
        H.linear_attn_state_bwd(H.BF16, B, Hh, S, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["h0"], p["do"], p["dhT"], p["dq"], p["dk"], p["dv"],
                                p["dg"], p["dh0"], workspace=lws.ptr, workspace_bytes=lws.nbytes)

    def step(T):   # the first T D values of every head's q, k, v serve as its [T, D] operands; the state decays, so it stays bounded
        def run():
            for _ in range(STEP_BATCH):
                H.linear_attn_step(H.BF16, B, Hh, T, D, D, scale, p["q"], p["k"], p["v"], p["g"], p["st"], p["o"])
        return run

    def copy():
        for _ in range(STEP_BATCH):
            H.check(H.lib().kf_memcpy_d2d(p["hT"], p["st"], bufs["st"].nbytes, None))

    def attn():
        H.attn_fwd(H.BF16, B, Hh, S, S, D, p["q"], p["k"], p["v"], p["ao"], p["lse"])
        H.attn_bwd(H.BF16, B, Hh, S, S, D, p["q"], p["k"], p["v"], p["ao"], p["lse"], p["do"], p["dq"], p["dk"], p["dv"], aws.ptr, aws.nbytes)

    out = {"B": B, "H": Hh, "S": S, "D": D, "forward_workgroups": B * Hh * D // 64, "backward_workgroups_per_walk": B * Hh}
    H.check(H.lib().kf_memcpy_d2d(p["st"], p["h0"], bufs["st"].nbytes, None))
    calls = {"linear_fwd": lin_fwd, "state_fwd": state_fwd, "linear_bwd": lin_bwd, "state_bwd": state_bwd, "attn": attn}
    t = rotate_times({f"{n}_{x}": f for n, f in calls.items() for x in "ab"}, args.iters, args.warmup, event_ms)
    ts = rotate_times({f"{n}_{x}": f for n, f in dict(step_T1=step(1), step_T4=step(4), copy=copy).items() for x in "ab"}, args.iters, args.warmup,
                      event_ms)
    if args.check:   # after the timing: the last writer of dq, dk, dv must be the backward under check
        lin_fwd(), lin_bwd()
        H.device_sync()
        out["check"] = check_heads(B, Hh, S, D, scale, bufs, False)
        state_fwd(), state_bwd()
        H.device_sync()
        out["check_state"] = check_heads(B, Hh, S, D, scale, bufs, True)
    ff, fb = linear_flops(B, Hh, S, D)
    best = lambda r, n: min(r[n + "_a"]["median"], r[n + "_b"]["median"])
    a, lin = best(t, "attn"), best(t, "linear_fwd") + best(t, "linear_bwd")
    t["linear_fwd"], t["linear_bwd"] = {"median": best(t, "linear_fwd")}, {"median": best(t, "linear_bwd")}
    cp, nb = best(ts, "copy") / STEP_BATCH, bufs["st"].nbytes
    out.update({"spread_ms": {n: abs(t[n + "_a"]["median"] - t[n + "_b"]["median"]) for n in calls},
                "state_over_stateless": {"fwd": best(t, "state_fwd") / best(t, "linear_fwd"), "bwd": best(t, "state_bwd") / best(t, "linear_bwd")},
                "step": {"calls_per_event_pair": STEP_BATCH, "state_bytes": nb, "workgroups": B * Hh * D // 64, "batch_time_ms": ts,
                         "copy_TBps": 2 * nb / cp / 1e9,
                         **{f"T{T}": {"ms_per_call": best(ts, f"step_T{T}") / STEP_BATCH, "TBps_of_state_bytes": 2 * nb / best(ts, f"step_T{T}") * STEP_BATCH / 1e9,
                                      "fraction_of_copy_rate": cp / best(ts, f"step_T{T}") * STEP_BATCH} for T in (1, 4)}}})
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
    if args.check and not all(r["check"]["ok"] and r["check_state"]["ok"] for r in out["shapes"]):
        raise SystemExit("linear_attn_bench --check: an output is outside its bound")


if __name__ == "__main__":
    main()
