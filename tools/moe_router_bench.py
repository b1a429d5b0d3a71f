#!/usr/bin/env python3
"""The fused mixture-of-experts router (kf_moe_router_fwd / kf_moe_router_bwd) against the composition it replaces, and the auxiliary
losses (kf_moe_aux_loss_fwd / kf_moe_aux_loss_bwd) against a copy of their algorithmic bytes, C ABI.

Cases, T 32768: Mixtral-like (bf16, E 8, k 2, softmax + normalize), Qwen3-MoE-like (bf16, E 128, k 8, softmax + normalize), E 256 k 8
with sigmoid + normalize (bf16), and the Qwen3-MoE shape in f32. Per case and operation, interleaved in one loop whose order rotates,
the median of --iters HIP-event times:
  new    the entry: router_fwd, router_bwd, aux_fwd (the walk and the fold), aux_bwd
  comp   what a layer ran before (the router only):
           router_fwd   kf_softmax_fwd, then topk's stable descending kf_sort of every [T, E] row with int64 positions, then
                        kf_moe_gate_fwd (the copy of the first k columns that topk makes is NOT timed, and the sort orders the
                        logits, not p: both in the composition's favour; a sigmoid score has no composed form and is timed against
                        the softmax one)
           router_bwd   kf_moe_gate_bwd, then kf_softmax_bwd
  copy   kf_memcpy_d2d moving the operation's algorithmic bytes (half read, half written), es = the element size:
           router_fwd   T E es + T k (8 + es)              router_bwd   2 T E es + T k (8 + es)
           aux_fwd      T E es                             aux_bwd      2 T E es
--check holds sampled rows of every output (and the three scalars of the loss, against all rows) to tests/moe_router_ref.py's bounds
before timing. Prints one JSON object; --json saves it (default profiles/r06_moe_router_bench.json), stamped with moe_router.hip's
content hash."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from tests import moe_router_ref as R  # noqa: E402

SOURCES = ("moe_router.hip", "float_pack.h", "common.h")
# (label, dtype code, T, E, k, score, normalize)
SHAPES = [("mixtral", R.BF16, 32768, 8, 2, R.SOFTMAX, True), ("qwen3-moe", R.BF16, 32768, 128, 8, R.SOFTMAX, True),
          ("e256 k8 sigmoid", R.BF16, 32768, 256, 8, R.SIGMOID, True), ("qwen3-moe f32", R.F32, 32768, 128, 8, R.SOFTMAX, True)]
BALANCE_COEF, Z_COEF, DLOSS = 1e-2, 1e-3, 0.75


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def bench_case(shape, args):
    label, code, T, E, k, score, normalize = shape
    es, ut = R.ES[code], R.UINT[code]
    rng = np.random.default_rng(E + k + es)
    b = R.draw_logits(rng, "normal", code, T, E)
    dgb = R.draw_dgate(rng, code, T, k)
    logits, dgate = H.DevBuf.from_numpy(b), H.DevBuf.from_numpy(dgb)
    ids, gate, dlogits = H.DevBuf(8 * T * k), H.DevBuf(es * T * k), H.DevBuf(es * T * E)
    offsets, row_pair, pair_row = H.DevBuf(8 * (E + 1)), H.DevBuf(4 * T * k), H.DevBuf(4 * T * k)
    plan_bytes = H.moe_plan_workspace_bytes(T, k, E)
    plan_ws = H.DevBuf(plan_bytes)
    aux_bytes = H.moe_aux_loss_workspace_bytes(T, E)
    aux_ws = H.DevBuf(aux_bytes)
    scalars = H.DevBuf.from_numpy(np.array([0, 0, 0, DLOSS], np.float32))   # loss, L_bal, L_z, dloss
    # the composition's operands
    p, keys, pos, dp = H.DevBuf(es * T * E), H.DevBuf(es * T * E), H.DevBuf(8 * T * E), H.DevBuf(es * T * E)
    sort_bytes = H.lib().kf_sort_workspace_bytes(code, T, E)
    sort_ws = H.DevBuf(max(sort_bytes, 16))
    copy_src, copy_dst = H.DevBuf(es * T * E + 16 * T * k), H.DevBuf(es * T * E + 16 * T * k)

    new = {
        "router_fwd": lambda: H.moe_router_fwd(code, T, E, k, score, normalize, logits.ptr, E, ids.ptr, gate.ptr, k),
        "router_bwd": lambda: H.moe_router_bwd(code, T, E, k, score, normalize, logits.ptr, E, ids.ptr, dgate.ptr, k, dlogits.ptr, E),
        "aux_fwd": lambda: H.moe_aux_loss_fwd(code, T, E, k, logits.ptr, E, offsets.ptr, BALANCE_COEF, Z_COEF, scalars.ptr, scalars.ptr + 4, aux_ws.ptr,
                                              aux_bytes),
        "aux_bwd": lambda: H.moe_aux_loss_bwd(code, T, E, k, logits.ptr, E, offsets.ptr, BALANCE_COEF, Z_COEF, scalars.ptr + 12, dlogits.ptr, E),
    }

    def comp_fwd():
        H.softmax_fwd(H.SOFTMAX, code, T, E, 1.0, logits.ptr, E, p.ptr, E)
        H.check(H.lib().kf_sort(code, logits.ptr, keys.ptr, pos.ptr, T, E, 1, sort_ws.ptr if sort_bytes else None, sort_bytes, None))
        H.moe_gate_fwd(code, T, k, E, ids.ptr, p.ptr, E, normalize, gate.ptr, k)

    def comp_bwd():
        H.moe_gate_bwd(code, T, k, E, ids.ptr, p.ptr, E, normalize, gate.ptr, k, dgate.ptr, k, dp.ptr, E)
        H.softmax_bwd(H.SOFTMAX, code, T, E, 1.0, p.ptr, E, dp.ptr, E, dp.ptr, E)

    comp = {"router_fwd": comp_fwd, "router_bwd": comp_bwd}
    nbytes = {"router_fwd": T * E * es + T * k * (8 + es), "router_bwd": 2 * T * E * es + T * k * (8 + es), "aux_fwd": T * E * es, "aux_bwd": 2 * T * E * es}

    def copy(op):
        H.check(H.lib().kf_memcpy_d2d(copy_dst.ptr, copy_src.ptr, nbytes[op] // 2, None))

    # the ids and the plan every later call reads
    new["router_fwd"]()
    H.moe_plan(ids.ptr, T, k, E, offsets.ptr, row_pair.ptr, pair_row.ptr, plan_ws.ptr if plan_bytes else None, plan_bytes)
    H.device_sync()

    checks = []
    if args.check:
        x, dg = R.floats(b, code), R.floats(dgb, code)
        want = R.select(b, code, k)
        got_ids = ids.to_numpy((T, k), np.int64)
        ok = bool(np.array_equal(got_ids, want))
        checks.append({"what": "ids (all rows)", "worst_error_over_bound": 0.0 if ok else float("inf"), "ok": ok})
        rows = np.unique(np.random.default_rng(3).integers(0, T, 64))
        ref = R.gate(x[rows], want[rows], score, normalize)
        got = R.floats(gate.to_numpy((T, k), ut), code)[rows]
        worst = float((np.abs(got - ref) / R.gate_bound(code, ref)).max())
        checks.append({"what": "gate", "worst_error_over_bound": worst, "ok": worst <= 1.0})
        new["router_bwd"]()
        H.device_sync()
        ref = R.router_backward(x[rows], want[rows], dg[rows], score, normalize)
        got = R.floats(dlogits.to_numpy((T, E), ut), code)[rows]
        worst = float((np.abs(got - ref) / R.router_backward_bound(code, E, k, dg[rows], ref)).max())
        checks.append({"what": "router dlogits", "worst_error_over_bound": worst, "ok": worst <= 1.0})
        counts = np.diff(offsets.to_numpy(E + 1, np.int64))
        assert np.array_equal(counts, R.counts_of(want, E))
        new["aux_fwd"]()
        new["aux_bwd"]()
        H.device_sync()
        wanted = R.aux_forward(x, counts, k, BALANCE_COEF, Z_COEF)
        got = scalars.to_numpy(3, np.float32)
        worst = max(abs(float(g) - r) / R.loss_bound(r) for g, r in zip(got, wanted))
        checks.append({"what": "loss, L_bal, L_z", "values": [float(g) for g in got], "worst_error_over_bound": worst, "ok": worst <= 1.0})
        ref = R.aux_backward(x, counts, k, BALANCE_COEF, Z_COEF, DLOSS)
        got = R.floats(dlogits.to_numpy((T, E), ut), code)
        worst = float((np.abs(got - ref) / R.aux_backward_bound(code, x, counts, k, BALANCE_COEF, Z_COEF, DLOSS, ref))[rows].max())
        checks.append({"what": "aux dlogits", "worst_error_over_bound": worst, "ok": worst <= 1.0})

    comp_fwd()   # p and gate as the composition's backward reads them
    H.device_sync()
    res = {"shape": label, "dtype": R.CODE_NAME[code], "T": T, "E": E, "k": k, "score": R.SCORE_NAME[score], "normalize": bool(normalize), "ops": {}}
    for op in ("router_fwd", "router_bwd", "aux_fwd", "aux_bwd"):
        runs = {"new": new[op], "copy": lambda op=op: copy(op)}
        if op in comp:
            runs["comp"] = comp[op]
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        H.device_sync()
        ms = {name: [] for name in runs}
        names = list(runs)
        for i in range(args.iters):   # interleaved, and the order rotates: each follows each
            for j in range(len(names)):
                name = names[(i + j) % len(names)]
                ms[name].append(event_ms(runs[name]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        out = {"bytes": nbytes[op], "new_us": 1e3 * med["new"], "copy_us": 1e3 * med["copy"], "new_over_copy": med["new"] / med["copy"],
               "new_TBs": nbytes[op] / med["new"] / 1e9, "spread_new_us": [1e3 * min(ms["new"]), 1e3 * max(ms["new"])]}
        if op in comp:
            out.update({"comp_us": 1e3 * med["comp"], "new_over_comp": med["new"] / med["comp"]})
        res["ops"][op] = out
    if checks:
        res["check"] = checks
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="hold sampled rows to the reference's bounds before timing")
    ap.add_argument("--only", default="", help="run the shapes whose label contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_moe_router_bench.json")
    args = ap.parse_args()
    if args.iters < 10:
        raise SystemExit("moe_router_bench: a median of fewer than 10 calls is not reported")
    if H.device_count() == 0:
        raise SystemExit("moe_router_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"tool": "tools/moe_router_bench.py", "iters": args.iters, "warmup": args.warmup, "cases": []}
    for shape in SHAPES:
        if args.only in shape[0]:
            out["cases"].append(bench_case(shape, args))
    out.update(bench.stamp(SOURCES))
    bad = [c for c in out["cases"] for chk in c.get("check", []) if not chk["ok"]]
    print(json.dumps(out))
    if bad:
        raise SystemExit("moe_router_bench --check: an output is outside its bound of the f64 reference")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
