#!/usr/bin/env python3
"""The chunked linear + cross-entropy loss (kfunca.linear_cross_entropy) against the composition it replaces, in time and in memory, and
its row kernel (kf_ce_fused_rows) against a copy of its algorithmic bytes.

Shapes, T 32768: bf16 (d, V) = (4096, 128256), (2048, 151936), (768, 50304) and f32 (1024, 32000). Per shape, interleaved in one process in
an order that rotates every round, the median of --iters wall-clock times between two device synchronisations (a call is tens of
milliseconds: the host's share does not show):
  fused   forward + backward at chunk_rows 1024 / 2048 / 4096 / 8192
  comp    gemm -> cross_entropy -> backward (cross-entropy's backward, then the two gemm_ex products of the linear layer), the SAME call
          timed twice (comp_a, comp_b): the distance between the two medians is the box's spread, the yardstick for fused vs comp
  rows    kf_ce_fused_rows alone (f32 logits -> the operands' dtype, one chunk of 4096 rows) beside a kf_memcpy_d2d that moves the same
          bytes (the logits read once as the algorithm needs them, the gradient written once; the kernel's second read is its own cost)
Memory: the growth of the allocator's pool (memstat_dict active + cached bytes) across one forward + backward that starts from a pool
emptied by release_cached() - everything the call had to obtain, the chunk buffers it freed again included - for every fused chunk size
and for the composition; `held` is the same after another release_cached(), with the loss still alive.
Per-kernel times of one fused call at the default chunk_rows come from kf_profile_* (no profiler tracing).
The default chunk_rows rule: the fastest chunk size of the (4096, 128256) sweep whose pool growth stays under a quarter of the
composition's; `default_rule` reports what the rule picks on this run.
The operands are small random tiles repeated down the rows (x: 61 rows, weight: 257 rows), so gigabytes are filled without building them
on the host, and --check can hold sampled rows of dX, sampled rows of dW and the loss to an f64 reference computed on the tiles.
Prints one JSON object; --json saves it (default profiles/r06_linear_ce_bench.json), stamped with ce_fused.hip's content hash."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
import kfunca_amd as kfunca  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

SOURCES = ("ce_fused.hip", "float_pack.h", "common.h", "gemm.hip")
# (label, dtype, T, d, V)
SHAPES = [("bf16 d4096 V128256", "bf16", 32768, 4096, 128256), ("bf16 d2048 V151936", "bf16", 32768, 2048, 151936),
          ("bf16 d768 V50304", "bf16", 32768, 768, 50304), ("f32 d1024 V32000", "f32", 32768, 1024, 32000)]
CHUNKS = (1024, 2048, 4096, 8192)
CODES = {"bf16": H.BF16, "f32": H.F32}
OUT_R = {"bf16": 2.0 ** -8, "f32": 2.0 ** -16}
XT, WT = 61, 257   # distinct rows of x and of the weight


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def tiled(tile_store, rows, dtype):
    """A [rows, cols] device tensor whose row r holds tile row r % len(tile): uploaded in blocks of whole tiles."""
    n, cols = tile_store.shape
    t = kfunca.empty([rows, cols], getattr(kfunca.dtype, "bfloat16" if dtype == "bf16" else "float"), 0)
    reps = max(1, (32 << 20) // tile_store.nbytes)
    block = np.ascontiguousarray(np.tile(tile_store, (reps, 1)))
    row_bytes = cols * tile_store.itemsize
    for r0 in range(0, rows, n * reps):
        m = min(n * reps, rows - r0)
        H.check(H.lib().kf_memcpy_h2d(t.data_ptr() + r0 * row_bytes, block.ctypes.data, m * row_bytes, None))
    return t


def pool():
    s = kfunca.memstat_dict(0)
    return s["active_bytes"] + s["cached_bytes"]


def reference(xt, wt, t, T, V):
    """f64, on the tiles: the mean loss, and functions giving row i of dX and row v of dW (nothing ignored, g = 1, mean)."""
    logits = xt @ wt.T                                     # [XT, WT]: row i of the real logits is logits[i % XT] repeated along V
    reps = np.bincount(np.arange(V) % WT, minlength=WT)    # how often each tile column occurs among the V classes
    m = logits.max(1, keepdims=True)
    lse = (m + np.log((np.exp(logits - m) * reps).sum(1, keepdims=True)))[:, 0]
    p = np.exp(logits - lse[:, None])                      # the probability of ONE class of each tile column
    rows = np.arange(T) % XT
    loss = (lse[rows] - logits[rows, t % WT]).mean()
    nrow = np.bincount(rows, minlength=XT)

    def dx_row(i):
        r = i % XT
        d = (p[r] * reps) @ wt - wt[t[i] % WT]
        a = (p[r] * reps) @ np.abs(wt) + np.abs(wt[t[i] % WT])
        return d / T, a / T

    def dw_row(v):
        hit = np.bincount(rows[t == v], minlength=XT)
        d = (p[:, v % WT] * nrow) @ xt - hit @ xt
        a = (p[:, v % WT] * nrow) @ np.abs(xt) + hit @ np.abs(xt)
        return d / T, a / T

    return loss, dx_row, dw_row


def bench_shape(shape, args):
    label, dtype, T, d, V = shape
    code = CODES[dtype]
    rng = np.random.default_rng(d + V)
    xs = O.from_float(rng.uniform(-1, 1, (XT, d)).astype(np.float32), code)
    ws = O.from_float((rng.uniform(-1, 1, (WT, d)) * (4.0 / np.sqrt(d))).astype(np.float32), code)
    t = rng.integers(0, V, T).astype(np.int64)
    tx, tw = tiled(xs, T, dtype), tiled(ws, V, dtype)
    twt = tw.permute(1, 0).contiguous()                  # [d, V]: the composition's gemm takes the head this way
    tt = kfunca.from_numpy(t, 0)
    one = kfunca.from_numpy(np.ones(1, np.float32), 0)
    for p in (tx, tw, twt):
        p.set_requires_grad(True)

    def clear():
        for p in (tx, tw, twt):
            p.zero_grad()

    def fused(chunk):
        def call():
            loss = kfunca.linear_cross_entropy(tx, tw, tt, chunk_rows=chunk)
            loss.backward(one)
            return loss
        return call

    def comp():
        loss = kfunca.cross_entropy(kfunca.gemm(tx, twt, 1.0, 0.0), tt)
        loss.backward(one)
        return loss

    calls = {f"fused_{c}": fused(c) for c in CHUNKS}
    calls["comp_a"] = comp
    calls["comp_b"] = comp
    res = {"label": label, "dtype": dtype, "T": T, "d": d, "V": V, "logits_bytes": T * V * H.DTYPE_SIZE[code]}

    # memory first, each call from an emptied pool
    mem = {}
    for name, call in calls.items():
        if name == "comp_b":
            continue
        clear()
        kfunca.synchronize(0)
        kfunca.release_cached(0)
        base = pool()
        loss = call()
        kfunca.synchronize(0)
        grown = pool() - base
        clear()
        kfunca.release_cached(0)
        held = pool() - base
        del loss
        mem[name.replace("comp_a", "comp")] = {"pool_growth_bytes": grown, "held_bytes": held}
    res["memory"] = mem

    if args.check:
        want_loss, dx_row, dw_row = reference(O.to_float(xs, code).astype(np.float64), O.to_float(ws, code).astype(np.float64), t, T, V)
        clear()
        loss = fused(0)()
        kfunca.synchronize(0)
        got_loss = float(loss.numpy()[0])
        dx, dw = tx.grad(), tw.grad()
        worst = {"dX": 0.0, "dW": 0.0}
        pick = np.random.default_rng(1)
        for name, g, fn, idx in (("dX", dx, dx_row, np.r_[0, T - 1, pick.choice(T, 6, replace=False)]),
                                 ("dW", dw, dw_row, np.r_[0, V - 1, t[:3], pick.choice(V, 3, replace=False)])):
            for i in idx:
                raw = np.empty(d, xs.dtype)   # row i of a dense [*, d] gradient, straight from the device
                H.check(H.lib().kf_memcpy_d2h(raw.ctypes.data, g.data_ptr() + int(i) * raw.nbytes, raw.nbytes, None))
                row = O.to_float(raw, code).astype(np.float64)
                want, asum = fn(int(i))
                worst[name] = max(worst[name], float(np.max(np.abs(row - want) / (OUT_R[dtype] * (asum + np.abs(want)) + 1e-7))))
        loss_err = abs(got_loss - want_loss) / (1e-4 + 1e-5 * abs(want_loss))
        res["check"] = {"loss": got_loss, "loss_ref": want_loss, "loss_err_over_tol": loss_err, "dX_err_over_bound": worst["dX"],
                        "dW_err_over_bound": worst["dW"], "ok": bool(loss_err <= 1 and worst["dX"] <= 1 and worst["dW"] <= 1)}
        del loss, dx, dw

    # time: every call once per round, the order rotating
    names = list(calls)
    ms = {n: [] for n in names}
    for it in range(args.warmup + args.iters):
        order = names[it % len(names):] + names[:it % len(names)]
        for n in order:
            clear()
            kfunca.synchronize(0)
            t0 = time.perf_counter()
            loss = calls[n]()
            kfunca.synchronize(0)
            dt = 1e3 * (time.perf_counter() - t0)
            del loss
            if it >= args.warmup:
                ms[n].append(dt)
    med = {n: statistics.median(v) for n, v in ms.items()}
    comp_ms = min(med["comp_a"], med["comp_b"])
    res["time_ms"] = {n: {"median": med[n], "min": min(ms[n]), "max": max(ms[n])} for n in names}
    res["comp_spread_ms"] = abs(med["comp_a"] - med["comp_b"])
    res["fused_over_comp"] = {n: med[n] / comp_ms for n in names if n.startswith("fused")}

    # per-kernel times of one fused call at the default chunk size
    clear()
    kfunca.synchronize(0)
    H.profile_reset()
    H.profile_enable(True)
    loss = fused(0)()
    kfunca.synchronize(0)
    H.profile_enable(False)
    res["default_chunk_rows"] = int(kfunca._linear_ce_chunk_rows(0))
    res["kernels_ms_at_default"] = {k: {"ms": v[0], "launches": v[1]} for k, v in sorted(H.profile_results().items(), key=lambda kv: -kv[1][0])}
    del loss
    clear()
    del tx, tw, twt
    kfunca.release_cached(0)

    # the row kernel alone: one chunk of f32 logits -> the operands' dtype, beside a copy of its algorithmic bytes
    rows = 4096
    es = H.DTYPE_SIZE[code]
    lt = rng.uniform(-4, 4, (XT, V)).astype(np.float32)
    bx, bd = H.DevBuf(rows * V * 4), H.DevBuf(rows * V * 4)
    for r0 in range(0, rows, XT):
        n = min(XT, rows - r0)
        H.check(H.lib().kf_memcpy_h2d(bx.ptr + r0 * V * 4, lt.ctypes.data, n * V * 4, None))
    bt, bl = H.DevBuf.from_numpy(t[:rows]), H.DevBuf(4 * rows)
    inplace = code == H.F32
    nbytes = rows * V * (4 + es)

    def rows_call():
        H.check(H.lib().kf_ce_fused_rows(H.F32, code, rows, V, V, bx.ptr, bt.ptr, -100, 0.0, 0.0, bl.ptr, None, bx.ptr if inplace else bd.ptr, V, None, 0, None))

    def copy_call():
        H.check(H.lib().kf_memcpy_d2d(bd.ptr, bx.ptr, nbytes // 2 // 256 * 256, None))

    for _ in range(3):
        rows_call(), copy_call()
    H.device_sync()
    rk, ck = [], []
    for _ in range(max(args.iters, 10)):
        ck.append(event_ms(copy_call))
        rk.append(event_ms(rows_call))
    r_ms, c_ms = statistics.median(rk), statistics.median(ck)
    res["rows_kernel"] = {"rows": rows, "V": V, "pair": f"f32->{dtype}", "in_place": inplace, "bytes": nbytes, "ms": r_ms, "TBps": nbytes / r_ms / 1e9,
                          "copy_ms": c_ms, "copy_TBps": nbytes / c_ms / 1e9, "of_copy": c_ms / r_ms}
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def default_rule(case):
    """The fastest fused chunk size whose pool growth stays under a quarter of the composition's."""
    cap = case["memory"]["comp"]["pool_growth_bytes"] / 4
    ok = [c for c in CHUNKS if case["memory"][f"fused_{c}"]["pool_growth_bytes"] < cap]
    return min(ok, key=lambda c: case["time_ms"][f"fused_{c}"]["median"]) if ok else None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--check", action="store_true", help="hold sampled rows of dX and dW and the loss to the f64 reference before timing")
    ap.add_argument("--only", default="", help="run the shapes whose label contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_linear_ce_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("linear_ce_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"tool": "tools/linear_ce_bench.py", "iters": args.iters, "warmup": args.warmup, "chunks": list(CHUNKS), "cases": []}
    for shape in SHAPES:
        if args.only in shape[0]:
            out["cases"].append(bench_shape(shape, args))
    for c in out["cases"]:
        if (c["d"], c["V"]) == (4096, 128256):
            out["default_rule"] = {"picks": default_rule(c), "default_chunk_rows": c["default_chunk_rows"]}
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    if any(not c.get("check", {"ok": True})["ok"] for c in out["cases"]):
        raise SystemExit("linear_ce_bench --check: an output is outside its bound of the f64 reference")


if __name__ == "__main__":
    main()
