#!/usr/bin/env python3
"""Mixture-of-experts routing on the device (kf_moe_plan, kf_moe_dispatch, kf_moe_combine, kf_moe_combine_bwd) against a copy of the same
bytes and against the composition these entries replace, C ABI, bf16.

Cases: Mixtral-like (T 32768, k 2, E 8, d 4096), Qwen3-MoE-like (T 32768, k 8, E 128, d 2048) and k 8, E 256, d 7168 (T 32768), each with
balanced and Zipf-skewed expert choices. Per case and operation, interleaved in one loop whose order rotates, median of --iters HIP-event times:
  moe    the new entry
  copy   kf_memcpy_d2d moving the same number of bytes (half read, half written): the rate a row mover can hope for
  comp   what a layer did before, built on the device from the older entries:
           plan         kf_sort of the flattened ids with positions, kf_segment_offsets, kf_index_put of arange for the inverse
           dispatch     kf_index_get(x, token)                                (token = position // k, prepared outside the timed span)
           combine      ys * gate (kf_elementwise), k x kf_index_get by a column of the inverse, k - 1 x kf_elementwise add
           combine_bwd  zero + k x kf_index_add (each a stable sort of T indices plus run sums) for d(ys gate), then * gate for dys, and
                        * ys with a kf_reduce over the row for dgate
         (the contiguous index columns the gathers need are prepared outside the timed span, in the composition's favour)
Algorithmic bytes: dispatch (T + T k) d, combine (T k + T) d, combine_bwd (T + 2 T k) d elements of 2 bytes; the plan is reported in time only.
--check compares the plan with numpy and sampled tokens of the three row movers with f64 numpy on the rounded inputs before timing.
Prints one JSON object; --json saves it (default profiles/r06_moe_route_bench.json), stamped with moe.hip's content hash."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from tests import gemm_views as V  # noqa: E402
from tests import moe_ref as M  # noqa: E402

SOURCES = ("moe.hip", "float_pack.h", "common.h", "sort.hip")
BF, ES = H.BF16, 2
BLOCK = 1 << 22   # elements of the repeated random block the row operands are filled with: element i holds block[(i + phase) % BLOCK]
CHUNK_BYTES = 1 << 30   # the older entries index 32 bits: the composition walks its rows in pieces of at most this many bytes
# (label, T, k, E, d)
SHAPES = [("mixtral", 32768, 2, 8, 4096), ("qwen3-moe", 32768, 8, 128, 2048), ("k8 e256 d7168", 32768, 8, 256, 7168)]
DISTS = ("balanced", "zipf")


def draw_ids(rng, dist, T, k, E):
    """k distinct experts per token, uniformly or with Zipf weights (Gumbel top-k)."""
    w = np.ones(E) if dist == "balanced" else 1.0 / np.arange(1, E + 1)
    score = np.log(w)[None, :] + rng.gumbel(size=(T, E))
    return np.ascontiguousarray(np.argsort(-score, axis=1)[:, :k]).astype(np.int64)


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


class Filled:
    """A device buffer of n bf16 elements holding block[(i + phase) % BLOCK]."""

    def __init__(self, n, block, phase):
        self.block, self.phase = block, phase
        self.buf = H.DevBuf(n * ES)
        rolled = np.ascontiguousarray(np.roll(block, -phase))
        for at in range(0, n, BLOCK):
            H.check(H.lib().kf_memcpy_h2d(self.buf.ptr + at * ES, rolled.ctypes.data, min(BLOCK, n - at) * ES, None))
        self.ptr = self.buf.ptr

    def rows(self, r, d):
        """f64 values of the rows r of a [*, d] operand."""
        idx = np.asarray(r, dtype=np.int64)[:, None] * d + np.arange(d)[None, :]
        return V.decode(self.block[(idx + self.phase) % BLOCK], "bf16")


def read_rows(ptr, r, d):
    out = np.empty((len(r), d), dtype=np.uint16)
    for i, row in enumerate(r):
        H.check(H.lib().kf_memcpy_d2h(out[i].ctypes.data, ptr + int(row) * d * ES, d * ES, None))
    return V.decode(out, "bf16")


def bench_case(shape, dist, args):
    label, T, k, E, d = shape
    n = T * k
    rng = np.random.default_rng(E + d + len(dist))
    block = V.encode(rng.uniform(-1, 1, BLOCK), "bf16")
    ids_h = draw_ids(rng, dist, T, k, E)
    gate_h = M.rnd(rng.uniform(0.05, 1.0, (T, k)), "bf16")
    ids = H.DevBuf.from_numpy(ids_h)
    gate = H.DevBuf.from_numpy(V.encode(gate_h, "bf16"))
    x, ys, dy = Filled(T * d, block, 0), Filled(n * d, block, 4321), Filled(T * d, block, 99)
    xs, y, dys, dgate = H.DevBuf(n * d * ES), H.DevBuf(T * d * ES), H.DevBuf(n * d * ES), H.DevBuf(n * ES)
    offsets, row_pair, pair_row = H.DevBuf(8 * (E + 1)), H.DevBuf(4 * n), H.DevBuf(4 * n)
    ws_bytes = H.moe_plan_workspace_bytes(T, k, E)
    ws = H.DevBuf(ws_bytes)
    n_valid = offsets.ptr + 8 * E
    copy_src, copy_dst = ys.buf, dys     # the largest operands: every copy below fits them

    moe = {
        "plan": lambda: H.moe_plan(ids.ptr, T, k, E, offsets.ptr, row_pair.ptr, pair_row.ptr, ws.ptr, ws_bytes),
        "dispatch": lambda: H.moe_dispatch(BF, T, k, d, row_pair.ptr, x.ptr, d, xs.ptr, d),
        "combine": lambda: H.moe_combine(BF, T, k, d, pair_row.ptr, n_valid, gate.ptr, k, ys.ptr, d, y.ptr, d),
        "combine_bwd": lambda: H.moe_combine_bwd(BF, T, k, d, pair_row.ptr, n_valid, gate.ptr, k, ys.ptr, d, dy.ptr, d, dys.ptr, d, dgate.ptr, k),
    }
    elems = {"dispatch": (T + n) * d, "combine": (n + T) * d, "combine_bwd": (T + 2 * n) * d}

    def copy(op):
        half = elems[op] * ES // 2
        at = 0
        while at < half:   # pieces that fit the operands; together the same bytes
            m = min(half - at, n * d * ES)
            H.check(H.lib().kf_memcpy_d2d(copy_dst.ptr, copy_src.ptr, m, None))
            at += m

    # ---- the composition, from the older entries --------------------------------------------------------------------------------------------
    moe["plan"]()
    H.device_sync()
    rp_h, pr_h = row_pair.to_numpy(n, np.int32), pair_row.to_numpy(n, np.int32)
    token = H.DevBuf.from_numpy((rp_h.astype(np.int64) // k))
    inv_cols = [H.DevBuf.from_numpy(np.ascontiguousarray(pr_h.reshape(T, k)[:, j].astype(np.int64))) for j in range(k)]
    gate_rows = H.DevBuf.from_numpy(V.encode(gate_h.reshape(-1)[rp_h], "bf16"))      # the gate of every sorted row (the old layer's embedding of p)
    arange = H.DevBuf.from_numpy(np.arange(n, dtype=np.int64))
    keys, pos, inv = H.DevBuf(8 * n), H.DevBuf(8 * n), H.DevBuf(8 * n)
    sort_bytes = H.lib().kf_sort_workspace_bytes(H.I64, 1, n)
    sort_ws = H.DevBuf(max(sort_bytes, 16))
    add_bytes = H.lib().kf_index_add_workspace_bytes(T)
    add_ws = H.DevBuf(max(add_bytes, 16))
    yg, tmp, dgate_rows = H.DevBuf(n * d * ES), H.DevBuf(T * d * ES), H.DevBuf(n * ES)
    rows_per = max(1, CHUNK_BYTES // (d * ES))

    def pieces(rows):
        return [(r0, min(rows_per, rows - r0)) for r0 in range(0, rows, rows_per)]

    def ew(op, out, a, b, rows, b_is_column):
        """out = a op b over [rows, d] in pieces; b is [rows, d], or [rows, 1] broadcast along the row."""
        for r0, m in pieces(rows):
            vo = H.View(out + r0 * d * ES, (m, d), (d, 1), BF)
            va = H.View(a + r0 * d * ES, (m, d), (d, 1), BF)
            vb = H.View(b + r0 * ES, (m, 1), (1, 0), BF) if b_is_column else H.View(b + r0 * d * ES, (m, d), (d, 1), BF)
            H.elementwise(op, H.make_desc([vo], [va, vb]))

    def comp_plan():
        H.check(H.lib().kf_sort(H.I64, ids.ptr, keys.ptr, pos.ptr, 1, n, 0, sort_ws.ptr if sort_bytes else None, sort_bytes, None))
        H.segment_offsets(keys.ptr, n, E, offsets.ptr)
        sv = H.View(inv.ptr, (n,), (0,), H.I64)
        desc = H.make_desc([sv], [H.View(arange.ptr, (n,), (1,), H.I64), H.View(pos.ptr, (n,), (1,), H.I64)])
        H.index_put(desc, [n], [8])

    def comp_dispatch():
        for r0, m in pieces(n):
            H.index_get(x.ptr, T, d * ES, token.ptr + 8 * r0, m, xs.ptr + r0 * d * ES)

    def comp_combine():
        ew(H.EW_MUL, yg.ptr, ys.ptr, gate_rows.ptr, n, True)
        for j in range(k):
            for r0, m in pieces(T):
                H.index_get(yg.ptr, n, d * ES, inv_cols[j].ptr + 8 * r0, m, (y.ptr if j == 0 else tmp.ptr) + r0 * d * ES)
            if j:
                ew(H.EW_ADD, y.ptr, y.ptr, tmp.ptr, T, False)

    def comp_combine_bwd():
        H.check(H.lib().kf_memset_zero(yg.ptr, n * d * ES, None))
        for j in range(k):     # d(ys gate)[inv[t, j]] = dy[t]: the embedding's backward, one sort of T indices each
            H.check(H.lib().kf_index_add(BF, inv_cols[j].ptr, T, dy.ptr, d, n, yg.ptr, add_ws.ptr if add_bytes else None, add_bytes, None))
        ew(H.EW_MUL, dys.ptr, yg.ptr, gate_rows.ptr, n, True)
        ew(H.EW_MUL, yg.ptr, yg.ptr, ys.ptr, n, False)
        for r0, m in pieces(n):
            vi = H.View(yg.ptr + r0 * d * ES, (m, d), (d, 1), BF)
            vo = H.View(dgate_rows.ptr + r0 * ES, (m, 1), (1, 1), BF)
            desc = H.make_reduce_desc(vo, vi, 1)
            need = C.c_size_t(0)
            H.check(H.lib().kf_reduce_workspace_bytes(C.byref(desc), C.byref(need)))
            assert need.value <= red_ws.nbytes, need.value
            H.check(H.lib().kf_reduce(H.RED_SUM, C.byref(desc), red_ws.ptr if need.value else None, need.value, None))

    red_ws = H.DevBuf(1 << 26)
    comp = {"plan": comp_plan, "dispatch": comp_dispatch, "combine": comp_combine, "combine_bwd": comp_combine_bwd}

    # ---- --check: the plan in full, the row movers on sampled tokens ------------------------------------------------------------------------
    checks = []
    if args.check:
        for fn in moe.values():
            fn()
        H.device_sync()
        off_ref, rp_ref, pr_ref = M.plan(ids_h, E)
        ok = (np.array_equal(offsets.to_numpy(E + 1, np.int64), off_ref) and np.array_equal(row_pair.to_numpy(n, np.int32), rp_ref) and
              np.array_equal(pair_row.to_numpy(n, np.int32), pr_ref))
        checks.append({"what": "plan", "worst_error_over_tolerance": 0.0 if ok else float("inf"), "ok": bool(ok)})
        ts = np.unique(np.random.default_rng(3).integers(0, T, 6))
        pr = pr_ref.reshape(T, k).astype(np.int64)
        rows = pr[ts].reshape(-1)
        g = gate_h[ts]
        ys_r = ys.rows(rows, d).reshape(len(ts), k, d)
        dy_r = dy.rows(ts, d)
        # dispatch: bit for bit
        got = read_rows(xs.ptr, rows, d).reshape(len(ts), k, d)
        worst = 0.0 if np.array_equal(got, np.repeat(x.rows(ts, d)[:, None, :], k, 1)) else float("inf")
        checks.append({"what": "dispatch", "worst_error_over_tolerance": worst, "ok": worst <= 1.0})
        # combine: 2^-8 |ref| for the store, k 2^-23 sum |g ys| for the f32 sum
        ref, mag = (g[:, :, None] * ys_r).sum(1), np.abs(g[:, :, None] * ys_r).sum(1)
        tol = 2.0 ** -8 * np.abs(ref) + k * 2.0 ** -23 * mag + 1e-300
        worst = float((np.abs(read_rows(y.ptr, ts, d) - ref) / tol).max())
        checks.append({"what": "combine", "worst_error_over_tolerance": worst, "ok": worst <= 1.0})
        # combine_bwd: dys one rounding of an exact product; dgate 2^-8 |ref| + d 2^-23 sum |dy ys|
        ref = g[:, :, None] * dy_r[:, None, :]
        worst = float((np.abs(read_rows(dys.ptr, rows, d).reshape(len(ts), k, d) - ref) / (2.0 ** -8 * np.abs(ref) + 1e-300)).max())
        dref, dmag = (dy_r[:, None, :] * ys_r).sum(2), np.abs(dy_r[:, None, :] * ys_r).sum(2)
        dgot = read_rows(dgate.ptr, ts, k)
        worst = max(worst, float((np.abs(dgot - dref) / (2.0 ** -8 * np.abs(dref) + d * 2.0 ** -23 * dmag)).max()))
        checks.append({"what": "combine_bwd", "worst_error_over_tolerance": worst, "ok": worst <= 1.0})

    res = {"shape": label, "T": T, "k": k, "E": E, "d": d, "dist": dist, "largest_expert": int(np.bincount(ids_h.reshape(-1), minlength=E).max()),
           "smallest_expert": int(np.bincount(ids_h.reshape(-1), minlength=E).min()), "ops": {}}
    for op in ("plan", "dispatch", "combine", "combine_bwd"):
        runs = {"moe": moe[op], "comp": comp[op]}
        if op != "plan":
            runs["copy"] = lambda op=op: copy(op)
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        H.device_sync()
        ms = {name: [] for name in runs}
        names = list(runs)
        for i in range(args.iters):   # interleaved: drift of the clock or of the neighbours' load hits all alike; the order rotates, so
            for j in range(len(names)):   # that each follows each (what the one before left in the Infinity Cache differs)
                name = names[(i + j) % len(names)]
                ms[name].append(event_ms(runs[name]))
        med = {name: statistics.median(v) for name, v in ms.items()}
        out = {"moe_ms": med["moe"], "comp_ms": med["comp"], "moe_over_comp": med["moe"] / med["comp"], "spread_moe_ms": [min(ms["moe"]), max(ms["moe"])]}
        if op != "plan":
            nbytes = elems[op] * ES
            out.update({"bytes": nbytes, "copy_ms": med["copy"], "moe_TBs": nbytes / med["moe"] / 1e9, "copy_TBs": nbytes / med["copy"] / 1e9,
                        "moe_fraction_of_copy_rate": med["copy"] / med["moe"]})
        res["ops"][op] = out
    moe["plan"]()   # the composition's plan rewrote offsets with the same values; leave the tables as the entry builds them
    H.device_sync()
    if checks:
        res["check"] = checks
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="compare the plan and sampled tokens with numpy before timing")
    ap.add_argument("--only", default="", help="run the shapes whose label contains this text")
    ap.add_argument("--dist", default="", help="run the distributions whose name contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_moe_route_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("moe_route_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"tool": "tools/moe_route_bench.py", "dtype": "bf16", "iters": args.iters, "warmup": args.warmup, "cases": []}
    for shape in SHAPES:
        for dist in DISTS:
            if args.only in shape[0] and args.dist in dist:
                out["cases"].append(bench_case(shape, dist, args))
    out.update(bench.stamp(SOURCES))
    bad = [c for c in out["cases"] for chk in c.get("check", []) if not chk["ok"]]
    print(json.dumps(out))
    if bad:
        raise SystemExit("moe_route_bench --check: an output is outside its bound of the f64 reference")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
