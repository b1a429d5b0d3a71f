#!/usr/bin/env python3
"""Segmented expert GEMM (kf_gemm_segmented, kf_gemm_segmented_wgrad) against a dense product and against the per-expert route, C ABI.

Shapes (bf16): Mixtral-like E 8, 4096 -> 14336 and 14336 -> 4096 on 65536 rows; Qwen3-MoE-like E 128, 2048 -> 768 and back on 262144
rows; E 32, 7168 -> 2048 on 65536 rows. Each with balanced experts, Zipf-skewed experts, and a quarter of the experts empty; each timed
forward (y = x W_e), dX (dy W_e^T) and wgrad (x^T dy per expert). Per case, interleaved in one loop, median of --iters HIP-event times:
  seg    the segmented entry (its plan kernel included), offsets on the device
  dense  (a) ONE kf_gemm of the same rows through a single weight: the ceiling - no segment can be faster than no segments
  loop   (b) the only route without this entry: the offsets copied to the host (a synchronisation), then one kf_gemm per expert with
         its workspace; the copy and the wait are inside the timed span
and: the 128 x 128 x 64 tiles the segmented kernel executes (partial row tiles of short segments count whole; for wgrad, partial K
tiles) over the tiles of the dense product, and the time per executed tile of seg against dense. --check compares sampled outputs
of all three entries with f64 numpy on the rounded inputs within 2^-8 |ref| + K 2^-23 sum |a b| before timing.
Prints one JSON object; --json saves it (default profiles/r06_expert_gemm_bench.json), stamped with gemm_seg.hip's content hash."""
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
from tests import gemm_views as V  # noqa: E402

SOURCES = ("gemm_seg.hip", "gemm.hip", "common.h")
BF, ES = H.BF16, 2
BLOCK = 1 << 22   # elements of the repeated random block every operand is filled with: element i holds block[i % BLOCK]
# (label, E, rows, Din, Dout)
SHAPES = [("mixtral up", 8, 65536, 4096, 14336), ("mixtral down", 8, 65536, 14336, 4096), ("qwen3-moe up", 128, 262144, 2048, 768),
          ("qwen3-moe down", 128, 262144, 768, 2048), ("e32", 32, 65536, 7168, 2048)]
DISTS = ("balanced", "zipf", "quarter-empty")


def counts(dist, T, E):
    if dist == "balanced":
        w = np.ones(E)
    elif dist == "zipf":
        w = 1.0 / np.arange(1, E + 1)
    else:
        w = np.array([0.0 if e % 4 == 3 else 1.0 for e in range(E)])
    c = np.floor(w / w.sum() * T).astype(np.int64)
    c[0] += T - c.sum()
    return c


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
        self.n, self.block, self.phase = n, block, phase
        self.buf = H.DevBuf(n * ES)
        rolled = np.ascontiguousarray(np.roll(block, -phase))
        for at in range(0, n, BLOCK):
            m = min(BLOCK, n - at)
            H.check(H.lib().kf_memcpy_h2d(self.buf.ptr + at * ES, rolled.ctypes.data, m * ES, None))
        self.ptr = self.buf.ptr

    def at(self, idx):
        """f64 values of the elements at flat indices idx."""
        return V.decode(self.block[(np.asarray(idx, dtype=np.int64) + self.phase) % BLOCK], "bf16")


def read(ptr, idx):
    """f64 values of single bf16 elements of a device buffer (flat indices)."""
    out = np.empty(len(idx), dtype=np.uint16)
    one = np.empty(1, dtype=np.uint16)
    for i, j in enumerate(idx):
        H.check(H.lib().kf_memcpy_d2h(one.ctypes.data, ptr + int(j) * ES, ES, None))
        out[i] = one[0]
    return V.decode(out, "bf16")


def bench_shape(shape, dist, args):
    label, E, T, Din, Dout = shape
    rng = np.random.default_rng(E + Din)
    block = V.encode(rng.uniform(-1, 1, BLOCK), "bf16")
    cnt = counts(dist, T, E)
    off_h = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    off = H.DevBuf.from_numpy(off_h)
    x, dy, w = Filled(T * Din, block, 0), Filled(T * Dout, block, 12345), Filled(E * Din * Dout, block, 777)
    y, dx, dw = H.DevBuf(T * Dout * ES), H.DevBuf(T * Din * ES), H.DevBuf(E * Din * Dout * ES)
    ws_bytes = H.gemm_segmented_workspace_bytes(BF, T, E)
    ws = H.DevBuf(ws_bytes)
    # (ta, tb, M, N, K) of the dense / per-expert kf_gemm for `rows` rows
    geo = {"fwd": lambda rows: (0, 0, rows, Dout, Din), "dx": lambda rows: (0, 1, rows, Din, Dout), "wgrad": lambda rows: (1, 0, Din, Dout, rows)}
    need = max(H.gemm_workspace_bytes(BF, *geo[op](rows)) for op in geo for rows in {T} | {int(c) for c in cnt if c})
    gws = H.DevBuf(max(need, 16))
    host_off = np.empty(E + 1, dtype=np.int64)

    def gemm(op, rows, r0, e):
        ta, tb, M, N, K = geo[op](rows)
        if op == "fwd":
            a, lda, b, ldb, c, ldc = x.ptr + r0 * Din * ES, Din, w.ptr + e * Din * Dout * ES, Dout, y.ptr + r0 * Dout * ES, Dout
        elif op == "dx":
            a, lda, b, ldb, c, ldc = dy.ptr + r0 * Dout * ES, Dout, w.ptr + e * Din * Dout * ES, Dout, dx.ptr + r0 * Din * ES, Din
        else:
            a, lda, b, ldb, c, ldc = x.ptr + r0 * Din * ES, Din, dy.ptr + r0 * Dout * ES, Dout, dw.ptr + e * Din * Dout * ES, Dout
        H.gemm(BF, ta, tb, M, N, K, 1.0, a, lda, b, ldb, 0.0, c, ldc, H.EPI_NONE, None, gws.ptr, gws.nbytes)

    def seg(op):
        if op == "fwd":
            H.gemm_segmented(BF, 0, T, Dout, Din, E, off.ptr, 1.0, x.ptr, Din, w.ptr, Dout, Din * Dout, 0.0, y.ptr, Dout, ws.ptr, ws_bytes)
        elif op == "dx":
            H.gemm_segmented(BF, 1, T, Din, Dout, E, off.ptr, 1.0, dy.ptr, Dout, w.ptr, Dout, Din * Dout, 0.0, dx.ptr, Din, ws.ptr, ws_bytes)
        else:
            H.gemm_segmented_wgrad(BF, T, Din, Dout, E, off.ptr, 1.0, x.ptr, Din, dy.ptr, Dout, 0.0, dw.ptr, Dout, Din * Dout, ws.ptr, ws_bytes)

    def loop(op):
        H.check(H.lib().kf_memcpy_d2h(host_off.ctypes.data, off.ptr, host_off.nbytes, None))   # the counts to the host: a synchronisation
        for e in range(E):
            lo, hi = int(host_off[e]), int(host_off[e + 1])
            if hi > lo:
                gemm(op, hi - lo, lo, e)
            elif op == "wgrad":
                H.check(H.lib().kf_memset_zero(dw.ptr + e * Din * Dout * ES, Din * Dout * ES, None))

    def sample_check(op, who):
        """Sampled outputs against f64 numpy on the rounded inputs."""
        srng = np.random.default_rng(5)
        worst = 0.0
        live = [e for e in range(E) if cnt[e]]
        for e in (live[0], live[len(live) // 2], live[-1]):
            lo, hi = int(off_h[e]), int(off_h[e + 1])
            if op == "wgrad":
                m, n = srng.integers(0, Din, 6), srng.integers(0, Dout, 6)
                rows = np.arange(lo, hi)
                a, b = x.at(rows[:, None] * Din + m[None, :]), dy.at(rows[:, None] * Dout + n[None, :])
                ref, absref, K = (a * b).sum(0), np.abs(a * b).sum(0), hi - lo
                got = read(dw.ptr, e * Din * Dout + m * Dout + n)
            else:
                K, N = (Din, Dout) if op == "fwd" else (Dout, Din)
                r = np.array([lo, (lo + hi) // 2, hi - 1])[:, None]
                n = srng.integers(0, N, 4)[None, :]
                k = np.arange(K)[None, None, :]
                a = (x if op == "fwd" else dy).at(r[:, :, None] * K + k)
                b = w.at(e * Din * Dout + (k * Dout + n[:, :, None] if op == "fwd" else n[:, :, None] * Dout + k))
                ref, absref = (a * b).sum(2).ravel(), np.abs(a * b).sum(2).ravel()
                got = read((y if op == "fwd" else dx).ptr, (r * N + n).ravel())
            tol = 2.0 ** -8 * np.abs(ref) + K * 2.0 ** -23 * absref
            worst = max(worst, float((np.abs(got - ref) / tol).max()))
        return {"who": who, "worst_error_over_tolerance": worst, "ok": worst <= 1.0}

    cases = []
    for op in ("fwd", "dx", "wgrad"):
        runs = {"seg": lambda op=op: seg(op), "dense": lambda op=op: gemm(op, T, 0, 0), "loop": lambda op=op: loop(op)}
        checks = []
        if args.check:
            for who in ("loop", "seg"):   # seg last: the sampled buffers are re-read after each
                runs[who]()
                H.device_sync()
                checks.append(sample_check(op, who))
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        H.device_sync()
        ms = {k: [] for k in runs}
        for _ in range(args.iters):   # interleaved: drift of the clock or of the neighbours' load hits all three alike
            for k, fn in runs.items():
                ms[k].append(event_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        flops = 2.0 * T * Din * Dout
        if op == "wgrad":
            tiles = int(sum(-(-int(c) // 64) for c in cnt)) * (Din // 128) * (Dout // 128)
            dense_tiles = (T // 64) * (Din // 128) * (Dout // 128)
        else:
            N, K = (Dout, Din) if op == "fwd" else (Din, Dout)
            tiles = int(sum(-(-int(c) // 128) for c in cnt)) * (N // 128) * (K // 64)
            dense_tiles = (T // 128) * (N // 128) * (K // 64)
        res = {"shape": label, "E": E, "rows": T, "Din": Din, "Dout": Dout, "dist": dist, "op": op, "largest_expert": int(cnt.max()),
               "smallest_nonempty_expert": int(cnt[cnt > 0].min()), "empty_experts": int((cnt == 0).sum()),
               "seg_ms": med["seg"], "dense_ms": med["dense"], "loop_ms": med["loop"], "seg_TFLOPs": flops / med["seg"] / 1e9,
               "dense_TFLOPs": flops / med["dense"] / 1e9, "loop_TFLOPs": flops / med["loop"] / 1e9, "seg_over_dense": med["seg"] / med["dense"],
               "seg_over_loop": med["seg"] / med["loop"], "executed_tiles": tiles, "dense_tiles": dense_tiles,
               "tiles_over_dense": tiles / dense_tiles, "seg_ns_per_tile": med["seg"] * 1e6 / tiles, "dense_ns_per_tile": med["dense"] * 1e6 / dense_tiles,
               "spread_seg_ms": [min(ms["seg"]), max(ms["seg"])]}
        if checks:
            res["check"] = checks
        cases.append(res)
        print(json.dumps(res), file=sys.stderr, flush=True)
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true", help="compare sampled outputs with f64 numpy before timing")
    ap.add_argument("--only", default="", help="run the shapes whose label contains this text")
    ap.add_argument("--dist", default="", help="run the distributions whose name contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_expert_gemm_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("expert_gemm_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"tool": "tools/expert_gemm_bench.py", "dtype": "bf16", "iters": args.iters, "warmup": args.warmup, "cases": []}
    for shape in SHAPES:
        for dist in DISTS:
            if args.only in shape[0] and args.dist in dist:
                out["cases"] += bench_shape(shape, dist, args)
    out.update(bench.stamp(SOURCES))
    bad = [c for c in out["cases"] for k in c.get("check", []) if not k["ok"]]
    print(json.dumps(out))
    if bad:
        raise SystemExit("expert_gemm_bench --check: a sampled output is outside 2^-8 |ref| + K 2^-23 sum |a b| of the f64 reference")
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
