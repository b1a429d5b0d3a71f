#!/usr/bin/env python3
"""The symmetric product and the Muon step built on it (kf_gemm_sym, kf_muon_prepare, kf_muon_apply, kfunca.Muon) beside the same work
composed from kf_gemm calls, at the bf16 weight shapes (4096, 4096), (4096, 14336), (14336, 4096) and (2048, 768).

  sym     kf_gemm_sym beside the kf_gemm (NT) of the same product, for both symmetric products of an iteration: X X^T (M = m, K = n) and
          A A (M = K = m), m = min(rows, cols), n = max(rows, cols). kf_gemm is timed TWICE (gemm_a, gemm_b): the distance between its two
          medians is the box's spread, the yardstick for the difference. Median event times, the three calls interleaved in one process in
          an order that rotates every round; uniform random operands.
  ns      five Newton-Schulz steps as kfunca.newton_schulz runs them (`new`: per step kf_gemm NT for A, kf_gemm_sym with D = A and gamma,
          kf_gemm) and with A on kf_gemm_sym too (`all_sym`), beside the composition a user could write before: kf_gemm NT, a copy of A,
          kf_gemm with beta, a copy of X, kf_gemm with beta.
  step    kfunca.Muon.step() over the four weights beside kf_muon_prepare + that composition + kf_muon_apply per weight: wall-clock
          medians between two device synchronisations.
  --check sampled rows of every timed kf_gemm_sym against the f64 product of the operand rows read back, within tests/test_gpu_gemm_sym.py's
          bound; the Newton-Schulz result of (2048, 768) against the f64 iteration (e <= 0.03 and <= 1.5 times the composition's e); at
          the larger shapes sampled rows of the two routes against each other, within 0.06 of their norm (two results each within 0.03
          of the f64 iteration).
Prints one JSON object; --json saves it (default profiles/r06_muon_bench.json), stamped with the content hashes of gemm_sym.hip and
muon.hip."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
import kfunca_amd as kfunca  # noqa: E402
from kfunca_amd import hip_abi as H  # noqa: E402
from tests import gemm_views as V  # noqa: E402
from tools.gemm_fp8_bench import bf16_seed, event_ms, fill, read, rotate_times  # noqa: E402

SOURCES = ("gemm_sym.hip", "muon.hip")
SHAPES = [(4096, 4096), (4096, 14336), (14336, 4096), (2048, 768)]
A, B, C = 3.4445, -4.7750, 2.0315


def copy(dst, src, nbytes):
    H.check(H.lib().kf_memcpy_d2d(dst, src, nbytes, None))


class Scratch:
    """The matrices of one weight's iteration: two X [m, n], A, B [m, m], and kf_gemm's split-K scratch."""

    def __init__(self, m, n, rng):
        self.m, self.n = m, n
        self.x = [H.DevBuf(m * n * 2) for _ in range(2)]
        self.a, self.b = H.DevBuf(m * m * 2), H.DevBuf(m * m * 2)
        # uniform bf16 values scaled to |X0|_F = 1, as kf_muon_prepare leaves them: the iteration starts inside its basin
        self.x0 = np.ascontiguousarray(V.encode(V.decode(bf16_seed(rng).astype(np.uint16), "bf16") / np.sqrt(m * n / 3.0), "bf16"))
        need = max(H.gemm_workspace_bytes(H.BF16, 0, tb, m, N, K) for tb, N, K in ((1, m, n), (0, m, m), (0, n, m)))
        self.ws, self.ws_bytes = (H.DevBuf(need) if need else None), need

    def reset(self):
        fill(self.x[0].ptr, self.m * self.n * 2, self.x0)

    def gemm(self, tb, N, K, alpha, a, lda, b, ldb, beta, c):
        H.gemm(H.BF16, 0, tb, self.m, N, K, alpha, a, lda, b, ldb, beta, c, N, workspace=self.ws.ptr if self.ws else None, workspace_bytes=self.ws_bytes)

    def ns_new(self, steps=5, all_sym=False):
        m, n, cur = self.m, self.n, 0
        for _ in range(steps):
            if all_sym:
                H.gemm_sym(H.BF16, m, n, 1.0, self.x[cur].ptr, n, self.a.ptr, m)
            else:
                self.gemm(1, m, n, 1.0, self.x[cur].ptr, n, self.x[cur].ptr, n, 0.0, self.a.ptr)
            H.gemm_sym(H.BF16, m, m, C, self.a.ptr, m, self.b.ptr, m, beta=B, D=self.a.ptr, ldd=m, gamma=A)
            self.gemm(0, n, m, 1.0, self.b.ptr, m, self.x[cur].ptr, n, 0.0, self.x[cur ^ 1].ptr)
            cur ^= 1
        return cur

    def ns_composed(self, steps=5):
        m, n, cur = self.m, self.n, 0
        for _ in range(steps):
            self.gemm(1, m, n, 1.0, self.x[cur].ptr, n, self.x[cur].ptr, n, 0.0, self.a.ptr)
            copy(self.b.ptr, self.a.ptr, m * m * 2)
            self.gemm(0, m, m, C, self.a.ptr, m, self.a.ptr, m, B, self.b.ptr)
            copy(self.x[cur ^ 1].ptr, self.x[cur].ptr, m * n * 2)
            self.gemm(0, n, m, 1.0, self.b.ptr, m, self.x[cur].ptr, n, A, self.x[cur ^ 1].ptr)
            cur ^= 1
        return cur


def rows_of(ptr, rows, ld, count):
    return np.stack([V.decode(read(ptr + int(r) * ld * 2, count, np.uint16), "bf16") for r in rows])


def check_sym(s, K, xptr, pick):
    """Sampled rows of C = X X^T in s.a against f64, as a fraction of the bound r |ref| + K 2^-23 absref."""
    m = s.m
    rows = np.r_[0, m - 1, pick.choice(m, 6, replace=False)]
    X = V.decode(read(xptr, m * K, np.uint16), "bf16").reshape(m, K)
    ref, absref = X[rows] @ X.T, np.abs(X[rows]) @ np.abs(X).T
    got = rows_of(s.a.ptr, rows, m, m)
    return float((np.abs(got - ref) / (2.0 ** -8 * np.abs(ref) + K * 2.0 ** -23 * absref + 1e-300)).max())


def bench_sym(shape, s, args):
    m, n = s.m, s.n
    out = {"rows": shape[0], "cols": shape[1], "m": m, "n": n}
    s.reset()
    for name, K, x in (("XXt", n, s.x[0]), ("AA", m, s.b)):
        if name == "AA":
            copy(s.b.ptr, s.x[0].ptr, m * m * 2)     # any [m, m] bf16 operand of the iteration's magnitude
        calls = {"sym": lambda: H.gemm_sym(H.BF16, m, K, 1.0, x.ptr, K, s.a.ptr, m),
                 "gemm_a": lambda: s.gemm(1, m, K, 1.0, x.ptr, K, x.ptr, K, 0.0, s.a.ptr)}
        calls["gemm_b"] = calls["gemm_a"]
        res = {}
        if args.check:
            calls["sym"]()
            H.device_sync()
            frac = check_sym(s, K, x.ptr, np.random.default_rng(m + K))
            res["check"] = {"worst_fraction_of_bound": frac, "ok": bool(frac <= 1.0)}
        t = rotate_times(calls, args.iters, args.warmup, event_ms)
        g = min(t["gemm_a"]["median"], t["gemm_b"]["median"])
        res.update({"K": K, "time_ms": t, "gemm_spread_ms": abs(t["gemm_a"]["median"] - t["gemm_b"]["median"]), "sym_speed_over_gemm": g / t["sym"]["median"],
                    "gemm_TFLOPs": 2.0 * m * m * K / g / 1e9, "sym_TFLOPs_of_the_full_product": 2.0 * m * m * K / t["sym"]["median"] / 1e9})
        out[name] = res
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def ns64(X, steps=5):
    for _ in range(steps):
        G = X @ X.T
        X = A * X + (B * G + C * G @ G) @ X
    return X


def bench_ns(shape, s, args):
    m, n = s.m, s.n
    out = {"rows": shape[0], "cols": shape[1]}
    if args.check:
        s.reset()
        H.device_sync()
        pick = np.r_[0, m - 1, np.random.default_rng(m).choice(m, 14, replace=False)] if m * n > 1 << 22 else np.arange(m)
        X0 = V.decode(read(s.x[0].ptr, m * n, np.uint16), "bf16").reshape(m, n) if len(pick) == m else None
        got = {}
        for name, fn in (("new", s.ns_new), ("all_sym", lambda: s.ns_new(all_sym=True)), ("composed", s.ns_composed)):
            s.reset()
            cur = fn()
            H.device_sync()
            got[name] = rows_of(s.x[cur].ptr, pick, n, n)
        if X0 is not None:
            Y = ns64(X0)
            e = {k: float(np.linalg.norm(v - Y) / np.linalg.norm(Y)) for k, v in got.items()}
            out["check"] = {"e_new": e["new"], "e_all_sym": e["all_sym"], "e_composed": e["composed"],
                            "ok": bool(max(e["new"], e["all_sym"]) <= min(0.03, 1.5 * e["composed"]))}
        else:
            d = {k: float(np.linalg.norm(got[k] - got["composed"]) / np.linalg.norm(got["composed"])) for k in ("new", "all_sym")}
            out["check"] = {"sampled_rows": int(len(pick)), "new_vs_composed": d["new"], "all_sym_vs_composed": d["all_sym"], "ok": bool(max(d.values()) <= 0.06)}

    s.reset()   # once: five steps leave a matrix of singular values near 1 in x[1], and the next five run on x[0], which holds step four's
    t = rotate_times({"new": s.ns_new, "all_sym": lambda: s.ns_new(all_sym=True), "composed_a": s.ns_composed, "composed_b": s.ns_composed}, args.iters,
                     args.warmup, event_ms)
    c = min(t["composed_a"]["median"], t["composed_b"]["median"])
    out.update({"time_ms": t, "composed_spread_ms": abs(t["composed_a"]["median"] - t["composed_b"]["median"]), "new_speed_over_composed": c / t["new"]["median"],
                "all_sym_speed_over_composed": c / t["all_sym"]["median"]})
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def bench_step(scratch, args, rng):
    ps, gs, bufs = [], [], []
    for rows, cols in SHAPES:
        p = kfunca.empty([rows, cols], kfunca.dtype.bfloat16, 0)
        fill(p.data_ptr(), rows * cols * 2, bf16_seed(rng))
        p.set_requires_grad(True)
        one = kfunca.empty([rows, cols], kfunca.dtype.bfloat16, 0)
        fill(one.data_ptr(), rows * cols * 2, bf16_seed(rng))
        (p * one).backward(one)                                   # a dense bf16 grad: both routes read this one tensor
        ps.append(p), gs.append(p.grad())
        bufs.append((H.DevBuf(rows * cols * 4), H.DevBuf(rows * cols * 4)))   # the composition's momentum and master
        bufs[-1][0].zero(), bufs[-1][1].zero()
    opt = kfunca.Muon(ps, lr=0.02)
    lr = H.DevBuf.from_numpy(np.float32([0.02]))
    ws = H.DevBuf(H.muon_prepare_workspace_bytes(1, 1))

    def composed():
        for (rows, cols), p, g, (mom, master), s in zip(SHAPES, ps, gs, bufs, scratch):
            H.muon_prepare(H.BF16, rows, cols, g.data_ptr(), mom.ptr, 0.95, 1, s.x[0].ptr, s.m, s.n, s.n, workspace=ws.ptr, workspace_bytes=ws.nbytes)
            cur = s.ns_composed()
            H.muon_apply(H.BF16, rows, cols, p.data_ptr(), master.ptr, s.x[cur].ptr, s.n, lr.ptr, scale=float(np.sqrt(max(1.0, rows / cols))))

    def wall(fn):
        H.device_sync()
        t0 = time.perf_counter()
        fn()
        H.device_sync()
        return 1e3 * (time.perf_counter() - t0)

    t = rotate_times({"Muon.step": opt.step, "composed_a": composed, "composed_b": composed}, args.iters, args.warmup, wall)
    c = min(t["composed_a"]["median"], t["composed_b"]["median"])
    out = {"weights": SHAPES, "time_ms": t, "composed_spread_ms": abs(t["composed_a"]["median"] - t["composed_b"]["median"]),
           "step_speed_over_composed": c / t["Muon.step"]["median"]}
    print(json.dumps(out), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="hold sampled outputs to their bounds")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_muon_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("muon_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    rng = np.random.default_rng(950)
    scratch = [Scratch(min(s), max(s), rng) for s in SHAPES]
    out = {"tool": "tools/muon_bench.py", "iters": args.iters, "warmup": args.warmup, "dtype": "bf16"}
    out["sym"] = [bench_sym(sh, s, args) for sh, s in zip(SHAPES, scratch)]
    out["ns"] = [bench_ns(sh, s, args) for sh, s in zip(SHAPES, scratch)]
    out["step"] = bench_step(scratch, args, rng)
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    checks = [r[k]["check"]["ok"] for r in out["sym"] for k in ("XXt", "AA") if "check" in r[k]] + [r["check"]["ok"] for r in out["ns"] if "check" in r]
    if args.check and not all(checks):
        raise SystemExit("muon_bench --check: an output is outside its bound")


if __name__ == "__main__":
    main()
