#!/usr/bin/env python3
"""The per-tensor scaled FP8 path (kf_gemm_fp8, kf_fp8_amax, kf_fp8_quantize, kfunca.linear_fp8) beside what it stands next to: the
same-shape bf16 kf_gemm, a copy of the quantize kernels' algorithmic bytes, and the bf16 linear layer forward + backward.

  gemm      kf_gemm_fp8 (e4m3 x e4m3, bf16 out) at 4096^3, 8192^3 and T 32768 with (K, N) = (4096, 14336), (14336, 4096), (4096, 6144),
            beside the bf16 kf_gemm of the same shape with B transposed (the same [N, K] weight layout), which is timed TWICE (bf16_a,
            bf16_b): the distance between its two medians is the box's spread, the yardstick for fp8 vs bf16. Median event times, the three
            calls interleaved in one process in an order that rotates every round; uniform random operands.
  quantize  kf_fp8_amax and kf_fp8_quantize without and with the transposed copy at 32768 x 4096 and 32768 x 14336 in bf16, each beside
            a kf_memcpy_d2d that moves the same algorithmic bytes (x read once, q and qt written once).
  linear    kfunca.linear_fp8 forward + backward beside kfunca.gemm forward + backward (bf16) at the gemm shapes: wall-clock medians
            between two device synchronisations, interleaved, the bf16 call timed twice.
  --check   sampled outputs of every timed kf_gemm_fp8 against the f64 product of the operand rows read back from the device, within
            tests/fp8_ref.gemm_bound; and `block_sum`: on the shapes of tests/test_gpu_gemm_fp8.py with random codes over the formats'
            whole range and f32 output, the worst |got - c| / mag per shape - the figure tests/fp8_ref.ACC_TERM is twice the worst of.
Prints one JSON object; --json saves it (default profiles/r06_gemm_fp8_bench.json), stamped with the content hashes of fp8.hip and
gemm_fp8.hip."""
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
from tests import fp8_ref as R  # noqa: E402

SOURCES = ("fp8.hip", "gemm_fp8.hip")
# (label, M, N, K)
GEMM_SHAPES = [("4096^3", 4096, 4096, 4096), ("8192^3", 8192, 8192, 8192), ("T32768 K4096 N14336", 32768, 14336, 4096),
               ("T32768 K14336 N4096", 32768, 4096, 14336), ("T32768 K4096 N6144", 32768, 6144, 4096)]
QUANT_SHAPES = [(32768, 4096), (32768, 14336)]
BLOCK_SUM_SHAPES = [(1, 1, 16), (16, 16, 128), (64, 64, 112), (128, 128, 144), (130, 70, 272), (257, 129, 128), (256, 384, 1024), (512, 512, 4096)]
SEED_BYTES = 8 << 20


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def fill(ptr, nbytes, seed):
    """nbytes of device memory from a host block of random content: the block is uploaded once and doubled on the device."""
    n0 = min(nbytes, seed.nbytes)
    H.check(H.lib().kf_memcpy_h2d(ptr, seed.ctypes.data, n0, None))
    done = n0
    while done < nbytes:
        n = min(done, nbytes - done)
        H.check(H.lib().kf_memcpy_d2d(ptr + done, ptr, n, None))
        H.device_sync()
        done += n


def fp8_seed(rng):
    return (rng.integers(0, 256, SEED_BYTES).astype(np.uint8) & 0xbf)          # e4m3 magnitudes below 2, no NaN


def bf16_seed(rng):
    return O.from_float(rng.uniform(-1, 1, SEED_BYTES // 2).astype(np.float32), O.BF16)


def rotate_times(calls, iters, warmup, timer):
    names = list(calls)
    ms = {n: [] for n in names}
    for it in range(warmup + iters):
        for n in names[it % len(names):] + names[:it % len(names)]:
            dt = timer(calls[n])
            if it >= warmup:
                ms[n].append(dt)
    return {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in ms.items()}


def read(ptr, count, dtype):
    out = np.empty(count, dtype=dtype)
    H.check(H.lib().kf_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None))
    return out


def bench_gemm(shape, args, rng):
    label, M, N, K = shape
    a8, b8, a16, b16 = H.DevBuf(M * K), H.DevBuf(N * K), H.DevBuf(M * K * 2), H.DevBuf(N * K * 2)
    c = H.DevBuf(M * N * 2)
    fill(a8.ptr, M * K, fp8_seed(rng)), fill(b8.ptr, N * K, fp8_seed(rng))
    fill(a16.ptr, M * K * 2, bf16_seed(rng)), fill(b16.ptr, N * K * 2, bf16_seed(rng))
    one = H.DevBuf.from_numpy(np.array([0.5], dtype=np.float32))
    need = H.gemm_workspace_bytes(H.BF16, 0, 1, M, N, K)
    ws = H.DevBuf(need) if need else None

    def fp8():
        H.gemm_fp8(H.FP8_E4M3, H.FP8_E4M3, H.BF16, M, N, K, a8.ptr, K, b8.ptr, K, one.ptr, one.ptr, c.ptr, N)

    def bf16():
        H.gemm(H.BF16, 0, 1, M, N, K, 1.0, a16.ptr, K, b16.ptr, K, 0.0, c.ptr, N, workspace=ws.ptr if ws else None, workspace_bytes=need)

    res = {"label": label, "M": M, "N": N, "K": K}
    if args.check:
        fp8()
        H.device_sync()
        pick = np.random.default_rng(M + N)
        rows, cols = np.r_[0, M - 1, pick.choice(M, 6, replace=False)], np.r_[0, N - 1, pick.choice(N, 62, replace=False)]
        ar = np.stack([read(a8.ptr + int(m) * K, K, np.uint8) for m in rows])
        br = np.stack([read(b8.ptr + int(n) * K, K, np.uint8) for n in cols])
        got = np.stack([R.to_f32(read(c.ptr + int(m) * N * 2, N, np.uint16), "bf16")[cols] for m in rows]).astype(np.float64)
        want, mag = R.product(ar, R.E4M3, br, R.E4M3, 0.5, 0.5)
        frac = R.gemm_frac(got, want, mag, "bf16")
        res["check"] = {"sampled": int(got.size), "worst_fraction_of_bound": frac, "ok": bool(frac <= 1.0)}
    t = rotate_times({"fp8": fp8, "bf16_a": bf16, "bf16_b": bf16}, args.iters, args.warmup, event_ms)
    flop = 2.0 * M * N * K
    bf = min(t["bf16_a"]["median"], t["bf16_b"]["median"])
    res.update({"time_ms": t, "fp8_TFLOPs": flop / t["fp8"]["median"] / 1e9, "bf16_TFLOPs": flop / bf / 1e9,
                "bf16_spread_ms": abs(t["bf16_a"]["median"] - t["bf16_b"]["median"]), "fp8_speed_over_bf16": bf / t["fp8"]["median"]})
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def bench_quantize(rows, cols, args, rng):
    x, q, qt = H.DevBuf(rows * cols * 2), H.DevBuf(rows * cols), H.DevBuf(rows * cols)
    dst = H.DevBuf(rows * cols * 2)                  # the copies' destination: at most 2 n bytes move
    fill(x.ptr, rows * cols * 2, bf16_seed(rng))
    amax, sinv = H.DevBuf(4), H.DevBuf(4)
    n = rows * cols
    calls = {
        "amax": (lambda: H.fp8_amax(H.BF16, rows, cols, cols, x.ptr, amax.ptr), 2 * n),
        "quantize": (lambda: H.fp8_quantize(H.BF16, H.FP8_E4M3, rows, cols, cols, x.ptr, amax.ptr, q.ptr, cols, sinv.ptr), 3 * n),
        "quantize_t": (lambda: H.fp8_quantize(H.BF16, H.FP8_E4M3, rows, cols, cols, x.ptr, amax.ptr, q.ptr, cols, sinv.ptr, qt.ptr, rows), 4 * n),
    }
    res = {"rows": rows, "cols": cols, "dtype": "bf16"}
    calls["amax"][0]()
    for name, (fn, nbytes) in calls.items():
        def copy(nbytes=nbytes):
            H.check(H.lib().kf_memcpy_d2d(dst.ptr, x.ptr, nbytes // 2 // 256 * 256, None))
        t = rotate_times({"kernel": fn, "copy": copy}, max(args.iters, 10), args.warmup, event_ms)
        k, c = t["kernel"]["median"], t["copy"]["median"]
        res[name] = {"bytes": nbytes, "ms": k, "TBps": nbytes / k / 1e9, "copy_ms": c, "copy_TBps": nbytes / c / 1e9, "of_copy": c / k}
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def device_tensor(shape, seed, requires_grad):
    t = kfunca.empty(list(shape), kfunca.dtype.bfloat16, 0)
    fill(t.data_ptr(), int(np.prod(shape)) * 2, seed)
    t.set_requires_grad(requires_grad)
    return t


def bench_linear(shape, args, rng):
    label, T, N, K = shape
    x, w = device_tensor((T, K), bf16_seed(rng), True), device_tensor((N, K), bf16_seed(rng), True)
    wt = device_tensor((K, N), bf16_seed(rng), True)            # the bf16 layer's gemm takes the weight this way
    dy = device_tensor((T, N), bf16_seed(rng), False)

    def run(fn):
        for p in (x, w, wt):
            p.zero_grad()
        kfunca.synchronize(0)
        t0 = time.perf_counter()
        y = fn()
        y.backward(dy)
        kfunca.synchronize(0)
        return 1e3 * (time.perf_counter() - t0)

    fp8, bf16 = (lambda: kfunca.linear_fp8(x, w)), (lambda: kfunca.gemm(x, wt, 1.0, 0.0))
    t = rotate_times({"linear_fp8": fp8, "gemm_a": bf16, "gemm_b": bf16}, args.iters, args.warmup, run)
    bf = min(t["gemm_a"]["median"], t["gemm_b"]["median"])
    res = {"label": label, "T": T, "N": N, "K": K, "time_ms": t, "gemm_spread_ms": abs(t["gemm_a"]["median"] - t["gemm_b"]["median"]),
           "fp8_speed_over_bf16": bf / t["linear_fp8"]["median"]}
    for p in (x, w, wt):
        p.zero_grad()
    del x, w, wt, dy
    kfunca.release_cached(0)
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def block_sum(rng):
    """Worst |got - c| / mag per shape, f32 out, random finite codes over each format's whole range."""
    out = []
    for M, N, K in BLOCK_SUM_SHAPES:
        worst = 0.0
        for fa, fb in ((R.E4M3, R.E4M3), (R.E5M2, R.E5M2), (R.E5M2, R.E4M3), (R.E4M3, R.E5M2)):
            ops = []
            for rows, fmt in ((M, fa), (N, fb)):
                c = rng.integers(0, 256, (rows, K)).astype(np.uint8)
                if fmt == R.E4M3:
                    c[(c & 0x7f) == 0x7f] = 0x35
                else:
                    c &= 0xbf
                ops.append(c)
            want, mag = R.product(ops[0], fa, ops[1], fb)
            ba, bb, bc = H.DevBuf.from_numpy(ops[0]), H.DevBuf.from_numpy(ops[1]), H.DevBuf(M * N * 4)
            one = H.DevBuf.from_numpy(np.ones(1, np.float32))
            H.gemm_fp8(fa, fb, H.F32, M, N, K, ba.ptr, K, bb.ptr, K, one.ptr, one.ptr, bc.ptr, N)
            H.device_sync()
            got = bc.to_numpy((M, N), np.float32).astype(np.float64)
            worst = max(worst, float((np.abs(got - want) / mag).max()))
        out.append({"M": M, "N": N, "K": K, "worst_err_over_mag": worst, "times_1e-6": worst / R.CHECKS_ACC_TERM, "of_ACC_TERM": worst / R.ACC_TERM})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="hold sampled outputs to the f64 reference and record the block-sum figures")
    ap.add_argument("--only", default="", help="run the gemm / linear shapes whose label contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_gemm_fp8_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("gemm_fp8_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    rng = np.random.default_rng(950)
    out = {"tool": "tools/gemm_fp8_bench.py", "iters": args.iters, "warmup": args.warmup, "acc_term": R.ACC_TERM}
    if args.check:
        out["block_sum"] = block_sum(rng)
    out["gemm"] = [bench_gemm(s, args, rng) for s in GEMM_SHAPES if args.only in s[0]]
    out["quantize"] = [bench_quantize(r, c, args, rng) for r, c in QUANT_SHAPES]
    out["linear"] = [bench_linear(s, args, rng) for s in GEMM_SHAPES if args.only in s[0]]
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    if args.json:
        args.json.parent.mkdir(parents=True, exist_ok=True)
        args.json.write_text(json.dumps(out, indent=1) + "\n")
    if args.check and (any(not c["check"]["ok"] for c in out["gemm"]) or any(b["of_ACC_TERM"] > 1.0 for b in out["block_sum"])):
        raise SystemExit("gemm_fp8_bench --check: an output is outside its bound of the f64 reference")


if __name__ == "__main__":
    main()
