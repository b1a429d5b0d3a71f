#!/usr/bin/env python3
"""The fused per-head QK-norm + rotary embedding (kf_qk_norm_rope_fwd / _bwd) against kf_rope, the box's own copy rate and the composition
from today's operators, through the C ABI and the operator API.

For each case the call is timed with HIP events (median of --iters after --warmup), interleaved in the same loop with
  - a kf_memcpy_d2d of the same algorithmic bytes,
  - kf_rope on the same tensor, TWICE (rope_a, rope_b): the two medians of one kernel in one loop are the box's own spread,
  - for the forward cases, the composition a user writes today: split q and k out into contiguous copies, rms_norm each, write them back
    into a packed tensor, rope_qkv (operator API on its own stream, so timed by the host clock between device-wide syncs; skipped with
    --no-composition).
Algorithmic bytes: out of place the whole packed tensor is read and written (2 T W s); in place only the q and k heads (2 T (Hq + Hk) D s);
the backward reads x and dy and writes dx (3 T W s, a copy of 1.5 tensors). TB/s = those bytes / median time.
`over_rope` = time / kf_rope's time for the same direction's bytes (the forward moves exactly kf_rope's bytes); `spread` = |rope_a - rope_b| /
min of them. --check compares sampled tokens of every case with the f64 reference (tests/qk_norm_ref.py) before timing.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (the kernels are qkn_packed / qkn_elem / qkn_fold).
Prints one JSON object; --json saves it (default profiles/r06_qk_norm_bench.json), stamped with qk_norm.hip's content hash."""
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
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import qk_norm_ref as R  # noqa: E402

CODES = {"bf16": H.BF16, "f16": H.F16, "f32": H.F32}
SOURCES = ("qk_norm.hip", "float_pack.h", "rope.hip")
# (name, dtype, B, S, Hq, Hkv, D, R, mode)
CASES = [
    ("bf16 32/32/32 D128 fwd", "bf16", 8, 4096, 32, 32, 128, 128, "fwd"),
    ("bf16 32/32/32 D128 fwd in place", "bf16", 8, 4096, 32, 32, 128, 128, "inplace"),
    ("bf16 32/32/32 D128 bwd", "bf16", 8, 4096, 32, 32, 128, 128, "bwd"),
    ("GQA 32/8/8 bf16 fwd", "bf16", 8, 4096, 32, 8, 128, 128, "fwd"),
    ("GQA 32/8/8 bf16 bwd", "bf16", 8, 4096, 32, 8, 128, 128, "bwd"),
    ("D 64 / H 64 bf16 fwd", "bf16", 8, 4096, 64, 64, 64, 64, "fwd"),
    ("R = D/2 bf16 fwd", "bf16", 8, 4096, 32, 32, 128, 64, "fwd"),
    ("R = 0 bf16 fwd", "bf16", 8, 4096, 32, 32, 128, 0, "fwd"),
    ("f32 fwd", "f32", 8, 4096, 32, 32, 128, 128, "fwd"),
    ("f32 bwd", "f32", 8, 4096, 32, 32, 128, 128, "bwd"),
]
TILE = 61


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def wall_ms(fn):
    """An operator-API route runs on the host core's own stream: device-wide syncs and the host clock (a dozen launches of overhead in ~ms)."""
    H.device_sync()
    t0 = time.perf_counter()
    fn()
    H.device_sync()
    return (time.perf_counter() - t0) * 1e3


def composition(case, xs_tile, wq, wk, args):
    """The operator-API route of today on the same shape: -> a callable, or None."""
    import kfunca_amd as kfunca
    _, name, B, S, Hq, Hkv, D, rot, mode = case
    if args.no_composition or mode != "fwd" or rot == 0:
        return None
    T, W = B * S, (Hq + 2 * Hkv) * D
    x32 = np.tile(O.to_float(xs_tile, CODES[name]), (T // TILE + 1, 1))[:T]
    conv = {"bf16": lambda t: t.bfloat16(), "f16": lambda t: t.half(), "f32": lambda t: t}[name]
    qkv = conv(kfunca.from_numpy(np.ascontiguousarray(x32, np.float32), 0))
    tq, tk = conv(kfunca.from_numpy(O.to_float(wq, CODES[name]).astype(np.float32), 0)), conv(kfunca.from_numpy(O.to_float(wk, CODES[name]).astype(np.float32), 0))
    cos, sin = kfunca.rope_table(S, rot, 10000.0, 0)

    def step():
        q, k, v = qkv.split([Hq * D, Hkv * D, Hkv * D], 1)
        qn = kfunca.rms_norm(q.contiguous().view(T * Hq, D), tq, 1e-6).view(T, Hq * D)
        kn = kfunca.rms_norm(k.contiguous().view(T * Hkv, D), tk, 1e-6).view(T, Hkv * D)
        return kfunca.rope_qkv(kfunca.cat([qn, kn, v], 1), cos, sin, B, S, Hq, Hkv)

    return step


def check_case(case, bufs, xs_tile, dys_tile, wq, wk, cos, sin):
    """Sampled tokens of the result against the f64 reference: -> the worst fraction of the bound."""
    _, name, B, S, Hq, Hkv, D, rot, mode = case
    code = CODES[name]
    es = H.DTYPE_SIZE[code]
    T, W = B * S, (Hq + 2 * Hkv) * D
    r = R.ROUNDING[name]
    f = lambda a: O.to_float(a, code).astype(np.float64)  # noqa: E731
    worst = 0.0
    for tok in (0, 1, TILE, S - 1, S, T // 2 + 3, T - 1):
        row = np.empty(W, xs_tile.dtype)
        H.check(H.lib().kf_memcpy_d2h(row.ctypes.data, bufs["out"].ptr + tok * W * es, W * es, None))
        x, dy = f(xs_tile[tok % TILE])[None], f(dys_tile[tok % TILE])[None]
        a = (f(wq), f(wk), cos, sin, np.array([tok % S]), 1, 1, Hq, Hkv, Hkv, D, rot, False, 1e-6)
        if mode == "bwd":
            rb = R.backward(x, dy, *a)
            ok, frac = R.within(f(row)[None], rb["dx"], rb["dx_tol"], r, R.SUBNORMAL_ROUNDING[name])
        else:
            y, tol = R.forward(x, *a)
            ok, frac = R.within(f(row)[None], y, tol, r, R.SUBNORMAL_ROUNDING[name])
        if not ok:
            raise SystemExit(f"{case[0]}: token {tok} misses the bound (fraction {frac})")
        worst = max(worst, frac)
    return worst


def bench_case(case, args):
    label, name, B, S, Hq, Hkv, D, rot, mode = case
    code = CODES[name]
    es = H.DTYPE_SIZE[code]
    Ht, nh = Hq + 2 * Hkv, Hq + Hkv
    W, T = Ht * D, B * S
    nbytes = T * W * es
    rng = np.random.default_rng(T + W)
    xs_tile = O.from_float(rng.uniform(-2, 2, (TILE, W)).astype(np.float32), code)
    dys_tile = O.from_float(rng.uniform(-1, 1, (TILE, W)).astype(np.float32), code)
    wq, wk = (O.from_float(rng.uniform(0.5, 1.5, D).astype(np.float32), code) for _ in range(2))
    bx, bg, bo = H.DevBuf(nbytes), H.DevBuf(nbytes), H.DevBuf(nbytes)
    for buf, tile in ((bx, xs_tile), (bg, dys_tile)):
        for r0 in range(0, T, TILE):
            n = min(TILE, T - r0)
            H.check(H.lib().kf_memcpy_h2d(buf.ptr + r0 * W * es, tile.ctypes.data, n * W * es, None))
    bwq, bwk = H.DevBuf.from_numpy(wq), H.DevBuf.from_numpy(wk)
    bdq, bdk = H.DevBuf(D * es), H.DevBuf(D * es)
    Rt = rot if rot else D   # kf_rope needs a rotation: the R = 0 case is timed against the full one
    cos, sin = H.DevBuf(S * Rt // 2 * 4), H.DevBuf(S * Rt // 2 * 4)
    H.rope_table(10000.0, Rt, S, cos.ptr, sin.ptr)
    hc, hs = cos.to_numpy((S, Rt // 2), np.float32), sin.to_numpy((S, Rt // 2), np.float32)
    ws = H.DevBuf(max(H.qk_norm_rope_bwd_workspace_bytes(code, B, S, Hq, Hkv, Hkv, D), 4))
    lay = (S * W, D, W)
    kw = dict(wq=bwq.ptr, wk=bwk.ptr, cos=cos.ptr if rot else None, sin=sin.ptr if rot else None, table_rows=S if rot else 0, rotary_dim=rot)
    if mode == "inplace":
        moved = 2 * T * nh * D * es
    elif mode == "bwd":
        moved = 3 * nbytes
    else:
        moved = 2 * nbytes
    copy_bytes = (moved // 2) // 256 * 256
    big = H.DevBuf(copy_bytes) if copy_bytes > nbytes else None   # (the backward's 1.5 tensors)
    src = H.DevBuf(copy_bytes) if big else None

    def kernel():
        if mode == "inplace":
            H.qk_norm_rope_fwd(code, B, S, Hq, Hkv, Hkv, D, bo.ptr, W, None, None, **kw)
        elif mode == "bwd":
            H.qk_norm_rope_bwd(code, B, S, Hq, Hkv, Hkv, D, bx.ptr, W, bg.ptr, W, bo.ptr, W, dwq=bdq.ptr, dwk=bdk.ptr, workspace=ws.ptr,
                               workspace_bytes=ws.nbytes, **kw)
        else:
            H.qk_norm_rope_fwd(code, B, S, Hq, Hkv, Hkv, D, bx.ptr, W, bo.ptr, W, **kw)

    def rope():
        if mode == "inplace":
            H.rope(code, B, Ht, S, D, bg.ptr, lay, None, None, cos.ptr, sin.ptr, S, Rt, nh)
        else:
            H.rope(code, B, Ht, S, D, bg.ptr, lay, bo.ptr, lay, cos.ptr, sin.ptr, S, Rt, nh, inverse=mode == "bwd")

    def copy():
        H.check(H.lib().kf_memcpy_d2d((big or bo).ptr, (src or bx).ptr, copy_bytes, None))

    worst = None
    if args.check and mode != "inplace":
        kernel()
        H.device_sync()
        worst = check_case(case, {"out": bo}, xs_tile, dys_tile, wq, wk, hc if rot else None, hs if rot else None)
    comp = composition(case, xs_tile, wq, wk, args)
    fns = {"copy": copy, "rope_a": rope, "kernel": kernel, "rope_b": rope}
    if comp:
        fns["composition"] = comp
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
            H.device_sync()
    ms = {k: [] for k in fns}
    for _ in range(args.iters):  # interleaved: drift of the clock or of the neighbours' load hits every side alike
        for k, fn in fns.items():
            ms[k].append(wall_ms(fn) if k == "composition" else event_ms(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rope_ms = min(med["rope_a"], med["rope_b"])
    res = {"case": label, "dtype": name, "B": B, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "R": rot, "mode": mode, "bytes": moved, "ms": med["kernel"],
           "TBps": moved / med["kernel"] / 1e9, "copy_ms": med["copy"], "copy_TBps": 2 * copy_bytes / med["copy"] / 1e9,
           "rope_a_ms": med["rope_a"], "rope_b_ms": med["rope_b"], "spread": abs(med["rope_a"] - med["rope_b"]) / rope_ms,
           "over_rope": med["kernel"] / rope_ms, "spread_ms": [min(ms["kernel"]), max(ms["kernel"])],
           "composition_ms": med.get("composition", "not measured")}
    res["time_over_copy"] = res["copy_TBps"] / res["TBps"]
    if comp:
        res["composition_over_fused"] = med["composition"] / med["kernel"]
    if worst is not None:
        res["check_worst_fraction_of_bound"] = worst
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true", help="compare sampled tokens with the f64 reference before timing")
    ap.add_argument("--no-composition", action="store_true")
    ap.add_argument("--only", default="", help="run the cases whose label contains this text")
    ap.add_argument("--json", type=Path, default=ROOT / "profiles" / "r06_qk_norm_bench.json")
    args = ap.parse_args()
    if H.device_count() == 0:
        raise SystemExit("qk_norm_bench needs a GPU: nothing here falls back to a CPU path")
    H.set_device(0)
    out = {"cases": [bench_case(c, args) for c in CASES if args.only in c[0]], "iters": args.iters, "warmup": args.warmup}
    out.update(bench.stamp(SOURCES))
    print(json.dumps(out))
    args.json.parent.mkdir(parents=True, exist_ok=True)
    args.json.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
