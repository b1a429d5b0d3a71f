#!/usr/bin/env python3
"""Full (non-causal) attention (kf_attn_full_fwd / kf_attn_full_bwd) through the C ABI: median HIP-event times of forward and backward
on encoder, cross-attention, padded-batch and grouped-query shapes (bf16, D 128 and 64), beside the project's own causal hand kernels.

For each case, in one interleaved loop of --iters after --warmup:
  full_fwd / full_bwd       kf_attn_full_fwd / kf_attn_full_bwd (backward = delta + dQ + dK/dV kernels)
  causal_fwd / causal_bwd   (Sq == Skv, S % 128 == 0, no key lengths) kf_attn_fwd_gqa / kf_attn_bwd_gqa under KF_ATTN_FWD_V3=1,
                            KF_ATTN_DKV_V4=1, KF_ATTN_SPLIT_BWD=1: the hand-written causal kernels with the recomputing dQ - the yardstick
  torch_fwd / torch_bwd     torch's scaled_dot_product_attention, non-causal, same shape (context only; --no-torch skips it)
Both sides are expressed per visited tile = (128 queries x 64 keys) of one query head: the full call visits every tile below a batch's
key length, the causal call those at or below the diagonal (about half). TFLOP/s count the matrix products actually executed on the
visible region: forward 2 (4 Sq len D flop per head), backward 7 (S and dP in both kernels, dQ, dK, dV: 14 Sq len D).
--check samples two heads per case against the float64 reference (tests/attn_full_ref.py) under the project's bounds.
Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (name, B, Hq, Hkv, Sq, Skv, D, key lengths as fractions of Skv per batch (cycled) or None)
CASES = [
    ("encoder S1024 D128", 32, 16, 16, 1024, 1024, 128, None),
    ("encoder S576 D128", 32, 16, 16, 576, 576, 128, None),
    ("encoder S1024 D64", 32, 16, 16, 1024, 1024, 64, None),
    ("encoder S576 D64", 32, 16, 16, 576, 576, 64, None),
    ("cross 4096x1024 D128", 8, 16, 16, 4096, 1024, 128, None),
    ("cross 1024x4096 D128", 8, 16, 16, 1024, 4096, 128, None),
    ("padded S1024 D128", 32, 16, 16, 1024, 1024, 128, (1.0, 0.25, 0.6, 0.9, 0.1, 0.75, 0.5, 0.33)),
    ("GQA 32/8 S2048 D128", 8, 32, 8, 2048, 2048, 128, None),
]
CAUSAL_KNOBS = dict(KF_ATTN_FWD_V3="1", KF_ATTN_DKV_V4="1", KF_ATTN_SPLIT_BWD="1")


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def torch_times(B, Hq, Hkv, Sq, Skv, D, lens, iters, warmup):
    import torch
    import torch.nn.functional as F
    dev = "cuda"
    G = Hq // Hkv
    q = torch.rand(B, Hq, Sq, D, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k, v = (torch.rand(B, Hkv, Skv, D, device=dev, dtype=torch.bfloat16).repeat_interleave(G, dim=1).requires_grad_(True) for _ in range(2))
    go = torch.rand_like(q)
    mask = None if lens is None else (torch.arange(Skv, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None])[:, None, None, :]
    tf, tb = [], []
    for it in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        e[1].record()
        o.backward(go)
        e[2].record()
        torch.cuda.synchronize()
        q.grad = k.grad = v.grad = None
        if it >= warmup:
            tf.append(e[0].elapsed_time(e[1]))
            tb.append(e[1].elapsed_time(e[2]))
    return statistics.median(tf), statistics.median(tb)


def run_case(case, args):
    name, B, Hq, Hkv, Sq, Skv, D, fr = case
    code = H.BF16
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    rng = np.random.default_rng(len(name))
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * max(Sq, Skv) * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    q, go = take(0, (B, Hq, Sq, D)), take(1024, (B, Hq, Sq, D))
    k, v = take(2048, (B, Hkv, Skv, D)), take(3072, (B, Hkv, Skv, D))
    lens = None if fr is None else [max(1, int(Skv * fr[b % len(fr)])) for b in range(B)]
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    bl = None if lens is None else H.DevBuf.from_numpy(np.asarray(lens, np.int64))
    lp = None if bl is None else bl.ptr
    bo, blse, bdq, bdk, bdv = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * Sq), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
    ws = H.DevBuf(need)
    full_fwd = lambda: H.attn_full_fwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, kv_len=lp)  # noqa: E731
    full_bwd = lambda: H.attn_full_bwd(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr,  # noqa: E731
                                       bdv.ptr, ws.ptr, need, kv_len=lp)
    timed = {"full_fwd": full_fwd, "full_bwd": full_bwd}
    causal = Sq == Skv and Sq % 128 == 0 and lens is None
    if causal:
        bo2, blse2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * Sq)
        with H.knobs(**CAUSAL_KNOBS):
            _, cmin = H.attn_bwd_gqa_workspace_bytes(code, B, Hq, Hkv, Sq, Skv, D)
        cws = H.DevBuf(cmin)

        def causal_fwd():
            H.attn_fwd_gqa(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo2.ptr, blse2.ptr)

        def causal_bwd():
            H.attn_bwd_gqa(code, B, Hq, Hkv, Sq, Skv, D, scale, bq.ptr, bk.ptr, bv.ptr, bo2.ptr, blse2.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, cws.ptr, cmin)

        timed.update(causal_fwd=causal_fwd, causal_bwd=causal_bwd)
    t = {n: [] for n in timed}
    for it in range(args.warmup + args.iters):
        for n, fn in timed.items():
            if n.startswith("causal"):
                with H.knobs(**CAUSAL_KNOBS):
                    ms = event_ms(fn)
            else:
                ms = event_ms(fn)
            if it >= args.warmup:
                t[n].append(ms)
    vis = [Skv] * B if lens is None else lens
    tiles = Hq * sum(((Sq + 127) // 128) * ((ln + 63) // 64) for ln in vis)
    pairs = Hq * Sq * sum(vis)                       # visible (query, key) pairs over all heads
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "Sq": Sq, "Skv": Skv, "D": D, "kv_len": lens, "workspace_bytes": need, "tiles": tiles}
    med = {n: statistics.median(x) for n, x in t.items()}
    out.update({f"{n}_ms": round(m, 4) for n, m in med.items()})
    out.update(full_fwd_tflops=round(4 * pairs * D / (med["full_fwd"] * 1e-3) / 1e12, 1), full_bwd_tflops=round(14 * pairs * D / (med["full_bwd"] * 1e-3) / 1e12, 1),
               full_fwd_ns_per_tile=round(med["full_fwd"] * 1e6 / tiles, 2), full_bwd_ns_per_tile=round(med["full_bwd"] * 1e6 / tiles, 2))
    if causal:
        # 256-query blocks x 64-key tiles at or below the diagonal, counted in the same 128 x 64 unit
        ctiles = 2 * B * Hq * sum((min(Skv, min(Sq, (qb + 1) * 256)) + 63) // 64 for qb in range((Sq + 255) // 256))
        cpairs = B * Hq * Sq * (Sq + 1) // 2
        out.update(causal_tiles=ctiles, causal_fwd_tflops=round(4 * cpairs * D / (med["causal_fwd"] * 1e-3) / 1e12, 1),
                   causal_bwd_tflops=round(14 * cpairs * D / (med["causal_bwd"] * 1e-3) / 1e12, 1),
                   causal_fwd_ns_per_tile=round(med["causal_fwd"] * 1e6 / ctiles, 2), causal_bwd_ns_per_tile=round(med["causal_bwd"] * 1e6 / ctiles, 2))
        out.update(fwd_per_tile_vs_causal=round(out["full_fwd_ns_per_tile"] / out["causal_fwd_ns_per_tile"], 3),
                   bwd_per_tile_vs_causal=round(out["full_bwd_ns_per_tile"] / out["causal_bwd_ns_per_tile"], 3))
    if not args.no_torch:
        try:
            tf, tb = torch_times(B, Hq, Hkv, Sq, Skv, D, lens, args.iters, args.warmup)
            out.update(torch_fwd_ms=round(tf, 4), torch_bwd_ms=round(tb, 4))
        except (ImportError, RuntimeError) as e:   # context only: a box whose torch sees no device still measures the kernels
            out["torch"] = f"unavailable: {e}"
    if args.check:
        from oracle import checks as K
        from tests.attn_full_ref import attn_ref64_vis, check_lse, key_len_vis
        full_fwd()
        full_bwd()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, Sq), np.float32), bdq.to_numpy(q.shape, q.dtype)
        dk, dv = bdk.to_numpy(k.shape, k.dtype), bdv.to_numpy(k.shape, k.dtype)
        G = Hq // Hkv
        for b, j in ((0, 0), (B - 1, Hkv - 1)):   # a whole group: its query heads and their K/V head
            hs = slice(j * G, (j + 1) * G)
            sl = lambda x, s: x[b:b + 1, s]  # noqa: E731
            vis_ = key_len_vis(None if lens is None else lens[b:b + 1], Sq, Skv, 1)
            ref = attn_ref64_vis(sl(q, hs), sl(k, slice(j, j + 1)), sl(v, slice(j, j + 1)), sl(go, hs), vis_, code)
            for nm, got in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, slice(j, j + 1))), ("dv", sl(dv, slice(j, j + 1)))):
                K.check_one(nm, got, ref, code, f"{name} b{b} kv-head {j}")
            check_lse(sl(lse, hs), ref, name)
        out["check"] = "ok"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--json")
    args = ap.parse_args()
    H.set_device(0)
    cases = [c for c in CASES if not args.cases or c[0] in args.cases.split(",")]
    props = H.device_props(0)
    import bench
    res = {"tool": "attn_full_bench", "device": props.name.decode(), "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_full.hip", "attention.hip", "common.h", "runtime.hip")))   # the sources both sides of the table come from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
