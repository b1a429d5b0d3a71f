#!/usr/bin/env python3
"""Prefix-LM / padded-causal attention (kf_attn_prefix_fwd / kf_attn_prefix_bwd) through the C ABI: median HIP-event times of forward
and backward (bf16, D 128 and 64) beside full attention and the project's own causal hand kernels on the same tensors.

For each case, in one interleaved loop of --iters after --warmup:
  prefix_fwd / prefix_bwd   kf_attn_prefix_fwd / kf_attn_prefix_bwd (backward = delta + dQ + dK/dV kernels)
  full_fwd / full_bwd       kf_attn_full_fwd / kf_attn_full_bwd on the same tensors and key lengths: the same kernels without the mask,
                            so every tile below the key length - what the tile skipping has to beat
  causal_fwd / causal_bwd   (Sq == Skv, S % 128 == 0, no lengths, no prefix) kf_attn_fwd_gqa / kf_attn_bwd_gqa under KF_ATTN_FWD_V3=1,
                            KF_ATTN_DKV_V4=1, KF_ATTN_SPLIT_BWD=1: the hand-written causal kernels, tools/attn_full_bench.py's yardstick
A visited tile is a (128-query block, 64-key tile) pair of one query head that the forward's workgroup walks: tiles below
min(len_b, max(pre_b, last query of the block + 1)). Causal at S 2048 walks 272 of the 512 pairs per head (528 of 1024 in 64 x 64
units). Times are reported per visited tile of the prefix call, and as the ratio to the full call.
--check samples two K/V heads per case against the float64 reference (tests/attn_full_ref.py under tests/attn_prefix_ref.py's
visibility) with the project's bounds. Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

MIXED = (1.0, 0.25, 0.6, 0.9, 0.1, 0.75, 0.5, 0.33)
# (name, B, Hq, Hkv, S, key lengths as fractions of S per batch (cycled) or None, prefixes per batch (cycled) or None); each at D 128 and 64
SHAPES = [
    ("causal S1024", 32, 16, 16, 1024, None, None),
    ("causal S2048", 8, 16, 16, 2048, None, None),
    ("prefix 256|576 S2048", 8, 16, 16, 2048, None, (256, 576)),
    ("padded causal S1024", 32, 16, 16, 1024, MIXED, None),
    ("GQA 32/8 causal S2048", 8, 32, 8, 2048, None, None),
]
CASES = [(f"{s[0]} D{D}",) + s[1:5] + (D,) + s[5:] for D in (128, 64) for s in SHAPES]
CAUSAL_KNOBS = dict(KF_ATTN_FWD_V3="1", KF_ATTN_DKV_V4="1", KF_ATTN_SPLIT_BWD="1")


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def visited_tiles(S, lens, pres):
    """(128-query block, 64-key tile) pairs per query head the prefix forward walks, and those the full forward walks"""
    nxb = (S + 127) // 128
    walk = sum((min(ln, max(pre, min(S, xb * 128 + 128))) + 63) // 64 for ln, pre in zip(lens, pres) for xb in range(nxb))
    return walk, sum(nxb * ((ln + 63) // 64) for ln in lens)


def run_case(case, args):
    name, B, Hq, Hkv, S, D, fr, pf = case
    code = H.BF16
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    rng = np.random.default_rng(len(name))
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * S * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    q, go = take(0, (B, Hq, S, D)), take(1024, (B, Hq, S, D))
    k, v = take(2048, (B, Hkv, S, D)), take(3072, (B, Hkv, S, D))
    lens = None if fr is None else [max(1, int(S * fr[b % len(fr)])) for b in range(B)]
    pres = None if pf is None else [pf[b % len(pf)] for b in range(B)]
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    bl = None if lens is None else H.DevBuf.from_numpy(np.asarray(lens, np.int64))
    bp = None if pres is None else H.DevBuf.from_numpy(np.asarray(pres, np.int64))
    lp, pp = None if bl is None else bl.ptr, None if bp is None else bp.ptr
    bo, blse, bdq, bdk, bdv = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    bo2, blse2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S)     # the yardsticks' outputs: the prefix call's stay for --check
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    ws = H.DevBuf(need)
    fwd_args = (code, B, Hq, Hkv, S, S, D, scale, bq.ptr, bk.ptr, bv.ptr)
    prefix_fwd = lambda: H.attn_prefix_fwd(*fwd_args, bo.ptr, blse.ptr, kv_len=lp, prefix_len=pp)  # noqa: E731
    prefix_bwd = lambda: H.attn_prefix_bwd(*fwd_args, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, kv_len=lp, prefix_len=pp)  # noqa: E731
    full_fwd = lambda: H.attn_full_fwd(*fwd_args, bo2.ptr, blse2.ptr, kv_len=lp)  # noqa: E731
    full_bwd = lambda: H.attn_full_bwd(*fwd_args, bo2.ptr, blse2.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, kv_len=lp)  # noqa: E731
    timed = {"prefix_fwd": prefix_fwd, "full_fwd": full_fwd, "prefix_bwd": prefix_bwd, "full_bwd": full_bwd}
    hand = S % 128 == 0 and lens is None and pres is None
    if hand:
        with H.knobs(**CAUSAL_KNOBS):
            _, cmin = H.attn_bwd_gqa_workspace_bytes(code, B, Hq, Hkv, S, S, D)
        cws = H.DevBuf(cmin)
        timed["causal_fwd"] = lambda: H.attn_fwd_gqa(*fwd_args, bo2.ptr, blse2.ptr)
        timed["causal_bwd"] = lambda: H.attn_bwd_gqa(*fwd_args, bo2.ptr, blse2.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, cws.ptr, cmin)
    t = {n: [] for n in timed}
    for it in range(args.warmup + args.iters):
        for n, fn in timed.items():   # each backward follows its own forward: o and lse are its family's
            if n.startswith("causal"):
                with H.knobs(**CAUSAL_KNOBS):
                    ms = event_ms(fn)
            else:
                ms = event_ms(fn)
            if it >= args.warmup:
                t[n].append(ms)
    walk, every = visited_tiles(S, lens or [S] * B, pres or [0] * B)
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "kv_len": lens, "prefix_len": pres, "visited_tiles": Hq * walk,
           "full_tiles": Hq * every, "visited_fraction": round(walk / every, 4)}
    med = {n: statistics.median(x) for n, x in t.items()}
    out.update({f"{n}_ms": round(m, 4) for n, m in med.items()})
    for d in ("fwd", "bwd"):
        out[f"prefix_{d}_ns_per_tile"] = round(med[f"prefix_{d}"] * 1e6 / (Hq * walk), 2)
        out[f"full_{d}_ns_per_tile"] = round(med[f"full_{d}"] * 1e6 / (Hq * every), 2)
        out[f"{d}_vs_full"] = round(med[f"prefix_{d}"] / med[f"full_{d}"], 3)
        if hand:
            out[f"{d}_vs_causal"] = round(med[f"prefix_{d}"] / med[f"causal_{d}"], 3)
    if args.check:
        from oracle import checks as K
        from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis
        from tests.attn_prefix_ref import prefix_vis
        prefix_fwd()
        prefix_bwd()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), bdq.to_numpy(q.shape, q.dtype)
        dk, dv = bdk.to_numpy(k.shape, k.dtype), bdv.to_numpy(k.shape, k.dtype)
        G = Hq // Hkv
        for b, j in ((1 % B, 0), (B - 1, Hkv - 1)):   # a whole group: its query heads and their K/V head
            hs, js = slice(j * G, (j + 1) * G), slice(j, j + 1)
            sl = lambda x, s: x[b:b + 1, s]  # noqa: E731
            vis = prefix_vis(None if lens is None else lens[b:b + 1], None if pres is None else pres[b:b + 1], S, S, 1)
            ops = (sl(q, hs), sl(k, js), sl(v, js), sl(go, hs))
            ref, fl = attn_ref64_vis(*ops, vis, code), format_floor_vis(*ops, vis, code)
            for nm, got in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, js)), ("dv", sl(dv, js))):
                K.check_one(nm, got, ref, code, f"{name} b{b} kv-head {j}", floor=fl.get(nm))
            check_lse(sl(lse, hs), ref, name)
        out["check"] = "ok"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cases", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--json")
    args = ap.parse_args()
    H.set_device(0)
    cases = [c for c in CASES if not args.cases or c[0] in args.cases.split(",")]
    props = H.device_props(0)
    import bench
    res = {"tool": "attn_prefix_bench", "device": props.name.decode(), "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_full.hip", "attention.hip", "common.h", "runtime.hip")))   # the sources every column of the table comes from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
