#!/usr/bin/env python3
"""Document-masked attention of packed rows (kf_attn_doc_fwd / kf_attn_doc_bwd) through the C ABI: median HIP-event times of forward and
backward (bf16, D 128 and 64) beside two baselines on the same buffers.

For each case, in one interleaved loop of --iters after --warmup:
  doc_fwd / doc_bwd             kf_attn_doc_fwd / kf_attn_doc_bwd under the tables kf_attn_doc_table wrote (backward = delta + dQ + dK/dV)
  unmasked_fwd / unmasked_bwd   (a) the same row WITHOUT the document mask: kf_attn_prefix_* without a prefix (causal cases) or kf_attn_full_*
                                (non-causal ones) with the row's key length - more work and a wrong result: the cost of not having the feature
  batched_fwd / batched_bwd     (b) documents of one length L only: the same older family's call on the [B n, H, L, D] view of the same
                                buffers (strided layouts; the cases with equal documents have B = 1, where that view exists). It walks the same
                                tiles: the yardstick.
A visited tile is a (128-query block, 64-key tile) pair of one query head that the forward's workgroup walks: under the document mask the
tiles start[q0] / 64 .. ceil(min(len, end[qe - 1], causal: qe) / 64) - 1 of the block [q0, qe). Times are reported per visited tile, as
the ratio doc / batched (over_batched, fwd and bwd) and, beside (a), as time_ratio next to tile_ratio with their quotient (excess: 1.0 is
"time follows the tiles").
--check compares sampled documents (their query heads of one K/V group) against the float64 reference (tests/attn_full_ref.py) on the
document's own slice - documents are independent, so the slice under the causal or full mask is the whole truth for its tokens - with the
project's bounds, and the tokens in no document against zeros. Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

# (name, B, Hq, Hkv, S, causal, the documents' lengths per row (cycled over the batch)); each at D 128 and 64
SHAPES = [
    ("LM 16 x 512 S8192", 1, 16, 16, 8192, True, [[512] * 16]),
    ("LM mixed S8192", 2, 16, 16, 8192, True, [[3000, 2500, 1500, 700, 400, 92], [92, 400, 700, 1500, 2500, 3000]]),
    ("LM padded tail S8192", 2, 16, 16, 8192, True, [[2000, 1900, 1100, 1000], [4000, 100, 77]]),
    ("ViT 16 x 1024 S16384", 1, 16, 16, 16384, False, [[1024] * 16]),
    ("GQA 32/8 LM 16 x 512 S8192", 1, 32, 8, 8192, True, [[512] * 16]),
]
CASES = [(f"{s[0]} D{D}",) + s[1:5] + (D,) + s[5:] for D in (128, 64) for s in SHAPES]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def visited_tiles(S, cu, causal):
    """(128-query block, 64-key tile) pairs per query head: those the document forward walks, those baseline (a) walks"""
    from tests.attn_doc_ref import doc_table
    kv, start, end = doc_table(cu, S)
    doc = unmasked = 0
    for b in range(cu.shape[0]):
        ln = int(kv[b])
        for q0 in range(0, S, 128):
            qe = min(S, q0 + 128)
            hi = min(ln, int(end[b, qe - 1]), qe if causal else S)
            doc += max(0, (hi + 63) // 64 - min(int(start[b, q0]), ln) // 64)
            unmasked += (min(ln, qe if causal else S) + 63) // 64
    return doc, unmasked


def run_case(case, args):
    name, B, Hq, Hkv, S, D, causal, rows = case
    from tests.attn_doc_ref import cu_of
    code = H.BF16
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    cu = cu_of([rows[b % len(rows)] for b in range(B)])
    lens = cu[:, -1].copy()
    equal = B == 1 and len(set(rows[0])) == 1 and sum(rows[0]) == S
    rng = np.random.default_rng(len(name))
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * S * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    q, go = take(0, (B, Hq, S, D)), take(1024, (B, Hq, S, D))
    k, v = take(2048, (B, Hkv, S, D)), take(3072, (B, Hkv, S, D))
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    bcu, bkv, bs, be = H.DevBuf.from_numpy(cu), H.DevBuf(8 * B), H.DevBuf(4 * B * S), H.DevBuf(4 * B * S)
    H.attn_doc_table(B, S, cu.shape[1] - 1, bcu.ptr, bkv.ptr, bs.ptr, be.ptr)
    bo, blse, bdq, bdk, bdv = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    bo2, blse2, bdq2, bdk2, bdv2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    ws = H.DevBuf(need)
    ops = (bq.ptr, bk.ptr, bv.ptr)
    dkw = dict(kv_len=bkv.ptr, doc_start=bs.ptr, doc_end=be.ptr, causal=causal)
    old_fwd, old_bwd = (H.attn_prefix_fwd, H.attn_prefix_bwd) if causal else (H.attn_full_fwd, H.attn_full_bwd)
    timed = {
        "doc_fwd": lambda: H.attn_doc_fwd(code, B, Hq, Hkv, S, D, scale, *ops, bo.ptr, blse.ptr, **dkw),
        "doc_bwd": lambda: H.attn_doc_bwd(code, B, Hq, Hkv, S, D, scale, *ops, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, **dkw),
        "unmasked_fwd": lambda: old_fwd(code, B, Hq, Hkv, S, S, D, scale, *ops, bo2.ptr, blse2.ptr, kv_len=bkv.ptr),
        "unmasked_bwd": lambda: old_bwd(code, B, Hq, Hkv, S, S, D, scale, *ops, bo2.ptr, blse2.ptr, bgo.ptr, bdq2.ptr, bdk2.ptr, bdv2.ptr, ws.ptr, need,
                                        kv_len=bkv.ptr),
    }
    if equal:   # the [n, H, L, D] view of the [1, H, S, D] buffers: sequence j starts L rows further, a head S rows further
        n, L = len(rows[0]), rows[0][0]
        lay = (L * D, S * D, D)
        need_b = H.attn_full_bwd_workspace_bytes(code, n, Hq, Hkv, L, L, D)
        assert need_b <= need
        timed["batched_fwd"] = lambda: old_fwd(code, n, Hq, Hkv, L, L, D, scale, *ops, bo2.ptr, blse2.ptr, layouts=(lay,) * 4)
        timed["batched_bwd"] = lambda: old_bwd(code, n, Hq, Hkv, L, L, D, scale, *ops, bo2.ptr, blse2.ptr, bgo.ptr, bdq2.ptr, bdk2.ptr, bdv2.ptr, ws.ptr,
                                               need_b, layouts=(lay,) * 8)
    t = {n_: [] for n_ in timed}
    for it in range(args.warmup + args.iters):
        for n_, fn in timed.items():   # each backward follows its own forward: o and lse are its family's
            ms = event_ms(fn)
            if it >= args.warmup:
                t[n_].append(ms)
    doc_tiles, un_tiles = visited_tiles(S, cu, causal)
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "causal": causal, "doc_lens": [rows[b % len(rows)] for b in range(B)],
           "kv_len": [int(x) for x in lens], "visited_tiles": Hq * doc_tiles, "unmasked_tiles": Hq * un_tiles, "tile_ratio": round(doc_tiles / un_tiles, 4)}
    med = {n_: statistics.median(x) for n_, x in t.items()}
    out.update({f"{n_}_ms": round(m, 4) for n_, m in med.items()})
    for d in ("fwd", "bwd"):
        out[f"doc_{d}_ns_per_tile"] = round(med[f"doc_{d}"] * 1e6 / (Hq * doc_tiles), 2)
        out[f"unmasked_{d}_ns_per_tile"] = round(med[f"unmasked_{d}"] * 1e6 / (Hq * un_tiles), 2)
        out[f"{d}_time_ratio"] = round(med[f"doc_{d}"] / med[f"unmasked_{d}"], 3)
        out[f"{d}_excess"] = round(med[f"doc_{d}"] / med[f"unmasked_{d}"] / (doc_tiles / un_tiles), 3)
        if equal:   # (b) walks the tiles the document call walks
            out[f"batched_{d}_ns_per_tile"] = round(med[f"batched_{d}"] * 1e6 / (Hq * doc_tiles), 2)
            out[f"{d}_over_batched"] = round(med[f"doc_{d}"] / med[f"batched_{d}"], 3)
    if args.check:
        from oracle import checks as K
        from tests.attn_full_ref import attn_ref64_vis, check_lse, format_floor_vis
        timed["doc_fwd"]()
        timed["doc_bwd"]()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), bdq.to_numpy(q.shape, q.dtype)
        dk, dv = bdk.to_numpy(k.shape, k.dtype), bdv.to_numpy(k.shape, k.dtype)
        G = Hq // Hkv
        for b, j, doc in ((0, 0, 1), (B - 1, Hkv - 1, len(rows[(B - 1) % len(rows)]) - 1)):   # (row, K/V head, document): a whole group
            lo, hi = int(cu[b, doc]), int(cu[b, doc + 1])
            hs, js, tok = slice(j * G, (j + 1) * G), slice(j, j + 1), slice(lo, hi)
            sl = lambda x, s: x[b:b + 1, s, tok]  # noqa: E731
            L = hi - lo
            vis = (np.tril(np.ones((L, L), bool)) if causal else np.ones((L, L), bool))[None]
            sops = (sl(q, hs), sl(k, js), sl(v, js), sl(go, hs))
            ref, fl = attn_ref64_vis(*sops, vis, code), format_floor_vis(*sops, vis, code)
            for nm, got in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, js)), ("dv", sl(dv, js))):
                K.check_one(nm, got, ref, code, f"{name} row {b} kv-head {j} document {doc}", floor=fl.get(nm))
            check_lse(sl(lse, hs), ref, name)
        for b in range(B):   # the tokens in no document
            ln = int(lens[b])
            for x in (o, dq, dk, dv):
                assert not x[b, :, ln:].view(np.uint16).any(), f"{name} row {b}: a token in no document is not zero"
            assert np.isneginf(lse[b, :, ln:]).all()
        out["check"] = "ok"
    tail = f", {out['fwd_over_batched']} / {out['bwd_over_batched']} of the batched call (fwd / bwd)" if equal else ""
    print(f"[attn_doc_bench] {name}: fwd {out['fwd_time_ratio']} of unmasked for {out['tile_ratio']} of its tiles{tail}", file=sys.stderr, flush=True)
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
    res = {"tool": "attn_doc_bench", "device": props.name.decode(), "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_full.hip", "common.h", "runtime.hip")))   # the sources every column of the table comes from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
