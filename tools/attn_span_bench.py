#!/usr/bin/env python3
"""Packed rows under a causal sliding window (kf_attn_span_fwd / kf_attn_span_bwd) through the C ABI: median HIP-event times of forward
and backward (bf16) beside two baselines on the same buffers.

For each case, in one interleaved loop of --iters after --warmup:
  span_fwd / span_bwd           kf_attn_span_* under the tables kf_attn_span_table wrote for causal = 1 and the case's window, with the
                                case's soft-cap and sinks (backward = delta + dQ + dK/dV + the sink gradient)
  again_fwd / again_bwd         the same two calls a second time in the same loop: the spread of one call against itself
  doc_fwd / doc_bwd             (a) the causal document mask WITHOUT the window on the same tensors, with the same modifiers
                                (kf_attn_ext_* with KF_ATTN_MASK_DOC, which is kf_attn_doc_* when there is no modifier): what a packed
                                batch could run before - more tiles and the wrong mask
  batched_fwd / batched_bwd     (b) documents of one length L only: kf_attn_window_* on the [B n, H, L, D] view of the same buffers
                                (strided layouts, B = 1). It walks the same tiles: the yardstick.
A visited tile is a (128-query block, 64-key tile) pair of one query head that the forward's workgroup walks: the tiles
key_lo[q0] / 64 .. ceil(key_hi[qe - 1] / 64) - 1 of the block [q0, qe). Times are reported per visited tile, as the ratio to (a)
beside the tile ratio (excess: 1.0 is "time follows the tiles") and as the ratio to (b).
--check compares sampled documents (the query heads of one K/V group) against the float64 reference with the case's modifiers
(tests/attn_ext_ref.py) on the document's own slice - documents are independent, so the slice under the causal window is the whole truth
for its tokens - with the project's bounds, and the tokens in no document against zeros. Prints one JSON object; --json saves it."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from kfunca_amd import hip_abi as H  # noqa: E402
from oracle import oracle as O  # noqa: E402

MIXED = [[3000, 2500, 1500, 700, 400, 92], [92, 400, 700, 1500, 2500, 3000]]
# (name, B, Hq, Hkv, S, D, window_left, softcap, sinks, the documents' lengths per row (cycled over the batch))
CASES = [
    ("gpt-oss-like LM mixed S8192 D64 H64/8 w128 sinks", 2, 64, 8, 8192, 64, 128, 0.0, True, MIXED),
    ("Gemma-like LM mixed S8192 D128 H32/8 w1024 cap50", 2, 32, 8, 8192, 128, 1024, 50.0, False, MIXED),
    ("Gemma-like LM mixed S8192 D128 H32/8 w4096 cap50", 2, 32, 8, 8192, 128, 4096, 50.0, False, MIXED),
    ("LM 16 x 512 S8192 D128 H16 w128", 1, 16, 16, 8192, 128, 128, 0.0, False, [[512] * 16]),
    ("LM 16 x 512 S8192 D64 H16 w128", 1, 16, 16, 8192, 64, 128, 0.0, False, [[512] * 16]),
]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    fn()
    b.record()
    b.sync()
    return a.elapsed_ms(b)


def visited_tiles(S, cu, wl):
    """(128-query block, 64-key tile) pairs per query head: those the span forward walks, those baseline (a) walks"""
    from tests.attn_span_ref import span_table
    _, klo, khi, _, _ = span_table(cu, S, 1, wl, 0)
    _, dlo, dhi, _, _ = span_table(cu, S, 1)
    span = doc = 0
    for b in range(cu.shape[0]):
        for q0 in range(0, S, 128):
            qe = min(S, q0 + 128)
            span += max(0, (int(khi[b, qe - 1]) + 63) // 64 - int(klo[b, q0]) // 64)
            doc += max(0, (int(dhi[b, qe - 1]) + 63) // 64 - int(dlo[b, q0]) // 64)
    return span, doc


def run_case(case, args):
    name, B, Hq, Hkv, S, D, wl, softcap, with_sink, rows = case
    from tests.attn_doc_ref import cu_of
    from tests.attn_ext_ref import sinks_for
    code = H.BF16
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    cu = cu_of([rows[b % len(rows)] for b in range(B)])
    n_docs = cu.shape[1] - 1
    lens = cu[:, -1].copy()
    equal = B == 1 and len(set(rows[0])) == 1 and sum(rows[0]) == S
    rng = np.random.default_rng(len(name))
    base = O.f32_to_bf16(rng.uniform(-1, 1, (B * Hq * S * D + 4096,)).astype(np.float32))
    take = lambda off, shp: np.ascontiguousarray(base[off:off + int(np.prod(shp))].reshape(shp))  # noqa: E731  (four windows of one draw)
    q, go = take(0, (B, Hq, S, D)), take(1024, (B, Hq, S, D))
    k, v = take(2048, (B, Hkv, S, D)), take(3072, (B, Hkv, S, D))
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    sink = sinks_for(Hq) if with_sink else None
    bsink = None if sink is None else H.DevBuf.from_numpy(sink)
    bds, bds2 = H.DevBuf(4 * Hq), H.DevBuf(4 * Hq)
    bcu, bkv, bkv2 = H.DevBuf.from_numpy(cu), H.DevBuf(8 * B), H.DevBuf(8 * B)
    tabs = [H.DevBuf(4 * B * S) for _ in range(6)]      # key_lo, key_hi, query_lo, query_hi; doc_start, doc_end
    H.attn_span_table(B, S, n_docs, bcu.ptr, bkv.ptr, *(t.ptr for t in tabs[:4]), causal=True, window_left=wl, window_right=0)
    H.attn_doc_table(B, S, n_docs, bcu.ptr, bkv2.ptr, tabs[4].ptr, tabs[5].ptr)
    bo, blse, bdq, bdk, bdv = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    bo2, blse2, bdq2, bdk2, bdv2 = H.DevBuf(q.nbytes), H.DevBuf(4 * B * Hq * S), H.DevBuf(q.nbytes), H.DevBuf(k.nbytes), H.DevBuf(k.nbytes)
    need = H.attn_full_bwd_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    ws = H.DevBuf(need)
    ops = (bq.ptr, bk.ptr, bv.ptr)
    mods = dict(softcap=softcap, sink=None if bsink is None else bsink.ptr)
    fkw = dict(kv_len=bkv.ptr, key_lo=tabs[0].ptr, key_hi=tabs[1].ptr, **mods)
    bkw = dict(fkw, query_lo=tabs[2].ptr, query_hi=tabs[3].ptr, dsink=None if bsink is None else bds.ptr)
    dmask = H.attn_mask(H.ATTN_MASK_DOC, kv_len=bkv2.ptr, doc_start=tabs[4].ptr, doc_end=tabs[5].ptr, causal=1)
    span_fwd = lambda: H.attn_span_fwd(code, B, Hq, Hkv, S, D, scale, *ops, bo.ptr, blse.ptr, **fkw)  # noqa: E731
    span_bwd = lambda: H.attn_span_bwd(code, B, Hq, Hkv, S, D, scale, *ops, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr, bdv.ptr, ws.ptr, need, **bkw)  # noqa: E731
    timed = {
        "span_fwd": span_fwd, "span_bwd": span_bwd,
        "doc_fwd": lambda: H.attn_ext_fwd(code, B, Hq, Hkv, S, S, D, scale, *ops, bo2.ptr, blse2.ptr, mask=dmask, **mods),
        "doc_bwd": lambda: H.attn_ext_bwd(code, B, Hq, Hkv, S, S, D, scale, *ops, bo2.ptr, blse2.ptr, bgo.ptr, bdq2.ptr, bdk2.ptr, bdv2.ptr, ws.ptr, need,
                                          mask=dmask, dsink=None if bsink is None else bds2.ptr, **mods),
        "again_fwd": span_fwd, "again_bwd": span_bwd,
    }
    if equal:   # the [n, H, L, D] view of the [1, H, S, D] buffers: sequence j starts L rows further, a head S rows further
        n, L = len(rows[0]), rows[0][0]
        lay = (L * D, S * D, D)
        need_b = H.attn_full_bwd_workspace_bytes(code, n, Hq, Hkv, L, L, D)
        assert need_b <= need and not softcap and sink is None
        wkw = dict(window_left=wl, window_right=0)
        timed["batched_fwd"] = lambda: H.attn_window_fwd(code, n, Hq, Hkv, L, L, D, scale, *ops, bo2.ptr, blse2.ptr, layouts=(lay,) * 4, **wkw)
        timed["batched_bwd"] = lambda: H.attn_window_bwd(code, n, Hq, Hkv, L, L, D, scale, *ops, bo2.ptr, blse2.ptr, bgo.ptr, bdq2.ptr, bdk2.ptr, bdv2.ptr,
                                                         ws.ptr, need_b, layouts=(lay,) * 8, **wkw)
    t = {n_: [] for n_ in timed}
    for it in range(args.warmup + args.iters):
        for n_, fn in timed.items():   # each backward follows its own forward: o and lse are its mask's
            ms = event_ms(fn)
            if it >= args.warmup:
                t[n_].append(ms)
    span_tiles, doc_tiles = visited_tiles(S, cu, wl)
    out = {"case": name, "B": B, "Hq": Hq, "Hkv": Hkv, "S": S, "D": D, "window": [wl, 0], "softcap": softcap, "sinks": with_sink,
           "doc_lens": [rows[b % len(rows)] for b in range(B)], "visited_tiles": Hq * span_tiles, "doc_tiles": Hq * doc_tiles,
           "tile_ratio": round(span_tiles / doc_tiles, 4)}
    med = {n_: statistics.median(x) for n_, x in t.items()}
    out.update({f"{n_}_ms": round(m, 4) for n_, m in med.items()})
    for d in ("fwd", "bwd"):
        out[f"span_{d}_ns_per_tile"] = round(med[f"span_{d}"] * 1e6 / (Hq * span_tiles), 2)
        out[f"doc_{d}_ns_per_tile"] = round(med[f"doc_{d}"] * 1e6 / (Hq * doc_tiles), 2)
        out[f"{d}_time_ratio"] = round(med[f"span_{d}"] / med[f"doc_{d}"], 3)
        out[f"{d}_excess"] = round(med[f"span_{d}"] / med[f"doc_{d}"] / (span_tiles / doc_tiles), 3)
        out[f"{d}_spread"] = round(abs(med[f"span_{d}"] - med[f"again_{d}"]) / min(med[f"span_{d}"], med[f"again_{d}"]), 4)
        if equal:   # (b) walks the tiles the span call walks
            out[f"batched_{d}_ns_per_tile"] = round(med[f"batched_{d}"] * 1e6 / (Hq * span_tiles), 2)
            out[f"{d}_over_batched"] = round(med[f"span_{d}"] / med[f"batched_{d}"], 3)
    if args.check:
        from oracle import checks as K
        from tests.attn_ext_ref import attn_ref64_ext, check_lse_ext
        from tests.attn_full_ref import format_floor_vis
        span_fwd()
        span_bwd()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), bdq.to_numpy(q.shape, q.dtype)
        dk, dv = bdk.to_numpy(k.shape, k.dtype), bdv.to_numpy(k.shape, k.dtype)
        G = Hq // Hkv
        for b, j in ((0, 0), (B - 1, Hkv - 1)):   # (row, K/V head): a whole group on the row's shortest document the window bites on
            ln = np.diff(cu[b])                     # (no such document: the mask is the causal document mask; the shortest of 400 tokens or more)
            wide = [i for i in range(n_docs) if ln[i] > wl + 1] or [i for i in range(n_docs) if ln[i] >= 400]
            doc = min(wide, key=lambda i: ln[i])
            lo, hi = int(cu[b, doc]), int(cu[b, doc + 1])
            hs, js, tok = slice(j * G, (j + 1) * G), slice(j, j + 1), slice(lo, hi)
            sl = lambda x, s: x[b:b + 1, s, tok]  # noqa: E731
            L = hi - lo
            m, n = np.arange(L)[:, None], np.arange(L)[None, :]
            vis = ((n <= m) & (n >= m - wl))[None]
            sops = (sl(q, hs), sl(k, js), sl(v, js), sl(go, hs))
            ref = attn_ref64_ext(*sops, vis, code, softcap=softcap or None, sink=None if sink is None else sink[hs])
            fl = format_floor_vis(*sops, vis, code)
            for nm, got in (("o", sl(o, hs)), ("dq", sl(dq, hs)), ("dk", sl(dk, js)), ("dv", sl(dv, js))):
                K.check_one(nm, got, ref, code, f"{name} row {b} kv-head {j} document {doc}", floor=fl.get(nm))
            check_lse_ext(sl(lse, hs), ref, softcap or None, None if sink is None else sink[hs], name)
        for b in range(B):   # the tokens in no document
            ln = int(lens[b])
            for x in (o, dq, dk, dv):
                assert not x[b, :, ln:].view(np.uint16).any(), f"{name} row {b}: a token in no document is not zero"
            if sink is None:
                assert np.isneginf(lse[b, :, ln:]).all()
        out["check"] = "ok"
    tail = f", {out['fwd_over_batched']} / {out['bwd_over_batched']} of the batched window call" if equal else ""
    print(f"[attn_span_bench] {name}: fwd {out['fwd_time_ratio']} / bwd {out['bwd_time_ratio']} of the document call for {out['tile_ratio']} of its tiles{tail}",
          file=sys.stderr, flush=True)
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
    res = {"tool": "attn_span_bench", "device": props.name.decode(), "iters": args.iters, "results": [run_case(c, args) for c in cases]}
    res.update(bench.stamp(("attn_ext.hip", "attn_full.hip", "attn_full_kernels.h", "common.h", "runtime.hip")))   # the sources every column comes from
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
