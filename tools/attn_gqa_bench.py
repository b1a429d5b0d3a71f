#!/usr/bin/env python3
"""Grouped-query attention (kf_attn_fwd_gqa / kf_attn_bwd_gqa) against the multi-head call and against the same work composed from
existing operators, through the C ABI.

For each case (bf16; Hq query heads, Hkv K/V heads, G = Hq / Hkv), median HIP-event times over --iters after --warmup, all in one
interleaved loop:
  gqa_fwd / gqa_bwd   kf_attn_fwd_gqa / kf_attn_bwd_gqa with the recommended workspace
  mha_fwd / mha_bwd   kf_attn_fwd_scaled / kf_attn_bwd_scaled at the same Hq, every query head reading one shared K/V (the same
                      matrix work; only the K/V bytes differ)
  composed_*          repeat K and V to [B, Hq, S, D] (kf_elementwise copy, stride 0 over the group), the multi-head call, and (backward)
                      dK, dV summed over each group (kf_reduce): what a GQA model runs without this entry
  group_sum           the attn_bwd_dkv_group_sum kernel alone (its kf_profile samples inside the gqa backward), and TB/s of its
                      algorithmic bytes: read 2 B Hq Skv D es, write 2 B Hkv Skv D es
--check samples two heads per case against the f64 numpy reference (o, lse and dq; oracle/checks.attn_check).
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

# (name, B, S, D, Hq, Hkv)
CASES = [
    ("MHA 32/32", 8, 4096, 128, 32, 32),
    ("GQA 32/8", 8, 4096, 128, 32, 8),
    ("GQA 32/4", 8, 4096, 128, 32, 4),
    ("MQA 32/1", 8, 4096, 128, 32, 1),
    ("GQA 64/8 D64", 8, 4096, 64, 64, 8),
]


def event_ms(fn):
    a, b = H.Event(), H.Event()
    a.record()
    keep = fn()  # (workspaces a call hands back stay alive until the events have completed)
    b.record()
    b.sync()
    del keep
    return a.elapsed_ms(b)


def run_case(case, args):
    name, B, S, D, Hq, Hkv = case
    G, code, es = Hq // Hkv, H.BF16, 2
    scale = float(np.float32(1.0) / np.sqrt(np.float32(D)))
    rng = np.random.default_rng(len(name))
    r = lambda shp: O.f32_to_bf16(rng.uniform(-1, 1, shp).astype(np.float32))  # noqa: E731
    q, go = r((B, Hq, S, D)), r((B, Hq, S, D))
    k, v = r((B, Hkv, S, D)), r((B, Hkv, S, D))
    nq, nkv = q.nbytes, k.nbytes
    bq, bgo, bk, bv = (H.DevBuf.from_numpy(x) for x in (q, go, k, v))
    bo, blse, bdq, bdk, bdv = H.DevBuf(nq), H.DevBuf(4 * B * Hq * S), H.DevBuf(nq), H.DevBuf(nkv), H.DevBuf(nkv)
    rec, mn = H.attn_bwd_gqa_workspace_bytes(code, B, Hq, Hkv, S, S, D)
    ws = H.DevBuf(rec)
    # the multi-head baseline: one shared K/V (head 0 of every batch: stride 0 over heads through repeated pointers is not expressible,
    # so the repeated tensors are materialised once, outside the timed loop) and the composition's buffers
    brk, brv, bdkr, bdvr = H.DevBuf(nq), H.DevBuf(nq), H.DevBuf(nq), H.DevBuf(nq)
    mha_need = H.attn_bwd_workspace_bytes(code, B, Hq, S, S, D)
    mws = H.DevBuf(mha_need)
    src = lambda p: H.View(p, (B, Hkv, G, S, D), (Hkv * S * D, S * D, 0, D, 1), code)  # noqa: E731
    dst = lambda p: H.View(p, (B, Hkv, G, S, D), (Hkv * G * S * D, G * S * D, S * D, D, 1), code)  # noqa: E731
    red = lambda p: H.View(p, (B, Hkv, 1, S, D), (Hkv * S * D, S * D, S * D, D, 1), code)  # noqa: E731

    def repeat():
        H.elementwise(H.EW_COPY, H.make_desc([dst(brk.ptr)], [src(bk.ptr)]), code)
        H.elementwise(H.EW_COPY, H.make_desc([dst(brv.ptr)], [src(bv.ptr)]), code)

    def gsum():
        keep = [H.reduce(H.RED_SUM, H.make_reduce_desc(red(bdk.ptr), dst(bdkr.ptr), 2)), H.reduce(H.RED_SUM, H.make_reduce_desc(red(bdv.ptr), dst(bdvr.ptr), 2))]
        return keep

    repeat()
    H.device_sync()
    gqa_fwd = lambda: H.attn_fwd_gqa(code, B, Hq, Hkv, S, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr)  # noqa: E731
    gqa_bwd = lambda: H.attn_bwd_gqa(code, B, Hq, Hkv, S, S, D, scale, bq.ptr, bk.ptr, bv.ptr, bo.ptr, blse.ptr, bgo.ptr, bdq.ptr, bdk.ptr,  # noqa: E731
                                     bdv.ptr, ws.ptr, rec)
    mha_fwd = lambda: H.check(H.lib().kf_attn_fwd_scaled(code, B, Hq, S, S, D, scale, bq.ptr, brk.ptr, brv.ptr, bo.ptr, blse.ptr, None))  # noqa: E731
    mha_bwd = lambda: H.check(H.lib().kf_attn_bwd_scaled(code, B, Hq, S, S, D, scale, bq.ptr, brk.ptr, brv.ptr, bo.ptr, blse.ptr, bgo.ptr,  # noqa: E731
                                                         bdq.ptr, bdkr.ptr, bdvr.ptr, mws.ptr, mha_need, None))

    def comp_fwd():
        repeat()
        mha_fwd()

    def comp_bwd():
        repeat()
        mha_bwd()
        return gsum()

    timed = {"gqa_fwd": gqa_fwd, "gqa_bwd": gqa_bwd, "mha_fwd": mha_fwd, "mha_bwd": mha_bwd}
    if G > 1:
        timed.update(composed_fwd=comp_fwd, composed_bwd=comp_bwd)
    t = {n: [] for n in timed}
    for it in range(args.warmup + args.iters):
        for n, fn in timed.items():
            ms = event_ms(fn)
            if it >= args.warmup:
                t[n].append(ms)
    out = {"case": name, "B": B, "S": S, "D": D, "Hq": Hq, "Hkv": Hkv, "workspace_recommended": rec, "workspace_minimum": mn}
    out.update({f"{n}_ms": round(statistics.median(v), 4) for n, v in t.items()})
    if G > 1:
        H.profile_reset()
        H.profile_enable(True)
        for _ in range(args.iters):
            gqa_bwd()
        H.profile_enable(False)
        s = H.profile_samples().get("attn_bwd_dkv_group_sum")
        gs = float(np.median(s))
        nbytes = 2 * B * Hq * S * D * es + 2 * B * Hkv * S * D * es
        out.update(group_sum_ms=round(gs, 4), group_sum_tbps=round(nbytes / (gs * 1e-3) / 1e12, 2), group_sum_bytes=nbytes)
    if args.check:
        from oracle import checks as K
        gqa_fwd()
        gqa_bwd()
        H.device_sync()
        o, lse, dq = bo.to_numpy(q.shape, q.dtype), blse.to_numpy((B, Hq, S), np.float32), bdq.to_numpy(q.shape, q.dtype)
        for b, h in ((0, 0), (B - 1, Hq - 1)):
            j = h // G
            sl = lambda x, hh: x[b:b + 1, hh:hh + 1]  # noqa: E731
            K.attn_check(sl(q, h), sl(k, j), sl(v, j), code, o=sl(o, h), lse=sl(lse, h), d_o=sl(go, h), dq=sl(dq, h), what=f"{name} b{b} h{h}")
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
    res = {"tool": "attn_gqa_bench", "results": [run_case(c, args) for c in cases]}
    print(json.dumps(res, indent=1))
    if args.json:
        Path(args.json).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
